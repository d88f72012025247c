"""Factor importance without a device: the float64 reference of tests/importance_ref.py against the C oracle, its float32 twin
against the rounding bound (the check that the bound is not vacuous), the extension header against its signature table, the
symbols the library exports, and explained_deviance's aggregation.

The C oracle has the normal, Bernoulli and Poisson models; on the cases that hold squared-hinge columns the data losses come
from hinge_ref.reference, the float64 model that tests/test_hinge_cases.py holds equal to the oracle on the oracle's kinds."""
import copy
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import abi_header
import hinge_ref as hr
import importance_ref as ir
from problems import to_oracle

CASES = list(ir.cases())


def data_loss(p):
    if (hr.kinds_of(p) == 3).any():
        return hr.reference(p)["data_loss"]
    return to_oracle(p).loss_and_grads()[1]["data_loss"]


@pytest.mark.parametrize("name", CASES)
def test_the_reference_sums_to_the_oracles_losses(name):
    """sum_j full[j] is the data loss; sum_j delta[k, j] the data loss with row k of X zeroed minus the data loss, both to
    1e-10 of the larger loss (the difference of two losses has no better scale); sum_j null[j] the loss with X zeroed."""
    p = ir.cases()[name]
    r, _ = ir.reference_of(p)
    L = data_loss(p)
    assert abs(r["full"].sum() - L) <= 1e-10 * abs(L), (r["full"].sum(), L)
    q = copy.copy(p)
    q["X"] = np.zeros_like(p["X"])
    L0 = data_loss(q)
    assert abs(r["null"].sum() - L0) <= 1e-10 * abs(L0)
    for k in range(p["K"]):
        q["X"] = np.array(p["X"], order="F")
        q["X"][k] = 0
        Lk = data_loss(q)
        assert abs(r["delta"][k].sum() - (Lk - L)) <= 1e-10 * max(abs(Lk), abs(L)), (k, r["delta"][k].sum(), Lk - L)
    assert np.array_equal(r["n_obs"], np.isfinite(p["D"]).sum(0))


@pytest.mark.parametrize("name", CASES)
def test_the_float32_twin_is_within_a_bound_that_says_something(name):
    p = ir.cases()[name]
    r, b = ir.reference_of(p)
    tw = ir.twin(p)
    ir.check(tw, p)
    rd, rf, rn = ir.worst_ratios(p, r, tw)
    print(f"{name}: twin error / bracket: delta {rd:.3f} (C_DELTA {ir.C_DELTA}), full {rf:.3f} (C_FULL {ir.C_FULL}), "
          f"null {rn:.3f} (C_NULL {ir.C_NULL})")
    assert 4 * rd <= ir.C_DELTA and 4 * rf <= ir.C_FULL and 4 * rn <= ir.C_NULL, (rd, rf, rn)   # the margin of 4 still holds
    for k in ("delta", "full", "null"):
        share = float(np.mean(b[k] > 0.1 * np.abs(r[k])))
        print(f"{name}: {k}: bound above a tenth of the value on {100 * share:.2f} % of the elements")
        assert share <= 0.05, (k, share)


def test_the_twin_flushes_its_chain_and_zero_terms_are_exactly_absent():
    p = copy.copy(ir.cases()["mix-45x37-k2"])
    reps = 30                                                                  # 1350 rows: three chains per column
    p.update(M=45 * reps, D=np.asfortranarray(np.tile(p["D"], (reps, 1))), X=np.asfortranarray(np.tile(p["X"], (1, reps))))
    assert p["M"] > 2 * ir.CHAIN and not p["batch_views"]
    p["X"][1] = 0
    r = ir.reference(p)
    tw = ir.twin(p)
    ir.check(tw, p, ref=(r, ir.bounds(r)))
    assert (r["delta"][1] == 0).all() and (tw["delta"][1] == 0).all() and (ir.bounds(r)["delta"][1] == 0).all()
    assert (r["delta"][0] != 0).all()


def test_the_extension_header_matches_its_signature_table(pkg, monkeypatch):
    from test_abi import signature_errors
    monkeypatch.setattr(abi_header, "HEADER", abi_header.HEADER.parent / "pmf_hip_importance.h")
    protos, structs = abi_header.parse()
    abi = pkg._abi
    assert structs == {} and len(protos) == 2
    assert list(protos) == list(abi.IMPORTANCE_SIGNATURES)
    assert signature_errors(abi, abi.IMPORTANCE_SIGNATURES, protos) == []
    assert not set(abi.IMPORTANCE_SIGNATURES) & (set(abi.SIGNATURES) | set(abi.THRESHOLD_SIGNATURES))
    lib = pkg._lib.load_library()
    for name, (restype, argtypes) in abi.IMPORTANCE_SIGNATURES.items():
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    with pytest.raises(ctypes.ArgumentError):
        lib.pmf_factor_importance(None, 1.5, None, None, None)
    txt = abi_header.HEADER.read_text()
    assert f"#define PMF_IMPORTANCE_CHAIN {abi.IMPORTANCE_CHAIN}\n" in txt and abi.IMPORTANCE_CHAIN == ir.CHAIN


def test_every_new_symbol_is_exported(pkg):
    lib = ctypes.CDLL(str(pkg._lib.LIB_PATH))
    for name in pkg._abi.IMPORTANCE_SIGNATURES:
        assert hasattr(lib, name), f"{name} declared in include/pmf_hip_importance.h but not exported"
    assert pkg.factor_importance is pkg.importance.factor_importance and pkg.explained_deviance is pkg.importance.explained_deviance


def test_explained_deviance_aggregates_by_view(pkg):
    # views in order of first appearance (Julia's unique), not sorted; "none" has no observed entry
    model = SimpleNamespace(feature_views=["rna", "rna", "cnv", "rna", "none", "cnv"])
    delta = np.array([[1.0, 2.0, 3.0, 4.0, 0.0, 5.0], [0.5, 0.5, -1.0, 1.0, 0.0, 3.0]])
    imp = pkg.FactorImportance(delta, np.array([1.0, 1.0, 2.0, 2.0, 0.0, 2.0]), np.array([4.0, 4.0, 8.0, 2.0, 0.0, 8.0]),
                               np.array([3, 3, 3, 3, 0, 3]))
    with np.errstate(all="raise"):                                             # NaN without a warning
        e = pkg.explained_deviance(model, imp)
    assert e["views"] == ["rna", "cnv", "none"]
    assert e["factor"].shape == (2, 3) and e["total"].shape == (3,)
    assert np.allclose(e["factor"][:, 0], [7.0 / 10.0, 2.0 / 10.0]) and np.allclose(e["factor"][:, 1], [8.0 / 16.0, 2.0 / 16.0])
    assert np.allclose(e["total"][:2], [1 - 4.0 / 10.0, 1 - 4.0 / 16.0])
    assert np.isnan(e["factor"][:, 2]).all() and np.isnan(e["total"][2])
    assert np.array_equal(pkg.explained_deviance(model, tuple(imp))["factor"], e["factor"], equal_nan=True)
