"""Host-side conditions that make the device comparison of tests/test_gpu_thresholds.py mean something: the float64 reference
(tests/threshold_ref.py) is a gradient, the problems exercise every finite threshold well above the tolerance, the faults a
kernel could have are each far outside it, the trajectories compared are descents, the clamp problem does cross, the
initialisation rule has its known answer, and the extension header agrees with the binding's table.

The problems are layouts A and B of tests/hinge_ref.py with every finite threshold raised by SHIFT = 0.4 (problem()).  At the
thresholds the layouts' data were drawn with, a group's gradient nearly vanishes -- the entries below a threshold pull it one
way, those above it the other -- while its error scale adds magnitudes: the smallest |G| / tolerance is then 16 .. 217 per
problem, below the 100 required here on half of them.  Away from that stationary point it is 1300 or more on every problem."""
import ctypes
import functools

import numpy as np
import pytest

import abi_header
import hinge_ref as hr
import threshold_ref as tr
from problems import LAYER_TAU

OPT = dict(adagrad=dict(kind="adagrad", lr=0.05, eps=1e-8, beta1=0.9, beta2=0.999),
           adam=dict(kind="adam", lr=0.01, eps=1e-8, beta1=0.9, beta2=0.999))
GRAD_PROBLEMS = [(n, K, b) for n in "AB" for K in hr.KS for b in (False, True)]
TRAJ_PROBLEMS = [("A", 20), ("B", 80)]           # batch variants (the plain ones rise at the second epoch under AdaGrad 0.05)
EPOCHS = 6
SHIFT = 0.4


@functools.lru_cache(maxsize=None)
def problem(name, K, batch=False):
    """hinge_ref.layout(name, K, batch) with every finite threshold raised by SHIFT (a shared object: do not modify it)."""
    p = hr.layout(name, K, batch)
    tg = tr.group_thresholds(p)
    return tr.with_thresholds(p, np.where(np.isfinite(tg), tg + SHIFT, tg))


def big(name, K, M=600):
    """Layout `name` at M rows (several row panels at both wave counts, ragged at the end): the M = 70 problem tiled."""
    p = dict(problem(name, K, True))
    reps = -(-M // p["M"])
    rng = np.random.default_rng(K + M)
    p["X"] = np.asfortranarray(np.tile(p["X"], (1, reps))[:, :M] + (0.05 * rng.standard_normal((K, M))).astype(np.float32))
    p["D"] = np.asfortranarray(np.tile(p["D"], (reps, 1))[:M])
    p["batch_views"] = [dict(v, batch_of_row=np.tile(v["batch_of_row"], reps)[:M]) for v in p["batch_views"]]
    p["M"] = M
    return p


def clamp_problem():
    """Layout B, K = 20, batch views, whose first group starts too wide, at (-inf, -1, 1): the gradient pulls t1 up and t2
    down, and one AdaGrad step of lr 1.2 (nearly lr sign(g) each) carries them past each other."""
    p = dict(problem("B", 20, True))
    p["noise_thr"] = [(-np.inf, -1.0, 1.0)] + list(p["noise_thr"][1:])
    return p


CLAMP_OPT = dict(kind="adagrad", lr=1.2, eps=1e-8, beta1=0.9, beta2=0.999)


def test_the_reference_gradient_matches_central_differences():
    for name, K, batch in [("A", 20, False), ("B", 80, True), ("A", 128, True)]:
        p = problem(name, K, batch)
        G, tg = tr.group_grad(p), tr.group_thresholds(p)
        h = 1e-6
        for r in range(tg.shape[0]):
            for m in range(3):
                if not np.isfinite(tg[r, m]):
                    assert G[r, m] == 0.0
                    continue
                lo, hi = tg.copy(), tg.copy()
                lo[r, m] -= h
                hi[r, m] += h
                fd = (hr.reference(tr.with_thresholds(p, hi))["data_loss"] - hr.reference(tr.with_thresholds(p, lo))["data_loss"]) / (2 * h)
                assert abs(fd - G[r, m]) <= 1e-6 * abs(G[r, m]), (name, K, batch, r, m, fd, G[r, m])


@pytest.mark.parametrize("name,K,batch", GRAD_PROBLEMS)
def test_every_finite_threshold_is_exercised(name, K, batch):
    """|G| > 100 tolerances for every finite threshold of every problem the device tests use."""
    p = problem(name, K, batch)
    G, tol = tr.group_grad(p), LAYER_TAU * tr.group_scale(p)
    fin = np.isfinite(tr.group_thresholds(p))
    print("THRESH ratio", name, K, batch, np.round(np.abs(G[fin]) / tol[fin], 1))
    assert fin.any() and (np.abs(G[fin]) > 100 * tol[fin]).all(), (G, tol)


@pytest.mark.parametrize("name,K,batch", GRAD_PROBLEMS)
def test_every_fault_shows(name, K, batch):
    p = problem(name, K, batch)
    G, tol = tr.group_grad(p), LAYER_TAU * tr.group_scale(p)
    fin = np.isfinite(tr.group_thresholds(p))
    gc, tc = tr.col_grad(p), LAYER_TAU * tr.col_scale(p)
    for fault in ("off_by_one", "swap_ab", "drop_ragged") + (("neighbour",) if name == "B" else ()):
        bad = tr.group_grad(p, fault)
        assert (np.abs(bad - G)[fin] > 10 * tol[fin]).any(), fault
        k3 = ~np.isnan(gc[:, 0])
        assert (np.abs(tr.col_grad(p, fault) - gc)[k3] > 10 * tc[k3]).any(), fault


@pytest.mark.parametrize("name,K", [("A", 48), ("B", 128)])
def test_the_large_problems_are_exercised_too(name, K):
    """The M = 600 problems of the grid-capped device test."""
    p = big(name, K)
    G, tol = tr.group_grad(p), LAYER_TAU * tr.group_scale(p)
    fin = np.isfinite(tr.group_thresholds(p))
    assert (np.abs(G[fin]) > 100 * tol[fin]).all(), np.abs(G[fin]) / tol[fin]


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
@pytest.mark.parametrize("name,K", TRAJ_PROBLEMS)
def test_the_compared_trajectories_descend(name, K, opt):
    p = problem(name, K, True)
    state, losses = tr.fresh_state(p, OPT[opt]), []
    for t in range(1, EPOCHS + 2):
        p, state, info = tr.joint_epoch(p, state, OPT[opt], t)
        losses.append(info["loss"])
    assert (np.diff(losses) < 0).all(), losses
    t0, t1 = tr.group_thresholds(problem(name, K, True)), tr.group_thresholds(p)
    fin = np.isfinite(t0)
    assert (t1[fin] != t0[fin]).all() and np.array_equal(t1[~fin], t0[~fin])


def test_the_clamp_problem_crosses_before_the_clamp():
    p = clamp_problem()
    G, tol = tr.group_grad(p), LAYER_TAU * tr.group_scale(p)
    fin = np.isfinite(tr.group_thresholds(p))
    assert (np.abs(G[fin]) > 100 * tol[fin]).all()
    _, _, info = tr.joint_epoch(p, tr.fresh_state(p, CLAMP_OPT), CLAMP_OPT, 1)
    raw = info["raw"][0]
    assert raw[2] < raw[1], raw
    assert tr.clamp(raw)[2] == raw[1]


def test_init_known_answer():
    t = tr.init_thresholds([0, 5, 3, 1], (-np.inf, -0.5, 0.5))
    assert np.isneginf(t[0])
    assert t[1] == np.float32(np.log(0.995)) and t[2] == np.float32(np.log(4.955)), t
    # class-0 entries of an ordinal range are not an allowed class: they change nothing
    assert np.array_equal(tr.init_thresholds([7, 5, 3, 1], (-np.inf, -0.5, 0.5)), t)


def test_the_package_states_the_same_rule(pkg):
    f = pkg.fit.ordinal_thresholds_from_counts
    for counts, triple in [([0, 5, 3, 1], (-np.inf, -0.5, 0.5)), ([9, 5, 3, 1], (-np.inf, 0.0, 1.0)), ([4, 6, 0, 0], (0.0, np.inf, np.inf)),
                           ([1, 2, 3, 4], (-1.0, 0.0, 1.0))]:
        assert np.array_equal(np.asarray(f(counts, triple), np.float32), tr.init_thresholds(counts, triple)), (counts, triple)
    nm = pkg.matfac.CompositeNoise(["normal"] * 3 + ["ordinal_sq_hinge3"] * 4)
    assert nm.train_thresholds is False and nm.train_thresholds_(True).train_thresholds is True


def test_the_extension_header_matches_its_signature_table(pkg, monkeypatch):
    from test_abi import signature_errors
    monkeypatch.setattr(abi_header, "HEADER", abi_header.HEADER.parent / "pmf_hip_thresholds.h")
    protos, structs = abi_header.parse()
    abi = pkg._abi
    assert structs == {} and len(protos) == 6
    assert list(protos) == list(abi.THRESHOLD_SIGNATURES)
    assert signature_errors(abi, abi.THRESHOLD_SIGNATURES, protos) == []
    assert not set(abi.THRESHOLD_SIGNATURES) & set(abi.SIGNATURES)
    lib = pkg._lib.load_library()
    for name, (restype, argtypes) in abi.THRESHOLD_SIGNATURES.items():
        f = getattr(lib, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name
    with pytest.raises(ctypes.ArgumentError):
        lib.pmf_set_threshold_training(None, 1.5)
