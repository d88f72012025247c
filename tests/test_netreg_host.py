"""The pathway-graph regularizers on the host (no GPU): the package's constructors against the reference's literals
(tests/golden/network_reg.json <- test/runtests.jl:637-733, 795-811), the composites of construct_X_reg / construct_Y_reg
(runtests.jl:996-1079), the marshalled CSR arrays, reweight_eb_ / reorder against hand formulas, and the f32 restatement of
the device's CG rule (tests/netreg_ref.py) against the exact fp64 solve on the five graph families of the design note."""
import json
from pathlib import Path

import numpy as np
import pytest

import netreg_ref as NR

GOLD = json.loads((Path(__file__).resolve().parent / "golden" / "network_reg.json").read_text())


def _dense(A):
    return np.asarray(A.todense())


def test_network_constructor_literals(pkg):
    R = pkg.regularizers
    g = GOLD["synthetic"]
    nr = R.NetworkRegularizer(g["data_features"], g["edgelists"])
    assert len(nr.AA) == g["n_factors"] == len(nr.AB) == len(nr.BB) == len(nr.x_virtual)
    assert nr.AA[0].shape == (3, 3) and nr.AB[0].shape == (3, 1) and nr.BB[0].shape == (1, 1)
    assert np.array_equal(_dense(nr.AA[0]), np.array(g["AA1"]))          # runtests.jl:648-652 (==, not isapprox)
    assert np.array_equal(_dense(nr.AB[0]), np.array(g["AB1"]))
    assert np.array_equal(_dense(nr.BB[0]), np.array(g["BB1"]))
    assert np.array_equal(nr.cur_weights, np.ones(2))
    assert all(np.array_equal(x, np.zeros(B.shape[0])) for x, B in zip(nr.x_virtual, nr.BB))
    nr = R.NetworkRegularizer(g["model_features"], g["edgelists"])      # every node observed: runtests.jl:661-666
    s = g["all_observed_shapes"]
    assert nr.AA[0].shape == tuple(s["AA"]) and nr.AB[0].shape == tuple(s["AB"]) and nr.BB[0].shape == tuple(s["BB"])
    g = GOLD["star"]
    nr = R.NetworkRegularizer(g["data_features"], g["edgelists"])
    assert len(nr.AA) == 1
    assert np.array_equal(_dense(nr.AA[0]), np.array(g["AA1"]))
    assert np.array_equal(_dense(nr.AB[0]), np.array(g["AB1"]))
    assert np.array_equal(_dense(nr.BB[0]), np.array(g["BB1"]))


def test_selective_l1_literal(pkg):
    g = GOLD["selective_l1"]
    reg = pkg.regularizers.SelectiveL1Reg(g["data_features"], g["edgelists"])
    assert reg.l1_idx.dtype == bool and np.array_equal(reg.l1_idx.astype(int), np.array(g["l1_idx"]))
    assert np.array_equal(reg.weight, np.ones(2, np.float32))
    l1 = pkg.regularizers.L1Regularizer(3, 2.5)
    assert np.array_equal(l1.weights, np.full(3, 2.5, np.float32))


def test_constructors_agree_with_the_independent_restatement(pkg):
    """repeated edges (the last counts), signed weights, epsilon and weight, virtual nodes sorted and appended"""
    rng = np.random.default_rng(11)
    n = 17
    el = NR.random_graph(rng, n, 6, 60)
    el += [[el[3][0], el[3][1], 0.25], [el[5][1], el[5][0], -2.0]]           # duplicates, one of them reversed
    nr = pkg.regularizers.NetworkRegularizer(list(range(n)), [el, []], epsilon=0.3, weight=1.7)
    AA, AB, BB = NR.dense_blocks(list(range(n)), el, epsilon=0.3, weight=1.7)
    np.testing.assert_allclose(_dense(nr.AA[0]), AA, rtol=1e-15, atol=0)
    np.testing.assert_allclose(_dense(nr.AB[0]), AB, rtol=1e-15, atol=0)
    np.testing.assert_allclose(_dense(nr.BB[0]), BB, rtol=1e-15, atol=0)
    assert nr.AB[1].shape == (n, 0) and nr.BB[1].shape == (0, 0)                # an empty edge list is legal
    np.testing.assert_allclose(_dense(nr.AA[1]), 0.3 * 1.7 * np.eye(n), rtol=1e-15)


def test_marshalled_csr_densifies_to_the_blocks(pkg):
    rng = np.random.default_rng(12)
    el = NR.random_graph(rng, 9, 4, 25)
    nr = pkg.regularizers.NetworkRegularizer(list(range(9)), [el])
    for A in (nr.AA[0], nr.AB[0], nr.BB[0]):
        shape, rp, col, val = pkg._lib.csr_arrays(A)
        assert rp.dtype == np.int64 and col.dtype == np.int32 and val.dtype == np.float32 and rp[0] == 0
        D = np.zeros(shape, np.float32)
        for i in range(shape[0]):
            cs = col[rp[i]:rp[i + 1]]
            assert np.all(np.diff(cs) > 0)                                       # sorted rows, no repeats
            D[i, cs] = val[rp[i]:rp[i + 1]]
        assert np.array_equal(D, _dense(A).astype(np.float32))


def test_composites_have_the_reference_types_order_and_weights(pkg):
    R = pkg.regularizers
    g = GOLD["selective_l1"]
    K, N, M = 2, 5, 4
    fid, fg = g["data_features"], g["edgelists"]
    views = [1] * N
    y = R.construct_Y_reg(K, N, fid, views, None, fg, 1.0, None, 1.0, False, False, None, 1.001, 0.8)   # runtests.jl:996-1002
    assert len(y.regularizers) == 3 and isinstance(y.regularizers[0], R.GroupRegularizer)
    assert isinstance(y.regularizers[1], R.ZeroReg) and isinstance(y.regularizers[2], R.NetworkRegularizer)
    assert y.mixture_p == (0.5, 0.0, 0.5)
    y = R.construct_Y_reg(K, N, fid, views, None, fg, 1.0, 1.0, None, False, False, None, 1.001, 0.8)   # :1013-1019
    assert isinstance(y.regularizers[1], R.SelectiveL1Reg) and isinstance(y.regularizers[2], R.ZeroReg)
    y = R.construct_Y_reg(K, N, fid, views, None, fg, None, 1.0, 1.0, False, False, None, 1.001, 0.8)   # :1021-1028
    assert isinstance(y.regularizers[1], R.SelectiveL1Reg) and isinstance(y.regularizers[2], R.NetworkRegularizer)
    assert y.mixture_p == (0.0, 0.5, 0.5) and np.all(y.regularizers[1].weight == 1.0)
    sg = [[[1, 2, 1.0]], [[3, 4, 1.0], [4, 9, 1.0]]]
    x = R.construct_X_reg(K, M, [1, 2, 3, 4], None, sg, None, 1.0, 1.0, False, False)                # :1048-1054
    assert len(x.regularizers) == 3 and isinstance(x.regularizers[2], R.NetworkRegularizer)
    assert np.all(x.regularizers[2].cur_weights == 1.0) and x.mixture_p == (0.0, 0.0, 1.0)
    x = R.construct_X_reg(K, M, [1, 2, 3, 4], [1, 1, 2, 2], sg, None, 5.678, 1.234, False, False)    # :1056-1066
    assert isinstance(x.regularizers[1], R.GroupRegularizer) and isinstance(x.regularizers[2], R.NetworkRegularizer)
    assert all(np.allclose(w, 5.678) for w in x.regularizers[1].group_weights)
    assert np.all(x.regularizers[2].cur_weights == 1.234) and x.mixture_p == (0.0, 0.5, 0.5)
    assert x.regularizers[2].BB[1].shape == (1, 1)                                                     # node 9 is virtual


def test_make_model_derives_K_from_the_graphs(pkg):
    rng = np.random.default_rng(5)
    D = rng.standard_normal((6, 5)).astype(np.float32)
    g = GOLD["selective_l1"]
    m = pkg.model.make_model(D, feature_ids=g["data_features"], feature_graphs=g["edgelists"], lambda_Y_graph=1.0,
                             lambda_Y_selective_l1=1.0, rng=np.random.default_rng(1))
    R = pkg.regularizers
    assert m.matfac.Y.shape == (2, 5)
    assert isinstance(m.matfac.Y_reg.regularizers[1], R.SelectiveL1Reg)
    assert isinstance(m.matfac.Y_reg.regularizers[2], R.NetworkRegularizer)


def test_reweight_eb_hand_formulas(pkg):
    R, F = pkg.regularizers, pkg.fit
    g = GOLD["selective_l1"]
    rng = np.random.default_rng(13)
    Y = rng.standard_normal((2, 5))
    var1 = np.array([np.sum((r - r.mean()) ** 2) / (len(r) - 1) for r in Y])       # Julia's var: n - 1
    l1 = R.L1Regularizer(2, 1.0)
    F.reweight_eb_(l1, Y, mixture_p=0.5)                                           # regularizers.jl:88-92
    np.testing.assert_allclose(l1.weights, 0.5 / var1, rtol=1e-6)
    sel = R.SelectiveL1Reg(g["data_features"], g["edgelists"])
    F.reweight_eb_(sel, Y, mixture_p=0.5)                                          # :149-159
    sx = np.where(np.array(g["l1_idx"], bool), Y, 0.0)
    want = 0.5 * np.sqrt(2.0 / (np.mean(sx ** 2, axis=1) - np.mean(sx, axis=1) ** 2))
    np.testing.assert_allclose(sel.weight, want, rtol=1e-6)
    sel.l1_idx[1, :] = False                                                        # zero variance: weight 1 (:157)
    F.reweight_eb_(sel, Y)
    assert sel.weight[1] == 1.0
    nr = R.NetworkRegularizer([1, 2, 3, 4, 5], g["edgelists"], weight=2.0)
    AA0 = [_dense(A) for A in nr.AA]
    BB0 = [_dense(A) for A in nr.BB]
    F.reweight_eb_(nr, Y, mixture_p=0.5)                                           # :313-328
    for k in range(2):
        np.testing.assert_allclose(_dense(nr.AA[k]), AA0[k] * (0.5 / var1[k]) / 2.0, rtol=1e-12)
        np.testing.assert_allclose(_dense(nr.BB[k]), BB0[k] * (0.5 / var1[k]) / 2.0, rtol=1e-12)
    np.testing.assert_allclose(nr.cur_weights, 0.5 / var1, rtol=1e-12)
    comp = R.construct_composite_reg([R.SelectiveL1Reg(g["data_features"], g["edgelists"]), R.L1Regularizer(2, 1.0)], [0.25, 0.75])
    F.reweight_eb_(comp, Y)                                                        # :634-638: the mixture weight goes in
    np.testing.assert_allclose(comp.regularizers[1].weights, 0.75 / var1, rtol=1e-6)


def test_reorder_permutes_the_graph_terms(pkg):
    R, F = pkg.regularizers, pkg.fit
    g = GOLD["synthetic"]
    nr = R.NetworkRegularizer(g["data_features"], g["edgelists"])
    nr.cur_weights[...] = [1.0, 2.0]
    nr.x_virtual = (np.array([7.0]), np.array([8.0]))
    a0, a1 = _dense(nr.AA[0]), _dense(nr.AA[1])
    F._reorder_reg(nr, np.array([1, 0]))                                           # regularizers.jl:330-338
    assert np.array_equal(_dense(nr.AA[0]), a1) and np.array_equal(_dense(nr.AA[1]), a0)
    assert nr.x_virtual[0][0] == 8.0 and list(nr.cur_weights) == [2.0, 1.0]
    sel = R.SelectiveL1Reg([1, 2, 3, 4, 5], [[[1, 2, 1.0]], [[3, 4, 1.0]]])
    m0 = sel.l1_idx.copy()
    F._reorder_reg(sel, np.array([1, 0]))                                          # :161-163
    assert np.array_equal(sel.l1_idx, m0[[1, 0]])
    l1 = R.L1Regularizer(np.array([1.0, 2.0, 3.0]))
    F._reorder_reg(l1, np.array([2, 0, 1]))                                        # :98-100
    assert list(l1.weights) == [3.0, 1.0, 2.0]


def _families():
    rng = np.random.default_rng(2026)
    yield "random-120", 300, NR.random_graph(rng, 300, 120, 900)
    yield "random-900", 700, NR.random_graph(rng, 700, 900, 5000)
    yield "random-400", 500, NR.random_graph(rng, 500, 400, 2500)
    yield "hub-899", 600, NR.hub_graph(600, 299)
    yield "chain-1000", 200, NR.chain_graph(1000, 800)


@pytest.mark.parametrize("name,n,el", list(_families()), ids=lambda x: x if isinstance(x, str) else "")
def test_f32_cg_rule_against_the_exact_solve(name, n, el):
    """The device's CG rule (f32 vectors, f64 dot products, stop at |r| <= 1e-6 |t| or 2 v iterations) restated on the CPU:
    its gradient stays within 2e-6 of max|g| of the exact fp64 Schur-complement form -- the tolerance
    tests/test_gpu_reg_literals.py grants f32 gradients -- far below the 2 v cap.  Measured: <= 3.9e-7, 2 to 42 iterations."""
    rng = np.random.default_rng(7)
    b = NR.dense_blocks(list(range(n)), el)
    p = rng.standard_normal(n)
    loss, g, u = NR.exact_one(*b, p)
    loss32, g32, u32, it = NR.restated_one(*b, p.astype(np.float32))
    _, g64p, _ = NR.exact_one(*b, p.astype(np.float32))                  # the same f32-rounded input in f64
    dev = np.max(np.abs(g32 - g64p)) / np.max(np.abs(g64p))
    print(f"{name}: v = {b[2].shape[0]}, cond(BB) = {np.linalg.cond(b[2]):.1f}, CG iterations {it}, "
          f"gradient deviation {dev:.3e} of max|g|, loss deviation {abs(loss32 - loss) / abs(loss):.3e}")
    assert dev < 2e-6
    assert it < 2 * b[2].shape[0]
    # a warm start at the solution stops at once, a warm start nearby takes fewer iterations
    _, _, _, it_warm = NR.restated_one(*b, p.astype(np.float32), u0=u32)
    assert it_warm <= 1
