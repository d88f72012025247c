"""The pathway-graph regularizers on the DEVICE (csrc/pmf_netreg.hip, k_reg_step<true>): NetworkRegularizer, SelectiveL1Reg and
L1Regularizer marshalled through the C ABI and evaluated on the GPU, against the reference's literals
(tests/golden/network_reg.json) and the exact fp64 restatement of tests/netreg_ref.py.  Value and gradient are read as
tests/test_gpu_reg_literals.py does: data term off (every entry of D missing), one Adam step at lr -> 0, gradient = first
moment / (1 - beta1).

Tolerances.  The device follows the CG rule of DESIGN.md section 2 (f32 vectors, f64 sums, stop at |r| <= 1e-6 |t|); the
same rule restated on the CPU (netreg_ref.restated) deviates from the exact solve by some d of max|g| on each input, and
the device is granted 10 d with a floor of 2e-6 (the f32 gradient tolerance of test_gpu_reg_literals.py).  d is computed
here from the restatement, never from the device."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import netreg_ref as NR
from problems import make_problem, rel_err, shard_problem, to_context

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLD = json.loads((ROOT / "tests" / "golden" / "network_reg.json").read_text())
B1 = 0.9
FLOOR = 2e-6


def _bare(ctx, M, N, K, X=None, Y=None):
    ctx.comm_set_chunks(0)
    ctx.set_data(np.full((M, N), np.nan, np.float32))          # no observed entry: data loss 0, data gradient 0
    ctx.set_factors(np.zeros((K, M), np.float32) if X is None else np.asarray(X, np.float32),
                    np.zeros((K, N), np.float32) if Y is None else np.asarray(Y, np.float32))
    ctx.set_col_params(np.zeros(N, np.float32), np.zeros(N, np.float32))
    ctx.set_batch_views([])
    ctx.set_noise([(1, N)], ["normal"], np.ones(N, np.float32))
    ctx.clear_xreg()
    ctx.clear_yreg()
    ctx.set_layer_regs()


def _value_and_grad(ctx, which):
    ctx.set_optimizer("adam", lr=1e-30, beta1=B1)               # lr -> 0: the parameters do not move
    o = ctx.make_opts(update_X=which == "X", update_Y=which == "Y")
    ctx.epoch_begin(o)
    ctx.epoch_step_local(o)
    ctx.epoch_step_shared(o)
    loss, shared = ctx.epoch_loss()
    _, mom = ctx.get_opt_state(which)
    value = shared if which == "Y" else loss - shared
    assert loss == value                                         # nothing but this regularizer contributes
    return value, mom.astype(np.float64) / (1.0 - B1)


def _attach(ctx, which, blocks, p=1.0, u0=None):
    ctx.add_reg_network(which, [NR.to_csr(b[0]) for b in blocks], [NR.to_csr(b[1]) for b in blocks],
                        [NR.to_csr(b[2]) for b in blocks], u0=u0, p=p)


def _iters(ctx, which, K):
    return [ctx.get_reg_network_state(which, k)[1] for k in range(K)]


# ---- the reference's literals ------------------------------------------------------------------------------------------
def test_star_graph_literal(pkg, ctx):
    """runtests.jl:699-716 (the reference asserts only the gradient's shape; the values are the exact Schur form):
    x = [1, 1, 1]: u = 3/3.1, value 1.65 - 9/6.2 = 0.19838709677, gradient 1.1 - 3/3.1 = 0.13225806452 per entry."""
    g = GOLD["star"]
    nr = pkg.regularizers.NetworkRegularizer(g["data_features"], g["edgelists"])
    _bare(ctx, 2, 3, 1, Y=np.array([g["x"]]))
    nr.add_to(ctx, "Y")
    val, grad = _value_and_grad(ctx, "Y")
    assert grad.shape == tuple(g["grad_shape"])
    assert val == pytest.approx(g["value_exact"], rel=1e-6)
    np.testing.assert_allclose(grad, g["grad_exact"], rtol=2e-6)
    u, it = ctx.get_reg_network_state("Y", 0)
    assert u[0] == pytest.approx(3 / 3.1, rel=1e-6) and it == 1
    nr.read_back(ctx, "Y")
    assert nr.x_virtual[0][0] == pytest.approx(3 / 3.1, rel=1e-6)


def test_selective_l1_literal_and_sign_of_zero(pkg, ctx):
    """runtests.jl:720-733: value sum |l1_idx .* Y|, gradient at ones(2, 5) = l1_idx; sign(0) = 0; L1Regularizer = full mask."""
    g = GOLD["selective_l1"]
    reg = pkg.regularizers.SelectiveL1Reg(g["data_features"], g["edgelists"])
    _bare(ctx, 2, 5, 2, Y=np.ones((2, 5)))
    reg.add_to(ctx, "Y")
    val, grad = _value_and_grad(ctx, "Y")
    assert val == 2.0
    np.testing.assert_allclose(grad, np.array(g["grad_at_ones"]), rtol=2e-6, atol=0)                               # :736
    rng = np.random.default_rng(21)
    Y = rng.standard_normal((2, 5)).astype(np.float32)
    Y[0, 4] = 0.0
    _bare(ctx, 2, 5, 2, Y=Y)
    reg.add_to(ctx, "Y")
    val, grad = _value_and_grad(ctx, "Y")
    assert val == pytest.approx(float(np.sum(np.abs(np.array(g["l1_idx"]) * Y.astype(np.float64)))), rel=1e-6)   # :729
    np.testing.assert_allclose(grad, np.array(g["l1_idx"]) * np.sign(Y), rtol=2e-6, atol=0)
    X = rng.standard_normal((3, 7)).astype(np.float32)
    X[1, 2] = 0.0
    _bare(ctx, 7, 4, 3, X=X)
    w = np.array([0.5, 2.0, 3.0], np.float32)
    pkg.regularizers.L1Regularizer(w).add_to(ctx, "X", p=0.25)
    val, grad = _value_and_grad(ctx, "X")
    assert val == pytest.approx(0.25 * float(np.sum(w[:, None] * np.abs(X.astype(np.float64)))), rel=1e-6)
    np.testing.assert_allclose(grad, 0.25 * w[:, None] * np.sign(X), rtol=2e-6, atol=0)


def test_composite_literal(pkg, ctx):
    """runtests.jl:795-811: construct_composite_reg([l1, net], [0.5, 0.5])(Y) = 0.5 (l1(Y) + net(Y))."""
    g = GOLD["selective_l1"]
    R = pkg.regularizers
    comp = R.construct_composite_reg([R.SelectiveL1Reg(g["data_features"], g["edgelists"]),
                                      R.NetworkRegularizer(g["data_features"], g["edgelists"])], GOLD["composite"]["mixture_p"])
    assert len(comp.regularizers) == 2
    Y = np.random.default_rng(22).standard_normal((2, 5)).astype(np.float32)
    _bare(ctx, 3, 5, 2, Y=Y)
    comp.add_to(ctx, "Y")
    val, grad = _value_and_grad(ctx, "Y")
    blocks = [NR.dense_blocks(g["data_features"], el) for el in g["edgelists"]]
    net, gnet, _ = NR.exact(blocks, Y.astype(np.float64))
    l1 = float(np.sum(np.abs(np.array(g["l1_idx"]) * Y.astype(np.float64))))
    assert val == pytest.approx(0.5 * (l1 + net), rel=2e-6)
    want = 0.5 * (np.array(g["l1_idx"]) * np.sign(Y) + gnet)
    assert np.max(np.abs(grad - want)) <= FLOOR * np.max(np.abs(want))


# ---- graph families against the exact fp64 form -------------------------------------------------------------------------
def _family(rng, kind, n):
    if kind == "random":
        return NR.random_graph(rng, n, int(rng.integers(3, 40)), int(rng.integers(50, 200)))
    if kind == "hub":
        return NR.hub_graph(n - 3, 11)
    if kind == "chain":
        return NR.chain_graph(n + 30, 40)                       # 10 observed nodes stay outside the chain
    if kind == "all_observed":
        return NR.random_graph(rng, n, 0, 60)                   # v = 0
    if kind == "empty":
        return []
    if kind == "isolated":                                      # half of the observed nodes touch no edge
        return NR.random_graph(rng, n, 9, 70, n_used=n // 2)
    raise ValueError(kind)


KINDS = ["random", "hub", "chain", "all_observed", "empty", "isolated"]


def _graphs(seed, K, n, big=None):
    rng = np.random.default_rng(seed)
    els = [_family(rng, KINDS[k % len(KINDS)], n) for k in range(K)]
    if big == "hub":                                            # a virtual hub of degree 899
        els[0] = NR.hub_graph(n - 1, 899 - (n - 1))
    if big == "global":                                         # v_k above the LDS budget of the solve kernel (4096)
        els[min(1, K - 1)] = NR.random_graph(rng, n, 4300, 9000)
    if big == "random-900":
        els[0] = NR.random_graph(rng, n, 900, 5000)
    return [NR.dense_blocks(list(range(n)), el) for el in els]


CASES = [(K, 77, None) for K in (1, 3, 32, 33, 64, 96, 128)] + [(3, 1301, "random-900"), (2, 613, "hub"), (3, 203, "global")]


@pytest.mark.parametrize("which", ["X", "Y"])
@pytest.mark.parametrize("K,n,big", CASES, ids=[f"K{K}-n{n}-{b}" for K, n, b in CASES])
def test_network_value_and_gradient_against_exact_fp64(ctx, which, K, n, big):
    blocks = _graphs(100 + K + n, K, n, big)
    rng = np.random.default_rng(K * 1000 + n)
    P = rng.standard_normal((K, n)).astype(np.float32)
    p_mix = 0.75
    m_other = 37                                                 # the other dimension: no multiple of a tile either
    if which == "X":
        _bare(ctx, n, m_other, K, X=P)
    else:
        _bare(ctx, m_other, n, K, Y=P)
    _attach(ctx, which, blocks, p=p_mix)
    val, grad = _value_and_grad(ctx, which)
    it_dev = _iters(ctx, which, K)
    loss64, g64, _ = NR.exact(blocks, P.astype(np.float64))
    loss32, g32, _, it_ref = NR.restated(blocks, P)
    gmax = np.max(np.abs(g64))
    d_g = np.max(np.abs(g32 - g64)) / gmax
    d_l = abs(loss32 - loss64) / abs(loss64)
    tol_g, tol_l = max(10 * d_g, FLOOR), max(10 * d_l, FLOOR)
    e_g = np.max(np.abs(grad - p_mix * g64)) / (p_mix * gmax)
    e_l = abs(val - p_mix * loss64) / abs(p_mix * loss64)
    vs = [b[2].shape[0] for b in blocks]
    print(f"\n{which} K={K} n={n} {big}: v_k max {max(vs)}; CG iterations device max {max(it_dev)} / restatement max {max(it_ref)}; "
          f"gradient error {e_g:.3e} (restatement {d_g:.3e}, tolerance {tol_g:.3e}); value error {e_l:.3e} (restatement {d_l:.3e}, "
          f"tolerance {tol_l:.3e})")
    assert e_g <= tol_g and e_l <= tol_l
    for k in range(K):                                           # below the 2 v_k cap wherever the restatement is
        if it_ref[k] < 2 * vs[k]:
            assert it_dev[k] < 2 * vs[k], (k, it_dev[k], it_ref[k], vs[k])
        if vs[k] == 0:
            assert it_dev[k] == 0
    # the solution itself, and a second evaluation from it: the warm start stops at once
    _, _, u64 = NR.exact(blocks, P.astype(np.float64))
    for k in (0, K - 1):
        u, _ = ctx.get_reg_network_state(which, k)
        if vs[k]:
            assert np.max(np.abs(u - u64[k])) <= 1e-5 * max(np.max(np.abs(u64[k])), 1e-30)
    val2, grad2 = _value_and_grad(ctx, which)
    assert max(_iters(ctx, which, K)) <= 2                       # (a rounded f32 solution may sit a hair above the bound)
    assert np.max(np.abs(grad2 - p_mix * g64)) / (p_mix * gmax) <= tol_g


# ---- with a live data term -----------------------------------------------------------------------------------------------
LIVE = dict(M=301, N=420, K=33, seed=41, nan_frac=0.1, weights=True, col_params=True, xreg="group", random_init=True, scale=0.5)


def _live_blocks(p, seed=9):
    return (_graphs(seed, p["K"], p["N"]), _graphs(seed + 1, p["K"], p["M"]))


def _attach_live(ctx, p, by, bx, with_x=True, u0=None, l1=True):
    to_context(p, ctx)                                            # (its xreg group term stays attached)
    _attach(ctx, "Y", by, p=0.5, u0=u0)
    if l1:
        ctx.add_reg_l1("Y", np.full(p["K"], 0.01, np.float32), None, 1.0)
    if with_x:
        _attach(ctx, "X", bx, p=0.5)


def test_additivity_with_a_live_data_term(ctx):
    """Adam's first moment after one step = (1 - beta1) (pmf_get_grad + regularizer gradient), at the parity tolerance of
    tests/test_gpu_parity.py (GRAD_TOL = 2e-4 of the largest entry)."""
    p = make_problem(**{**LIVE, "xreg": None})
    by, bx = _live_blocks(p)
    ctx.comm_set_chunks(0)
    to_context(p, ctx)
    _attach(ctx, "Y", by, p=0.5)
    _attach(ctx, "X", bx, p=2.0)
    ctx.set_optimizer("adam", lr=1e-30, beta1=B1)
    o = ctx.make_opts(update_X=True, update_Y=True)
    ctx.epoch_begin(o)
    gX, gY = ctx.get_grad("X").astype(np.float64), ctx.get_grad("Y").astype(np.float64)
    ctx.epoch_step_local(o)
    ctx.epoch_step_shared(o)
    loss, shared = ctx.epoch_loss()
    ly, ry, _ = NR.exact(by, p["Y"].astype(np.float64))
    lx, rx, _ = NR.exact(bx, p["X"].astype(np.float64))
    assert shared == pytest.approx(0.5 * ly, rel=1e-5)
    for which, g, r, w in (("X", gX, rx, 2.0), ("Y", gY, ry, 0.5)):
        mom = ctx.get_opt_state(which)[1].astype(np.float64) / (1.0 - B1)
        assert rel_err(mom, g + w * r) <= 2e-4, (which, rel_err(mom, g + w * r))
        assert rel_err(mom - g, w * r) <= 2e-4


def test_adagrad_descent_on_the_regularizer_alone(ctx):
    """20 AdaGrad epochs with every data entry missing against an fp64 numpy loop of the same epochs (exact solves): loss
    trace and parameters.  Tolerance: 10 x what the f32 restatement of the same loop (f32 parameters and accumulators, the
    device's CG rule with its warm start) deviates from the fp64 loop, floors 2e-6 (loss) and 2e-6 of max|Y| (parameters)."""
    K, n, lr, eps, epochs = 3, 203, 0.05, 1e-8, 20
    blocks = _graphs(7, K, n)
    Y0 = np.random.default_rng(8).standard_normal((K, n)).astype(np.float32)
    _bare(ctx, 5, n, K, Y=Y0)
    _attach(ctx, "Y", blocks)
    ctx.set_optimizer("adagrad", lr=lr, eps=eps)
    r = ctx.fit(update_Y=True, max_epochs=epochs, abs_tol=0, rel_tol=0)
    _, Yd = ctx.get_factors()

    def loop(dtype):
        Y, acc, u, tr = Y0.astype(dtype), np.full((K, n), eps, dtype), None, []
        for _ in range(epochs):
            if dtype == np.float64:
                l, g, _ = NR.exact(blocks, Y)
            else:
                l, g, u, _ = NR.restated(blocks, Y, u)
            tr.append(l)
            g = g.astype(dtype)
            acc = acc + g * g
            Y = Y - g * (dtype(lr) / (np.sqrt(acc) + dtype(eps)))
        return np.array(tr), Y
    t64, Y64 = loop(np.float64)
    t32, Y32 = loop(np.float32)
    tol_l = max(10 * np.max(np.abs(t32 - t64) / t64), FLOOR)
    tol_y = max(10 * rel_err(Y32, Y64), FLOOR)
    e_l, e_y = np.max(np.abs(r["loss"] - t64) / t64), rel_err(Yd, Y64)
    print(f"\nAdaGrad descent: loss error {e_l:.3e} (tolerance {tol_l:.3e}), parameter error {e_y:.3e} (tolerance {tol_y:.3e})")
    assert r["term_code"] == "max_epochs" and len(r["loss"]) == epochs
    assert e_l <= tol_l and e_y <= tol_y
    assert np.all(np.diff(r["loss"]) < 0)


# ---- same bits ---------------------------------------------------------------------------------------------------------
def _live_fit(ctx, p, by, bx, epochs=8, **kw):
    _attach_live(ctx, p, by, bx, **kw)
    ctx.set_optimizer("adagrad", lr=0.05)
    flags = dict(update_X=True, update_Y=True, max_epochs=epochs, abs_tol=0, rel_tol=0)
    return ctx.fit(**flags), ctx.get_factors()


def test_two_fresh_contexts_give_the_same_bits(pkg):
    p = make_problem(**LIVE)
    by, bx = _live_blocks(p)
    outs = []
    for _ in range(2):
        c = pkg.Context(0)
        try:
            outs.append(_live_fit(c, p, by, bx))
        finally:
            c.close()
    (r0, (X0, Y0)), (r1, (X1, Y1)) = outs
    assert np.all(np.isfinite(r0["loss"])) and len(r0["loss"]) == 8
    np.testing.assert_array_equal(r0["loss"], r1["loss"])
    np.testing.assert_array_equal(X0, X1)
    np.testing.assert_array_equal(Y0, Y1)


def test_python_loop_and_c_loop_give_the_same_bits(pkg, ctx):
    p = make_problem(**LIVE)
    by, bx = _live_blocks(p)
    ctx.comm_set_chunks(0)
    rc, (Xc, Yc) = _live_fit(ctx, p, by, bx)
    uc = [ctx.get_reg_network_state("Y", k)[0] for k in range(p["K"])]
    _attach_live(ctx, p, by, bx)
    ctx.set_optimizer("adagrad", lr=0.05)
    rp = pkg.parallel.fit_distributed(ctx, dist=None, update_X=True, update_Y=True, max_epochs=8, abs_tol=0, rel_tol=0)
    Xp, Yp = ctx.get_factors()
    assert rp["term_code"] == rc["term_code"] and rp["epochs"] == rc["epochs"]
    np.testing.assert_array_equal(rp["loss"], rc["loss"])
    np.testing.assert_array_equal(Xp, Xc)
    np.testing.assert_array_equal(Yp, Yc)
    for k in range(p["K"]):
        np.testing.assert_array_equal(ctx.get_reg_network_state("Y", k)[0], uc[k])


def test_y_stepped_in_column_chunks_gives_the_same_bits(ctx):
    """The ordering hazard: pmf_fit steps Y one column chunk at a time, and the network term couples columns across chunks,
    so its gradient must come from the whole pre-step Y.  With every data entry missing the data gradient is exactly zero
    whatever the chunking, so 1, 3 and 4 chunks must give the same parameters bit for bit (the loss is the same sum in
    another order).  With a live data term the chunked passes sum in another order: parity tolerance."""
    K, n = 33, 420
    blocks = _graphs(17, K, n)
    Y0 = np.random.default_rng(18).standard_normal((K, n)).astype(np.float32)
    outs = []
    try:
        for chunks in (1, 3, 4):
            _bare(ctx, 64, n, K, Y=Y0)
            ctx.comm_set_chunks(chunks)
            _attach(ctx, "Y", blocks)
            ctx.add_reg_l2("Y", np.full(K, 0.1, np.float32), 1.0)
            ctx.set_optimizer("adagrad", lr=0.05)
            r = ctx.fit(update_Y=True, max_epochs=6, abs_tol=0, rel_tol=0)
            assert ctx.comm_info()["n_chunks"] == chunks
            outs.append((r, ctx.get_factors()[1]))
        for r, Y in outs[1:]:
            np.testing.assert_array_equal(Y, outs[0][1])
            np.testing.assert_allclose(r["loss"], outs[0][0]["loss"], rtol=1e-12)
        assert not np.array_equal(outs[0][1], Y0)
        p = make_problem(**LIVE)
        by, bx = _live_blocks(p)
        live = []
        for chunks in (1, 3, 4):
            ctx.comm_set_chunks(chunks)
            live.append(_live_fit(ctx, p, by, bx))
        for r, (X, Y) in live[1:]:
            np.testing.assert_allclose(r["loss"], live[0][0]["loss"], rtol=5e-6)
            assert rel_err(X, live[0][1][0]) <= 2e-3 and rel_err(Y, live[0][1][1]) <= 2e-3
    finally:
        ctx.comm_set_chunks(0)


def test_interrupted_fit_continues_from_the_read_back_state(ctx):
    """5 epochs, u_k read back with pmf_get_reg_network_state, the regularizer cleared and re-attached with u0, 5 more
    epochs: the same bits as 10 uninterrupted epochs (the warm start is part of the state)."""
    p = make_problem(**LIVE)
    by, bx = _live_blocks(p)
    ctx.comm_set_chunks(0)
    flags = dict(update_Y=True, abs_tol=0, rel_tol=0)
    _attach_live(ctx, p, by, bx, with_x=False)
    ctx.set_optimizer("adagrad", lr=0.05)
    r10 = ctx.fit(max_epochs=10, **flags)
    Y10 = ctx.get_factors()[1]
    _attach_live(ctx, p, by, bx, with_x=False)
    ctx.set_optimizer("adagrad", lr=0.05)
    r5 = ctx.fit(max_epochs=5, **flags)
    u = [ctx.get_reg_network_state("Y", k)[0] for k in range(p["K"])]
    assert any(np.any(x != 0) for x in u)
    ctx.clear_yreg()
    _attach(ctx, "Y", by, p=0.5, u0=u)
    ctx.add_reg_l1("Y", np.full(p["K"], 0.01, np.float32), None, 1.0)
    rb = ctx.fit(max_epochs=10, epoch=6, **flags)
    np.testing.assert_array_equal(np.concatenate([r5["loss"], rb["loss"]]), r10["loss"])
    np.testing.assert_array_equal(ctx.get_factors()[1], Y10)


# ---- two ranks over the host-staged transport -----------------------------------------------------------------------------
def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist
    import pmf_import
    pkg = pmf_import.load()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    p = make_problem(**LIVE)
    by, bx = _live_blocks(p)
    lo, hi = pkg.parallel.shard_rows(p["M"], world, rank)
    ctx = pkg.Context(0)

    def allreduce(arr):
        dist.all_reduce(torch.from_numpy(arr))

    ctx.comm_init_host(rank, world, allreduce)
    q = shard_problem(p, lo, hi)
    flags = dict(update_X=True, update_Y=True, max_epochs=8, abs_tol=0, rel_tol=0)
    # an X network term: refused before any collective (both ranks refuse alike), the communicator stays usable
    to_context(q, ctx)
    _attach(ctx, "X", [tuple(np.ascontiguousarray(m) for m in (b[0][lo:hi, lo:hi], b[1][lo:hi], b[2])) for b in bx])
    ctx.set_optimizer("adagrad", lr=0.05)
    n_coll = ctx.comm_info()["n_collectives"]
    msg = ""
    try:
        ctx.fit(**flags)
    except pkg.PMFError as e:
        msg = str(e)
    refused_clean = ctx.comm_info()["n_collectives"] == n_coll
    # a Y network term: every rank evaluates it on its own
    _attach_live(ctx, q, by, bx, with_x=False, l1=False)
    ctx.set_optimizer("adagrad", lr=0.05)
    h = ctx.fit(**flags)
    X, Y = ctx.get_factors()
    np.savez(Path(outdir) / f"rank{rank}.npz", X=X, Y=Y, loss=h["loss"], msg=msg, refused_clean=refused_clean, lo=lo, hi=hi,
             n_chunks=ctx.comm_info()["n_chunks"])
    ctx.comm_destroy()
    ctx.close()
    dist.destroy_process_group()


def test_two_ranks_y_term_matches_one_rank_and_x_term_is_refused(ctx, tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_netreg as t; "
            "t._worker(int(sys.argv[1]), 2, int(sys.argv[2]), sys.argv[3])") % (str(ROOT), str(ROOT / "tests"))
    procs = [subprocess.Popen([sys.executable, "-c", code, str(r), str(port), str(tmp_path)]) for r in range(2)]
    for pr in procs:
        assert pr.wait(timeout=600) == 0
    outs = [np.load(tmp_path / f"rank{k}.npz") for k in range(2)]
    p = make_problem(**LIVE)
    by, bx = _live_blocks(p)
    assert int(outs[0]["n_chunks"]) == int(outs[1]["n_chunks"])
    ctx.comm_set_chunks(int(outs[0]["n_chunks"]))                 # the same column chunks as the ranks chose
    try:
        _attach_live(ctx, p, by, bx, with_x=False, l1=False)
        ctx.set_optimizer("adagrad", lr=0.05)
        r1 = ctx.fit(update_X=True, update_Y=True, max_epochs=8, abs_tol=0, rel_tol=0)
        X1, Y1 = ctx.get_factors()
    finally:
        ctx.comm_set_chunks(0)
    X = np.concatenate([o["X"] for o in outs], axis=1)
    for o in outs:
        m = str(o["msg"])
        assert "NetworkRegularizer on X" in m and "sharded" in m and "2 ranks" in m, m
        assert "unusable" not in m and bool(o["refused_clean"])
        np.testing.assert_allclose(o["loss"], r1["loss"], rtol=2e-5)
    np.testing.assert_array_equal(outs[0]["loss"], outs[1]["loss"])
    np.testing.assert_array_equal(outs[0]["Y"], outs[1]["Y"])            # the replicated Y stays bit-identical
    assert rel_err(outs[0]["Y"], Y1) <= 2e-4 and rel_err(X, X1) <= 2e-4, (rel_err(outs[0]["Y"], Y1), rel_err(X, X1))


# ---- error paths ---------------------------------------------------------------------------------------------------------
def test_error_paths_return_errors_and_leave_the_context_usable(pkg, ctx):
    import scipy.sparse as sp
    K, n = 2, 6
    blocks = [NR.dense_blocks(list(range(n)), NR.random_graph(np.random.default_rng(k), n, 3, 12)) for k in range(K)]
    Y = np.random.default_rng(5).standard_normal((K, n)).astype(np.float32)
    fresh = pkg.Context(0)
    try:
        fresh.set_data(np.full((3, n), np.nan, np.float32))
        with pytest.raises(pkg.PMFError, match="factors must be set"):
            _attach(fresh, "Y", blocks)
        with pytest.raises(pkg.PMFError, match="factors must be set"):
            fresh.K = K                                  # (the binding's own shape check would stop the call earlier)
            fresh.add_reg_l1("Y", np.ones(K, np.float32))
    finally:
        fresh.close()
    _bare(ctx, 3, n, K, Y=Y)
    with pytest.raises(pkg.PMFError, match="K=2"):
        _attach(ctx, "Y", blocks + blocks[:1])                                        # K differs from the context's
    with pytest.raises(pkg.PMFError, match="expected 6 x 6"):
        _attach(ctx, "Y", [(b[0][:5, :5], b[1][:5], b[2]) for b in blocks])          # AA of the wrong shape
    with pytest.raises(pkg.PMFError, match="AB"):
        _attach(ctx, "Y", [(b[0], b[1][:, :2], b[2]) for b in blocks])               # AB and BB disagree about v_k
    with pytest.raises(pkg.PMFError, match="expected 3 x 3"):
        _attach(ctx, "X", blocks)                                                     # n of X is M = 3
    AA, AB, BB = ([sp.csr_matrix(b[q]) for b in blocks] for q in range(3))

    def raw(AAc, which="Y"):
        """the C entry with hand-made CSR arrays (the Python binding sorts and range-checks by construction)"""
        import ctypes as C
        L = pkg._lib
        keep, arrs = [], []
        for mats in (AAc, [L.csr_arrays(m) for m in AB], [L.csr_arrays(m) for m in BB]):
            a = (L.Csr * K)()
            for k, (shape, rp, col, val) in enumerate(mats):
                keep.append((rp, col, val))
                a[k] = L.Csr(shape[0], shape[1], rp.ctypes.data_as(C.POINTER(C.c_int64)), col.ctypes.data_as(C.POINTER(C.c_int32)),
                             val.ctypes.data_as(C.POINTER(C.c_float)))
            arrs.append(a)
        f = ctx.lib.pmf_add_yreg_network if which == "Y" else ctx.lib.pmf_add_xreg_network
        rc = f(ctx._h, K, arrs[0], arrs[1], arrs[2], None, C.c_float(1.0))
        return rc, ctx.lib.pmf_last_error().decode()
    good = [pkg._lib.csr_arrays(m) for m in AA]
    bad = [tuple(x.copy() if hasattr(x, "copy") else x for x in g) for g in good]
    bad[1][2][0] = n                                                                  # a column index out of range
    rc, msg = raw(bad)
    assert rc < 0 and "out of range" in msg
    bad = [tuple(x.copy() if hasattr(x, "copy") else x for x in g) for g in good]
    row = next(i for i in range(n) if bad[0][1][i + 1] - bad[0][1][i] >= 2)
    e = bad[0][1][row]
    bad[0][2][e], bad[0][2][e + 1] = bad[0][2][e + 1], bad[0][2][e]                   # unsorted row
    rc, msg = raw(bad)
    assert rc < 0 and "not sorted" in msg
    bad = [tuple(x.copy() if hasattr(x, "copy") else x for x in g) for g in good]
    bad[0][1][0] = 1                                                                  # 1-based row pointers
    rc, msg = raw(bad)
    assert rc < 0 and "0-based" in msg
    with pytest.raises(pkg.PMFError, match="no network term"):
        ctx.get_reg_network_state("Y", 0)
    _attach(ctx, "Y", blocks)
    with pytest.raises(pkg.PMFError, match="only one network term"):
        _attach(ctx, "Y", blocks)
    with pytest.raises(pkg.PMFError, match="out of range"):
        ctx.get_reg_network_state("Y", K)
    import ctypes as C
    assert ctx.lib.pmf_get_reg_network_state(ctx._h, 3, 0, None, None) < 0 and "neither X nor Y" in ctx.lib.pmf_last_error().decode()
    with pytest.raises(pkg.PMFError, match="K x n"):
        ctx.add_reg_l1("Y", np.ones(K, np.float32), np.ones((K, n + 1), bool))
    assert C.sizeof(pkg._lib.Csr) == 40
    # the context still works, with the one term that was attached
    val, grad = _value_and_grad(ctx, "Y")
    loss64, g64, _ = NR.exact(blocks, Y.astype(np.float64))
    assert val == pytest.approx(loss64, rel=1e-5) and rel_err(grad, g64) <= 1e-5
    ctx.clear_yreg()                                                                   # drops the term and its state
    with pytest.raises(pkg.PMFError, match="no network term"):
        ctx.get_reg_network_state("Y", 0)
    val, _ = _value_and_grad(ctx, "Y")
    assert val == 0.0


# ---- the public interface, end to end -------------------------------------------------------------------------------------
def test_make_model_with_feature_graphs_fits_end_to_end(pkg):
    """make_model(D, feature_ids, feature_graphs, lambda_Y_graph, lambda_Y_selective_l1) -> K = number of graphs
    (model.jl:121-128), then fit_(fit_reg_weight="EB") runs fit_non_ard_ to the end: finite parameters and loss, and every
    mf_fit_adapt_lr_ stage ends no higher than it began."""
    rng = np.random.default_rng(31)
    M, N, K = 120, 90, 4
    ids = [f"g{j}" for j in range(N)]
    graphs = []
    for k in range(K):
        el = NR.random_graph(rng, N, 12, 80, signed=False, n_used=60)
        graphs.append([[ids[a] if isinstance(a, int) else f"virt{a[1]}", ids[b] if isinstance(b, int) else f"virt{b[1]}", w] for a, b, w in el])
    Xt, Yt = rng.standard_normal((K, M)), rng.standard_normal((K, N))
    D = (Xt.T @ Yt + 0.1 * rng.standard_normal((M, N))).astype(np.float32)
    D[rng.random((M, N)) < 0.05] = np.nan
    views = ["a"] * 50 + ["b"] * 40
    model = pkg.model.make_model(D, feature_ids=ids, feature_views=views, feature_graphs=graphs, lambda_Y_graph=1.0,
                                 lambda_Y_selective_l1=1.0, rng=np.random.default_rng(2))
    R = pkg.regularizers
    assert model.matfac.Y.shape == (K, N)
    net = model.matfac.Y_reg.regularizers[2]
    assert isinstance(model.matfac.Y_reg.regularizers[1], R.SelectiveL1Reg) and isinstance(net, R.NetworkRegularizer)
    hist = pkg.fit_(model, verbosity=0, lr=0.05, max_epochs=150, rel_tol=1e-5, abs_tol=1e-5, fit_reg_weight="EB", keep_history=True)
    mf = model.matfac
    assert np.all(np.isfinite(mf.X)) and np.all(np.isfinite(mf.Y))
    stages = [d for d in hist if str(d.get("name", "")).startswith("mf_fit_lr=")]
    assert len(stages) >= 2
    for d in stages:
        assert np.all(np.isfinite(d["loss"])) and d["loss"][-1] <= d["loss"][0], d.get("name")
    names = [d.get("name") for d in hist]
    assert "reweight_eb" in names and names[-1] == "finish"
    assert any(np.any(x != 0) for x in net.x_virtual)               # the virtual nodes were read back from the device
    assert np.all(np.isfinite(net.cur_weights)) and not np.all(net.cur_weights == 1.0)
    model.release_device()
