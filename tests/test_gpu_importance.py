"""pmf_factor_importance (include/pmf_hip_importance.h) on the device against tests/importance_ref.py,
element by element within that file's rounding bound: the geometry and model-mix cases of its table (whose bound
tests/test_importance_cases.py holds meaningful), both storage types of D, exact zeros and empty cases, consistency with
pmf_loss and pmf_fit, the two refusals, and row shards.  Long sweeps and unit / grid edges: tests/test_gpu_importance_edges.py."""
import copy
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import hinge_ref as hr
import importance_ref as ir
from test_gpu_split_bf16 import bf16_round

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FLAT = dict(abs_tol=0, rel_tol=0)


def run(ctx, p, **kw):
    hr.to_context(p, ctx)
    return dict(zip(("delta", "full", "null", "n_obs"), ctx.factor_importance(**kw)))


def changed(p, **kw):
    """A private copy of a shared problem with some arrays replaced."""
    q = copy.copy(p)
    q.update(kw)
    return q


# ---- geometry and model mix ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ir.cases()))
def test_the_table_matches_the_reference(ctx, name):
    p = ir.cases()[name]
    got = run(ctx, p)
    ir.check(got, p)
    d = ctx.debug_factor_importance()
    KB = (p["K"] + 31) // 32
    assert (d["kb"], d["nw"], d["db"]) == (KB, 8 if KB <= 2 else 4, 0), d
    assert d["n_units"] == -(-p["N"] // 32) * d["ranges"] and d["launches"] == 1, d
    assert got["delta"].shape == (p["K"], p["N"]) and got["n_obs"].dtype == np.int64


# ---- storage -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mix-70x100-k40", "hinge-A-k128-batch", "mix-45x37-k65"])
def test_bf16_stored_data(ctx, name):
    p = ir.cases()[name]
    q = changed(p, D=np.asfortranarray(bf16_round(p["D"])))
    hr.to_context(q, ctx)
    ctx.set_data(q["D"], store="bf16")
    try:
        got = dict(zip(("delta", "full", "null", "n_obs"), ctx.factor_importance()))
        assert ctx.debug_factor_importance()["db"] == 1
    finally:
        ctx.set_data(q["D"])
    ref = ir.reference(q)
    ir.check(got, q, ref=(ref, ir.bounds(ref)))
    f32 = dict(zip(("delta", "full", "null", "n_obs"), ctx.factor_importance()))     # the same values stored as f32: the same bits
    for k in f32:
        assert np.array_equal(f32[k], got[k]), k


# ---- exact zeros and empty cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mix-70x100-k40", "hinge-A-k20-batch", "mix-45x37-k65"])
def test_a_zero_row_of_a_factor_is_exactly_absent(ctx, name):
    p = ir.cases()[name]
    K = p["K"]
    kx, ky = 1 % K, (K - 1)
    X, Y = np.array(p["X"], order="F"), np.array(p["Y"], order="F")
    X[kx] = 0
    Y[ky] = 0
    q = changed(p, X=X, Y=Y)
    got = run(ctx, q)
    for k in {kx, ky}:
        assert (got["delta"][k] == 0.0).all() and not np.signbit(got["delta"][k]).any(), k
    ref = ir.reference(q)
    ir.check(got, q, ref=(ref, ir.bounds(ref)))
    assert (got["delta"][[k for k in range(K) if k not in (kx, ky)]] != 0).any()


def test_empty_columns_missing_rows_and_zero_weights(ctx):
    p = ir.cases()["hinge-A-k20-batch"]
    base = run(ctx, p)
    # a column with no observed entry, a column of weight 0
    D = np.array(p["D"], order="F")
    D[:, 3] = np.nan
    D[:, 40] = np.nan
    w = np.array(p["col_weight"])
    w[[7, 100]] = 0
    q = changed(p, D=D, col_weight=w)
    got = run(ctx, q)
    ref = ir.reference(q)
    ir.check(got, q, ref=(ref, ir.bounds(ref)))
    for j in (3, 40, 7, 100):
        assert (got["delta"][:, j] == 0.0).all() and got["full"][j] == 0.0 and got["null"][j] == 0.0 and got["n_obs"][j] == 0, j
    keep = np.setdiff1d(np.arange(p["N"]), [3, 40, 7, 100])
    for k in base:
        assert np.array_equal(got[k][..., keep], base[k][..., keep]), k            # the other columns: the same bits
    # a fully missing last row changes nothing: the same bits as the matrix without it
    M = p["M"]
    D = np.array(p["D"], order="F")
    D[M - 1] = np.nan
    a = run(ctx, changed(p, D=D))
    short = changed(p, M=M - 1, D=np.asfortranarray(p["D"][:M - 1]), X=np.asfortranarray(p["X"][:, :M - 1]),
                    batch_views=[dict(v, batch_of_row=np.ascontiguousarray(v["batch_of_row"][:M - 1])) for v in p["batch_views"]])
    b = run(ctx, short)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_one_factor_explains_what_the_null_model_lacks(ctx):
    p = ir.cases()["mix-45x37-k1"]
    got = run(ctx, p)
    _, b = ir.reference_of(p)
    assert (np.abs(got["delta"][0] - (got["null"] - got["full"])) <= b["delta"][0] + b["null"] + b["full"]).all()


# ---- consistency on the device -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mix-70x100-k40", "hinge-A-k128-batch"])
def test_full_sums_to_the_data_loss_and_calls_repeat_bitwise(ctx, name):
    p = ir.cases()[name]
    a = run(ctx, p)
    _, b = ir.reference_of(p)
    assert abs(a["full"].sum() - ctx.loss()["data"]) <= b["full"].sum()        # the summed bound
    c = dict(zip(("delta", "full", "null", "n_obs"), ctx.factor_importance()))
    for k in a:
        assert np.array_equal(a[k], c[k]), k
    # partial outputs: NULL pointers for the others, the same bits
    only = ctx.factor_importance(delta=False, null=False, n_obs=False)
    assert only[0] is None and only[2] is None and only[3] is None and np.array_equal(only[1], a["full"])
    only = ctx.factor_importance(full=False)
    assert only[1] is None and np.array_equal(only[0], a["delta"]) and np.array_equal(only[3], a["n_obs"])
    none = ctx.factor_importance(False, False, False, False)
    assert none == (None, None, None, None)


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
def test_a_call_between_two_fit_segments_leaves_the_trace_alone(pkg, opt):
    p = ir.cases()["hinge-A-k20-batch"]
    traces = []
    for call in (False, True):
        c = pkg.Context(0)
        try:
            hr.to_context(p, c)
            c.set_optimizer(opt, lr=0.02)
            h1 = c.fit(update_X=True, update_Y=True, update_col_layers=True, max_epochs=3, **FLAT)
            if call:
                out = c.factor_importance()
                assert np.isfinite(out[0]).all()
            h2 = c.fit(update_X=True, update_Y=True, update_col_layers=True, max_epochs=6, epoch=4, **FLAT)
            X, Y = c.get_factors()
            traces.append((np.concatenate([h1["loss"], h2["loss"]]), X, Y, *c.get_col_params()))
        finally:
            c.close()
    for a, b in zip(*traces):
        assert np.array_equal(a, b)
    assert len(traces[0][0]) == 6


# ---- errors ------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg):
    p = ir.cases()["mix-45x37-k2"]
    c = pkg.Context(0)
    try:
        with pytest.raises(pkg.PMFError, match="data not set"):
            c.factor_importance()
        c.set_data(p["D"])
        with pytest.raises(pkg.PMFError, match="factors not set"):
            c.factor_importance()
        got = run(c, p)                                    # the context is usable afterwards
        ir.check(got, p)
    finally:
        c.close()


# ---- row shards ----------------------------------------------------------------------------------------------------------------------
M, N, K, CUT = 70, 96, 6, 40


def _model(pkg, lo=None, hi=None):
    """70 x 96: view 1 = 20 Bernoulli + 28 normal columns, view 2 = 48 normal columns, 5 % missing, three row batches per view;
    every rank draws the parameters of the WHOLE model in one order and keeps its columns of X."""
    rng = np.random.default_rng(17)
    batches = {1: ["p"] * 25 + ["q"] * 25 + ["r"] * 20, 2: ["u"] * 30 + ["v"] * 22 + ["w"] * 18}
    Z = rng.standard_normal((M, K)) @ rng.standard_normal((K, N)) * 0.5
    D = (Z + 0.3 * rng.standard_normal((M, N))).astype(np.float32)
    D[:, :20] = Z[:, :20] > 0
    D[rng.random((M, N)) < 0.05] = np.nan
    kw = dict(K=K, sample_conditions=["c1"] * 30 + ["c2"] * 40, feature_views=[1] * 48 + [2] * 48, feature_ids=[f"x_{j}" for j in range(N)],
              feature_distributions=["bernoulli"] * 20 + ["normal"] * 76, batch_dict=batches)
    if lo is None:
        lo, hi = 0, M
        model = pkg.make_model(D, rng=np.random.default_rng(3), **kw)
    else:
        model = pkg.make_model(D[lo:hi], rng=np.random.default_rng(3), row_shard=(lo, hi, M), **kw)
    mf, ct = model.matfac, model.matfac.col_transform
    mf.X[...] = (0.4 * rng.standard_normal((K, M)))[:, lo:hi]
    mf.Y[...] = 0.4 * rng.standard_normal((K, N))
    ct.unwrapped(3).mu[...] = 0.3 * rng.standard_normal(N)
    ct.unwrapped(1).logsigma[...] = 0.2 * rng.standard_normal(N)
    for v in ct.unwrapped(4).theta.values:
        v[...] = 0.5 * rng.standard_normal(v.shape)
    for v in ct.unwrapped(2).logdelta.values:
        v[...] = 0.1 * rng.standard_normal(v.shape)
    mf.noise_model.set_weight_((0.5 + rng.random(N)).astype(np.float32))
    return model


def _problem_of(pkg, model):
    """The whole model as a problem of tests/importance_ref.py."""
    mf = model.matfac
    ct, nm = mf.col_transform, mf.noise_model
    views, _, _ = pkg.matfac._batch_views(ct)
    return dict(M=model.data.shape[0], N=mf.Y.shape[1], K=mf.X.shape[0], D=np.asfortranarray(model.data), X=np.asfortranarray(mf.X),
                Y=np.asfortranarray(mf.Y), logsigma=np.array(ct.unwrapped(1).logsigma), mu=np.array(ct.unwrapped(3).mu),
                batch_views=[dict(v, batch_of_row=np.asarray(v["batch_of_row"], np.int32), logdelta=np.array(v["logdelta"], np.float32),
                                  theta=np.array(v["theta"], np.float32)) for v in views],
                noise_ranges=[(r.start, r.stop) for r in nm.col_ranges], noise_kinds=list(nm.noises), noise_thr=list(nm.thresholds),
                col_weight=np.array(nm.weights, np.float32))


def _whole(pkg):
    model = _model(pkg)
    p = _problem_of(pkg, model)
    ref = ir.reference(p)
    return model, p, (ref, ir.bounds(ref))


def test_two_local_shards_add_up_to_the_whole_matrix(pkg):
    whole, p, ref = _whole(pkg)
    parts = []
    try:
        ir.check(pkg.factor_importance(whole), p, ref=ref)
        views = pkg.explained_deviance(whole)
        assert views["views"] == [1, 2] and views["factor"].shape == (K, 2) and np.isfinite(views["total"]).all()
        for rank, (lo, hi) in enumerate(((0, CUT), (CUT, M))):
            m = _model(pkg, lo, hi)
            m.attach_comm(rank, 2, host_allreduce=lambda arr: None)           # (never called: reduce=False)
            try:
                ctx = m.device_context()
                uploads = m._ctx_data_id
                parts.append(pkg.factor_importance(m, reduce=False))
                parts.append(pkg.factor_importance(m, reduce=False))              # the live context, the resident data
                assert m.device_context() is ctx and m._ctx_data_id == uploads
            finally:
                m.release_device()
    finally:
        whole.release_device()
    for a, b in ((0, 1), (2, 3)):
        for x, y in zip(parts[a], parts[b]):
            assert np.array_equal(x, y)
    total = dict(zip(("delta", "full", "null", "n_obs"), (x + y for x, y in zip(parts[0], parts[2]))))
    ir.check(total, p, ref=ref)
    assert parts[0].n_obs.sum() < total["n_obs"].sum()


def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist
    import pmf_import
    pkg = pmf_import.load()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []

    def allreduce(arr):
        calls.append(arr.size)
        dist.all_reduce(torch.from_numpy(arr))

    lo, hi = ((0, CUT), (CUT, M))[rank]
    model = _model(pkg, lo, hi)
    model.attach_comm(rank, world, host_allreduce=allreduce)
    n0, c0 = model.device_context().comm_info()["n_collectives"], len(calls)
    imp = pkg.factor_importance(model)
    n1, sizes = model.device_context().comm_info()["n_collectives"], list(calls[c0:])
    local = pkg.factor_importance(model, reduce=False)
    np.savez(Path(outdir) / f"imp{rank}.npz", delta=imp.delta, full=imp.full, null=imp.null, n_obs=imp.n_obs, local_full=local.full,
             collectives=np.array(n1 - n0), calls=np.array(sizes, np.int64), calls_after=np.array(len(calls) - c0))
    model.release_device()
    dist.destroy_process_group()


def test_two_ranks_reduce_to_the_whole_matrix(pkg, tmp_path):
    """Two rank processes on real HIP contexts sharing the one GPU, the host-staged transport (as tests/test_gpu_shard_fit.py)."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_importance as t; "
            "t._worker(int(sys.argv[1]), 2, int(sys.argv[2]), sys.argv[3])") % (str(ROOT), str(ROOT / "tests"))
    procs = [subprocess.Popen([sys.executable, "-c", code, str(r), str(port), str(tmp_path)]) for r in range(2)]
    try:
        for pr in procs:
            assert pr.wait(timeout=240) == 0
    finally:
        for pr in procs:      # (a rank left waiting in a collective must not outlive the test)
            if pr.poll() is None:
                pr.kill()
    a, b = (np.load(tmp_path / f"imp{k}.npz") for k in range(2))
    whole, p, ref = _whole(pkg)
    for k in ("delta", "full", "null", "n_obs"):
        assert np.array_equal(a[k], b[k]), k                                   # every rank leaves with the same arrays
    ir.check({k: a[k] for k in ("delta", "full", "null", "n_obs")}, p, ref=ref)
    assert a["n_obs"].dtype == np.int64
    assert int(a["collectives"]) == int(b["collectives"]) == 1                  # ONE all-reduce, all four arrays in it
    for r in (a, b):                                                           # ... as the host's reducer saw it; none with reduce=False
        assert r["calls"].tolist() == [K * N + 3 * N] and int(r["calls_after"]) == 1, (r["calls"], r["calls_after"])
    assert not np.array_equal(a["local_full"], b["local_full"])
    assert np.allclose(a["local_full"] + b["local_full"], a["full"], rtol=1e-12, atol=0)
