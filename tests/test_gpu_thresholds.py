"""Trainable squared-hinge thresholds on the device (include/pmf_hip_thresholds.h) against tests/threshold_ref.py: the
threshold pass (pmf_threshold_grad) per column and per group, the joint epochs of pmf_fit, the thresholds' optimizer state,
the clamp, the refusals, the device-built tables, class counts and the initialisation from them.

The problems are those of tests/hinge_ref.py (layouts A and B, M = 70) with every finite threshold raised by 0.4
(test_threshold_cases.problem: away from the stationary point the data were drawn at), tiled to M = 600 where the grid is capped;
tests/test_threshold_cases.py holds the conditions that make the comparison mean something.  Tolerances: LAYER_TAU times the
scale of threshold_ref for a gradient, step_ref's one-step bounds for the first epoch, FIT_TOL of tests/test_gpu_parity.py after
six; none is new."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import hinge_ref as hr
import step_ref as sr
import threshold_ref as tr
from problems import LAYER_TAU, rel_err, shard_problem
from test_gpu_parity import FIT_TOL
from test_gpu_split_bf16 import bf16_round
from test_threshold_cases import CLAMP_OPT, EPOCHS, OPT, TRAJ_PROBLEMS, big, clamp_problem, problem

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
INF = np.inf
FLAT = dict(abs_tol=0, rel_tol=0)


def worst(got, want, scale):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ok = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~ok), "NaN pattern (columns of the other kinds)"
    if not ok.any():
        return 0.0
    assert np.isfinite(got[ok]).all()
    return float(np.max(np.abs(got - want)[ok] / (LAYER_TAU * scale[ok] + 1e-30)))


def check_grad(ctx, p, tag):
    """pmf_threshold_grad against the reference, per column and per group; a second call is bitwise equal."""
    g, gc = ctx.threshold_grad()
    g2, gc2 = ctx.threshold_grad()
    assert np.array_equal(g, g2) and np.array_equal(gc, gc2, equal_nan=True), "the second pass differs"
    assert ctx.get_threshold_groups() == tr.groups_of(p)
    rc, rg = worst(gc, tr.col_grad(p), tr.col_scale(p)), worst(g, tr.group_grad(p), tr.group_scale(p))
    print(f"THRESH {tag} col_ratio={rc:.3f} group_ratio={rg:.3f}")
    assert rc <= 1.0 and rg <= 1.0, (rc, rg)
    tg = tr.group_thresholds(p)
    assert (g[~np.isfinite(tg)] == 0).all()
    return g, gc


# ---- 1. the threshold pass -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [False, True], ids=["plain", "batch"])
@pytest.mark.parametrize("K", hr.KS)
@pytest.mark.parametrize("name", ["A", "B"])
def test_threshold_gradients_match_the_reference(ctx, name, K, batch):
    p = problem(name, K, batch)
    hr.to_context(p, ctx)
    g, gc = check_grad(ctx, p, f"{name}-k{K}-{'batch' if batch else 'plain'}")
    ctx.set_precision("bf16x3")                          # the pass is exact f32 whatever the precision mode
    try:
        g2, gc2 = ctx.threshold_grad()
    finally:
        ctx.set_precision("f32")
    assert np.array_equal(g, g2) and np.array_equal(gc, gc2, equal_nan=True)
    assert ctx.get_threshold_state()["thr"].tolist() == tr.group_thresholds(p).astype(np.float32).tolist()


# ---- 2. several units per workgroup, more than one row range, both wave counts ------------------------------------------------
@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("name,K", [("A", 48), ("B", 128)])
def test_the_unit_loop_and_the_row_ranges(ctx, monkeypatch, name, K, grid):
    p = big(name, K)
    hr.to_context(p, ctx)
    monkeypatch.setenv("PMF_THRESH_GRID", str(grid))
    n0 = ctx.debug_threshold_pass()["passes"]
    check_grad(ctx, p, f"big-{name}-k{K}-grid{grid}")
    d = ctx.debug_threshold_pass()
    k3 = hr.kinds_of(p) == 3
    n_tiles = len({j // 32 for j in np.flatnonzero(k3)})
    assert d["passes"] == n0 + 2 and d["grid"] == grid and d["n_tiles"] == n_tiles, d
    assert d["n_units"] > d["n_tiles"] and d["n_units"] >= 2 * grid, d      # more than one row range; every workgroup loops


# ---- 3. D stored as bf16 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,K", [("A", 20), ("B", 80)])
def test_bf16_stored_data(ctx, name, K):
    p = dict(problem(name, K, True))
    p["D"] = np.asfortranarray(bf16_round(p["D"]))
    hr.to_context(p, ctx)
    ctx.set_data(p["D"], store="bf16")
    try:
        g, gc = ctx.threshold_grad()
        assert worst(gc, tr.col_grad(p), tr.col_scale(p)) <= 1.0 and worst(g, tr.group_grad(p), tr.group_scale(p)) <= 1.0
        got = ctx.class_counts(p["noise_ranges"])
    finally:
        ctx.set_data(p["D"])
    assert np.array_equal(got, tr.class_counts(p, p["noise_ranges"]))


# ---- 4. a noise model without kind 3 ------------------------------------------------------------------------------------------
def test_no_groups_no_pass_and_the_same_fit(pkg):
    p = dict(problem("A", 20, True))
    p["noise_kinds"] = ["bernoulli", "normal", "normal", "normal", "poisson"]
    p["noise_thr"] = [None] * 5
    outs = []
    for train in (False, True):
        c = pkg.Context(0)
        try:
            hr.to_context(p, c)
            assert c.get_threshold_groups() == []
            g, gc = c.threshold_grad()
            assert g.shape == (0, 3) and np.isnan(gc).all() and c.debug_threshold_pass()["passes"] == 0
            c.set_optimizer("adagrad", lr=0.05)
            h = c.fit(update_X=True, update_Y=True, update_noise_models=train, max_epochs=4, **FLAT)
            outs.append((h["loss"], *c.get_factors()))
            assert c.debug_threshold_pass()["passes"] == 0
        finally:
            c.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


# ---- 5. joint epochs of X, Y and the thresholds ---------------------------------------------------------------------------------
def _fit(c, opt_kw, **kw):
    return c.fit(update_X=True, update_Y=True, update_noise_models=True, **FLAT, **kw)


@pytest.mark.parametrize("opt", ["adagrad", "adam"])
@pytest.mark.parametrize("name,K", TRAJ_PROBLEMS)
def test_six_joint_epochs_follow_the_reference(pkg, name, K, opt):
    p0, kw = problem(name, K, True), OPT[opt]
    c = pkg.Context(0)
    try:
        hr.to_context(p0, c)
        c.set_optimizer(kw["kind"], lr=kw["lr"], eps=kw["eps"], beta1=kw["beta1"], beta2=kw["beta2"])
        h1 = _fit(c, kw, max_epochs=1)
        s1 = c.get_threshold_state()
        # the reference's first epoch, and the one-step bounds of step_ref given the gradient bound of the pass
        st0 = tr.fresh_state(p0, kw)
        p1, st1, info = tr.joint_epoch(p0, st0, kw, 1)
        t0, G, dG = tr.group_thresholds(p0), info["G"], LAYER_TAU * tr.group_scale(p0)
        fin = np.isfinite(t0)
        t1 = tr.group_thresholds(p1)
        sens = sr.step_sensitivity(G, st0["T"][0], st0["T"][1], kw, 1)
        lim_p = sr.p_tol(opt, 1) * (np.abs(t0) + np.abs(t1 - t0)) + sens * dG
        assert (np.abs(s1["thr"] - t1)[fin] <= lim_p[fin]).all(), (s1["thr"], t1, lim_p)
        b2 = 1.0 if opt == "adagrad" else 1.0 - kw["beta2"]
        lim_a = sr.ACC_TOL * (G * G + np.abs(st0["T"][0])) + b2 * (2 * np.abs(G) + dG) * dG
        assert (np.abs(s1["acc"] - st1["T"][0])[fin] <= lim_a[fin]).all(), (s1["acc"], st1["T"][0])
        lim_m = sr.MOM_TOL * np.abs(G) + (1.0 - kw["beta1"]) * dG
        assert (np.abs(s1["mom"] - st1["T"][1])[fin] <= lim_m[fin]).all(), (s1["mom"], st1["T"][1])
        assert np.array_equal(s1["thr"][~fin], t0[~fin].astype(np.float32))
        assert (s1["mom"][~fin] == 0).all() and (s1["acc"][~fin] == (np.float32(kw["eps"]) if opt == "adagrad" else 0)).all()
        assert abs(h1["loss"][0] - info["loss"]) <= 5e-5 * abs(info["loss"])
        # five more
        h = _fit(c, kw, max_epochs=EPOCHS, epoch=2)
        losses, p, st = [info["loss"]], p1, st1
        for t in range(2, EPOCHS + 1):
            p, st, info = tr.joint_epoch(p, st, kw, t)
            losses.append(info["loss"])
        np.testing.assert_allclose(np.concatenate([h1["loss"], h["loss"]]), losses, rtol=5e-5)
        X, Y = c.get_factors()
        s6 = c.get_threshold_state()
        t6 = tr.group_thresholds(p)
        print(f"THRESH traj-{name}-k{K}-{opt} X={rel_err(X, p['X']):.2e} Y={rel_err(Y, p['Y']):.2e} "
              f"thr={rel_err(s6['thr'][fin], t6[fin]):.2e} acc={rel_err(s6['acc'][fin], st['T'][0][fin]):.2e}")
        assert rel_err(X, p["X"]) <= FIT_TOL and rel_err(Y, p["Y"]) <= FIT_TOL
        assert rel_err(s6["thr"][fin], t6[fin]) <= FIT_TOL
        assert rel_err(s6["acc"][fin], st["T"][0][fin]) <= FIT_TOL and rel_err(s6["mom"][fin], st["T"][1][fin]) <= FIT_TOL + (opt == "adagrad")
        # the host copy follows: what the getter reports is the trained triple on every column of its group
        thr = c.get_noise_thresholds()
        for r, (s, e) in enumerate(tr.groups_of(p0)):
            assert (thr[s - 1:e] == s6["thr"][r]).all()
    finally:
        c.close()


# ---- 6. / 7. state, and infinite thresholds ---------------------------------------------------------------------------------------
def test_state_survives_a_remarshal_and_resets_with_the_optimizer(pkg):
    p, kw = problem("B", 20, True), OPT["adagrad"]
    c = pkg.Context(0)
    try:
        hr.to_context(p, c)
        c.set_optimizer("adagrad", lr=kw["lr"])
        s0 = c.get_threshold_state()
        assert (s0["acc"] == np.float32(1e-8)).all() and (s0["mom"] == 0).all()
        _fit(c, kw, max_epochs=2)
        s2 = c.get_threshold_state()
        fin = np.isfinite(s2["thr"])
        assert (s2["acc"][fin] > 1e-8).all() and (s2["acc"][~fin] == np.float32(1e-8)).all()
        assert np.array_equal(np.isfinite(s2["thr"]), np.isfinite(tr.group_thresholds(p)))       # infinite ones come back infinite
        # the mf_fit_adapt_lr_ pattern: the model is marshalled again with the trained triples, the rate halved
        trained = [tuple(t) for t in s2["thr"]]
        c.set_noise(p["noise_ranges"], p["noise_kinds"], p["col_weight"])
        c.set_noise_thresholds(tr.groups_of(p), trained)
        c.set_lr(kw["lr"] / 2)
        s3 = c.get_threshold_state()
        assert np.array_equal(s3["acc"], s2["acc"]) and np.array_equal(s3["thr"], s2["thr"])
        _fit(c, kw, max_epochs=3, epoch=3)
        s4 = c.get_threshold_state()
        assert (s4["acc"][fin] > s2["acc"][fin]).all()
        c.reset_optimizer_state()
        _fit(c, kw, max_epochs=1)
        s5 = c.get_threshold_state()
        assert (s5["acc"][fin] < s4["acc"][fin]).all()           # one squared gradient on top of eps, not five
        # other groups: the state starts over
        c.set_noise([(1, 50), (51, 77)], [3, 3], p["col_weight"])
        s6 = c.get_threshold_state()
        assert s6["acc"].shape == (2, 3) and (s6["acc"] == np.float32(1e-8)).all()
    finally:
        c.close()


# ---- 8. the clamp -------------------------------------------------------------------------------------------------------------------
def test_crossing_thresholds_are_clamped(pkg):
    p = clamp_problem()
    c = pkg.Context(0)
    try:
        hr.to_context(p, c)
        c.set_optimizer("adagrad", lr=CLAMP_OPT["lr"])
        c.fit(update_noise_models=True, max_epochs=1, **FLAT)           # thresholds alone
        _, _, info = tr.joint_epoch(p, tr.fresh_state(p, CLAMP_OPT), CLAMP_OPT, 1, train_xy=False)
        s = c.get_threshold_state()["thr"]
        assert info["raw"][0][2] < info["raw"][0][1]
        assert s[0][1] == s[0][2] and abs(s[0][1] - info["raw"][0][1]) <= 1e-5 * CLAMP_OPT["lr"], (s, info["raw"])
        t = c.get_noise_thresholds()
        assert (t[:, 0] <= t[:, 1]).all() and (t[:, 1] <= t[:, 2]).all()
        c.loss()                                                          # the rebuilt tables serve the next pass
    finally:
        c.close()


# ---- 9. a group with different triples ------------------------------------------------------------------------------------------
def test_non_uniform_triples_are_refused(pkg):
    p = problem("B", 20, True)
    c = pkg.Context(0)
    try:
        hr.to_context(p, c)
        c.set_noise_thresholds([(10, 12)], [(-INF, -0.4, 0.6)])
        c.set_optimizer("adagrad", lr=0.05)
        X0, Y0 = c.get_factors()
        with pytest.raises(pkg.PMFError, match="1:40"):
            _fit(c, OPT["adagrad"], max_epochs=2)
        X1, Y1 = c.get_factors()
        assert np.array_equal(X0, X1) and np.array_equal(Y0, Y1)
        h = c.fit(update_X=True, update_Y=True, max_epochs=2, **FLAT)     # with training off the same context fits
        assert np.isfinite(h["loss"]).all()
        c.set_noise_thresholds([(1, 40)], [(-INF, -0.5, 0.5)])
        _fit(c, OPT["adagrad"], max_epochs=2)
    finally:
        c.close()


# ---- 10. the device-built tables are the host's ------------------------------------------------------------------------------------
def test_device_tables_equal_host_tables(pkg):
    p = problem("A", 48, True)
    c, d = pkg.Context(0), pkg.Context(0)
    try:
        hr.to_context(p, c)
        c.set_optimizer("adagrad", lr=0.05)
        c.fit(update_noise_models=True, max_epochs=3, **FLAT)             # thresholds alone: X and Y stay
        trained = c.get_threshold_state()["thr"]
        assert not np.array_equal(trained, tr.group_thresholds(p).astype(np.float32))
        hr.to_context(p, d)
        d.set_noise_thresholds(tr.groups_of(p), [tuple(t) for t in trained])
        assert np.array_equal(c.get_noise_thresholds(), d.get_noise_thresholds(), equal_nan=True)
        assert c.loss() == d.loss()
        gc, gd = c.threshold_grad(), d.threshold_grad()
        assert np.array_equal(gc[0], gd[0]) and np.array_equal(gc[1], gd[1], equal_nan=True)
    finally:
        c.close()
        d.close()
    dev, pinned = pkg._lib.live_bytes()
    c = pkg.Context(0)
    hr.to_context(p, c)
    c.threshold_grad()
    c.close()
    assert pkg._lib.live_bytes() == (dev, pinned)


# ---- 11. class counts and the initialisation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [70, 600])
def test_class_counts_are_exact(ctx, M):
    p = dict(problem("A", 20, True) if M == 70 else big("A", 48, M))
    D = np.array(p["D"])
    D[3, 110:165] = 0.0                                   # class-0 entries in the ordinal columns
    D[5, 20:40] = 7.0                                     # clamped to class 3
    p["D"] = np.asfortranarray(D)
    hr.to_context(p, ctx)
    ranges = list(p["noise_ranges"]) + [(1, p["N"]), (30, 130), (64, 64)]
    got = ctx.class_counts(ranges)
    assert got.dtype == np.int64 and np.array_equal(got, tr.class_counts(p, ranges))
    assert got[:, 0].sum() > 0 and got[3, 0] > 0
    assert got[5].sum() == np.isfinite(D).sum()


def test_basic_fit_initialises_the_ordinal_thresholds(pkg):
    rng = np.random.default_rng(5)
    M, N = 90, 60
    dists = ["normal"] * 20 + ["ordinal_sq_hinge3"] * 30 + ["bernoulli_sq_hinge"] * 10
    D = rng.standard_normal((M, N)).astype(np.float32)
    D[:, 20:50] = rng.choice([1.0, 2.0, 3.0], size=(M, 30), p=[0.55, 0.3, 0.15])
    D[:, 50:] = rng.integers(0, 2, (M, 10))
    D[rng.random((M, N)) < 0.1] = np.nan
    model = pkg.make_model(D, K=4, feature_distributions=dists, feature_views=[1] * N, feature_ids=[f"f{j}" for j in range(N)],
                           rng=np.random.default_rng(1))
    nm = model.matfac.noise_model
    r = nm.noises.index("ordinal_sq_hinge3")
    cr = nm.col_ranges[r]
    cols = np.asarray(model.data)[:, cr.start - 1:cr.stop]
    counts = [int((cols == k).sum()) for k in range(4)]
    before = list(nm.thresholds)
    try:
        pkg.basic_fit_(model, init_ordinal=True, verbosity=0)
    finally:
        model.release_device()
    want = tr.init_thresholds(counts, (-INF, -0.5, 0.5))
    assert np.array_equal(np.asarray(nm.thresholds[r], np.float32), want), (nm.thresholds[r], want)
    assert want[1] < want[2] and tuple(want[1:]) != (-0.5, 0.5)
    assert [t for k, t in enumerate(nm.thresholds) if k != r] == [t for k, t in enumerate(before) if k != r]


# ---- 12. two ranks over the host transport -----------------------------------------------------------------------------------------
SHARD = ("B", 80)


def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist
    import pmf_import
    pkg = pmf_import.load()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    p = problem(*SHARD, True)
    lo, hi = pkg.parallel.shard_rows(p["M"], world, rank)
    c = pkg.Context(0)

    def allreduce(arr):
        dist.all_reduce(torch.from_numpy(arr))

    c.comm_init_host(rank, world, allreduce)
    c.comm_set_chunks(2)
    hr.to_context(shard_problem(p, lo, hi), c)
    kw = OPT["adagrad"]
    c.set_optimizer("adagrad", lr=kw["lr"])
    n0 = c.comm_info()["n_collectives"]
    h = _fit(c, kw, max_epochs=EPOCHS)
    s = c.get_threshold_state()
    X, Y = c.get_factors()
    np.savez(Path(outdir) / f"rank{rank}.npz", X=X, Y=Y, loss=h["loss"], n_coll=c.comm_info()["n_collectives"] - n0, **s)
    c.comm_destroy()
    c.close()
    dist.destroy_process_group()


def test_two_ranks_train_the_same_thresholds(pkg, tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_thresholds as t; "
            "t._worker(int(sys.argv[1]), 2, int(sys.argv[2]), sys.argv[3])") % (str(ROOT), str(ROOT / "tests"))
    procs = [subprocess.Popen([sys.executable, "-c", code, str(r), str(port), str(tmp_path)]) for r in range(2)]
    for pr in procs:
        assert pr.wait(timeout=600) == 0
    outs = [np.load(tmp_path / f"rank{k}.npz") for k in range(2)]
    for k in ("thr", "acc", "mom", "Y", "loss"):
        assert np.array_equal(outs[0][k], outs[1][k]), k
    # per epoch: two grad(Y) chunks, the loss, and the thresholds' group sums
    assert int(outs[0]["n_coll"]) >= 4 * EPOCHS
    p, kw = problem(*SHARD, True), OPT["adagrad"]
    c = pkg.Context(0)
    try:
        hr.to_context(p, c)
        c.set_optimizer("adagrad", lr=kw["lr"])
        h = _fit(c, kw, max_epochs=EPOCHS)
        s = c.get_threshold_state()
    finally:
        c.close()
    fin = np.isfinite(s["thr"])
    np.testing.assert_allclose(outs[0]["loss"], h["loss"], rtol=2e-5)
    assert rel_err(outs[0]["thr"][fin], s["thr"][fin]) <= FIT_TOL and rel_err(outs[0]["acc"][fin], s["acc"][fin]) <= FIT_TOL


# ---- 13. fit_ end to end ---------------------------------------------------------------------------------------------------------------
def _assay_model(pkg, train):
    rng = np.random.default_rng(11)
    M, N = 120, 96
    dists = ["bernoulli_sq_hinge"] * 32 + ["ordinal_sq_hinge3"] * 32 + ["normal"] * 32       # mutation, cna, mrnaseq
    Z = rng.standard_normal((M, 5)) @ rng.standard_normal((5, N))
    D = Z.astype(np.float32)
    D[:, :32] = (Z[:, :32] > 0.8)
    D[:, 32:64] = 1 + (Z[:, 32:64] > -1.0) + (Z[:, 32:64] > 1.5)
    D[rng.random((M, N)) < 0.05] = np.nan
    model = pkg.make_model(D, K=5, feature_distributions=dists, feature_views=[1] * 32 + [2] * 32 + [3] * 32,
                           feature_ids=[f"f{j}" for j in range(N)], rng=np.random.default_rng(2))
    model.matfac.noise_model.train_thresholds_(train)
    return model


def test_fit_end_to_end_trains_the_thresholds_only_when_asked(pkg):
    res = {}
    for train in (False, True):
        model = _assay_model(pkg, train)
        t0 = list(model.matfac.noise_model.thresholds)
        try:
            pkg.fit_(model, lr=0.05, max_epochs=30, verbosity=0)
        finally:
            model.release_device()
        res[train] = (t0, list(model.matfac.noise_model.thresholds))
    t0, t1 = res[False]
    assert t0 == t1                                                       # today's thresholds, exactly
    t0, t1 = res[True]
    for a, b in zip(t0, t1):
        if a is None:
            assert b is None
            continue
        a, b = np.asarray(a), np.asarray(b)
        fin = np.isfinite(a)
        assert np.array_equal(np.isfinite(b), fin) and np.array_equal(a[~fin], b[~fin])
        assert (b[fin] != a[fin]).all() and (b[:-1] <= b[1:]).all(), (a, b)
