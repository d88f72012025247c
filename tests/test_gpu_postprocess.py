"""The factor post-processing stages run inside the library (pmf_gram, pmf_stage_lambda_max, pmf_stage_whiten,
pmf_stage_rotate_by_svd, pmf_stage_reorder_by_importance; csrc/pmf_postprocess.hip; postprocess="library" in fit.py) against
oracle/postprocess_oracle.py (float64, the Gram / eigen route) applied to the same float32 inputs that were uploaded.

Shapes and bounds: tests/postprocess_cases.py -- (a) for Gram entries, (b) for every stored float32.
Further bounds used below, each derived where it is used:
  host path       pmf_stage_whiten stores where the host stores (Y is rounded after Y * x_rms and again after / c); x_rms
                  agrees with numpy's to ~1e-15 and c, which the host takes from the rounded Y, to 2^-24: each can move one of
                  the two roundings by one ulp, <= 2^-22 relative, held to 2^-21.
  X'Y invariant   each of the K terms X'_ki Y'_kj carries one float32 rounding per factor: 2^-23 sum_k |X'_ki Y'_kj|
                  (+ (b)'s absolute term).  This DEPARTS from the issue's wording, "(b)'s relative term" = 2^-23 |X'Y|_ij: that
                  is what each stored factor meets, but a sum of K rounded products cannot meet it where the products
                  cancel (|X'Y|_ij far below sum_k |X'_ki Y'_kj|), so the relative term is applied per product, not to the sum.
  Y Y' diagonal   each stored Y' element is off by 2^-24 |y|: an off-diagonal dot product by <= 2^-23 ||row a|| ||row b||."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import ctypes as C
import numpy as np
import pytest

from oracle import postprocess_oracle as PO
from postprocess_cases import GRAM_CHUNK, SHAPES, VIEWS, check_gram, make_factors, stored_deviation
from problems import rel_err
from test_gpu_shard_fit import FIT_KW, K as SK, M as SM, N as SN, _fit_outputs, _make, _seed_state

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SHAPE_IDS = [f"K{k}_M{m}_N{n}" for k, m, n in SHAPES]


def _upload(ctx, f, X=None, Y=None, logsigma=None):
    """The case's data and parameters on a raw context (float32 in, exactly what the oracle gets)."""
    ctx.set_data(f["D"])
    ctx.set_factors(f["X"] if X is None else X, f["Y"] if Y is None else Y)
    ctx.set_col_params(f["logsigma"] if logsigma is None else logsigma, f["mu"])
    ctx.set_batch_views([])
    ctx.set_noise([(1, f["D"].shape[1])], ["normal"])
    ctx.clear_xreg()
    ctx.clear_yreg()
    ctx.set_layer_regs()


@pytest.fixture(scope="module")
def pctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


# ---- 1. pmf_gram ---------------------------------------------------------------------------------------------------------
def _gram_groups(n):
    """several groups with a gap, a one-column group and (where the matrix is wide enough) one that straddles a chunk seam"""
    if n >= GRAM_CHUNK + 10:
        return [(1, 1), (3, 700), (GRAM_CHUNK - 5, GRAM_CHUNK + 7), (GRAM_CHUNK + 9, n)]
    if n >= 8:
        return [(1, 1), (3, n // 2), (n // 2 + 2, n)]
    return [(1, 1), (3, n)]


@pytest.mark.parametrize("K,M,N", SHAPES, ids=SHAPE_IDS)
def test_gram_matches_numpy(pctx, K, M, N):
    f = make_factors(K, M, N)
    _upload(pctx, f)
    worst = 0.0
    for which, P, n in ((0, f["X"], M), (1, f["Y"], N)):
        for ranges in ([(1, n)], _gram_groups(n)):
            G = pctx.gram(which, ranges)
            assert G.shape == (len(ranges), K, K)
            worst = max(worst, check_gram(G, P, ranges, (which, ranges)))
            np.testing.assert_array_equal(G, np.transpose(G, (0, 2, 1)))             # symmetric bit for bit
            d = pctx.gram(which, ranges, diag_only=True)
            np.testing.assert_array_equal(d, np.einsum("gkk->gk", G))                # the diagonal mode: the same bits
            np.testing.assert_array_equal(G, pctx.gram(which, ranges))               # two calls: the same bits
    # a group without columns (a row-sharded group with no local rows) gives zeros and leaves its neighbours alone
    G = pctx.gram(0, [(1, 2), (3, 2), (3, M)])
    assert not G[1].any() and G[0].any() and G[2].any()
    print(f"PP_GRAM K={K} M={M} N={N} worst error / bound (a) = {worst:.3e}")
    # "Pad rows are not read" is by construction and not observable here: no call of the C ABI can make rows K..Kp-1 anything
    # but zero (every upload pads with zeros, every kernel that stores whole columns writes zeros there), and the kernels
    # index rows < K only (k_pp_gram stages `k < K ? P[...] : 0`, k_pp_diag returns for k >= K).  K = 33 runs with Kp = 64.
    # nothing was written
    X, Y = pctx.get_factors()
    np.testing.assert_array_equal(X, f["X"])
    np.testing.assert_array_equal(Y, f["Y"])


# ---- 3. the three stages against the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K,M,N", SHAPES, ids=SHAPE_IDS)
def test_whiten_matches_the_oracle(pctx, K, M, N):
    f = make_factors(K, M, N)
    _upload(pctx, f)
    xr, c = pctx.stage_whiten(M, VIEWS[N])
    X, Y = pctx.get_factors()
    ls = pctx.get_col_params()[0]
    Xr, Yr, lsr = PO.whiten(f["X"], f["Y"], f["logsigma"], VIEWS[N])
    dev = dict(X=stored_deviation(X, Xr), Y=stored_deviation(Y, Yr), logsigma=stored_deviation(ls, lsr))
    print(f"PP_WHITEN K={K} M={M} N={N} deviation / bound (b): " + " ".join(f"{k}={v:.3e}" for k, v in dev.items()))
    assert max(dev.values()) <= 1.0, dev
    np.testing.assert_allclose(xr, PO.rms_rows(f["X"].astype(np.float64)), rtol=1e-13)
    assert c.shape == (len(VIEWS[N]),) and np.all(c > 0)
    np.testing.assert_array_equal(pctx.get_col_params()[1], f["mu"])                 # mu is not touched


@pytest.mark.parametrize("K,M,N", SHAPES, ids=SHAPE_IDS)
def test_rotate_by_svd_matches_the_oracle(pctx, K, M, N):
    f = make_factors(K, M, N)
    _upload(pctx, f)
    sing, U = pctx.stage_rotate_by_svd()
    X, Y = pctx.get_factors()
    Xr, Yr = PO.rotate_by_svd(f["X"], f["Y"])
    Xa, Ya = PO.align_signs(X, Y, Xr, Yr)
    dev = dict(X=stored_deviation(Xa, Xr), Y=stored_deviation(Ya, Yr))
    # the conventions: singular values descending and those of Y; U orthogonal; largest-magnitude component positive
    Y64 = f["Y"].astype(np.float64)
    G = Y64 @ Y64.T
    res = float(np.linalg.norm(G @ U - U * (sing ** 2)[None, :]))
    orth = float(np.linalg.norm(U.T @ U - np.eye(K)))
    wl, WU = np.linalg.eigh(G)
    res_l = float(np.linalg.norm(G @ WU - WU * wl[None, :]))
    orth_l = float(np.linalg.norm(WU.T @ WU - np.eye(K)))
    bound = 64 * K * 2.0 ** -53
    print(f"PP_ROTATE K={K} M={M} N={N} deviation / bound (b): X={dev['X']:.3e} Y={dev['Y']:.3e}; residual library={res:.3e} "
          f"lapack={res_l:.3e} (bound {bound * np.linalg.norm(G):.3e}); orthogonality library={orth:.3e} lapack={orth_l:.3e} "
          f"(bound {bound:.3e})")
    assert max(dev.values()) <= 1.0, dev
    assert res <= bound * np.linalg.norm(G) and orth <= bound
    assert np.all(np.diff(sing) <= 0)
    np.testing.assert_allclose(sing, np.linalg.svd(Y64, compute_uv=False), rtol=1e-12)
    assert np.all(U[np.argmax(np.abs(U), axis=0), np.arange(K)] > 0)
    # ... and the stored Y is U'Y of the returned U, the stored X is U'X: order and sign are the entry's own
    assert stored_deviation(Y, U.T @ Y64) <= 1.0 and stored_deviation(X, U.T @ f["X"].astype(np.float64)) <= 1.0


@pytest.mark.parametrize("K,M,N", SHAPES, ids=SHAPE_IDS)
def test_reorder_by_importance_matches_the_oracle(pctx, K, M, N):
    f = make_factors(K, M, N)
    _upload(pctx, f)
    perm = pctx.stage_reorder_by_importance()
    X, Y = pctx.get_factors()
    want = PO.reorder_by_importance(f["X"], f["Y"])
    assert list(perm) == list(want["order"]) == PO.importance_order(f["Y"])
    if K > 1:
        assert list(perm) != list(range(K))                                              # the case really reorders
    assert stored_deviation(X, want["X"]) == 0.0 and stored_deviation(Y, want["Y"]) == 0.0
    np.testing.assert_array_equal(X, want["X"])
    np.testing.assert_array_equal(Y, want["Y"])


def test_whiten_all_zero_view_and_all_zero_factor(pkg, pctx):
    K, M, N = SHAPES[2]
    f = make_factors(K, M, N)
    Y0, X0 = f["Y"].copy(), f["X"].copy()
    Y0[:, 3:1028] = 0                                          # view 3 of VIEWS[1068]
    X0[5, :] = 0
    _upload(pctx, f, X=X0, Y=Y0)
    xr, c = pctx.stage_whiten(M, VIEWS[N])
    X, Y = pctx.get_factors()
    ls = pctx.get_col_params()[0]
    assert xr[5] == 0 and c[2] == 0
    assert not Y[:, 3:1028].any() and np.all(ls[3:1028] == np.float32(-1e9))
    assert np.isnan(X[5]).all() and not Y[5].any() and np.isnan(X).sum() == M
    with np.errstate(invalid="ignore", divide="ignore"):
        Xr, Yr, lsr = PO.whiten(X0, Y0, f["logsigma"], VIEWS[N])
    assert max(stored_deviation(X, Xr), stored_deviation(Y, Yr), stored_deviation(ls, lsr)) <= 1.0


def test_whiten_nan_row_is_the_host_path_s(pkg):
    """An all-zero factor of X through fit.py: NaN in the same places as postprocess="host", the rest within one ulp per
    rounding step (module docstring: 2^-21 relative; logsigma: the same on its added log c)."""
    outs = {}
    for pp in ("host", "library"):
        model = _make(pkg)
        try:
            _seed_state(model, 310)
            model.matfac.X[2, :] = 0
            with np.errstate(invalid="ignore", divide="ignore"):
                pkg.whiten_(model, postprocess=pp)
            outs[pp] = (model.matfac.X.copy(), model.matfac.Y.copy(),
                        np.array(model.matfac.col_transform.unwrapped(1).logsigma, np.float32))
        finally:
            model.release_device()
    for name, g, w in zip(("X", "Y", "logsigma"), outs["library"], outs["host"]):
        assert np.array_equal(np.isnan(g), np.isnan(w)), name
        fin = np.isfinite(w)
        scale = np.abs(w[fin].astype(np.float64)) if name != "logsigma" else np.maximum(np.abs(w[fin].astype(np.float64)), 1.0)
        err = np.abs(g[fin].astype(np.float64) - w[fin].astype(np.float64))
        print(f"PP_WHITEN_HOST {name} worst |library - host| / (2^-21 scale) = {float(np.max(err / (2.0 ** -21 * scale + 1e-300))):.3e}")
        assert np.all(err <= 2.0 ** -21 * scale), name
    assert np.isnan(outs["library"][0][2]).all() and np.isnan(outs["library"][0]).sum() == SM


def test_rotate_rank_deficient_keeps_the_product(pctx):
    K, M, N = SHAPES[2]
    f = make_factors(K, M, N)
    Y0 = f["Y"].copy()
    Y0[7, :] = 0                                               # the case ARD produces: a factor switched off
    _upload(pctx, f, Y=Y0)
    sing, U = pctx.stage_rotate_by_svd()
    X, Y = (a.astype(np.float64) for a in pctx.get_factors())
    rows, cols = np.arange(0, M, max(M // 64, 1))[:64], np.arange(0, N, max(N // 64, 1))[:64]
    before = f["X"].astype(np.float64)[:, rows].T @ Y0.astype(np.float64)[:, cols]
    after = X[:, rows].T @ Y[:, cols]
    tol = 2.0 ** -23 * (np.abs(X[:, rows]).T @ np.abs(Y[:, cols])) + 1e-10 * np.max(np.abs(before))
    print(f"PP_RANKDEF worst |X'Y after - before| / bound = {float(np.max(np.abs(after - before) / tol)):.3e}, smallest singular "
          f"value {sing[-1]:.3e}")
    assert np.all(np.abs(after - before) <= tol)
    YY = Y @ Y.T
    nrm = np.sqrt(np.diag(YY))
    slack = 2.0 ** -23 * np.outer(nrm, nrm) + 1e-10 * np.max(nrm) ** 2
    off = np.abs(YY - np.diag(np.diag(YY)))
    assert np.all(off <= slack), float(np.max(off - slack))
    d = np.diag(YY)
    assert np.all(d[:-1] >= d[1:] - np.diag(slack)[:-1])
    assert sing[-1] <= 1e-7 * sing[0] and np.all(np.abs(Y[-1]) <= 1e-6)


def test_reorder_keeps_original_order_among_ties(pctx):
    K, M, N = SHAPES[2]
    f = make_factors(K, M, N)
    Y0 = f["Y"].copy()
    Y0[20] = Y0[4]                                             # two exactly equal rows ...
    Y0[9] = 0                                                  # ... and two all-zero rows
    Y0[30] = 0
    _upload(pctx, f, Y=Y0)
    perm = list(pctx.stage_reorder_by_importance())
    assert perm == PO.importance_order(Y0)
    assert perm.index(4) + 1 == perm.index(20) and perm[-2:] == [9, 30]
    X, Y = pctx.get_factors()
    np.testing.assert_array_equal(Y, Y0[perm])
    np.testing.assert_array_equal(X, f["X"][perm])


# ---- 4. lambda_max and reweight_eb_ ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,M,N", SHAPES, ids=SHAPE_IDS)
def test_lambda_max_matches_eigvalsh(pctx, K, M, N):
    f = make_factors(K, M, N)
    _upload(pctx, f)
    worst = 0.0
    for which, P, n in ((0, f["X"], M), (1, f["Y"], N)):
        for ranges in ([(1, n)], _gram_groups(n)):
            lam = pctx.stage_lambda_max(which, ranges)
            P64 = P.astype(np.float64)
            want = np.array([np.linalg.eigvalsh(P64[:, a - 1:b] @ P64[:, a - 1:b].T)[-1] for a, b in ranges])
            worst = max(worst, float(np.max(np.abs(lam - want) / want)))
            np.testing.assert_array_equal(lam, pctx.stage_lambda_max(which, ranges))
    print(f"PP_LAMBDA K={K} M={M} N={N} worst relative deviation = {worst:.3e} (bound 1e-12)")
    assert worst <= 1e-12


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))))


def test_reweight_eb_library_gives_the_host_weights(pkg):
    R = pkg.regularizers
    model = _make(pkg)
    try:
        _seed_state(model, 311)
        mf = model.matfac

        def regs(n):
            g = [(1, n // 3), (n // 3 + 1, n // 3 + 1), (n // 3 + 2, n)]   # a one-column group
            return (R.L2Regularizer(SK, 1.0), R.GroupRegularizer(group_idx=g, group_weights=[np.ones(SK, np.float32)] * 3))
        for P, n, side in ((mf.X, SM, "X"), (mf.Y, SN, "Y")):
            for i in range(2):
                host, lib = regs(n)[i], regs(n)[i]
                pkg.reweight_eb_(host, P, mixture_p=0.7)
                pkg.reweight_eb_(lib, P, mixture_p=0.7, model=model, postprocess="library")
                hw = host.weights if i == 0 else np.stack(host.group_weights)
                lw = lib.weights if i == 0 else np.stack(lib.group_weights)
                assert hw.dtype == lw.dtype == np.float32 and hw.shape == lw.shape
                print(f"PP_EB {side} {'L2' if i == 0 else 'Group'} worst deviation = {_ulps(lw, hw):.2f} ulp")
                assert _ulps(lw, hw) <= 1.0
                assert np.all(hw > 0) and not np.array_equal(hw, np.ones_like(hw))
        with pytest.raises(ValueError, match="needs model="):
            pkg.reweight_eb_(R.L2Regularizer(SK, 1.0), mf.X.copy(), model=model, postprocess="library")
        with pytest.raises(ValueError, match="'host' or 'library'"):
            pkg.whiten_(model, postprocess="device")
    finally:
        model.release_device()


# ---- 5. / 6. determinism, isolation, no stale cached image ---------------------------------------------------------------
ENTRIES = {
    "whiten": lambda ctx, M, views: ctx.stage_whiten(M, views),
    "rotate": lambda ctx, M, views: ctx.stage_rotate_by_svd(),
    "reorder": lambda ctx, M, views: (ctx.stage_reorder_by_importance(),),
    "lambda_max": lambda ctx, M, views: (ctx.stage_lambda_max(0, [(1, M)]), ctx.stage_lambda_max(1, views)),
    "gram": lambda ctx, M, views: (ctx.gram(0, [(1, M)]), ctx.gram(1, views, diag_only=True)),
}
WRITES = {"whiten": ("X", "Y", "logsigma"), "rotate": ("X", "Y"), "reorder": ("X", "Y"), "lambda_max": (), "gram": ()}


def _views_of(pkg, model):
    return [(cr.start, cr.stop) for cr in pkg.util.ids_to_ranges(model.feature_views)]


def _state(ctx, n_views):
    """Everything on the context an entry could touch: parameters, gradients, optimizer state, learning rate, noise weights."""
    groups = [("X", 0), ("Y", 0), ("logsigma", 0), ("mu", 0)] + [(w, v) for w in ("logdelta", "theta") for v in range(n_views)]
    X, Y = ctx.get_factors()
    ls, mu = ctx.get_col_params()
    st = {"X": X, "Y": Y, "logsigma": ls, "mu": mu, "lr": np.array(ctx.get_lr()), "noise_weights": ctx.get_noise_weights()}
    for v in range(n_views):
        st[f"logdelta{v}"], st[f"theta{v}"] = ctx.get_batch_view(v)
    for w, v in groups:
        st[f"grad.{w}{v}"] = ctx.get_grad(w, v)
        st[f"acc.{w}{v}"], st[f"mom.{w}{v}"] = ctx.get_opt_state(w, v)
    return st


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_entries_are_bitwise_reproducible_and_touch_nothing_else(pkg, entry):
    model = _make(pkg)
    try:
        _seed_state(model, 312)
        mf = model.matfac
        ctx = model.device_context()
        views = _views_of(pkg, model)
        n_views = len(ctx.view_shapes)
        runs = []
        for _ in range(2):
            pkg.matfac.marshal(mf, ctx, with_xreg=False, with_yreg=False)
            ctx.set_optimizer("adam", lr=0.0123)
            ctx.fit(update_X=True, update_Y=True, update_col_layers=True, max_epochs=2, abs_tol=0, rel_tol=0)   # a live state
            pkg.matfac.marshal(mf, ctx, with_xreg=False, with_yreg=False)
            before = _state(ctx, n_views)
            assert before["acc.X0"].any() and before["grad.Y0"].any() and before["mom.logsigma0"].any()
            out = [np.asarray(a) for a in ENTRIES[entry](ctx, SM, views)]
            after = _state(ctx, n_views)
            for k in before:
                if k in WRITES[entry]:
                    assert not np.array_equal(before[k], after[k]), k
                else:
                    np.testing.assert_array_equal(before[k], after[k], err_msg=k)
            runs.append(out + [after[k] for k in WRITES[entry]])
        for a, b in zip(*runs):
            np.testing.assert_array_equal(a, b)
    finally:
        model.release_device()


@pytest.mark.parametrize("precision", ["f32", "bf16x3"])
@pytest.mark.parametrize("entry", ["whiten", "rotate", "reorder"])
def test_fit_after_an_entry_is_the_fit_after_an_upload(pkg, entry, precision):
    model = _make(pkg)
    try:
        _seed_state(model, 313)
        mf = model.matfac
        ctx = model.device_context()
        ctx.set_precision(precision)
        views = _views_of(pkg, model)
        fits = []
        for uploaded in (False, True):
            # Both rounds reach the same state: marshalled, one epoch fitted.  That fit is the LAST thing before the entry --
            # no marshal, no pmf_set_col_params in between, either of which would drop the prepared column image by itself --
            # so the image of the pre-entry logsigma is live when the entry runs.  The closing fit leaves the column layers
            # alone (update_col_layers=False re-prepares only if `prepared` was cleared): a stale image would be used.
            pkg.matfac.marshal(mf, ctx, with_xreg=True, with_yreg=True)
            ctx.set_optimizer("adagrad", lr=0.05)
            r0 = ctx.fit(update_X=True, update_Y=True, max_epochs=1, abs_tol=0, rel_tol=0)
            ls0 = ctx.get_col_params()[0]
            if not uploaded:
                ENTRIES[entry](ctx, SM, views)
                X, Y = ctx.get_factors()
                ls = ctx.get_col_params()[0]
                assert not np.array_equal(Y, mf.Y)
                assert (entry == "whiten") == (not np.array_equal(ls, ls0))              # only whiten rewrites logsigma
            else:
                ctx.set_factors(X, Y)
                ctx.set_col_params(logsigma=ls)
            r = ctx.fit(update_X=True, update_Y=True, update_col_layers=False, max_epochs=3, abs_tol=0, rel_tol=0)
            fits.append((r0["loss"], r["loss"]) + ctx.get_factors() + ctx.get_col_params())
        assert np.all(np.isfinite(fits[0][1])) and len(fits[0][1]) == 3
        for a, b in zip(*fits):
            np.testing.assert_array_equal(a, b)
        if precision == "bf16x3":
            assert ctx.get_precision()[1] > 0                                              # the split kernels really ran
    finally:
        model.release_device()


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_name_their_cause_and_leave_the_context_usable(pkg):
    K, M, N = SHAPES[1]
    f = make_factors(K, M, N)
    ctx = pkg.Context(0)
    try:
        ctx.set_data(f["D"])
        for call in (lambda: ctx.gram(0, [(1, M)]), lambda: ctx.stage_lambda_max(1, [(1, N)]), lambda: ctx.stage_whiten(M, VIEWS[N]),
                     ctx.stage_rotate_by_svd, ctx.stage_reorder_by_importance):
            with pytest.raises(pkg.PMFError, match="factors not set"):
                call()
        _upload(ctx, f)
        with pytest.raises(pkg.PMFError, match=r"range 0 = 1:332 does not lie in 1\.\.331"):
            ctx.gram(0, [(1, M + 1)])
        with pytest.raises(pkg.PMFError, match=r"range 1 = 0:5 does not lie in 1\.\.96"):
            ctx.stage_lambda_max(1, [(1, 2), (0, 5)])
        with pytest.raises(pkg.PMFError, match=r"range 1 = 97:97 does not lie in 1\.\.96"):
            ctx.stage_whiten(M, [(1, 96), (97, 97)])
        with pytest.raises(pkg.PMFError, match="overlaps or precedes the range before it"):
            ctx.stage_whiten(M, [(1, 50), (50, 96)])
        with pytest.raises(pkg.PMFError, match="overlaps or precedes the range before it"):
            ctx.gram(1, [(40, 60), (1, 20)])
        with pytest.raises(pkg.PMFError, match=r"range 0 = 9:3 does not lie in 1\.\.96"):
            ctx.stage_lambda_max(1, [(9, 3)])
        with pytest.raises(pkg.PMFError, match=r"range 0 = 5:4 does not lie"):          # an empty view is not a view
            ctx.stage_whiten(M, [(5, 4)])
        with pytest.raises(pkg.PMFError, match="M_total = 330 is below the context's 331 rows"):
            ctx.stage_whiten(M - 1, VIEWS[N])
        for call in (lambda: ctx.gram(0, []), lambda: ctx.stage_lambda_max(1, []), lambda: ctx.stage_whiten(M, [])):
            with pytest.raises(pkg.PMFError, match="n_groups = 0 must be at least 1"):
                call()
        with pytest.raises(pkg.PMFError, match="which = 2"):
            ctx.gram(2, [(1, 3)])
        one = np.array([1], np.int64)
        p64 = one.ctypes.data_as(C.POINTER(C.c_int64))
        assert ctx.lib.pmf_gram(ctx._h, 0, 1, p64, p64, 0, None) != 0 and "null output" in ctx.lib.pmf_last_error().decode()
        assert ctx.lib.pmf_stage_lambda_max(ctx._h, 0, 1, p64, p64, None) != 0 and "null output" in ctx.lib.pmf_last_error().decode()
        assert ctx.lib.pmf_gram(ctx._h, 0, 1, None, p64, 0, None) != 0 and "null range pointer" in ctx.lib.pmf_last_error().decode()
        # nothing was written by any refused call, and the context is usable
        X, Y = ctx.get_factors()
        np.testing.assert_array_equal(X, f["X"])
        np.testing.assert_array_equal(Y, f["Y"])
        np.testing.assert_array_equal(ctx.get_col_params()[0], f["logsigma"])
        assert ctx.lib.pmf_stage_rotate_by_svd(ctx._h, None, None) == 0                   # either output may be NULL
        assert ctx.lib.pmf_stage_reorder_by_importance(ctx._h, None) == 0
        assert ctx.lib.pmf_stage_whiten(ctx._h, C.c_int64(M), 1, p64, np.array([N], np.int64).ctypes.data_as(C.POINTER(C.c_int64)),
                                        None, None) == 0
        r = ctx.fit(update_X=True, update_Y=True, max_epochs=2, abs_tol=0, rel_tol=0)
        assert np.all(np.isfinite(r["loss"]))
    finally:
        ctx.close()


# ---- 8. two ranks ---------------------------------------------------------------------------------------------------------
def _rank_entries(pkg, model):
    """Every entry from its own seeded state on the model's context.  Names that start with "X_" hold local columns of X; the
    collectives each entry issued are counted from pmf_comm_info."""
    out = {}
    mf = model.matfac
    ctx = model.device_context()
    views = _views_of(pkg, model)
    R = pkg.regularizers

    def counted(name, fn):
        pkg.matfac.marshal(mf, ctx, with_xreg=False, with_yreg=False)
        n0 = ctx.comm_info()["n_collectives"]
        r = fn()
        out[name + ".collectives"] = np.array(ctx.comm_info()["n_collectives"] - n0)
        return r

    _seed_state(model, 320)
    xr, c = counted("whiten", lambda: ctx.stage_whiten(model.M_total, views))
    out["whiten.x_rms"], out["whiten.c"] = xr, c
    out["X_whiten"], out["whiten.Y"] = ctx.get_factors()
    out["whiten.logsigma"] = ctx.get_col_params()[0]
    _seed_state(model, 321)
    out["rotate.sing"], out["rotate.U"] = counted("rotate", ctx.stage_rotate_by_svd)
    out["X_rotate"], out["rotate.Y"] = ctx.get_factors()
    _seed_state(model, 322)
    out["reorder.perm"] = counted("reorder", ctx.stage_reorder_by_importance)
    out["X_reorder"], out["reorder.Y"] = ctx.get_factors()
    _seed_state(model, 323)
    groups = [(1, 100), (101, 101), (102, 150), (200, SM)]            # groups 1-3 lie in rank 0's rows only, group 4 in rank 1's
    reg = R.GroupRegularizer(group_idx=groups, group_weights=[np.ones(SK, np.float32)] * 4)
    lo, hi, _ = model.row_shard
    if model.sharded:
        reg.row_shard = (lo, hi)
    out["lambda_x"] = counted("lambda_x", lambda: ctx.stage_lambda_max(0, pkg.fit._group_ranges_with_empties(reg)))
    out["lambda_y"] = counted("lambda_y", lambda: ctx.stage_lambda_max(1, views))
    out["gram_y"] = counted("gram_y", lambda: ctx.gram(1, views))
    # through fit.py: one collective for the X regularizer, none for Y's
    n0 = ctx.comm_info()["n_collectives"]
    pkg.reweight_eb_(reg, mf.X, model=model, postprocess="library")
    out["eb_x.collectives"] = np.array(ctx.comm_info()["n_collectives"] - n0)
    out["eb_x.weights"] = np.stack(reg.group_weights)
    return out


def _worker(rank, world, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist
    import pmf_import
    pkg = pmf_import.load()
    dist.init_process_group("gloo", rank=rank, world_size=world)

    def allreduce(arr):
        dist.all_reduce(torch.from_numpy(arr))

    lo, hi = pkg.parallel.shard_rows(SM, world, rank)
    model = _make(pkg, lo, hi)
    model.attach_comm(rank, world, host_allreduce=allreduce)
    out = _rank_entries(pkg, model)
    model.set_allreduce(lambda a: a)                                  # a reducer that is not the library's: refused
    try:
        pkg.whiten_(model, postprocess="library")
        out["set_allreduce_error"] = np.array("no error")
    except ValueError as e:
        out["set_allreduce_error"] = np.array(str(e))
    model.set_allreduce(None)
    np.savez(Path(outdir) / f"pp{rank}.npz", **out)
    model.release_device()
    dist.destroy_process_group()


def test_two_ranks_compute_identical_bits_within_the_bounds_of_the_unsharded_run(pkg, tmp_path):
    model = _make(pkg)                                                # the unsharded run first: after the workers no GPU work
    try:
        want = _rank_entries(pkg, model)
    finally:
        model.release_device()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_gpu_postprocess as t; "
            "t._worker(int(sys.argv[1]), 2, int(sys.argv[2]), sys.argv[3])") % (str(ROOT), str(ROOT / "tests"))
    procs = [subprocess.Popen([sys.executable, "-c", code, str(r), str(port), str(tmp_path)]) for r in range(2)]
    try:
        for pr in procs:                                              # each worker under its own time limit
            assert pr.wait(timeout=120) == 0
    finally:
        for pr in procs:                                              # a failing worker ends the test: its peer is killed
            if pr.poll() is None:
                pr.kill()
    a, b = [np.load(tmp_path / f"pp{k}.npz") for k in range(2)]
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        if not k.startswith("X_"):
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)      # every replicated output: the same bits on both ranks
    assert (a["X_whiten"].shape, b["X_whiten"].shape) == ((SK, 166), (SK, 165))
    counts = {k[:-len(".collectives")]: int(a[k]) for k in a.files if k.endswith(".collectives")}
    assert counts == dict(whiten=1, rotate=0, reorder=0, lambda_x=1, lambda_y=0, gram_y=0, eb_x=1), counts
    assert "set_allreduce" in str(a["set_allreduce_error"]), str(a["set_allreduce_error"])
    assert all(int(want[k]) == 0 for k in want if k.endswith(".collectives"))
    devs = {}
    for k in want:
        if k.endswith(".collectives"):
            continue
        got = np.concatenate([a[k], b[k]], axis=1) if k.startswith("X_") else a[k]
        if k in ("lambda_x", "lambda_y", "gram_y", "whiten.x_rms", "whiten.c", "rotate.sing", "rotate.U"):   # float64 outputs
            devs[k] = rel_err(got, want[k]) / 1e-12
        elif k == "reorder.perm":
            devs[k] = 0.0 if list(got) == list(want[k]) else np.inf
        else:
            devs[k] = stored_deviation(got, np.asarray(want[k], np.float64))
    print("PP_RANKS deviation / bound: " + " ".join(f"{k}={v:.3e}" for k, v in devs.items()))
    assert max(devs.values()) <= 1.0, devs
    assert np.all(a["lambda_x"] > 0)                                  # every group has its rows on one rank only


# ---- 9. fit_ end to end ----------------------------------------------------------------------------------------------------
def test_fit_with_library_postprocessing_follows_the_library_stages_run(pkg, monkeypatch):
    from test_gpu_library_stages import LIB_FIT_BOUND, _make_mixed
    calls = {}
    for name in ("stage_whiten", "stage_rotate_by_svd", "stage_reorder_by_importance", "stage_lambda_max"):
        def counted(self, *a, _name=name, _fn=getattr(pkg.Context, name), **kw):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(self, *a, **kw)
        monkeypatch.setattr(pkg.Context, name, counted)
    outs, ncalls = {}, {}
    for pp in ("host", "library"):
        model = _make_mixed(pkg)
        calls.clear()
        try:
            hist = pkg.fit_(model, keep_history=True, stages="library", postprocess=pp, **FIT_KW)
            ncalls[pp] = dict(calls)
            outs[pp] = _fit_outputs(pkg, model, hist)
            outs[pp]["X"] = model.matfac.X.copy()
        finally:
            model.release_device()
    want, got = outs["host"], outs["library"]
    # the keyword reached every stage: fit_feature_set_ard_ -> fit_ard_ -> basic_fit_ whitens and rotates once, fit_ard_
    # re-weights the Group term on X (one lambda_max; the ARD term on Y has none), fit_ whitens again and reorders
    assert ncalls["host"] == {}, ncalls
    lib = ncalls["library"]
    assert lib.get("stage_whiten", 0) >= 2 and lib.get("stage_rotate_by_svd", 0) >= 1, ncalls
    assert lib.get("stage_reorder_by_importance", 0) == 1 and lib.get("stage_lambda_max", 0) >= 1, ncalls
    for k in ("names", "terms", "epochs"):
        assert list(got[k]) == list(want[k]), (k, list(got[k]), list(want[k]))
    Xa, Ya = PO.align_signs(got["X"], got["Y"], want["X"], want["Y"])     # the loss is invariant under the joint sign flip
    assert len(got["losses"]) == len(want["losses"])
    err = dict(loss=abs(got["losses"][-1] - want["losses"][-1]) / abs(want["losses"][-1]), Y=rel_err(Ya, want["Y"]),
               X=rel_err(Xa, want["X"]),
               history=float(np.max(np.abs(got["losses"] - want["losses"]) / np.abs(want["losses"]))))
    print("PP_FIT " + " ".join(f"{k}={v:.3e}" for k, v in err.items()))
    bound = dict(LIB_FIT_BOUND, history=LIB_FIT_BOUND["loss"])
    for k, v in err.items():
        assert v <= bound[k] <= 2e-3, (k, v)
