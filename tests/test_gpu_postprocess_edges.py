"""csrc/pmf_postprocess.hip at the seams that tests/test_gpu_postprocess.py does not reach: postprocess_cases.EDGE_SHAPES /
EDGE_VIEWS (what each shape hits is asserted on the CPU by tests/test_postprocess_edge_cases.py) -- both sides of the K
thresholds of k_pp_gram<2|4|8> / k_pp_rotate<32|64|128>, Kp = 96, a Y of two and three Gram pieces behind every stage
(k_pp_diag with a row scale and k_pp_piece_sum over more than one slab), whole and single tiles of the in-place kernels
k_pp_rotate and k_pp_permute, and views that leave columns out (pp_find_range's -1) in counts of up to 65.

Same oracle (oracle/postprocess_oracle.py, float64, on the uploaded float32 inputs) and same bounds as the first file:
(a) for Gram entries, (b) for every stored float32, 1e-12 relative for eigenvalues and singular values, 64 K 2^-53 for the
eigen-residual and orthogonality; "bitwise" where the library promises a fixed order of operations.  No bound of its own.

Every test prints its worst ratio on a "PP_EDGE ..." line before it asserts: run with -s to see them.
Worst figures seen on an MI355X over the six shapes, each as a fraction of its bound (records, not bounds):
    gram          error / bound (a)                           3.1e-2
    lambda_max    relative deviation / 1e-12                  4.4e-3
    whiten        deviation / bound (b)                       X 0.50, Y 0.94, logsigma 0.49 (Y is rounded twice)
    rotate        deviation / bound (b)                       X 0.50, Y 0.50, the same against the returned U
                  residual / (64 K 2^-53 |G|)                 1.2e-2
                  orthogonality / (64 K 2^-53)                0.24
    reorder, columns in no view, fresh contexts, the fit after an entry: bitwise, no figure"""
import numpy as np
import pytest

from oracle import postprocess_oracle as PO
from postprocess_cases import EDGE_SHAPES, EDGE_VIEWS, GRAM_CHUNK, check_gram, make_factors, stored_deviation
from test_gpu_postprocess import _upload

pytestmark = pytest.mark.gpu
EDGE_IDS = [f"K{k}_M{m}_N{n}" for k, m, n in EDGE_SHAPES]
PAD_SHAPE = (65, 63, 4100)                                     # K < Kp = 96 < R = 128, three pieces of Y


@pytest.fixture(scope="module")
def pctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _range_sets(n, N):
    """The whole range; EDGE_VIEWS[N] (cut at n on the X side, whose n = M is below N); and, where n spans more than one
    piece, a short group and one that starts inside the first piece and ends inside the last."""
    views = [(a, min(b, n)) for a, b in EDGE_VIEWS[N] if a <= n]
    sets = [[(1, n)], views]
    if n > GRAM_CHUNK:
        stop = n - 1 if n - 1 > GRAM_CHUNK else n               # (N = 2049: the second piece is one column)
        sets.append([(3, 5), (GRAM_CHUNK - 5, stop)])
        assert (GRAM_CHUNK - 6) // GRAM_CHUNK == 0 < (stop - 1) // GRAM_CHUNK
    return sets


def _uncovered(N):
    seen = np.zeros(N, bool)
    for a, b in EDGE_VIEWS[N]:
        seen[a - 1:b] = True
    return np.nonzero(~seen)[0]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


# ---- pmf_gram and pmf_stage_lambda_max --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,M,N", EDGE_SHAPES, ids=EDGE_IDS)
def test_gram_matches_numpy(pctx, K, M, N):
    f = make_factors(K, M, N)
    _upload(pctx, f)
    worst = 0.0
    for which, P, n in ((0, f["X"], M), (1, f["Y"], N)):
        for ranges in _range_sets(n, N):
            G = pctx.gram(which, ranges)
            assert G.shape == (len(ranges), K, K)
            worst = max(worst, check_gram(G, P, ranges, (which, ranges)))
            np.testing.assert_array_equal(_bits(G), _bits(np.transpose(G, (0, 2, 1))))          # symmetric bit for bit
            d = pctx.gram(which, ranges, diag_only=True)
            np.testing.assert_array_equal(_bits(d), _bits(np.einsum("gkk->gk", G)))             # the diagonal mode: the same bits
            np.testing.assert_array_equal(_bits(G), _bits(pctx.gram(which, ranges)))            # two calls: the same bits
    print(f"PP_EDGE gram K={K} M={M} N={N} worst error / bound (a) = {worst:.3e}")
    X, Y = pctx.get_factors()                                                                   # nothing was written
    np.testing.assert_array_equal(_bits(X), _bits(f["X"]))
    np.testing.assert_array_equal(_bits(Y), _bits(f["Y"]))


@pytest.mark.parametrize("K,M,N", EDGE_SHAPES, ids=EDGE_IDS)
def test_lambda_max_matches_eigvalsh(pctx, K, M, N):
    f = make_factors(K, M, N)
    _upload(pctx, f)
    worst = 0.0
    for which, P, n in ((0, f["X"], M), (1, f["Y"], N)):
        P64 = P.astype(np.float64)
        for ranges in _range_sets(n, N):
            lam = pctx.stage_lambda_max(which, ranges)
            want = np.array([np.linalg.eigvalsh(P64[:, a - 1:b] @ P64[:, a - 1:b].T)[-1] for a, b in ranges])
            worst = max(worst, float(np.max(np.abs(lam - want) / want)))
            np.testing.assert_array_equal(_bits(lam), _bits(pctx.stage_lambda_max(which, ranges)))
    print(f"PP_EDGE lambda_max K={K} M={M} N={N} worst relative deviation / 1e-12 = {worst / 1e-12:.3e}")
    assert worst <= 1e-12


# ---- the three stages against the oracle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,M,N", EDGE_SHAPES, ids=EDGE_IDS)
def test_whiten_matches_the_oracle_and_leaves_columns_in_no_view_alone(pctx, K, M, N):
    f = make_factors(K, M, N)
    views = EDGE_VIEWS[N]
    _upload(pctx, f)
    xr, c = pctx.stage_whiten(M, views)
    X, Y = pctx.get_factors()
    ls, mu = pctx.get_col_params()
    Xr, Yr, lsr = PO.whiten(f["X"], f["Y"], f["logsigma"], views)
    dev = dict(X=stored_deviation(X, Xr), Y=stored_deviation(Y, Yr), logsigma=stored_deviation(ls, lsr))
    print(f"PP_EDGE whiten K={K} M={M} N={N} views={len(views)} deviation / bound (b): "
          + " ".join(f"{k}={v:.3e}" for k, v in dev.items()))
    assert max(dev.values()) <= 1.0, dev
    np.testing.assert_allclose(xr, PO.rms_rows(f["X"].astype(np.float64)), rtol=1e-13)
    assert c.shape == (len(views),) and np.all(c > 0)
    np.testing.assert_array_equal(_bits(mu), _bits(f["mu"]))                                    # mu is not touched
    # a column in no view: its logsigma keeps its bits, and Y has met x_rms only -- the third scale pass (Y / c, which
    # rewrites every column it finds a range for) and k_pp_logsigma pass it by
    out = _uncovered(N)
    np.testing.assert_array_equal(_bits(ls[out]), _bits(f["logsigma"][out]))
    want = (f["Y"][:, out].astype(np.float64) * xr[:, None]).astype(np.float32)
    np.testing.assert_array_equal(_bits(Y[:, out]), _bits(want))
    inside = np.setdiff1d(np.arange(N), out)
    assert not np.array_equal(ls[inside], f["logsigma"][inside])
    print(f"PP_EDGE whiten K={K} M={M} N={N} columns in no view: {out.size}, bitwise kept")


@pytest.mark.parametrize("K,M,N", EDGE_SHAPES, ids=EDGE_IDS)
def test_rotate_by_svd_matches_the_oracle(pctx, K, M, N):
    f = make_factors(K, M, N)
    _upload(pctx, f)
    sing, U = pctx.stage_rotate_by_svd()
    X, Y = pctx.get_factors()
    Xr, Yr = PO.rotate_by_svd(f["X"], f["Y"])
    Xa, Ya = PO.align_signs(X, Y, Xr, Yr)
    dev = dict(X=stored_deviation(Xa, Xr), Y=stored_deviation(Ya, Yr))
    Y64 = f["Y"].astype(np.float64)
    G = Y64 @ Y64.T
    res = float(np.linalg.norm(G @ U - U * (sing ** 2)[None, :]))
    orth = float(np.linalg.norm(U.T @ U - np.eye(K)))
    bound = 64 * K * 2.0 ** -53
    own = dict(X=stored_deviation(X, U.T @ f["X"].astype(np.float64)), Y=stored_deviation(Y, U.T @ Y64))
    print(f"PP_EDGE rotate K={K} M={M} N={N} deviation / bound (b): X={dev['X']:.3e} Y={dev['Y']:.3e}; against the returned U: "
          f"X={own['X']:.3e} Y={own['Y']:.3e}; residual / bound = {res / (bound * np.linalg.norm(G)):.3e}; orthogonality / bound = "
          f"{orth / bound:.3e}")
    assert max(dev.values()) <= 1.0, dev
    assert res <= bound * np.linalg.norm(G) and orth <= bound
    assert np.all(np.diff(sing) <= 0)
    np.testing.assert_allclose(sing, np.linalg.svd(Y64, compute_uv=False), rtol=1e-12)
    assert np.all(U[np.argmax(np.abs(U), axis=0), np.arange(K)] > 0)
    assert max(own.values()) <= 1.0, own


@pytest.mark.parametrize("K,M,N", EDGE_SHAPES, ids=EDGE_IDS)
def test_reorder_by_importance_matches_the_oracle(pctx, K, M, N):
    f = make_factors(K, M, N)
    _upload(pctx, f)
    perm = pctx.stage_reorder_by_importance()
    X, Y = pctx.get_factors()
    want = PO.importance_order(f["Y"])
    moved = sum(int(p != r) for r, p in enumerate(want))
    print(f"PP_EDGE reorder K={K} M={M} N={N} rows moved: {moved} of {K}; permutation equal: {list(perm) == want}")
    assert list(perm) == want and moved > 0
    np.testing.assert_array_equal(_bits(X), _bits(f["X"][want]))
    np.testing.assert_array_equal(_bits(Y), _bits(f["Y"][want]))


# ---- fresh contexts -----------------------------------------------------------------------------------------------------------
def _entry(ctx, name, M, views):
    if name == "whiten":
        return list(ctx.stage_whiten(M, views))
    if name == "rotate":
        return list(ctx.stage_rotate_by_svd())
    return [ctx.stage_reorder_by_importance()]


def test_two_fresh_contexts_give_the_same_bits(pkg):
    K, M, N = PAD_SHAPE
    f = make_factors(K, M, N)
    runs = []
    for _ in range(2):
        ctx = pkg.Context(0)
        try:
            out = []
            for name in ("whiten", "rotate", "reorder"):
                _upload(ctx, f)
                out += _entry(ctx, name, M, EDGE_VIEWS[N])
                out += list(ctx.get_factors()) + [ctx.get_col_params()[0]]
            runs.append(out)
        finally:
            ctx.close()
    assert len(runs[0]) == len(runs[1]) == 14
    for a, b in zip(*runs):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    print(f"PP_EDGE fresh contexts K={K} M={M} N={N}: {len(runs[0])} outputs of whiten, rotate and reorder bitwise equal")


# ---- a fit after an entry -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["whiten", "rotate", "reorder"])
def test_fit_after_an_entry_is_the_fit_of_a_fresh_context_after_an_upload(pkg, entry):
    """test_fit_after_an_entry_is_the_fit_after_an_upload of the first file at K = 65 < Kp = 96, in f32, on raw contexts
    (that test's model has one fixed shape).  An upload writes zeros into the pad rows K..Kp-1 of X and Y; the entry's kernels
    write them themselves.  The fused kernels read whole Kp-row columns, so a pad row that an entry left non-zero or NaN
    shows in the losses and factors of the fit that follows, and nowhere else."""
    K, M, N = PAD_SHAPE
    f = make_factors(K, M, N)
    fits, state = [], None
    for uploaded in (False, True):
        ctx = pkg.Context(0)
        try:
            ctx.set_precision("f32")
            _upload(ctx, f)
            ctx.set_optimizer("adagrad", lr=0.05)
            r0 = ctx.fit(update_X=True, update_Y=True, max_epochs=1, abs_tol=0, rel_tol=0)      # a live state and column image
            Y0, ls0 = ctx.get_factors()[1], ctx.get_col_params()[0]
            if not uploaded:
                _entry(ctx, entry, M, EDGE_VIEWS[N])
                state = ctx.get_factors() + (ctx.get_col_params()[0],)
                assert not np.array_equal(state[1], Y0)
                assert (entry == "whiten") == (not np.array_equal(state[2], ls0))               # only whiten rewrites logsigma
            else:
                ctx.set_factors(state[0], state[1])
                ctx.set_col_params(logsigma=state[2])
            r = ctx.fit(update_X=True, update_Y=True, update_col_layers=False, max_epochs=3, abs_tol=0, rel_tol=0)
            fits.append((np.asarray(r0["loss"]), np.asarray(r["loss"])) + ctx.get_factors() + ctx.get_col_params())
        finally:
            ctx.close()
    assert np.all(np.isfinite(fits[0][1])) and len(fits[0][1]) == 3
    same = [np.array_equal(_bits(a), _bits(b)) for a, b in zip(*fits)]
    print(f"PP_EDGE fit after {entry} K={K} Kp=96: losses {fits[0][1]} ; bitwise equal (first loss, losses, X, Y, logsigma, mu): {same}")
    for a, b in zip(*fits):
        np.testing.assert_array_equal(_bits(a), _bits(b))
