"""A second pass on a small, fresh context must find every buffer large enough for what ITS kernels address.

The library keeps its device buffers from pass to pass and only grows them, and it caches the work split under a key that
holds the shape and the tiling but not the kernel family (compute_work_split).  The session context of the suite has long
grown every buffer to the largest test, and tests/test_gpu_history.py runs one family per fresh context above one row panel,
so neither can see a pass that needs more of a buffer than the pass before it left there.  Here every case is a short
sequence of passes on a fresh context, at shapes of ONE row panel whatever its height, where two families share a cached
split: 70 rows are one panel of 256 rows (exact f32 at K <= 64, sb2) and one of 512 rows (sb8 at K <= 64, exact f32 with two
row blocks per wave), 33 rows one of 128 (exact, sb4 at K > 64) and one of 256 (sb8).  The problem is marshalled ONCE per
sequence: pmf_set_noise bumps the key's kind_version, which would recompute the split and hide the collision.

Each pass is checked four ways: the family that ran; the bytes its kernels address against the bytes allocated
(Context.pass_extents, before and after the pass -- a comparison of results alone passes whenever the memory behind a short
buffer happens to be mapped); bitwise equality with the same pass on a fresh context that ran nothing else; the fp64 oracle.
"""
import numpy as np
import pytest

from problems import make_problem, rel_err, to_context, to_oracle
from test_gpu_parity import GRAD_TOL, LOSS_RTOL, grads_of

pytestmark = pytest.mark.gpu

BOTH = dict(update_X=True, update_Y=True)
XONLY = dict(update_X=True)


def assert_fits(ext, where):
    for name, e in ext.items():
        assert e["need"] <= e["capacity"], f"{where}: the pass addresses {e['need']} bytes of {name}, {e['capacity']} allocated"


def xy(flags):
    return dict(update_X=bool(flags.get("update_X")), update_Y=bool(flags.get("update_Y")))


# ---- passes through the step-level API ---------------------------------------------------------------------------------
# A step: precision, gradient flags, family that must run, its row-panel height, whether the batch views are attached.
def step(prec, flags, fam, bm, views=True):
    return dict(prec=prec, flags=flags, fam=fam, bm=bm, views=views)


def problem_of(p, st):
    return p if st["views"] else dict(p, batch_views=[])


def run_step(ctx, p, st, where):
    """One checked pass on a context that already holds the problem."""
    ctx.set_precision(st["prec"])
    q = problem_of(p, st)
    ext = ctx.pass_extents(**xy(st["flags"]))
    assert_fits(ext, where + " (planned)")
    if st["flags"].get("update_X") and set(p["noise_kinds"]) == {"normal"}:
        # one row panel, fewer column tiles than workgroups and tiles of equal cost: one piece per tile, each a BM x Kp slot
        Kp, n_ct = (p["K"] + 31) // 32 * 32, (p["N"] + 31) // 32
        assert ext["gx_part"]["need"] == n_ct * st["bm"] * Kp * 4, (where, ext["gx_part"], st["bm"])
    loss, g = grads_of(ctx, q, **st["flags"])
    assert ctx.last_kernel() == st["fam"], (where, ctx.last_kernel(), st["fam"])
    assert_fits(ctx.pass_extents(**xy(st["flags"])), where + " (after the pass)")
    return loss, g


_SOLO, _ORACLE = {}, {}


def solo(pkg, key, p, st):
    """The step on a fresh context that runs nothing else (once per case and step)."""
    k = (key, st["prec"], tuple(sorted(st["flags"])), st["views"])
    if k not in _SOLO:
        ctx = pkg.Context(0)
        try:
            to_context(problem_of(p, st), ctx)
            _SOLO[k] = run_step(ctx, p, st, f"{key}: alone")
        finally:
            ctx.close()
    return _SOLO[k]


def oracle(key, p, st):
    k = (key, tuple(sorted(st["flags"])), st["views"])
    if k not in _ORACLE:
        m = to_oracle(problem_of(p, st))
        m.m.n_xreg = 0
        m.m.n_yreg = 0
        _ORACLE[k] = m.loss_and_grads(**st["flags"])[1]
    return _ORACLE[k]


def assert_bitwise(got, want, where):
    assert got[0] == want[0], (where, got[0], want[0])
    assert got[1].keys() == want[1].keys()
    for k in got[1]:
        assert np.array_equal(got[1][k], want[1][k]), f"{where}: grad({k}) differs from the same pass on a fresh context"


def assert_oracle(got, go, where):
    loss, g = got
    assert abs(loss - go["data_loss"]) <= LOSS_RTOL * abs(go["data_loss"]) + 1e-6, (where, loss, go["data_loss"])
    for k, v in g.items():
        assert np.isfinite(v).all(), f"{where}: non-finite grad({k})"
        assert rel_err(v, go[k]) <= GRAD_TOL, (where, k, rel_err(v, go[k]))


def run_sequence(pkg, key, p, steps):
    ctx = pkg.Context(0)
    got = []
    try:
        to_context(problem_of(p, steps[0]), ctx)   # once: see the module docstring
        views = steps[0]["views"]
        for i, st in enumerate(steps):
            if st["views"] != views:
                ctx.set_batch_views(p["batch_views"] if st["views"] else [])
                views = st["views"]
            got.append(run_step(ctx, p, st, f"{key}: pass {i + 1} of {len(steps)}"))
    finally:
        ctx.close()
    for i, (st, r) in enumerate(zip(steps, got)):
        where = f"{key}: pass {i + 1} of {len(steps)}"
        assert_bitwise(r, solo(pkg, key, p, st), where)
        assert_oracle(r, oracle(key, p, st), where)


def small_problem(M, N, K, **kw):
    return make_problem(M=M, N=N, K=K, seed=K + M, col_params=True, weights=True, nan_frac=0.05, scale=0.5, **kw)


PROBLEMS = {
    "kb2": lambda: small_problem(70, 100, 40),
    "kb2_mixed": lambda: small_problem(70, 100, 40, bernoulli_frac=0.2),
    "kb4": lambda: small_problem(33, 65, 100),
    "kb1": lambda: small_problem(70, 100, 20, n_views=2, batch_views=2, n_batches=3),
}
_P = {}


def problem(name):
    if name not in _P:
        _P[name] = PROBLEMS[name]()
    return _P[name]


# name: problem, steps.  Every pair shares one cached work split and differs in the panel height BM, i.e. in the bytes of a
# gX slot; the reverse orders shrink what is needed (nothing may rely on the larger buffer either: bitwise equality).
SEQUENCES = {
    "kb2_exact256_sb8_512": ("kb2", [step("f32", BOTH, 0, 256), step("bf16x3", BOTH, 8, 512)]),
    "kb2_sb8_512_exact256": ("kb2", [step("bf16x3", BOTH, 8, 512), step("f32", BOTH, 0, 256)]),
    "kb2_sb2_256_sb8_512": ("kb2", [step("bf16x3", XONLY, 2, 256), step("bf16x3", BOTH, 8, 512)]),
    "kb2_sb8_512_sb2_256": ("kb2", [step("bf16x3", BOTH, 8, 512), step("bf16x3", XONLY, 2, 256)]),
    "kb2_mixed_sb2_256_sb8_512": ("kb2_mixed", [step("bf16x3", XONLY, 2, 256), step("bf16x3", BOTH, 8, 512)]),
    "kb2_mixed_sb8_512_sb2_256": ("kb2_mixed", [step("bf16x3", BOTH, 8, 512), step("bf16x3", XONLY, 2, 256)]),
    "kb4_exact128_sb8_256": ("kb4", [step("f32", BOTH, 0, 128), step("bf16x3", BOTH, 8, 256)]),
    "kb4_sb8_256_exact128": ("kb4", [step("bf16x3", BOTH, 8, 256), step("f32", BOTH, 0, 128)]),
    "kb4_sb4_128_sb8_256": ("kb4", [step("bf16x3", XONLY, 4, 128), step("bf16x3", BOTH, 8, 256)]),
    "kb4_sb8_256_sb4_128": ("kb4", [step("bf16x3", BOTH, 8, 256), step("bf16x3", XONLY, 4, 128)]),
    # exact f32 at K <= 32: one row block per wave with batch views (256 rows), two without (512); clearing the views does
    # not touch the split's key
    "kb1_views_256_none_512": ("kb1", [step("f32", BOTH, 0, 256), step("f32", BOTH, 0, 512, views=False)]),
    "kb1_none_512_views_256": ("kb1", [step("f32", BOTH, 0, 512, views=False), step("f32", BOTH, 0, 256)]),
}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_family_switch_on_a_fresh_context(pkg, name):
    pname, steps = SEQUENCES[name]
    run_sequence(pkg, pname, problem(pname), steps)


# ---- a larger Kp and wider operand images on the same context ----------------------------------------------------------
@pytest.mark.parametrize("order", ["k40_then_k100", "k100_then_k40"])
def test_kp_and_image_width_growth(pkg, order):
    """sb8 at K = 40, N = 100 (Kp = 64: 16-KiB image blocks, slabs of 64 x 100, a padding tile of 32 x 64 floats) and at
    K = 100, N = 50 (Kp = 128: 32-KiB blocks, slabs of 128 x 50, a padding tile twice as large), either first."""
    cases = [("grow_k40", small_problem(70, 100, 40), step("bf16x3", BOTH, 8, 512)),
             ("grow_k100", small_problem(70, 50, 100), step("bf16x3", BOTH, 8, 256))]
    if order == "k100_then_k40":
        cases.reverse()
    ctx = pkg.Context(0)
    got = []
    try:
        for key, p, st in cases:
            to_context(p, ctx)
            got.append(run_step(ctx, p, st, f"{order}: {key}"))
    finally:
        ctx.close()
    for (key, p, st), r in zip(cases, got):
        assert_bitwise(r, solo(pkg, key, p, st), f"{order}: {key}")
        assert_oracle(r, oracle(key, p, st), f"{order}: {key}")


# ---- the sequence of the report: whole epochs through pmf_fit, batch layers, M below one panel --------------------------
def snapshot(ctx, p):
    """The problem with the context's current parameters."""
    q = dict(p)
    q["X"], q["Y"] = ctx.get_factors()
    q["logsigma"], q["mu"] = ctx.get_col_params()
    q["batch_views"] = []
    for v, b in enumerate(p["batch_views"]):
        ld, th = ctx.get_batch_view(v)
        q["batch_views"].append(dict(b, logdelta=ld, theta=th))
    return q


def fit_epoch(ctx, prec, flags):
    ctx.set_precision(prec)
    ctx.set_optimizer("adagrad", lr=0.05)   # (resets the optimizer state: the epoch depends on the parameters alone)
    r = ctx.fit(max_epochs=1, abs_tol=0, rel_tol=0, **flags)
    X, Y = ctx.get_factors()
    return dict(loss=r["loss"], term=r["term_code"], X=X, Y=Y)


def check_epoch(pkg, ctx, p, prec, flags, fam, where):
    """One checked pmf_fit epoch from the context's current parameters.  The epoch's loss is the loss at those parameters:
    it is compared with the oracle's there; the stepped factors with the same epoch on a fresh context."""
    start = snapshot(ctx, p)
    ctx.set_precision(prec)
    assert_fits(ctx.pass_extents(**xy(flags)), where + " (planned)")
    got = fit_epoch(ctx, prec, flags)
    assert ctx.last_kernel() == fam, (where, ctx.last_kernel(), fam)
    assert_fits(ctx.pass_extents(**xy(flags)), where + " (after the epoch)")
    alone = pkg.Context(0)
    try:
        to_context(start, alone)
        want = fit_epoch(alone, prec, flags)
    finally:
        alone.close()
    assert got["term"] == want["term"] and np.array_equal(got["loss"], want["loss"]), (where, got["loss"], want["loss"])
    assert np.array_equal(got["X"], want["X"]) and np.array_equal(got["Y"], want["Y"]), f"{where}: factors differ from a fresh context's"
    lo, _ = to_oracle(start).loss_and_grads(**flags)
    assert len(got["loss"]) == 1 and abs(got["loss"][0] - lo) <= LOSS_RTOL * abs(lo) + 1e-6, (where, got["loss"], lo)


def test_reported_sequence(pkg):
    """ADVICE (round 3): 70 x 100 at K = 40, then 33 x 65 at K = 100 on the same context, one batch view of two feature views
    (columns outside every batch view), 10 % missing: one f32 epoch with both gradients and column layers, then one bf16x3
    epoch with both gradients -- sb8 with batch layers below one row panel, on gX slots sized by the f32 epoch.  After the
    two epochs the gradients of one more sb8 pass are compared with the oracle and with a fresh context."""
    ctx = pkg.Context(0)
    try:
        for M, N, K in ((70, 100, 40), (33, 65, 100)):
            p = make_problem(M=M, N=N, K=K, seed=7, n_views=2, batch_views=1, n_batches=3, nan_frac=0.1, xreg="composite",
                             col_params=True, random_init=True)
            where = f"{M} x {N}, K = {K}"
            to_context(p, ctx)
            check_epoch(pkg, ctx, p, "f32", dict(BOTH, update_col_layers=True), 0, where + ": f32 epoch")
            check_epoch(pkg, ctx, p, "bf16x3", BOTH, 8, where + ": bf16x3 epoch")
            assert ctx.last_path()["bmode"] == 1
            now = snapshot(ctx, p)
            st = step("bf16x3", BOTH, 8, 512 if K <= 64 else 256)
            r = run_step(ctx, now, st, where + ": gradients")
            assert_bitwise(r, solo(pkg, where, now, st), where + ": gradients")
            assert_oracle(r, oracle(where, now, st), where + ": gradients")
    finally:
        ctx.close()


# ---- plan only: a seeded walk over shapes, K, precisions, gradient flags and batch views --------------------------------
WALK_SEED = 2052


def walk(pkg, seed, steps=100):
    rng = np.random.default_rng(seed)
    ctx = pkg.Context(0)
    fams = set()
    try:
        M = N = K = 0
        for i in range(steps):
            if i == 0 or rng.random() < 0.2:
                M, N = int(rng.integers(1, 601)), int(rng.integers(1, 201))
                D = rng.standard_normal((M, N)).astype(np.float32)
                D[rng.random((M, N)) < 0.05] = np.nan
                ctx.set_data(np.asfortranarray(D))
                K = 0
            if K == 0 or rng.random() < 0.3:
                K = int(rng.choice([20, 40, 80, 100]))
                ctx.set_factors(rng.standard_normal((K, M)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32))
            ctx.set_precision(str(rng.choice(["f32", "bf16x3"])))
            if rng.random() < 0.5:
                Nv = max(1, N // 2)
                bor = np.sort(rng.integers(0, 3, size=M)).astype(np.int32)
                ctx.set_batch_views([dict(start1=1, stop1=Nv, batch_of_row=bor, logdelta=np.zeros((3, Nv), np.float32),
                                          theta=np.zeros((3, Nv), np.float32))])
            else:
                ctx.set_batch_views([])
            flags = [dict(update_X=True, update_Y=True), dict(update_X=True), dict(update_Y=True), dict()][int(rng.integers(0, 4))]
            ext = ctx.pass_extents(**xy(flags))
            assert_fits(ext, f"step {i}: {M} x {N}, K = {K}, {ctx.get_precision()[0]}, {sorted(flags)}")
            fams.add((ext["xsb"]["need"] > 0, ext["btd"]["need"] > 0, ext["gx_part"]["need"] > 0))
    finally:
        ctx.close()
    assert len(fams) == 8   # split and exact families, with and without the batch table, with and without gX


def test_planned_extents_over_a_random_walk(pkg):
    """100 steps on one fresh context, no data pass launched: each step redraws some of (data shape 1..600 x 1..200, K of 20,
    40, 80, 100, precision, gradient flags, batch views) and keeps the others, so that consecutive steps often share a cached
    work split, and asks for the extents of the pass it would run.  Every step is a host computation and a small upload.  The
    seed is one whose walk meets the gX-slot collision of the sequences above (9 of the 150 seeds from 2026 on do, and draw
    every kind of family besides): with the slots sized only when the split is recomputed it stops at step 5, 129 x 76 at
    K = 20 in f32 with both gradients after the batch view is dropped, 196608 bytes of gx_part needed and 98304 allocated."""
    walk(pkg, WALK_SEED)


# ---- the guard ---------------------------------------------------------------------------------------------------------
def test_guard_refuses_a_short_buffer_and_names_it(pkg):
    """The comparison every data pass makes before its first launch, on capacities made up through the test-only argument of
    the debug entry (no buffer is really short, nothing is launched): it fails with the buffer's name, its need and the
    capacity, and leaves the context as it was."""
    p = problem("kb2")
    st = step("bf16x3", BOTH, 8, 512)
    ctx = pkg.Context(0)
    try:
        to_context(p, ctx)
        first = run_step(ctx, p, st, "guard: before")
        ext = ctx.pass_extents(**BOTH)
        for name in ("gx_part", "gy_slabs", "xsb", "ysb", "tflags", "loss_partial"):
            need = ext[name]["need"]
            assert need > 0, name
            with pytest.raises(pkg.PMFError) as e:
                ctx.pass_extents(capacity_override={name: need - 1}, **BOTH)
            msg = str(e.value)
            assert name in msg and str(need) in msg and str(need - 1) in msg, msg
            same = ctx.pass_extents(capacity_override={name: need}, **BOTH)   # exactly enough is enough
            assert same[name] == dict(need=need, capacity=need)
        with pytest.raises(pkg.PMFError):
            ctx.pass_extents(capacity_override={"no_such_buffer": 1}, **BOTH)
        assert ctx.pass_extents(**BOTH) == ext
        assert_bitwise(run_step(ctx, p, st, "guard: after"), first, "guard: after the refusals")
    finally:
        ctx.close()
