"""Problems at the batch-table edges of the fused data pass, and the selection rules restated (no GPU needed).

With batch layers a fused kernel family keeps a 32-column x 16-slot {delta, theta} table in LDS.  Slots are local to a
(row panel of the family's height BM, view): ensure_panel_slots (csrc/pmf_pass.hip) gives every distinct batch of the panel
one of the slots 0..14 and every row in no batch the identity slot 15.  A family therefore fits when no (panel, view) meets
more than 15 batches and its LDS has room for the views (max_bv); fused_geometry walks

    bf16x3, K <= 32       sb  (1, BM 256)                                 -> exact (BM 256)
    bf16x3, 32 < K <= 64  sb8 (8, BM 512, both gradients, max_bv 5) -> sb2 (2, BM 256) -> exact (BM 256)
    bf16x3, 64 < K <= 96  sb4 (4, BM 128)                                 -> exact (BM 128)
    bf16x3, 96 < K <= 128 sb8 (8, BM 256, both gradients) -> sb4 (4, BM 128) -> exact (BM 128)
    f32                   exact (BM 256 at K <= 64, 128 above)

and the exact kernel, where its own panels do not fit either, gathers {delta, theta} per entry (bmode 2).  The dense
[column][slots] table that all of them read has slots = the power of two >= max(16, nb_max + 1); from 256 batches on there
is none, and only bmode 2 is left.

The builders start from make_problem (mixed noise, column weights and parameters, 5 % missing entries) and replace its
batch views, so D does not follow the batch effects and residuals are O(0.3), as in tests/test_gpu_layer_edges.py.  Factor
scale: 0.4 at every K, the value tests/test_gpu_edges.py::data_kw uses above K = 64 and its mixed-noise cases use at every
K.  (data_kw's 1.0 at K <= 64 is for Gaussian columns: with Poisson columns z has a standard deviation of sqrt(K), exp(z)
reaches 1e10 and the max-norm of the gradients, the denominator of rel_err, would leave every other entry unchecked -- the
sensitivity condition of tests/test_batch_cases.py cannot hold there.)  For the same reason Y is scaled down on the Poisson
columns until z1 has a standard deviation of POISSON_SD = 0.5 there, and their counts are drawn from that z: at 0.4 and
K = 128 a few e^z entries still set the max-norm and a row in the wrong batch moved the gradients by 1e-5 of it.

Every builder is cached: the problems are shared between tests and must not be modified.
"""
import copy
import functools

import numpy as np

from problems import factor_scales, make_problem, to_oracle

GRADS = {"both": dict(update_X=True, update_Y=True), "X": dict(update_X=True), "Y": dict(update_Y=True)}
BOTH = GRADS["both"]

# (precision, K, gradients) -> (family, BM) without batch trouble; read off the family table of fused_geometry
PATHS = {
    ("f32", 20, "both"): (0, 256),
    ("f32", 48, "both"): (0, 256),
    ("f32", 80, "both"): (0, 128),
    ("f32", 128, "both"): (0, 128),
    ("bf16x3", 20, "both"): (1, 256),
    ("bf16x3", 48, "both"): (8, 512),
    ("bf16x3", 80, "both"): (4, 128),
    ("bf16x3", 128, "both"): (8, 256),
    ("bf16x3", 48, "X"): (2, 256),
    ("bf16x3", 128, "Y"): (4, 128),
}


def path_id(path):
    return f"{path[0]}-k{path[1]}-{path[2]}"


# ---- the selection rules, restated -----------------------------------------------------------------------------------
def dense_slots(nb_max):
    """Slots per column of the dense batch table; 0: no table (256 batches or more)."""
    if nb_max > 255:
        return 0
    s = 16
    while s < nb_max + 1:
        s *= 2
    return s


def family_chain(K, prec, both):
    """[(family, BM, max_bv)] in the order fused_geometry tries them; the exact kernel is last."""
    KB = (K + 31) // 32
    assert 1 <= KB <= 4
    chain = []
    if prec == "bf16x3":
        if KB == 1:
            chain = [(1, 256, 16)]
        elif KB == 2:
            chain = ([(8, 512, 5)] if both else []) + [(2, 256, 16)]
        elif KB == 3:
            chain = [(4, 128, 16)]
        else:
            chain = ([(8, 256, 16)] if both else []) + [(4, 128, 16)]
    return chain + [(0, 256 if KB <= 2 else 128, 16)]


def expected_batch_path(K, prec, both, n_bv, panel_counts, nb_max):
    """(family, BM, bmode, slots) of a data pass with n_bv >= 1 batch views.  panel_counts(BM): the largest number of
    distinct non-negative batches any (panel of BM rows, view) meets; nb_max: the largest batch count of a view."""
    assert n_bv >= 1
    slots = dense_slots(nb_max)
    chain = family_chain(K, prec, both)
    if slots:
        for fam, BM, max_bv in chain:
            if n_bv <= max_bv and panel_counts(BM) <= 15:
                return fam, BM, 1, slots
    return 0, chain[-1][1], 2, slots


def panel_counts_of(p):
    """BM -> the largest number of distinct non-negative batches over every (panel of BM rows, view) of problem p."""
    def counts(BM):
        worst = 0
        for bv in p["batch_views"]:
            bor = np.asarray(bv["batch_of_row"])
            for i0 in range(0, len(bor), BM):
                b = bor[i0:i0 + BM]
                worst = max(worst, len(np.unique(b[b >= 0])))
        return worst
    return counts


def nb_max_of(p):
    return max(np.asarray(bv["logdelta"]).shape[0] for bv in p["batch_views"])


def expected_of(p, path):
    prec, K, gname = path
    assert K == p["K"]
    return expected_batch_path(K, prec, gname == "both", len(p["batch_views"]), panel_counts_of(p), nb_max_of(p))


# ---- builders --------------------------------------------------------------------------------------------------------
SCALE = 0.4
POISSON_SD = 0.5


def batch_problem(M, N, K, seed, views, nan_frac=0.05, bernoulli_frac=0.2, poisson_frac=0.1):
    """views: (start1, stop1, batch_of_row, nb) per batch view.  logdelta and theta are drawn as make_problem draws them:
    a centre per batch (two batches differ by O(0.3) in z) plus per-(batch, column) scatter."""
    p = make_problem(M=M, N=N, K=K, seed=seed, bernoulli_frac=bernoulli_frac, poisson_frac=poisson_frac, nan_frac=nan_frac,
                     weights=True, col_params=True, scale=SCALE)
    rng = np.random.default_rng(seed + 1)
    for (s, e), kd in zip(p["noise_ranges"], p["noise_kinds"]):
        if kd == "poisson":       # sd(z1) = POISSON_SD on the Poisson columns, and counts drawn from that z
            sl = slice(s - 1, e)
            Y = p["Y"].copy()
            Y[:, sl] *= POISSON_SD / (SCALE * SCALE * np.sqrt(K))
            p["Y"] = np.asfortranarray(Y)
            z = p["X"].astype(np.float64).T @ Y[:, sl].astype(np.float64) * np.exp(p["logsigma"][sl].astype(np.float64))
            z += p["mu"][sl].astype(np.float64)
            D = p["D"].copy()
            D[:, sl] = np.where(np.isnan(D[:, sl]), np.nan, rng.poisson(np.exp(np.clip(z, -5, 3))))
            p["D"] = np.asfortranarray(D.astype(np.float32))
    bvs = []
    for s, e, bor, nb in views:
        cd = rng.standard_normal(nb)[:, None] * 0.25
        ct = rng.standard_normal(nb)[:, None] * 0.25
        bvs.append(dict(start1=int(s), stop1=int(e), batch_of_row=np.asarray(bor, np.int32),
                        logdelta=(cd + 0.25 * rng.standard_normal((nb, e - s + 1))).astype(np.float32),
                        theta=(ct + 0.25 * rng.standard_normal((nb, e - s + 1))).astype(np.float32)))
    p["batch_views"] = bvs
    return p


def sorted_rows(M, nb, first=0):
    """M rows in nb contiguous batches first..first+nb-1 of (almost) equal size."""
    return (first + np.arange(M) * nb // M).astype(np.int32)


def scrambled_rows(M, nb, rng):
    """Every batch non-empty, rows in random order."""
    return rng.permutation(np.concatenate([np.arange(nb), rng.integers(0, nb, size=M - nb)])).astype(np.int32)


@functools.lru_cache(maxsize=None)
def slots_edge(BM, K, n, mirror=False):
    """slots15 / slots16 (n = 15, 16): M = BM + n, one view over all 33 columns.  The first panel holds 3 sorted batches,
    every row of the ragged last panel is a batch of its own: n = 15 uses slot 14, next to the identity slot; n = 16 does
    not fit.  mirror: the n one-row batches are the top rows of the first panel, whose other rows are in no batch (they
    take the identity slot right after slot 14), and the 3 sorted batches fill the last panel."""
    M, N = BM + n, 33
    if mirror:
        bor = np.concatenate([np.arange(n), np.full(BM - n, -1), sorted_rows(n, 3, first=n)])
    else:
        bor = np.concatenate([sorted_rows(BM, 3), 3 + np.arange(n)])
    return batch_problem(M, N, K, seed=100 + n + K + BM + (7 if mirror else 0), views=[(1, N, bor, n + 3)])


@functools.lru_cache(maxsize=None)
def halves_fit(BM, K):
    """M = BM: rows 0 .. BM/2 - 1 in batches 0..7, the rest in 8..15.  The BM-row panel meets 16 batches, each half 8."""
    M, N = BM, 33
    bor = np.concatenate([sorted_rows(BM // 2, 8), sorted_rows(BM // 2, 8, first=8)])
    return batch_problem(M, N, K, seed=200 + K + BM, views=[(1, N, bor, 16)])


@functools.lru_cache(maxsize=None)
def unbatched(BM, K):
    """M = 2 BM + 33, two views.  View 0: 4 sorted batches in the first panel, the whole second panel and rows 0, BM - 1,
    BM and M - 1 in no batch, batches 5 and 6 in the last panel, batch 4 held by no row.  View 1: one batch, no row in it."""
    M, N = 2 * BM + 33, 70
    bor = np.concatenate([sorted_rows(BM, 4), np.full(BM, -1), sorted_rows(33, 2, first=5)])
    bor[[0, BM - 1, BM, M - 1]] = -1
    return batch_problem(M, N, K, seed=300 + K + BM, views=[(1, 40, bor, 7), (45, 70, np.full(M, -1), 1)])


SEAM_VIEWS = ((3, 10), (11, 11), (20, 40), (42, 75))


@functools.lru_cache(maxsize=None)
def view_seams(BM, K, N=75):
    """Batch views (3,10), (11,11), (20,40), (42,N): two leading columns in no view, a one-column view, three views in
    tile 0, gaps at columns 12-19 and 41, a seam inside tile 1, the last view ending in the ragged last tile.  M = BM + 33;
    rows sorted in views 0 and 2 (4 and 6 batches), scrambled with 15 batches in views 1 and 3."""
    M = BM + 33
    rng = np.random.default_rng(400 + K + BM + N)
    rngs = SEAM_VIEWS[:3] + ((SEAM_VIEWS[3][0], N),)
    rows = [(sorted_rows(M, 4), 4), (scrambled_rows(M, 15, rng), 15), (sorted_rows(M, 6), 6), (scrambled_rows(M, 15, rng), 15)]
    return batch_problem(M, N, K, seed=400 + K + BM + N, views=[(s, e, b, nb) for (s, e), (b, nb) in zip(rngs, rows)])


VIEW_WIDTHS = (2, 6, 3, 2, 4, 2, 5, 3, 2, 6, 2, 3, 4, 2, 3, 2)


def many_view_ranges(n, N=70):
    """n views of 2-6 columns from column 2 on, spread over the N columns with gaps of base + (1, -1, 0, ...) columns."""
    w = VIEW_WIDTHS[:n]
    base = (N - 2 - sum(w)) // max(n - 1, 1)
    assert base >= 1
    out, s = [], 2
    for v in range(n):
        out.append((s, s + w[v] - 1))
        s += w[v] + base + (1, -1, 0)[v % 3]
    assert out[-1][1] <= N
    return out


@functools.lru_cache(maxsize=None)
def many_views(BM, K, n=16):
    """views16 (views5, views6): N = 70, n batch views of 2-6 columns with gaps; nb alternates between 1 (every row in
    batch 0), 6 (sorted) and 15 (scrambled).  M = BM + 33."""
    M, N = BM + 33, 70
    rng = np.random.default_rng(500 + K + BM + n)
    views = []
    for v, (s, e) in enumerate(many_view_ranges(n, N)):
        nb = (1, 6, 15)[v % 3]
        bor = np.zeros(M, np.int32) if nb == 1 else (sorted_rows(M, 6) if nb == 6 else scrambled_rows(M, 15, rng))
        views.append((s, e, bor, nb))
    return batch_problem(M, N, K, seed=500 + K + BM + n, views=views)


@functools.lru_cache(maxsize=None)
def gather(K):
    """Scrambled rows with 20 batches in view 0 (no panel fits: per-entry gathers), 6 sorted batches and a few rows in no
    batch in view 1.  M = 128 + 33, N = 95."""
    M, N = 128 + 33, 95
    rng = np.random.default_rng(600 + K)
    b1 = sorted_rows(M, 6)
    b1[[0, 31, 32, 127, 128, M - 1]] = -1
    return batch_problem(M, N, K, seed=600 + K, views=[(1, 40, scrambled_rows(M, 20, rng), 20), (50, N, b1, 6)])


@functools.lru_cache(maxsize=None)
def many_batches(nb):
    """nb255 / nb256: nb sorted batches of 20 rows (a 256-row panel meets at most 14), one view, N = 33, K = 20."""
    M, N, K = 20 * nb, 33, 20
    return batch_problem(M, N, K, seed=700 + nb, views=[(1, N, np.arange(M) // 20, nb)])


WALK_M_SB8_512 = 2049 + 2 * 512   # rows at which the 512-row sb8 has more pieces than a 256-workgroup grid (250, 256, 280 pieces at 2049, 2561, 3073)


@functools.lru_cache(maxsize=None)
def walk(K, M=2049):
    """M x 2048, 40 sorted batches in each of two views that meet inside a tile (columns 1..1000 and 1001..2048; the
    batches of the second view are cut elsewhere than those of the first), 2 % missing entries, Bernoulli columns.  Every
    row panel meets other batches, so a workgroup that walks several pieces re-stages its slot map."""
    N = 2048
    b1 = np.minimum((np.arange(M) + 13) * 40 // M, 39)                          # every cut 13 rows earlier
    return batch_problem(M, N, K, seed=800 + K, views=[(1, 1000, sorted_rows(M, 40), 40), (1001, N, b1, 40)],
                         nan_frac=0.02, bernoulli_frac=0.1, poisson_frac=0.0)


@functools.lru_cache(maxsize=None)
def cache_states():
    """Three states of one model (K = 48, 700 x 95, two sorted batch views): A; B = A with the rows' batches in reverse
    order (same nb, same ranges); C = B with new theta and logdelta."""
    M, N, K = 700, 95, 48
    a = batch_problem(M, N, K, seed=900, views=[(1, 40, sorted_rows(M, 12), 12), (50, N, sorted_rows(M, 9), 9)])
    b = copy.deepcopy(a)
    for bv in b["batch_views"]:
        bv["batch_of_row"] = np.ascontiguousarray(bv["batch_of_row"][::-1])
    c = copy.deepcopy(b)
    rng = np.random.default_rng(901)
    for bv in c["batch_views"]:
        bv["theta"] = (bv["theta"] + 0.2 * rng.standard_normal(bv["theta"].shape)).astype(np.float32)
        bv["logdelta"] = (bv["logdelta"] + 0.2 * rng.standard_normal(bv["logdelta"].shape)).astype(np.float32)
    return a, b, c


# name -> builder(BM, K) of the cases that run on every path
EVERY_PATH = {
    "slots15": lambda BM, K: slots_edge(BM, K, 15),
    "slots16": lambda BM, K: slots_edge(BM, K, 16),
    "slots15_mirror": lambda BM, K: slots_edge(BM, K, 15, mirror=True),
    "slots16_mirror": lambda BM, K: slots_edge(BM, K, 16, mirror=True),
    "unbatched": unbatched,
    "view_seams": view_seams,
    "views16": many_views,
}


def all_cases():
    """[(id, problem builder, path or None, BM the case was built for)]: every problem the GPU file runs."""
    out = []
    for path, (fam, BM) in PATHS.items():
        K = path[1]
        for name, fn in EVERY_PATH.items():
            out.append((f"{name}-{path_id(path)}", functools.partial(fn, BM, K), path, BM))
    out.append(("halves_fit-bf16x3-k48-both", functools.partial(halves_fit, 512, 48), ("bf16x3", 48, "both"), 512))
    out.append(("halves_fit-bf16x3-k128-both", functools.partial(halves_fit, 256, 128), ("bf16x3", 128, "both"), 256))
    for n in (5, 6):
        out.append((f"views{n}-bf16x3-k48-both", functools.partial(many_views, 512, 48, n), ("bf16x3", 48, "both"), 512))
    for K in (80, 128):
        out.append((f"gather-f32-k{K}-both", functools.partial(gather, K), ("f32", K, "both"), 128))
    for nb in (255, 256):
        for prec in ("f32", "bf16x3"):
            out.append((f"nb{nb}-{prec}-k20-both", functools.partial(many_batches, nb), (prec, 20, "both"), 256))
    out.append(("view_seams161-f32-k48-both", functools.partial(view_seams, 256, 48, 161), ("f32", 48, "both"), 256))
    out.append(("view_seams161-bf16x3-k48-both", functools.partial(view_seams, 512, 48, 161), ("bf16x3", 48, "both"), 512))
    out.append(("walk-f32-k64-both", functools.partial(walk, 64), ("f32", 64, "both"), 256))
    out.append(("walk-bf16x3-k64-both", functools.partial(walk, 64), ("bf16x3", 64, "both"), 512))
    out.append(("walk3073-bf16x3-k64-both", functools.partial(walk, 64, WALK_M_SB8_512), ("bf16x3", 64, "both"), 512))
    out.append(("walk-bf16x3-k128-both",functools.partial(walk, 128), ("bf16x3", 128, "both"), 256))
    for i, s in enumerate("ABC"):
        out.append((f"cache_state{s}-bf16x3-k48-both", functools.partial(lambda i: cache_states()[i], i),
                    ("bf16x3", 48, "both"), 512))
    return out


# ---- the fp64 oracle, once per problem -------------------------------------------------------------------------------
_ORACLE = {}


def oracle_of(p):
    """fp64 data loss, gX and gY of problem p (cached by identity: the builders above return shared objects)."""
    key = id(p)
    if key not in _ORACLE:
        _, go = to_oracle(p).loss_and_grads(**BOTH)
        _ORACLE[key] = (p, dict(data_loss=go["data_loss"], X=go["X"], Y=go["Y"]))
    return _ORACLE[key][1]


_SCALES = {}


def scales_of(p):
    """problems.factor_scales(p), once per problem (cached by identity, like oracle_of)."""
    if id(p) not in _SCALES:
        _SCALES[id(p)] = (p, factor_scales(p))
    return _SCALES[id(p)][1]


# ---- mutants for the sensitivity condition ---------------------------------------------------------------------------
def mutants(p, BM):
    """{name: problem}: (a) one batched row moved to another batch its BM-row panel meets, (b) one row in no batch given
    batch 0, (c) one view boundary moved by one column -- each on the first view and row where it applies."""
    out = {}
    for v, bv in enumerate(p["batch_views"]):
        bor = np.asarray(bv["batch_of_row"])
        if "a" not in out:
            for i0 in range(0, len(bor), BM):
                blk = bor[i0:i0 + BM]
                ids = np.unique(blk[blk >= 0])
                if len(ids) >= 2:
                    idx = np.flatnonzero(blk >= 0)
                    i = i0 + int(idx[len(idx) // 2])                 # the middle one of the panel's batched rows
                    q = copy.deepcopy(p)
                    q["batch_views"][v]["batch_of_row"][i] = ids[-1] if bor[i] != ids[-1] else ids[0]
                    out["a"] = q
                    break
        if "b" not in out and (bor < 0).any():
            q = copy.deepcopy(p)
            q["batch_views"][v]["batch_of_row"][int(np.argmax(bor < 0))] = 0
            out["b"] = q
        if "c" not in out and bv["stop1"] > bv["start1"]:
            q = copy.deepcopy(p)
            qv = q["batch_views"][v]
            qv["stop1"] -= 1
            qv["logdelta"] = np.ascontiguousarray(qv["logdelta"][:, :-1])
            qv["theta"] = np.ascontiguousarray(qv["theta"][:, :-1])
            out["c"] = q
    return out
