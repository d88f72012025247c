"""Problems at the edges of the threshold pass's geometry (include/pmf_hip_thresholds.h), and the
faults a kernel could have there, restated on the float64 reference (tests/threshold_ref.py).  Plain numpy.

The pass works on the host's list of 32-column tiles that hold a kind-3 column; a unit is one tile x one of R ranges of row
panels (32 rows x 8 waves at K <= 64, x 4 above).  Layouts A and B of tests/hinge_ref.py have a kind-3 column in every tile,
triples with one or two finite values, at most 6 batches per view, 3 groups of at most 55 columns.  Here:

  C  N = 200, tiles 0..6 (the last ragged), kind-3 columns in tiles 1, 3, 4 and 6 only -- tile 4 holds two of them, the ragged
     tile is the list's entry 3 -- a full triple (-1, 0, 1), and two batch views (columns 50-120 and 125-195, scrambled rows,
     some in no batch) that leave kind-3 columns 41-49, 121-124 and 196-200 outside every view.  "narrow": 4 and 6 batches;
     "wide": 20 and 6, a dense batch table of 32 slots per column and the WIDE instances of the kernel.
  D  M = 70, K = 20, N = 800: groups of 520 and 257 columns (k_thresh_groups adds 3 and 2 columns per thread, with a partial
     last thread and idle ones).
  E  M = 70, K = 20, N = 350: 70 groups of 5 columns cycling through the three kinds of triple (k_thresh_step's second
     workgroup).

Built like the layouts of hinge_ref (layout_from), seeds 2000 + K, every finite threshold then raised by SHIFT = 0.4
(test_threshold_cases.problem: away from the stationary point the data were drawn at).  Every builder is cached: the problems
are shared between tests and must not be modified."""
import functools

import numpy as np

import batch_cases as bc
import hinge_ref as hr
import threshold_ref as tr

INF = np.inf
SHIFT = 0.4
FULL = (-1.0, 0.0, 1.0)
ORD = (-INF, -0.5, 0.5)
BER = (0.0, INF, INF)
LAYOUT_C = [((1, 40), "normal", None), ((41, 60), 3, FULL), ((61, 100), "bernoulli", None), ((101, 130), 3, ORD),
            ((131, 192), "normal", None), ((193, 200), 3, BER)]
C_TILES = [1, 3, 4, 6]
C_VIEWS = ((50, 120), (125, 195))
C_BATCHES = {"narrow": (4, 6), "wide": (20, 6)}
C_UNVIEWED = ((41, 49), (121, 124), (196, 200))          # the kind-3 columns outside every view
LAYOUT_D = [((1, 520), 3, ORD), ((521, 777), 3, BER), ((778, 800), "normal", None)]
LAYOUT_E = [((5 * g + 1, 5 * g + 5), 3, (FULL, ORD, BER)[g % 3]) for g in range(70)]


def shifted(p):
    tg = tr.group_thresholds(p)
    return tr.with_thresholds(p, np.where(np.isfinite(tg), tg + SHIFT, tg))


def waves(K):
    return 8 if K <= 64 else 4


def panels(M, K):
    """Row panels of the pass at M rows: 32 rows per wave."""
    return -(-M // (32 * waves(K)))


def tiles_of(p):
    return sorted({int(j) // 32 for j in np.flatnonzero(hr.kinds_of(p) == 3)})


def unbatch(bor, n):
    """n rows spread over the whole height taken out of every batch, each from a batch that other rows hold too."""
    cnt, left = np.bincount(bor), n
    for i in range(1, len(bor), len(bor) // n - 1):
        if left and cnt[bor[i]] >= 2:
            cnt[bor[i]] -= 1
            bor[i] = -1
            left -= 1
    assert left == 0
    return bor


@functools.lru_cache(maxsize=None)
def layout_c(K, M=70, variant=None):
    """Layout C; variant None (no batch views), "narrow" or "wide"."""
    def views(M, N, rng):
        out = []
        for (s, e), nb in zip(C_VIEWS, C_BATCHES[variant]):
            out.append((s, e, unbatch(bc.scrambled_rows(M, nb, rng), 5), nb))
        return out

    p = shifted(hr.layout_from(LAYOUT_C, M, K, 2000 + K, views if variant else None))
    assert tiles_of(p) == C_TILES
    return p


@functools.lru_cache(maxsize=None)
def layout_d():
    return shifted(hr.layout_from(LAYOUT_D, 70, 20, 2020))


@functools.lru_cache(maxsize=None)
def layout_e():
    return shifted(hr.layout_from(LAYOUT_E, 70, 20, 2020))


@functools.lru_cache(maxsize=None)
def many_batches_255(K=128, M=600):
    """Layout C, narrow, whose first view has 255 batches (ids 0..254, every one present, scrambled over the rows): a dense
    table of 256 slots per column, the batch index an unsigned char up to 254 and the identity slot 255."""
    def views(M, N, rng):
        b0 = unbatch(bc.scrambled_rows(M, 255, rng), 5)
        b1 = bc.scrambled_rows(M, 6, rng)
        return [(C_VIEWS[0][0], C_VIEWS[0][1], b0, 255), (C_VIEWS[1][0], C_VIEWS[1][1], b1, 6)]

    p = shifted(hr.layout_from(LAYOUT_C, M, K, 2255 + K, views))
    assert set(range(255)) <= set(p["batch_views"][0]["batch_of_row"].tolist())
    return p


def with_views(p, nbs, seed=7):
    """The batch views of p replaced by scrambled ones of nbs[v] batches over the same columns (a copy)."""
    rng = np.random.default_rng(seed)
    q = dict(p)
    q["batch_views"] = []
    for v, nb in zip(p["batch_views"], nbs):
        w = v["stop1"] - v["start1"] + 1
        q["batch_views"].append(dict(start1=v["start1"], stop1=v["stop1"], batch_of_row=bc.scrambled_rows(p["M"], nb, rng),
                                     logdelta=(0.25 * rng.standard_normal((nb, w))).astype(np.float32),
                                     theta=(0.25 * rng.standard_normal((nb, w))).astype(np.float32)))
    return q


# ---- the cascade: a full triple whose two upper thresholds both land below the lowest ----------------------------------
CASCADE_TRIPLE = (-1.2, 0.4, 1.0)
CASCADE_OPT = dict(adagrad=dict(kind="adagrad", lr=1.2, eps=1e-8, beta1=0.9, beta2=0.999),
                   adam=dict(kind="adam", lr=1.2, eps=1e-8, beta1=0.9, beta2=0.999))


@functools.lru_cache(maxsize=None)
def cascade_problem():
    """Layout C, narrow, K = 20, whose first group (the full triple, drawn at (-1, 0, 1)) holds CASCADE_TRIPLE: t0 too low,
    t1 and t2 too high and less than 2.4 above t0 (found by a scan of the
    reference's gradient signs over a grid of triples).  The first AdaGrad or Adam step is nearly lr sign(g) on each, so with
    lr = 1.2 t0 rises by 1.2 and t1, t2 fall by 1.2, both below the new t0: the clamp moves t1, then t2."""
    p = dict(layout_c(20, 70, "narrow"))
    p["noise_thr"] = list(p["noise_thr"])
    p["noise_thr"][1] = CASCADE_TRIPLE
    return p


# ---- the faults ----------------------------------------------------------------------------------------------------------
def later_panels_dropped(p, R):
    """Only the first row panel of each of the R row ranges contributes (running sums not carried along the sweep)."""
    rows, n_rp = 32 * waves(p["K"]), panels(p["M"], p["K"])
    keep = np.zeros(p["M"], bool)
    for rr in range(R):
        lo = rr * n_rp // R
        keep[lo * rows:(lo + 1) * rows] = True
    q = dict(p)
    q["D"] = np.asfortranarray(np.where(keep[:, None], p["D"], np.nan).astype(np.float32))
    return q


def tile_identity(p):
    """The data of the list's entry ti are read in place of those of tile tiles[ti] (columns past N: nothing observed)."""
    D = np.array(p["D"], np.float32)
    src = np.full((p["M"], 32 * (-(-p["N"] // 32))), np.nan, np.float32)
    src[:, :p["N"]] = p["D"]
    for ti, ct in enumerate(tiles_of(p)):
        n = min(32, p["N"] - 32 * ct)
        D[:, 32 * ct:32 * ct + n] = src[:, 32 * ti:32 * ti + n]
    q = dict(p)
    q["D"] = np.asfortranarray(D)
    return q


def unviewed_as_view0(p):
    """A kind-3 column outside every view takes delta and theta of its row's batch in view 0 (of view 0's column at the same
    offset into the run, modulo the view's width): extra views over those runs, with view 0's rows."""
    v0 = p["batch_views"][0]
    w0 = v0["stop1"] - v0["start1"] + 1
    q = dict(p)
    q["batch_views"] = list(p["batch_views"])
    covered = np.zeros(p["N"], bool)
    for v in p["batch_views"]:
        covered[v["start1"] - 1:v["stop1"]] = True
    cols = np.flatnonzero((hr.kinds_of(p) == 3) & ~covered)
    assert cols.size
    for run in np.split(cols, np.flatnonzero(np.diff(cols) > 1) + 1):
        idx = np.arange(run.size) % w0
        q["batch_views"].append(dict(start1=int(run[0]) + 1, stop1=int(run[-1]) + 1, batch_of_row=v0["batch_of_row"],
                                     logdelta=np.ascontiguousarray(v0["logdelta"][:, idx]),
                                     theta=np.ascontiguousarray(v0["theta"][:, idx])))
    return q


def wide_as_16(p):
    """The batch index wrapped mod 16 (a WIDE table read with the narrow kernel's 4-bit index)."""
    q = dict(p)
    q["batch_views"] = [dict(v, batch_of_row=np.where(np.asarray(v["batch_of_row"]) >= 0, np.asarray(v["batch_of_row"]) % 16,
                                                      -1).astype(np.int32)) for v in p["batch_views"]]
    return q


def group_tail_dropped(p):
    """(groups, 3): only the first 256 columns of a group are added."""
    gc = tr.col_grad(p)
    return np.array([gc[s - 1:min(e, s - 1 + 256)].sum(0) for s, e in tr.groups_of(p)], np.float64).reshape(-1, 3)
