"""CPU guard of postprocess_cases.EDGE_SHAPES / EDGE_VIEWS, the table that tests/test_gpu_postprocess_edges.py runs on the
device: the geometry of csrc/pmf_postprocess.hip is read from its source text (the piece length, the K thresholds of the
template classes, the tile widths of the in-place kernels, Kp from pmf_hip.hip) and every shape is held to the seam it is in
the table for, so that a changed constant or an edited shape fails here instead of quietly testing something else.  On the
oracle alone: every view has c > 0, reorder really reorders, and the spectrum of the rounded Y stays separated, which keeps
U determined up to sign."""
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from oracle import postprocess_oracle as PO
from postprocess_cases import EDGE_SHAPES, EDGE_VIEWS, GRAM_CHUNK, SHAPES, VIEWS, make_factors

CSRC = Path(__file__).resolve().parent.parent / "pathmatfac.jl_amd" / "csrc"
EDGE_IDS = [f"K{k}_M{m}_N{n}" for k, m, n in EDGE_SHAPES]


@lru_cache(maxsize=None)
def source_constants():
    """The geometry as the source states it: CHUNK, PERM_TC, K_MAX (upper K of the first two template classes), GRAM_T and
    ROTATE_R (template arguments by class), ROTATE_TC (columns per rotate tile by class), KP_UNIT, K_LIMIT."""
    txt = (CSRC / "pmf_postprocess.hip").read_text()
    out = {}
    out["CHUNK"] = int(re.search(r"#define PP_CHUNK (\d+)", txt).group(1))
    assert re.search(r"\(j / PP_CHUNK \+ 1\) \* PP_CHUNK", txt)                      # pieces are cut at its multiples
    out["PERM_TC"] = int(re.search(r"#define PP_PERM_TC (\d+)", txt).group(1))
    assert len(re.findall(r"\(c->[MN] \+ PP_PERM_TC - 1\) / PP_PERM_TC", txt)) == 2   # ... and so is the permute grid
    g = re.search(r"else if \(c->K <= (\d+)\) k_pp_gram<(\d+)><<<.*\n\s*else if \(c->K <= (\d+)\) k_pp_gram<(\d+)><<<.*\n"
                  r"\s*else k_pp_gram<(\d+)><<<", txt)
    r = re.search(r"if \(c->K <= (\d+)\) k_pp_rotate<(\d+)><<<\(unsigned\)\(\(n \+ (\d+)\) / (\d+)\).*\n"
                  r"\s*else if \(c->K <= (\d+)\) k_pp_rotate<(\d+)><<<\(unsigned\)\(\(n \+ (\d+)\) / (\d+)\).*\n"
                  r"\s*else k_pp_rotate<(\d+)><<<\(unsigned\)\(\(n \+ (\d+)\) / (\d+)\)", txt)
    gv, rv = [int(v) for v in g.groups()], [int(v) for v in r.groups()]
    out["K_MAX"] = (gv[0], gv[2])
    assert out["K_MAX"] == (rv[0], rv[4])                                             # both launchers switch at the same K
    out["GRAM_T"] = (gv[1], gv[3], gv[4])
    out["ROTATE_R"] = (rv[1], rv[5], rv[8])
    grid = ((rv[2], rv[3]), (rv[6], rv[7]), (rv[9], rv[10]))
    m = re.search(r"constexpr int NG = (\d+) / R, CJ = (\d+), TC = NG \* CJ", txt)
    threads, cj = int(m.group(1)), int(m.group(2))
    out["ROTATE_TC"] = tuple(threads // R * cj for R in out["ROTATE_R"])
    assert grid == tuple((tc - 1, tc) for tc in out["ROTATE_TC"])                     # the grid is ceil(n / TC) of the kernel's TC
    assert re.search(r"constexpr int R = 16 \* T", txt)                               # k_pp_gram<T> covers 16 T factors
    assert tuple(16 * t for t in out["GRAM_T"]) == out["ROTATE_R"]
    hip = (CSRC / "pmf_hip.hip").read_text()
    m = re.search(r"c->KB = \(K \+ (\d+)\) / (\d+);\s*c->Kp = (\d+) \* c->KB;", hip)
    assert int(m.group(1)) + 1 == int(m.group(2)) == int(m.group(3))
    out["KP_UNIT"] = int(m.group(3))
    out["K_LIMIT"] = int(re.search(r"K > (\d+)\) return pmf_fail\(\"K=%d unsupported", hip).group(1))
    return out


def geometry(K, n=None):
    """Template class (0, 1, 2), Kp and R of K; with n: the rotate tile, the remainder of n in it and in a permute tile, the
    piece count of 1..n and the length of its last piece."""
    sc = source_constants()
    cls = 0 if K <= sc["K_MAX"][0] else 1 if K <= sc["K_MAX"][1] else 2
    out = dict(cls=cls, Kp=sc["KP_UNIT"] * -(-K // sc["KP_UNIT"]), R=sc["ROTATE_R"][cls], T=sc["GRAM_T"][cls], TC=sc["ROTATE_TC"][cls])
    if n is not None:
        out.update(rot_rem=n % out["TC"], rot_tiles=-(-n // out["TC"]), perm_rem=n % sc["PERM_TC"], perm_tiles=-(-n // sc["PERM_TC"]),
                   pieces=-(-n // sc["CHUNK"]), last_piece=n - (-(-n // sc["CHUNK"]) - 1) * sc["CHUNK"])
    return out


def test_source_constants_are_the_ones_the_tables_were_made_for():
    sc = source_constants()
    assert sc == dict(CHUNK=2048, PERM_TC=64, K_MAX=(32, 64), GRAM_T=(2, 4, 8), ROTATE_R=(32, 64, 128), ROTATE_TC=(256, 128, 64),
                      KP_UNIT=32, K_LIMIT=128), sc
    assert GRAM_CHUNK == sc["CHUNK"]


def test_edge_shapes_extend_the_table_and_leave_it_alone():
    assert SHAPES == [(1, 5, 7), (6, 331, 96), (33, 257, 1068), (128, 4099, 1068)]
    assert EDGE_SHAPES == [(31, 255, 257), (32, 256, 2049), (64, 129, 2176), (65, 63, 4100), (96, 70, 130), (97, 64, 2047)]
    assert not set(EDGE_SHAPES) & set(SHAPES) and not set(EDGE_VIEWS) & set(VIEWS)
    assert sorted(EDGE_VIEWS) == sorted(n for _, _, n in EDGE_SHAPES)
    sc = source_constants()
    a, b = sc["K_MAX"]
    assert {a - 1, a, b, b + 1, 3 * sc["KP_UNIT"], 3 * sc["KP_UNIT"] + 1} == {k for k, _, _ in EDGE_SHAPES}   # both sides of each K seam
    # every N of the old table is one piece on the Y side; the new one has two- and three-piece Y's and a one-column piece
    assert all(geometry(k, n)["pieces"] == 1 for k, _, n in SHAPES)
    assert sorted(geometry(k, n)["pieces"] for k, _, n in EDGE_SHAPES) == [1, 1, 1, 2, 2, 3]
    # no old shape has a whole number of tiles of either in-place kernel on either side
    for k, m, n in SHAPES:
        for cols in (m, n):
            g = geometry(k, cols)
            assert g["rot_rem"] != 0 and g["perm_rem"] != 0


@pytest.mark.parametrize("K,M,N", EDGE_SHAPES, ids=EDGE_IDS)
def test_shape_hits_the_seam_it_is_listed_for(K, M, N):
    sc = source_constants()
    gm, gn = geometry(K, M), geometry(K, N)
    assert 1 <= K <= sc["K_LIMIT"]
    if (K, M, N) == EDGE_SHAPES[0]:      # Kp > K under <2>/<32>; M one column short of a rotate tile, N one past
        assert gm["cls"] == 0 and gm["Kp"] == gm["R"] == K + 1
        assert M == gm["TC"] - 1 and N == gn["TC"] + 1 and gn["pieces"] == 1
    elif (K, M, N) == EDGE_SHAPES[1]:    # K = Kp = R, the last K of the class; M one tile; Y two pieces, the second of one column
        assert gm["cls"] == 0 and geometry(K + 1)["cls"] == 1 and K == gm["Kp"] == gm["R"]
        assert M == gm["TC"] and (gm["rot_tiles"], gm["rot_rem"]) == (1, 0)
        assert (gn["pieces"], gn["last_piece"]) == (2, 1)
    elif (K, M, N) == EDGE_SHAPES[2]:    # <4>/<64> fully populated; N whole rotate and permute tiles; two pieces
        assert gm["cls"] == 1 and geometry(K + 1)["cls"] == 2 and K == gm["Kp"] == gm["R"]
        assert (gn["rot_tiles"], gn["rot_rem"], gn["perm_tiles"], gn["perm_rem"]) == (17, 0, 34, 0)
        assert gn["pieces"] == 2 and M == gm["TC"] + 1
    elif (K, M, N) == EDGE_SHAPES[3]:    # first K of <8>/<128>; K < Kp = 96 < R; M one short of a tile; three pieces, the last of 4
        assert gm["cls"] == 2 and geometry(K - 1)["cls"] == 1 and K < gm["Kp"] == 96 < gm["R"]
        assert M == gm["TC"] - 1 == sc["PERM_TC"] - 1
        assert (gn["pieces"], gn["last_piece"]) == (3, 4)
    elif (K, M, N) == EDGE_SHAPES[4]:    # K = Kp = 96 < R
        assert gm["cls"] == 2 and K == gm["Kp"] == 96 < gm["R"]
        assert gm["rot_rem"] and gn["rot_rem"] and gn["pieces"] == 1
    else:                                # Kp = 128 with 31 pad rows; M one tile of rotate and of permute; N one short of a piece
        assert (K, M, N) == EDGE_SHAPES[5]
        assert gm["cls"] == 2 and gm["Kp"] == gm["R"] == sc["K_LIMIT"] and gm["Kp"] - K == 31
        assert M == gm["TC"] == sc["PERM_TC"] and (gm["rot_tiles"], gm["perm_tiles"]) == (1, 1)
        assert N == sc["CHUNK"] - 1 and gn["pieces"] == 1


def _uncovered(N):
    seen = np.zeros(N + 1, bool)
    for a, b in EDGE_VIEWS[N]:
        assert not seen[a:b + 1].any()
        seen[a:b + 1] = True
    return [j for j in range(1, N + 1) if not seen[j]]


def test_views_leave_columns_out_straddle_seams_and_are_not_a_power_of_two():
    chunk = source_constants()["CHUNK"]
    for N, views in EDGE_VIEWS.items():                       # what pp_check_ranges asks for
        assert all(1 <= a <= b <= N for a, b in views)
        assert all(views[i][1] < views[i + 1][0] for i in range(len(views) - 1))
    assert _uncovered(257) == [3, 257] and _uncovered(2049) == [1, 2041, 2042, 2043, 2044]
    assert _uncovered(2176) == [61 * i for i in range(1, 36)]
    assert not _uncovered(4100) and not _uncovered(130) and not _uncovered(2047)
    # an uncovered first column, last column and inner column; one before the first range and one after the last
    assert 1 in _uncovered(2049) and 257 in _uncovered(257) and 3 in _uncovered(257)
    straddle = {N: [(a, b) for a, b in v if (a - 1) // chunk != (b - 1) // chunk] for N, v in EDGE_VIEWS.items()}
    assert straddle[2049] == [(2045, 2049)] and straddle[2176] == [(2014, 2073)] and not straddle[4100]
    assert [b for _, b in EDGE_VIEWS[4100]][:2] == [chunk, 2 * chunk]                 # ... and views that end exactly on a seam
    counts = sorted(len(v) for v in EDGE_VIEWS.values())
    assert counts == [1, 2, 3, 3, 36, 65]
    assert any(c > 4 and c & (c - 1) for c in counts)                                 # the binary search past 4 ranges
    assert max(len(v) for v in VIEWS.values()) == 4


@pytest.mark.parametrize("K,M,N", EDGE_SHAPES, ids=EDGE_IDS)
def test_oracle_keeps_the_case_from_passing_vacuously(K, M, N):
    f = make_factors(K, M, N)
    X64, Y64 = f["X"].astype(np.float64), f["Y"].astype(np.float64)
    xr = PO.rms_rows(X64)
    assert np.all(xr > 0)
    Ys = Y64 * xr[:, None]
    c = np.array([max(PO.rms_rows(Ys[:, a - 1:b])) for a, b in EDGE_VIEWS[N]])
    assert c.shape == (len(EDGE_VIEWS[N]),) and np.all(c > 0)                         # no view takes the all-zero branch
    order = PO.importance_order(f["Y"])
    assert sorted(order) == list(range(K)) and order != list(range(K))
    sing = np.linalg.svd(Y64, compute_uv=False)
    gap = float(np.min(-np.diff(sing)))
    print(f"PP_EDGE_CPU K={K} M={M} N={N} smallest singular-value gap {gap:.3e} (spacing {1.0 / (K - 1):.3e}) c in "
          f"[{c.min():.3e}, {c.max():.3e}]")
    assert gap >= 0.5 / (K - 1)
