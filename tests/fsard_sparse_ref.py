"""Helpers of the tests of pmf_fsard_update_A_csr (csrc/pmf_fsard_csr.hip, update_A! on a sparse S without the L x K
bound): the rows above the dense entry's capacity, made by fsard_ref.make_case, and one cached oracle run per row that the
tests share and leave unchanged.  The bounds are fsard_ref's (MEASURED, TOL, MARGIN): no tolerance of its own.
tests/test_fsard_sparse_cases.py guards the rows on the CPU, tests/test_gpu_fsard_csr.py runs them on the device.

GRID_ROWS are the rows past one grid (tests/test_gpu_fsard_csr_grid.py; the same CPU guard file): views wide enough that a
workgroup of k_fsc_forward walks its column slice in more than one trip, in slices that are no multiple of the step, with
trailing workgroups that have no column and more than 1024 loss partials for k_fsc_decide's 1024 threads; and one L x K
large enough for the second grid-stride trip of k_fsc_update.  launch_geometry() restates the launch from the source text."""
import functools
import re

import numpy as np

import fsard_ref as fr

F = np.float32

# every row has L * K above fsard_ref.CAPACITY; all with make_case's default 6 epochs.  K sits on the edges of the lane
# mapping (K <= 32: 64 / kp items per wave, kp = the power of two at or above K; one item per wave above; two factors per
# lane above 64): 1, 31, 33, 64, 65, 100, 128
SPARSE_ROWS = {
    "LK16385_16385x1": dict(L=16385, K=1, Nv=300, seed=201),            # the first value past the cap, both ways
    "LK16512_129x128": dict(L=129, K=128, Nv=300, seed=202),
    "K33_L497": dict(L=497, K=33, Nv=777, seed=203),
    "K65_L253": dict(L=253, K=65, Nv=777, seed=204),
    "K31_L530": dict(L=530, K=31, Nv=257, seed=205),
    "K64_L257_mid": dict(L=257, K=64, Nv=255, seed=206, N=292, c0=20),  # a view at neither end of the model
    "K100_L200_dense": dict(L=200, K=100, Nv=130, seed=207, dense=True),
    "wide_3000x25": dict(L=3000, K=25, Nv=2000, seed=208),
}
AGAINST_DENSE = (("BETA_DEST", "beta_dest"), ("OUTPUTS", "LK16384_128x128"))   # (table, row) of fsard_ref run through both entries
REPRO = ("K33_L497", "wide_3000x25")

# past one grid of pmf_fsard_csr.hip (the geometry is asserted in test_fsard_sparse_cases.py from launch_geometry)
GRID_ROWS = {
    "Nv8197_K33": dict(L=24, K=33, Nv=8197, seed=301),                   # step 4, 2048 workgroups of 5 columns: two trips; 408 empty
    "Nv16500_K65": dict(L=17, K=65, Nv=16500, seed=302),                 # 9 columns per workgroup: three trips; two factors per lane
    "Nv16390_K25": dict(L=20, K=25, Nv=16390, seed=303),                 # kp 32, two columns per wave, step 8, 9 per workgroup
    "Nv32800_K16_mid": dict(L=40, K=16, Nv=32800, seed=304, N=32850, c0=20),   # four columns per wave, step 16, 17 per workgroup
    "LK_8200x128": dict(L=8200, K=128, Nv=96, seed=305),                 # L K = 1,049,600: k_fsc_update's second grid-stride trip
}
GRID_WIDE = ("Nv8197_K33", "Nv16500_K65", "Nv16390_K25", "Nv32800_K16_mid")
GRID_AGAINST_DENSE = ("Nv8197_K33", "Nv16500_K65", "Nv16390_K25")           # L K <= fsard_ref.CAPACITY: legal for the dense entry
GRID_REPRO = ("Nv8197_K33", "LK_8200x128")
GRID_EARLY_STOP = ("Nv8197_K33", "atol_1e30")                               # (row, row of fsard_ref.STOP_RULES whose rule it takes)
CSR_SOURCE = fr.HIP_SOURCE.with_name("pmf_fsard_csr.hip")


@functools.lru_cache(maxsize=None)
def sparse_row(name):
    """(case, oracle run) of a row of SPARSE_ROWS, computed once per session; neither is to be modified."""
    case = fr.make_case(**SPARSE_ROWS[name])
    return case, fr.run_oracle(case)


@functools.lru_cache(maxsize=None)
def grid_row(name):
    """(case, oracle run) of a row of GRID_ROWS, computed once per session; neither is to be modified."""
    case = fr.make_case(**GRID_ROWS[name])
    return case, fr.run_oracle(case)


def early_stop_rule():
    """term_iter / atol of the stopping rule that GRID_EARLY_STOP names (its max_epochs too: the loop must end before it)."""
    spec = fr.STOP_RULES[GRID_EARLY_STOP[1]]
    return dict(term_iter=spec["term_iter"], atol=spec["atol"], max_epochs=spec["max_epochs"])


@functools.lru_cache(maxsize=None)
def early_stop_run():
    """(case, oracle run) of GRID_EARLY_STOP's row under that rule."""
    case = grid_row(GRID_EARLY_STOP[0])[0]
    return case, fr.run_oracle(case, **early_stop_rule())


@functools.lru_cache(maxsize=None)
def csr_source_constants():
    """The launch constants of pmf_fsard_update_A_csr as its source states them."""
    txt = CSR_SOURCE.read_text()
    out = {}
    m = re.search(r"const int n_wg = \(int\)std::max<int64_t>\(1, std::min<int64_t>\((\d+), \(Nv \+ step - 1\) / step\)\);", txt)
    out["N_WG_CAP"] = int(m.group(1)) if m else None
    m = re.search(r"const int g_upd = \(int\)std::max<int64_t>\(1, std::min<int64_t>\((\d+), \(n \+ (\d+)\) / (\d+)\)\);", txt)
    out["G_UPD_CAP"], out["UPD_THREADS"] = (int(m.group(1)), int(m.group(3))) if m and int(m.group(2)) + 1 == int(m.group(3)) else (None, None)
    m = re.search(r"const int64_t step = (\d+) \* pw;", txt)
    out["WAVES"] = int(m.group(1)) if m else None
    m = re.search(r"const int pw = (\d+) / kp;", txt)
    out["LANES"] = int(m.group(1)) if m else None
    m = re.search(r"int kp = (\d+), kp_shift = \d+;\s*if \(K <= (\d+)\) \{ kp = 1;", txt)
    out["KP_WIDE"], out["K_PACKED"] = (int(m.group(1)), int(m.group(2))) if m else (None, None)
    out["PER"] = bool(re.search(r"const int64_t per = \(Nv \+ n_wg - 1\) / n_wg;", txt))
    m = re.search(r"__launch_bounds__\((\d+)\) void k_fsc_decide", txt)
    n = re.search(r"hipLaunchKernelGGL\(k_fsc_decide, dim3\(1\), dim3\((\d+)\)", txt)
    out["DECIDE_THREADS"] = int(n.group(1)) if m and n and m.group(1) == n.group(1) else None
    m = re.search(r"hipLaunchKernelGGL\(k_fsc_update, dim3\(g_upd\), dim3\((\d+)\)", txt)
    out["UPD_BLOCK"] = int(m.group(1)) if m else None
    out["FORWARD_TRIP"] = bool(re.search(r"for \(int64_t j = j_lo \+ wave \* pw \+ sub; j < j_hi; j \+= (\d+) \* pw\)", txt))
    return out


def launch_geometry(L, K, Nv):
    """kp, step, n_wg, per and g_upd of pmf_fsard_update_A_csr for a shape, from csr_source_constants(); trips: passes of a
    workgroup of k_fsc_forward over its slice; empty: workgroups whose slice starts at or past Nv; upd_trips: trips of
    k_fsc_update's grid-stride loop."""
    sc = csr_source_constants()
    kp = sc["KP_WIDE"]
    if K <= sc["K_PACKED"]:
        kp = 1
        while kp < K:
            kp <<= 1
    step = sc["WAVES"] * (sc["LANES"] // kp)
    n_wg = max(1, min(sc["N_WG_CAP"], -(-Nv // step)))
    per = -(-Nv // n_wg)
    g_upd = max(1, min(sc["G_UPD_CAP"], -(-(L * K) // sc["UPD_THREADS"])))
    return dict(kp=kp, step=step, n_wg=n_wg, per=per, g_upd=g_upd, trips=-(-per // step),
                empty=sum(1 for w in range(n_wg) if w * per >= Nv), upd_trips=-(-(L * K) // (g_upd * sc["UPD_BLOCK"])))


@functools.lru_cache(maxsize=None)
def table_row(table, name):
    """(case, oracle run) of a row of fsard_ref.TABLES, computed once per session."""
    case = fr.make_case(**fr.TABLES[table][name])
    return case, fr.run_oracle(case)


def csr_by_nonzero(S):
    """The CSR of a dense matrix from np.nonzero (row-major order): what _lib.dense_to_csr is checked against."""
    S = np.asarray(S, F)
    r, c = np.nonzero(S)
    rowptr = np.zeros(S.shape[0] + 1, np.int64)
    np.add.at(rowptr, r + 1, 1)
    return np.cumsum(rowptr), c.astype(np.int32), S[r, c]


def csr_to_dense(rowptr, col, val, Nv):
    S = np.zeros((len(rowptr) - 1, Nv), F)
    for l in range(len(rowptr) - 1):
        S[l, col[rowptr[l]:rowptr[l + 1]]] = val[rowptr[l]:rowptr[l + 1]]
    return S
