"""Helpers of the tests of pmf_fsard_update_A_csr (csrc/pmf_fsard_csr.hip, update_A! on a sparse S without the L x K
bound): the rows above the dense entry's capacity, made by fsard_ref.make_case, and one cached oracle run per row that the
tests share and leave unchanged.  The bounds are fsard_ref's (MEASURED, TOL, MARGIN): no tolerance of its own.
tests/test_fsard_sparse_cases.py guards the rows on the CPU, tests/test_gpu_fsard_csr.py runs them on the device."""
import functools

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


@functools.lru_cache(maxsize=None)
def sparse_row(name):
    """(case, oracle run) of a row of SPARSE_ROWS, computed once per session; neither is to be modified."""
    case = fr.make_case(**SPARSE_ROWS[name])
    return case, fr.run_oracle(case)


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
