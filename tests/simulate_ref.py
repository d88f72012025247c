"""What pmf_simulate_data must compute, restated in numpy: the Philox4x32-10 stream and the per-entry rule.

    counter = (i_lo, i_hi, j_lo, j_hi) of the GLOBAL 0-based row i and the 0-based column j, key = (seed_lo, seed_hi)
    u1 = ((r0 >> 8) + 1) 2^-24, u2 = (r1 >> 8) 2^-24, n = sqrt(-2 log u1) cos(2 pi u2)
    u3 = (r2 >> 8) 2^-24 (missing when u3 < frac_missing), u4 = (r3 >> 8) 2^-24 (bernoulli: u4 < sigmoid(z))
    normal: z + noise n ; kind 3: the number of thresholds strictly below z ; then the missing mask.

The uniforms are 24-bit integers times 2^-24: the twin reproduces the device's bit for bit.  The normal is compared in float64
(`draws(...)["n"]`; `normal32` is the float32 form of the same expression, used on the host to bound what f32 evaluation costs).
Plain numpy; neither the package nor the C oracle is imported here."""
import copy

import numpy as np

import hinge_ref as hr
from impute_ref import BATCH, CASES, LINK, case_problem, impute_tol, link_space  # noqa: F401  (re-exported to the tests)

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32, S8 = np.uint64(32), np.uint64(8)

# Random123's known answers: counter words, key words -> output words
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox4x32(c, k):
    """Philox4x32-10 on arrays (or scalars) of 32-bit words held in uint64: c = (c0, c1, c2, c3), k = (k0, k1)."""
    c = [np.asarray(x, np.uint64) for x in c]
    k0, k1 = (np.asarray(x, np.uint64) for x in k)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> S32) ^ c[1] ^ k0, p1 & MASK, (p0 >> S32) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return c


def words(seed, rows, cols):
    """r0..r3 for the entries (rows[a], cols[b]) as four len(rows) x len(cols) arrays; rows are GLOBAL 0-based."""
    i = np.asarray(rows, np.uint64)[:, None] + np.zeros((1, len(cols)), np.uint64)
    j = np.asarray(cols, np.uint64)[None, :] + np.zeros((len(rows), 1), np.uint64)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return philox4x32((i & MASK, i >> S32, j & MASK, j >> S32), (np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)))


def uniforms(r):
    f = 2.0 ** -24
    return (((r[0] >> S8).astype(np.float64) + 1) * f, (r[1] >> S8).astype(np.float64) * f,
            (r[2] >> S8).astype(np.float64) * f, (r[3] >> S8).astype(np.float64) * f)


def normal64(u1, u2):
    return np.sqrt(-2 * np.log(u1)) * np.cos(2 * np.pi * u2)


def normal32(u1, u2):
    f = np.float32
    return np.sqrt(f(-2) * np.log(u1.astype(f))) * np.cos(f(6.28318530718) * u2.astype(f))


def draws(seed, M, N, row_offset=0):
    """dict(n (float64), u3, u4) for local rows 0..M-1 at `row_offset`, columns 0..N-1."""
    u1, u2, u3, u4 = uniforms(words(seed, np.arange(M) + row_offset, np.arange(N)))
    return dict(n=normal64(u1, u2), u3=u3, u4=u4)


def missing_mask(d, frac_missing):
    """u3 < frac in float32, as the device compares (u3 is exact in float32)."""
    return d["u3"].astype(np.float32) < np.float32(frac_missing)


# ---- problems ----------------------------------------------------------------------------------------------------------
def without_poisson(p):
    """The problem with its Poisson ranges re-declared normal (there is no Poisson sampler; such a context is refused)."""
    q = copy.copy(p)
    q["noise_kinds"] = ["normal" if (k == "poisson" or k == 2) else k for k in p["noise_kinds"]]
    return q


def sim_case(K, M, N, seed=None):
    """impute_ref.case_problem (mixed noise, batch views, rows in no batch) without Poisson."""
    return without_poisson(case_problem(K, M, N, seed))


def hinge_case(name, K):
    """hinge_ref.layout(name, K, batch=True) without Poisson (a copy: the layouts are shared)."""
    return without_poisson(hr.layout(name, K, batch=True))


def kinds_of(p):
    return hr.kinds_of(p)


def sigmoid64(z):
    return hr.sigmoid(np.asarray(z, np.float64))
