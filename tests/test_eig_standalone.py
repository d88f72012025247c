"""csrc/pmf_eig.h, the library's cyclic-Jacobi symmetric eigen-solver, tested without a GPU: tests/eig_check.cpp (its own
main, no HIP) is compiled with g++ and run.

Bound (c): ||G U - U L||_F <= 64 K 2^-53 ||G||_F and ||U'U - I||_F <= 64 K 2^-53 -- backward stability with a modest
polynomial in K.  The built-in run of eig_check checks it, the ordering and sign conventions, and the special inputs (1 x 1,
diagonal with ties, a repeated eigenvalue, a rank-deficient and a zero matrix; for the last three residual and orthogonality
only).  The second test decomposes the Gram matrices Y Y' of the four shapes of tests/test_gpu_postprocess.py and prints
LAPACK's residuals (numpy.linalg.eigh) beside the library's."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from postprocess_cases import SHAPES, make_factors

ROOT = Path(__file__).resolve().parent.parent
EPS53 = 2.0 ** -53


@pytest.fixture(scope="module")
def eig_check(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to build tests/eig_check.cpp"
    exe = tmp_path_factory.mktemp("eig") / "eig_check"
    subprocess.run([gxx, "-std=c++17", "-O2", "-I", str(ROOT / "pathmatfac.jl_amd" / "csrc"),
                    str(ROOT / "tests" / "eig_check.cpp"), "-o", str(exe)], check=True, timeout=120)
    return exe


def test_builtin_cases(eig_check):
    r = subprocess.run([str(eig_check)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "EIG all checks passed" in r.stdout
    for name in ("one_by_one", "diagonal", "repeated", "rank_deficient", "separated_128"):
        assert f"EIG {name} " in r.stdout


def _residuals(G, lam, U):
    return (float(np.linalg.norm(G @ U - U * lam[None, :])), float(np.linalg.norm(U.T @ U - np.eye(len(lam)))))


@pytest.mark.parametrize("K,M,N", SHAPES)
def test_gram_matrices_of_the_postprocess_shapes(eig_check, tmp_path, K, M, N):
    Y = make_factors(K, M, N)["Y"].astype(np.float64)
    G = Y @ Y.T
    G = 0.5 * (G + G.T)
    G.tofile(tmp_path / "g.bin")
    subprocess.run([str(eig_check), str(K), str(tmp_path / "g.bin"), str(tmp_path / "out.bin")], check=True, timeout=120)
    out = np.fromfile(tmp_path / "out.bin")
    lam, U = out[:K], out[K:].reshape(K, K)
    res, orth = _residuals(G, lam, U)
    wl, WU = np.linalg.eigh(G)
    res_l, orth_l = _residuals(G, wl, WU)
    bound = 64 * K * EPS53
    fro = float(np.linalg.norm(G))
    print(f"EIG_PY K={K} residual library={res:.3e} lapack={res_l:.3e} (bound {bound * fro:.3e}) "
          f"orthogonality library={orth:.3e} lapack={orth_l:.3e} (bound {bound:.3e})")
    assert res <= bound * fro and orth <= bound
    assert np.all(np.diff(lam) <= 0)                                        # descending
    np.testing.assert_allclose(lam, wl[::-1], rtol=0, atol=1e-12 * wl[-1])
    kmax = np.argmax(np.abs(U), axis=0)                                     # (argmax: the lowest index among ties)
    assert np.all(U[kmax, np.arange(K)] > 0)
    # the spectrum is separated: the vectors are LAPACK's up to sign
    dots = np.abs(np.sum(U * WU[:, ::-1], axis=0))
    assert np.all(dots > 1 - 1e-9), dots.min()
