"""The plain-run table (pmf_pass.hip, k_plain_table) against numpy.

For every row panel of 256 rows the table holds, per column tile c, the number of column tiles < c in which one of the
panel's eight 32 x 32 tiles has a missing value or lies beyond the matrix.  The exact kernel takes its plain tile loop
only where the difference of two entries is 0, so an entry that is too small lets a tile with a missing value, or a row
block that does not exist, into a loop that no longer masks.  Shapes: one panel with ragged rows and a ragged last column
tile; three panels, the last of one row, with 161 columns (one live column in the last tile, whose pad columns are NaN).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def expected_table(D):
    M, N = D.shape
    n_rp, n_ct = -(-M // 256), -(-N // 32)
    nrb = -(-M // 32)
    # tile (rb, ct) is all-finite iff its 32 x 32 entries, pad rows and columns (NaN on the device) included, are finite
    P = np.full((nrb * 32, n_ct * 32), np.nan, np.float32)
    P[:M, :N] = D
    fin = np.isfinite(P).reshape(nrb, 32, n_ct, 32).all(axis=(1, 3))
    bad = np.ones((n_rp * 8, n_ct), bool)          # row blocks beyond the matrix count as not finite
    bad[:nrb] = ~fin
    bad = bad.reshape(n_rp, 8, n_ct).any(axis=1)
    out = np.zeros((n_rp, n_ct + 1), np.int32)
    out[:, 1:] = np.cumsum(bad, axis=1)
    return out


@pytest.mark.parametrize("store", ["f32", "bf16"])
@pytest.mark.parametrize("M,N", [(300, 100), (513, 161)])
def test_table_is_the_running_count(ctx, M, N, store):
    rng = np.random.default_rng(M + N)
    D = rng.standard_normal((M, N)).astype(np.float32)
    D[rng.random((M, N)) < 0.05] = np.nan
    D = np.asfortranarray(D)
    ctx.set_data(D, store=store)
    try:
        got = ctx.plain_table()
    finally:
        if store != "f32":
            ctx.set_data(D)
    want = expected_table(D)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]


def test_table_separates_clean_tiles(ctx):
    """5 % NaN leaves no clean 256 x 32 strip: a matrix with NaNs in two known tiles tells counted from uncounted."""
    D = np.ones((513, 161), np.float32, order="F")
    D[40, 70] = np.nan          # panel 0, column tile 2
    D[300, 131] = np.inf        # panel 1, column tile 4
    ctx.set_data(D)
    got = ctx.plain_table()
    want = expected_table(D)
    assert np.array_equal(got, want)
    # (the last column tile holds one live column and 31 NaN pad columns: never all-finite)
    assert got[0].tolist() == [0, 0, 0, 1, 1, 1, 2] and got[1].tolist() == [0, 0, 0, 0, 0, 1, 2] and got[2].tolist() == list(range(7))
