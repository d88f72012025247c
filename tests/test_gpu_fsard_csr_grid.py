"""pmf_fsard_update_A_csr (csrc/pmf_fsard_csr.hip) past one grid: fsard_sparse_ref.GRID_ROWS, whose geometry
tests/test_fsard_sparse_cases.py asserts from the source text.  The four wide rows give k_fsc_forward 2048 workgroups that
walk slices of 5, 9, 9 and 17 columns in two or three trips of 4, 4, 8 and 16, the slices no multiple of the trip, with 118
to 408 trailing workgroups that have no column (their partial must be 0), in both instantiations (the loss pass and the
final beta), and give k_fsc_decide two loss partials per thread; LK_8200x128 gives k_fsc_update the second trip of its
grid-stride loop.

Every row goes against oracle/fsard_oracle.py in float64 on A and ssq_grad entry by entry, beta, the best loss and
epochs_run, at fsard_ref.TOL -- the dense entry's bounds, nothing of this file's own.  The three rows that the dense entry
accepts run through both entries on one context; two rows run on fresh contexts for equal bits; one wide row runs under a
stopping rule that ends the loop inside a batch of queued iterations.
Worst figures seen on an MI355X over all rows of this file, against the bounds 1.0e-5 / 9.0e-6 / 3.8e-4 / 4.2e-6:
A 2.2e-7, beta 3.7e-7, ssq_grad 2.0e-6, best loss 1.1e-7; sparse against dense (bounds twice those) 1.7e-7, 1.7e-8, 1.6e-6,
6.7e-11.  These are records, not bounds.
Every test prints its figures ("FSARD_ERR <row> ...") before it asserts: run with -s to see them."""
import numpy as np
import pytest

import fsard_ref as fr
import fsard_sparse_ref as fs
import test_gpu_fsard_edges as ed
from test_gpu_fsard_csr import run_csr, same_bits

pytestmark = pytest.mark.gpu
F = np.float32


def _structural(case, got):
    """What holds exactly: the feature set without a member keeps A = 0 and its accumulator, the uncovered column has
    beta = (alpha0 - 1) v0 in every factor."""
    assert not got["A"][case["zero_row"]].any()
    assert np.array_equal(got["ssq"][case["zero_row"]], fr.fresh_ssq(case)[case["zero_row"]])
    b0 = (F(case["alpha0"]) - F(1)) * F(case["v0"])
    assert np.array_equal(got["beta"][:, case["zero_col"]], np.full(case["K"], b0, F))
    assert got["beta"].shape == (case["K"], case["Nv"]) and np.all(got["beta"] >= b0)


@pytest.mark.parametrize("name", list(fs.GRID_ROWS))
def test_rows_past_one_grid(ctx, name):
    case, want = fs.grid_row(name)
    ed.load(ctx, case)
    got = run_csr(ctx, case)
    ed.check(name, got, want, fr.fresh_ssq(case))
    assert got["epochs"] == case["max_epochs"]
    _structural(case, got)
    # no column of a later trip kept the beta that was uploaded (the final pass writes into the attached term's array)
    assert np.all(got["beta"] != F(fr.BETA_UPLOADED))


@pytest.mark.parametrize("name", fs.GRID_AGAINST_DENSE)
def test_the_two_entries_agree_at_width(ctx, name):
    case, want = fs.grid_row(name)
    assert case["L"] * case["K"] <= fr.CAPACITY
    ed.load(ctx, case)
    dense = ed.run(ctx, case)
    sparse = run_csr(ctx, case)
    ed.check(name + "_dense", dense, want, fr.fresh_ssq(case))
    ed.check(name + "_sparse", sparse, want, fr.fresh_ssq(case))
    e = fr.errors(sparse, dense, fr.fresh_ssq(case))
    print(f"FSARD_ERR {name} sparse against dense " + " ".join(f"{k}={v:.3e}" for k, v in e.items()))
    assert sparse["epochs"] == dense["epochs"]
    for k, v in e.items():
        assert v <= 2 * fr.TOL[k], (k, v)


@pytest.mark.parametrize("name", fs.GRID_REPRO)
def test_bitwise_reproducible_on_fresh_contexts(pkg, name):
    case, want = fs.grid_row(name)
    runs = []
    for _ in range(2):
        fresh = pkg.Context(0)
        try:
            ed.load(fresh, case)
            runs.append(run_csr(fresh, case))
        finally:
            fresh.close()
    ed.check(name + "_fresh", runs[0], want, fr.fresh_ssq(case))
    same_bits(runs[0], runs[1])


def test_early_stop_at_width_ignores_the_launches_queued_past_the_end(ctx):
    """The loop ends on its termination counter inside a batch of queued iterations: the forward, gradient, decision and
    update launches behind that point walk the same multi-trip slices and must change nothing."""
    rule = fs.early_stop_rule()
    case, want = fs.early_stop_run()
    assert 0 < want["epochs"] < rule["max_epochs"]
    ed.load(ctx, case)
    got = run_csr(ctx, case, **rule)
    ed.check("_".join(fs.GRID_EARLY_STOP), got, want, fr.fresh_ssq(case))
    _structural(case, got)
    again = run_csr(ctx, case, **rule)
    same_bits(got, again)
