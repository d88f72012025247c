"""pmf_fsard_update_A_csr (csrc/pmf_fsard_csr.hip): update_A! on a sparse S without the dense entry's bound L * K <= 16384.

Every compared row goes against oracle/fsard_oracle.py in float64 on A, ssq_grad entry by entry, beta, the best loss and
epochs_run, at the bounds of the dense entry (fsard_ref.TOL = 20 x the float32 restatement's discrepancy; the table is in
tests/test_gpu_fsard_edges.py): the rows above the capacity (tests/fsard_sparse_ref.py, guarded on the CPU by
tests/test_fsard_sparse_cases.py) and every row of fsard_ref's tables, which carry the stopping rules, the iterations
enqueued past the end of the loop, the kept accumulator, the positions of the view and the destinations of beta.
Worst figures seen on an MI355X over all rows of this file, against the bounds 1.0e-5 / 9.0e-6 / 3.8e-4 / 4.2e-6:
A 5.5e-7, beta 4.9e-7, ssq_grad 2.1e-5, best loss 3.8e-7.
Two rows run through both entries on one context: each is within TOL of the oracle, so they agree within 2 x TOL.
Every test prints its figures ("FSARD_ERR <row> ...") before it asserts: run with -s to see them."""
import ctypes as C

import numpy as np
import pytest

import fsard_ref as fr
import fsard_sparse_ref as fs
import test_gpu_fsard_edges as ed

pytestmark = pytest.mark.gpu
F = np.float32


# ---- plumbing ------------------------------------------------------------------------------------------------------------
def run_csr(ctx, case, ssq=None, S=None, **over):
    kw = dict(max_epochs=case["max_epochs"], term_iter=case["term_iter"], atol=case["atol"])
    kw.update(over)
    ssq = fr.fresh_ssq(case) if ssq is None else ssq.copy()
    A, beta, best, epochs = ctx.fsard_update_A_csr(case["c0"], case["c1"], case["S"] if S is None else S, case["alpha"],
                                                   case["lam"], case["alpha0"], case["v0"], case["lr"], ssq, **kw)
    return dict(A=A, ssq=ssq, beta=beta, best=best, epochs=epochs)


def same_bits(a, b):
    for k in ("A", "ssq", "beta"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
    assert np.float64(a["best"]).view(np.uint64) == np.float64(b["best"]).view(np.uint64) and a["epochs"] == b["epochs"]


def raw_csr(ctx, start1, stop1, L, rowptr, col, val, alpha, lam, alpha0, v0, lr, ssq, A, max_epochs, term_iter, atol, beta=None):
    """pmf_fsard_update_A_csr as a C caller sees it.  -> (return code, best_loss, epochs_run, message)"""
    def p(a, t):
        return a.ctypes.data_as(C.POINTER(t)) if a is not None else C.POINTER(t)()
    best, ep = C.c_double(np.nan), C.c_int(-7)
    rc = ctx.lib.pmf_fsard_update_A_csr(ctx._h, C.c_int64(start1), C.c_int64(stop1), int(L), p(rowptr, C.c_int64),
                                        p(col, C.c_int32), p(val, C.c_float), p(alpha, C.c_float), p(lam, C.c_float),
                                        C.c_float(alpha0), C.c_float(v0), C.c_float(lr), p(ssq, C.c_float), p(A, C.c_float),
                                        int(max_epochs), int(term_iter), C.c_double(atol), C.byref(best), C.byref(ep),
                                        p(beta, C.c_float))
    return rc, best.value, ep.value, ctx.lib.pmf_last_error().decode()


# ---- above the dense entry's capacity --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fs.SPARSE_ROWS))
def test_rows_above_the_dense_capacity(ctx, name):
    case, want = fs.sparse_row(name)
    assert case["L"] * case["K"] > fr.CAPACITY
    ed.load(ctx, case)
    got = run_csr(ctx, case)
    ed.check(name, got, want, fr.fresh_ssq(case))
    assert not got["A"][case["zero_row"]].any()                                             # a set without a member stays at 0
    assert np.array_equal(got["ssq"][case["zero_row"]], fr.fresh_ssq(case)[case["zero_row"]])
    b0 = (F(case["alpha0"]) - F(1)) * F(case["v0"])
    assert np.array_equal(got["beta"][:, case["zero_col"]], np.full(case["K"], b0, F))      # an uncovered column: beta0 v0


# ---- the dense entry's tables through the sparse entry ---------------------------------------------------------------------
@pytest.mark.parametrize("table, name", [pytest.param(t, n, id=f"{t}-{n}") for t, n, _ in fr.all_cases()])
def test_the_dense_entrys_tables_through_the_sparse_entry(ctx, table, name):
    case, want = fs.table_row(table, name)
    ed.load(ctx, case)
    got = run_csr(ctx, case)
    ed.check(name, got, want, fr.fresh_ssq(case))
    if table == "MAX_EPOCHS":
        assert got["epochs"] == case["max_epochs"]
        if case["max_epochs"] == 0:                         # every queued launch but the first evaluation changes nothing
            assert not got["A"].any()
            assert np.array_equal(got["ssq"].view(np.uint32), fr.fresh_ssq(case).view(np.uint32))
    if table == "TERM_ITER":
        assert got["epochs"] < case["max_epochs"]
        assert fr.norm_err(fr.last_iterate(case, got["epochs"]), got["A"]) > fr.A_BEST_GAP  # A_best, not the last iterate
    if name in ("strong_lambda", "strong_lambda_negative_atol"):
        assert got["epochs"] == case["term_iter"] < case["max_epochs"] and not got["A"].any()
    if table == "NV_POSITIONS":                             # the attached term's device beta: new inside the view only
        value = ed.yreg_value(ctx)
        ref = fr.reg_value(fr.reg_alpha(case["N"]), fr.beta_after(case, got["beta"]), case["Y"])
        print(f"FSARD_REG {name} rel={abs(value - ref) / ref:.3e}")
        assert abs(value - ref) <= fr.REG_TOL * ref, (value, ref)


def test_second_call_starts_from_the_first_calls_accumulator(ctx):
    case, o1 = fs.table_row("STATE", "two_calls")
    ed.load(ctx, case)
    g1 = run_csr(ctx, case)
    ed.check("two_calls_1", g1, o1, fr.fresh_ssq(case))
    o2 = fr.run_oracle(case, ssq_in=o1["ssq"])
    g2 = run_csr(ctx, case, ssq=g1["ssq"])
    ed.check("two_calls_2", g2, o2, g1["ssq"], o1["ssq"])


def test_call_after_set_Y_reads_the_new_Y(ctx):
    a, oa = fs.table_row("STATE", "after_set_Y")
    b, _ = fs.table_row("STATE", "after_set_Y_second")
    ed.load(ctx, a)
    ed.check("set_Y_before", run_csr(ctx, a), oa, fr.fresh_ssq(a))
    ctx.set_Y(b["Y"])
    ed.check("set_Y_after", run_csr(ctx, a), fr.run_oracle(a, Y=b["Y"]), fr.fresh_ssq(a))


# ---- where beta goes -------------------------------------------------------------------------------------------------------
def test_beta_goes_into_an_attached_featureset_ard_term(ctx):
    case, want = fs.table_row("BETA_DEST", "beta_dest")
    ed.load(ctx, case, "fsard")
    got = run_csr(ctx, case)
    ed.check("beta_dest_fsard", got, want, fr.fresh_ssq(case))
    ref = fr.reg_value(fr.reg_alpha(case["N"]), fr.beta_after(case, got["beta"]), case["Y"])
    value = ed.yreg_value(ctx)
    assert abs(value - ref) <= fr.REG_TOL * ref, (value, ref)


def test_a_plain_ard_term_keeps_its_beta(ctx):
    case, want = fs.table_row("BETA_DEST", "beta_dest")
    al, be = ed.ard_arrays(case)
    ed.load(ctx, case, "ard")
    ed.check("beta_dest_ard", run_csr(ctx, case), want, fr.fresh_ssq(case))
    value = ed.yreg_value(ctx)
    untouched = fr.reg_value(al, be, case["Y"])
    print(f"FSARD_REG ard rel={abs(value - untouched) / untouched:.3e}")
    assert abs(value - untouched) <= fr.REG_TOL * untouched, (value, untouched)


def test_beta_without_a_Y_term_comes_from_a_temporary(ctx):
    case, want = fs.table_row("BETA_DEST", "beta_dest")
    ed.load(ctx, case, None)
    ed.check("beta_dest_none", run_csr(ctx, case), want, fr.fresh_ssq(case))


def test_beta_out_may_be_null(ctx):
    case, want = fs.table_row("BETA_DEST", "beta_dest")
    rowptr, col, val = ctx_csr(case)
    for yreg in ("fsard", None):
        ed.load(ctx, case, yreg)
        ssq, A = fr.fresh_ssq(case), np.full((case["L"], case["K"]), np.nan, F)
        rc, best, epochs, msg = raw_csr(ctx, case["c0"], case["c1"], case["L"], rowptr, col, val, case["alpha"], case["lam"],
                                        case["alpha0"], case["v0"], case["lr"], ssq, A, case["max_epochs"], case["term_iter"],
                                        case["atol"], beta=None)
        assert rc == 0, msg
        got = dict(A=A, ssq=ssq, beta=want["beta"], best=best, epochs=epochs)      # no beta came back: nothing to compare
        ed.check(f"beta_dest_null_{yreg}", got, want, fr.fresh_ssq(case))
        if yreg == "fsard":
            value = ed.yreg_value(ctx)
            ref = fr.reg_value(fr.reg_alpha(case["N"]), fr.beta_after(case, want["beta"]), case["Y"])
            assert abs(value - ref) <= 2 * fr.REG_TOL * ref, (value, ref)          # (the oracle's beta: once more rounding)


def ctx_csr(case):
    return fs.csr_by_nonzero(case["S"])


def test_a_triple_with_stored_zeros_gives_the_dense_arrays_result(ctx):
    """S as a (rowptr, col, val) triple; a stored zero adds a term of exactly 0 to a sum and changes no bit."""
    case, want = fs.table_row("BETA_DEST", "beta_dest")
    ed.load(ctx, case)
    a = run_csr(ctx, case)
    b = run_csr(ctx, case, S=ctx_csr(case))
    same_bits(a, b)
    S = case["S"]
    mask = S != 0
    mask[:, case["zero_col"]] = True                                                # the uncovered column, stored as zeros
    mask[case["zero_row"], ::7] = True                                              # the empty set, with stored zeros
    r, c = np.nonzero(mask)
    rowptr = np.concatenate([[0], np.cumsum(mask.sum(1))]).astype(np.int64)
    assert rowptr[-1] > np.count_nonzero(S)
    z = run_csr(ctx, case, S=(rowptr, c.astype(np.int32), S[r, c]))
    ed.check("stored_zeros", z, want, fr.fresh_ssq(case))
    same_bits(a, z)


# ---- against the dense entry -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table, name", fs.AGAINST_DENSE)
def test_the_two_entries_agree(ctx, table, name):
    case, want = fs.table_row(table, name)
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


# ---- reproducibility -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fs.REPRO)
def test_bitwise_reproducible(pkg, ctx, name):
    case, want = fs.sparse_row(name)
    ed.load(ctx, case)
    a, b = run_csr(ctx, case), run_csr(ctx, case)
    other = pkg.Context(0)
    try:
        ed.load(other, case)
        c = run_csr(other, case)
    finally:
        other.close()
    ed.check(name, a, want, fr.fresh_ssq(case))
    same_bits(a, b)
    same_bits(a, c)


# ---- routing in update_A_ --------------------------------------------------------------------------------------------------
def _reg(pkg, case):
    """A one-view FeatureSetARDReg holding the case (the view is the whole model: N = Nv)."""
    assert case["N"] == case["Nv"]
    reg = pkg.regularizers.FeatureSetARDReg(case["K"], [1] * case["N"], [case["S"]], [list(range(case["L"]))],
                                            alpha0=case["alpha0"], v0=case["v0"], lr=case["lr"])
    reg.alpha = case["alpha"].copy()
    reg.lambda_ = (case["lam"].copy(),)
    return reg


def _update_A(pkg, ctx, case, kernel):
    reg = _reg(pkg, case)
    ed.load(ctx, case)
    best = pkg.update_A_(reg, case["Y"], max_epochs=case["max_epochs"], term_iter=case["term_iter"], atol=case["atol"],
                         verbosity=0, ctx=ctx, kernel=kernel)
    sl = slice(case["c0"] - 1, case["c1"])
    return dict(A=reg.A[0], ssq=reg.ssq_grad[0], beta=np.asfortranarray(reg.beta[:, sl]), best=best[0], epochs=0), reg


def test_auto_takes_the_dense_entry_at_or_below_its_capacity(pkg, ctx):
    case = fr.make_case(**fr.BASE)
    auto, reg = _update_A(pkg, ctx, case, "auto")
    dense, _ = _update_A(pkg, ctx, case, "dense")
    sparse, reg_s = _update_A(pkg, ctx, case, "sparse")
    same_bits(auto, dense)
    assert "_S_csr" not in vars(reg) and "_S_csr" in vars(reg_s)
    want = fr.run_oracle(case)
    for k, v in fr.errors(sparse, want, fr.fresh_ssq(case)).items():
        assert v <= fr.TOL[k], (k, v)


def test_auto_takes_the_sparse_entry_above_it_and_dense_is_refused(pkg, ctx):
    case, want = fs.sparse_row("K33_L497")
    auto, reg = _update_A(pkg, ctx, case, "auto")
    sparse, _ = _update_A(pkg, ctx, case, "sparse")
    same_bits(auto, sparse)
    assert "_S_csr" in vars(reg)
    for k, v in fr.errors(auto, want, fr.fresh_ssq(case)).items():
        assert v <= fr.TOL[k], (k, v)
    with pytest.raises(pkg.PMFError, match="capacity"):
        _update_A(pkg, ctx, case, "dense")


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _args(case, **over):
    rowptr, col, val = ctx_csr(case)
    a = dict(start1=case["c0"], stop1=case["c1"], L=case["L"], rowptr=rowptr, col=col, val=val.copy(), alpha=case["alpha"],
             lam=case["lam"], max_epochs=case["max_epochs"], term_iter=case["term_iter"], ssq="fill", A="fill")
    a.update(over)
    return a


def _edit(arr, index, value):
    out = arr.copy()
    out[index] = value
    return out


def _swap_first_two_of_row0(case):
    rowptr, col, _ = ctx_csr(case)
    assert rowptr[1] >= 2
    out = col.copy()
    out[0], out[1] = col[1], col[0]
    return out


REFUSALS = {      # name -> (arguments, a word of the message)
    "empty_range": (lambda c: _args(c, start1=5, stop1=4), "col_start1"),
    "reversed_range": (lambda c: _args(c, start1=10, stop1=5), "col_start1"),
    "start_0": (lambda c: _args(c, start1=0, stop1=c["Nv"] - 1), "col_start1"),
    "stop_past_N": (lambda c: _args(c, start1=2, stop1=c["N"] + 1), "col_stop1"),
    "L_0": (lambda c: _args(c, L=0), "L must"),
    "L_negative": (lambda c: _args(c, L=-3), "L must"),
    "max_epochs_negative": (lambda c: _args(c, max_epochs=-1), "max_epochs"),
    "term_iter_0": (lambda c: _args(c, term_iter=0), "term_iter"),
    "term_iter_negative": (lambda c: _args(c, term_iter=-1), "term_iter"),
    "null_rowptr": (lambda c: _args(c, rowptr=None), "rowptr is"),
    "null_col": (lambda c: _args(c, col=None), "col is"),
    "null_val": (lambda c: _args(c, val=None), "val is"),
    "null_alpha": (lambda c: _args(c, alpha=None), "alpha is"),
    "null_lambda": (lambda c: _args(c, lam=None), "lambda is"),
    "null_ssq_grad": (lambda c: _args(c, ssq=None), "ssq_grad is"),
    "null_A": (lambda c: _args(c, A=None), "A is"),
    "rowptr0_not_0": (lambda c: _args(c, rowptr=_edit(ctx_csr(c)[0], 0, 1)), "rowptr[0]"),
    "rowptr_decreasing": (lambda c: _args(c, rowptr=_edit(ctx_csr(c)[0], 3, ctx_csr(c)[0][2] - 1)), "rowptr decreases"),
    "col_negative": (lambda c: _args(c, col=_edit(ctx_csr(c)[1], 0, -1)), "col["),
    "col_at_Nv": (lambda c: _args(c, col=_edit(ctx_csr(c)[1], ctx_csr(c)[0][1] - 1, c["Nv"])), "col["),
    "cols_unsorted": (lambda c: _args(c, col=_swap_first_two_of_row0(c)), "ascending"),
    "cols_repeated": (lambda c: _args(c, col=_edit(ctx_csr(c)[1], 1, ctx_csr(c)[1][0])), "ascending"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_name_the_argument_and_leave_the_context_usable(pkg, ctx, name):
    """Host-side argument checks, made before anything is allocated or launched: an error code and a message that names
    the argument, no output touched, and a good call right after.  No kernel runs on a refused input."""
    good, want = fs.table_row("REFUSALS", "good_after_refusal")
    ed.load(ctx, good)
    make, word = REFUSALS[name]
    a = make(good)
    rows = max(a["L"], good["L"], 1)
    ssq = None if a["ssq"] is None else np.full((rows, good["K"]), 0.25, F)
    A = None if a["A"] is None else np.full((rows, good["K"]), -1.0, F)
    beta = np.full((good["K"], good["Nv"] + 1), -2.0, F, order="F")
    rc, best, epochs, msg = raw_csr(ctx, a["start1"], a["stop1"], a["L"], a["rowptr"], a["col"], a["val"], a["alpha"], a["lam"],
                                    good["alpha0"], good["v0"], good["lr"], ssq, A, a["max_epochs"], a["term_iter"],
                                    good["atol"], beta)
    print(f"FSARD_REFUSAL {name}: {msg}")
    assert rc != 0 and "pmf_fsard_update_A_csr" in msg and word in msg, (rc, msg)
    assert np.isnan(best) and epochs == -7
    assert (ssq is None or np.all(ssq == F(0.25))) and (A is None or np.all(A == F(-1.0))) and np.all(beta == F(-2.0))
    with pytest.raises(pkg.PMFError):
        ctx._chk(rc)
    ed.check(name + "_then_good", run_csr(ctx, good), want, fr.fresh_ssq(good))


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_fit_of_a_model_whose_feature_sets_exceed_the_dense_capacity(pkg):
    """60 x 96, two views of 48 columns, K = 33, 500 feature sets of 3-8 members per view: L * K = 16500 per view, which
    the dense entry refuses.  fit_ completes; A >= 0 and not all zero; reg.beta is (alpha0 - 1)(v0 + A'S)."""
    rng = np.random.default_rng(11)
    M, N, K, L = 60, 96, 33, 500
    D = rng.standard_normal((M, N)).astype(F)
    fsets = {v: [sorted(int(j) for j in 48 * (v - 1) + 1 + rng.choice(48, size=rng.integers(3, 9), replace=False))
                 for _ in range(L)] for v in (1, 2)}
    model = pkg.make_model(D, K=K, feature_views=[1] * 48 + [2] * 48, feature_sets_dict=fsets, Y_fsard=True, rng=rng)
    reg = model.matfac.Y_reg
    assert all(S.shape == (L, 48) and S.shape[0] * K == 16500 > fr.CAPACITY for S in reg.S)
    pkg.fit_(model, max_epochs=5, fsard_max_iter=2, fsard_max_A_iter=20, verbosity=0)
    beta0 = np.float64(reg.alpha0) - 1.0
    for cr, S, A in zip(reg.col_ranges, reg.S, reg.A):
        assert np.all(np.isfinite(A)) and np.all(A >= 0) and A.any()
        want = beta0 * (np.float64(reg.v0) + A.astype(np.float64).T @ S.astype(np.float64))
        err = fr.norm_err(reg.beta[:, cr.slice0()], want)
        print(f"FSARD_FIT view {cr}: nonzero A {np.mean(A > 0):.3f} beta err {err:.3e}")
        assert err <= fr.TOL["beta"], err
