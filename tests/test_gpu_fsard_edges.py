"""pmf_fsard_update_A (csrc/pmf_fsard.hip, the FeatureSetARD outer loop) at its geometry, state and stopping edges, every
row against oracle/fsard_oracle.py in float64 on A, ssq_grad entry by entry, beta, the best loss and epochs_run.  The rows
and the conditions that keep them from passing vacuously are in tests/fsard_ref.py and tests/test_fsard_cases.py.

Bounds (fsard_ref.MEASURED / TOL).  "float32" is the worst discrepancy of a plain numpy float32 restatement of the loop
from the float64 oracle over every row of the tables; the bound is 20 x that; "device" is the worst figure seen on an
MI355X over the same rows (this file, and the two update_A tests of test_gpu_stages.py):

    quantity                                         float32    bound      device
    A          |dA| / |A|                            5.0e-7     1.0e-5     3.9e-7
    beta       |dbeta| / |beta|                      4.5e-7     9.0e-6     8.8e-7
    ssq_grad   max |d - d_o| / max(d_o, 1e-6 max d_o),
               d = ssq_grad out - in                 1.9e-5     3.8e-4     1.8e-5
    best loss  relative                              2.1e-7     4.2e-6     3.8e-7

The value of the attached Y regularizer (the only window on the device copy of its beta) is held to fsard_ref.REG_TOL =
1e-5 of its closed form (the reasoning is beside that constant); the device's worst was 4.1e-8.

Every test prints its figures ("FSARD_ERR <row> ...", "FSARD_REG <row> ...") before it asserts: run with -s to see them."""
import ctypes as C

import numpy as np
import pytest

import fsard_ref as fr

pytestmark = pytest.mark.gpu
F = np.float32


# ---- plumbing ------------------------------------------------------------------------------------------------------------
def load(ctx, case, yreg="fsard", Y=None):
    """The case's model on the context: Y resident, no data, and the chosen Y term with beta = BETA_UPLOADED everywhere."""
    N, K = case["N"], case["K"]
    ctx.set_data(np.full((1, N), np.nan, F))
    ctx.set_factors(np.zeros((K, 1), F), case["Y"] if Y is None else Y)
    ctx.clear_xreg()
    ctx.clear_yreg()
    if yreg == "fsard":
        ctx.add_yreg_fsard(fr.reg_alpha(N), np.full((K, N), fr.BETA_UPLOADED, F))
    elif yreg == "ard":
        ctx.add_yreg_ard([(1, N // 2), (N // 2 + 1, N)], ARD_ALPHA, ARD_BETA)
    else:
        assert yreg is None


ARD_ALPHA, ARD_BETA = [1.2, 1.3], [0.5, 0.7]       # a plain ARD term: (alpha, beta) per column range


def ard_arrays(case):
    """The plain ARD term of `load`, expanded to alpha[N] and beta[K x N]."""
    N, h = case["N"], case["N"] // 2
    al, be = np.full(N, ARD_ALPHA[0]), np.full((case["K"], N), ARD_BETA[0])
    al[h:], be[:, h:] = ARD_ALPHA[1], ARD_BETA[1]
    return al.astype(F), be.astype(F)


def run(ctx, case, ssq=None, **over):
    kw = dict(max_epochs=case["max_epochs"], term_iter=case["term_iter"], atol=case["atol"])
    kw.update(over)
    ssq = fr.fresh_ssq(case) if ssq is None else ssq.copy()
    A, beta, best, epochs = ctx.fsard_update_A(case["c0"], case["c1"], case["S"], case["alpha"], case["lam"], case["alpha0"],
                                               case["v0"], case["lr"], ssq, **kw)
    return dict(A=A, ssq=ssq, beta=beta, best=best, epochs=epochs)


def check(name, got, want, ssq_in, ssq_in_want=None):
    """Prints the four figures, then holds them to fsard_ref.TOL; epochs_run must be the oracle's."""
    e = fr.errors(got, want, ssq_in, ssq_in_want)
    print(f"FSARD_ERR {name} " + " ".join(f"{k}={v:.3e}" for k, v in e.items()) + f" epochs={got['epochs']}/{want['epochs']}")
    assert np.all(np.isfinite(got["A"])) and np.all(np.isfinite(got["ssq"])) and np.all(np.isfinite(got["beta"]))
    assert got["epochs"] == want["epochs"], (got["epochs"], want["epochs"])
    for k, v in e.items():
        assert v <= fr.TOL[k], (name, k, v, fr.TOL[k])
    return e


def yreg_value(ctx):
    """One evaluation of the attached Y regularizer (a step of 1e-6 moves Y after the value is taken)."""
    ctx.set_optimizer("adagrad", lr=1e-6)
    o = ctx.make_opts(update_Y=True)
    ctx.epoch_begin(o)
    ctx.epoch_step_shared(o)
    return ctx.epoch_loss()[1]


def compare_case(ctx, name, spec, yreg="fsard"):
    case = fr.make_case(**spec)
    load(ctx, case, yreg)
    got = run(ctx, case)
    check(name, got, fr.run_oracle(case), fr.fresh_ssq(case))
    return case, got


def raw_update_A(ctx, start1, stop1, L, S, alpha, lam, alpha0, v0, lr, ssq, A, max_epochs, term_iter, atol, beta=None):
    """pmf_fsard_update_A as a C caller sees it (the Python binding always passes beta_out and derives L and the range
    from S).  -> (return code, best_loss, epochs_run, message)"""
    def fp(a):
        return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else C.POINTER(C.c_float)()
    best, ep = C.c_double(np.nan), C.c_int(-7)
    rc = ctx.lib.pmf_fsard_update_A(ctx._h, C.c_int64(start1), C.c_int64(stop1), int(L), fp(S), fp(alpha), fp(lam),
                                    C.c_float(alpha0), C.c_float(v0), C.c_float(lr), fp(ssq), fp(A), int(max_epochs),
                                    int(term_iter), C.c_double(atol), C.byref(best), C.byref(ep), fp(beta))
    return rc, best.value, ep.value, ctx.lib.pmf_last_error().decode()


# ---- geometry --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fr.K_EDGES))
def test_K_edges(ctx, name):
    """K walks in chunks of 32; beta_out leaves the device with a pitch of Kp."""
    compare_case(ctx, name, fr.K_EDGES[name])


@pytest.mark.parametrize("name", list(fr.OUTPUTS))
def test_outputs_per_thread(ctx, name):
    """L * K at 255 / 256 / 257 (one output per thread or two), at the capacity 16384 both ways, L = 1, a dense S."""
    compare_case(ctx, name, fr.OUTPUTS[name])


@pytest.mark.parametrize("name", list(fr.CW_EDGES))
def test_sub_slice_width_boundary(ctx, name):
    """The last shapes that keep 256 columns per sub-slice and the first that halve it, each at N_v = CW - 1, CW, CW + 1,
    and 32 * 128 + 1 columns, where a workgroup walks two sub-slices."""
    spec = fr.CW_EDGES[name]
    cw = 256 if fr.lds_bytes(spec["L"], spec["K"], 256) <= 150 * 1024 else 128             # the LDS rule, restated
    assert cw == fr.sub_slice_width(spec["L"], spec["K"]) and spec["Nv"] in (cw - 1, cw, cw + 1, 32 * cw + 1)
    compare_case(ctx, name, spec)


@pytest.mark.parametrize("name", list(fr.NV_POSITIONS))
def test_view_width_and_position(ctx, name):
    """N_v around one sub-slice and around 32 of them, the view first, last and in the middle of a wider model: the
    call's results, and the attached term's device beta -- new inside the view, as uploaded outside it."""
    case, got = compare_case(ctx, name, fr.NV_POSITIONS[name])
    value = yreg_value(ctx)
    want = fr.reg_value(fr.reg_alpha(case["N"]), fr.beta_after(case, got["beta"]), case["Y"])
    print(f"FSARD_REG {name} rel={abs(value - want) / want:.3e}")
    assert abs(value - want) <= fr.REG_TOL * want, (value, want)


# ---- where beta goes -------------------------------------------------------------------------------------------------------
def test_beta_goes_into_an_attached_featureset_ard_term(ctx):
    case, got = compare_case(ctx, "beta_dest_fsard", fr.BETA_DEST)
    want = fr.reg_value(fr.reg_alpha(case["N"]), fr.beta_after(case, got["beta"]), case["Y"])
    value = yreg_value(ctx)
    assert abs(value - want) <= fr.REG_TOL * want, (value, want)


def test_beta_without_a_Y_term_comes_from_a_temporary(ctx):
    """No term attached: beta_out is filled from a temporary of the view's columns (K = 20 < Kp = 32)."""
    compare_case(ctx, "beta_dest_none", fr.BETA_DEST, yreg=None)


def test_beta_out_may_be_null(ctx):
    """A C caller that passes beta_out = NULL still gets A, ssq_grad, the loss -- and the attached term's device beta."""
    case = fr.make_case(**fr.BETA_DEST)
    want = fr.run_oracle(case)
    load(ctx, case, "fsard")
    ssq, A = fr.fresh_ssq(case), np.full((case["L"], case["K"]), np.nan, F)
    rc, best, epochs, msg = raw_update_A(ctx, case["c0"], case["c1"], case["L"], case["S"], case["alpha"], case["lam"],
                                         case["alpha0"], case["v0"], case["lr"], ssq, A, case["max_epochs"],
                                         case["term_iter"], case["atol"], beta=None)
    assert rc == 0, msg
    got = dict(A=A, ssq=ssq, beta=want["beta"], best=best, epochs=epochs)          # no beta came back: nothing to compare
    check("beta_dest_null", got, want, fr.fresh_ssq(case))
    value = yreg_value(ctx)
    ref = fr.reg_value(fr.reg_alpha(case["N"]), fr.beta_after(case, want["beta"]), case["Y"])
    assert abs(value - ref) <= 2 * fr.REG_TOL * ref, (value, ref)                  # (the oracle's beta: once more rounding)
    # ... and with no term either, the call has nowhere to put beta and still succeeds
    load(ctx, case, None)
    ssq2, A2 = fr.fresh_ssq(case), np.full((case["L"], case["K"]), np.nan, F)
    rc, best2, epochs2, msg = raw_update_A(ctx, case["c0"], case["c1"], case["L"], case["S"], case["alpha"], case["lam"],
                                           case["alpha0"], case["v0"], case["lr"], ssq2, A2, case["max_epochs"],
                                           case["term_iter"], case["atol"], beta=None)
    assert rc == 0, msg
    assert best2 == best and epochs2 == epochs and np.array_equal(A2, A) and np.array_equal(ssq2, ssq)


def test_a_plain_ard_term_keeps_its_beta(ctx):
    """include/pmf_hip.h: beta is written into the device copy of the Y regularizer's beta when one is attached with
    pmf_add_yreg_fsard.  fit_feature_set_ard_ runs update_A_ on a context that still holds the plain ARD term of fit_ard_:
    that term's value must be what it was, and beta_out must still be right."""
    case = fr.make_case(**fr.BETA_DEST)
    al, be = ard_arrays(case)
    load(ctx, case, "ard")
    got = run(ctx, case)
    want = fr.run_oracle(case)
    check("beta_dest_ard", got, want, fr.fresh_ssq(case))
    value = yreg_value(ctx)
    untouched = fr.reg_value(al, be, case["Y"])
    overwritten = be.astype(np.float64)
    overwritten[:, case["c0"] - 1:case["c1"]] = want["beta"]
    assert abs(fr.reg_value(al, overwritten, case["Y"]) - untouched) > 100 * fr.REG_TOL * untouched    # it would show
    print(f"FSARD_REG ard rel={abs(value - untouched) / untouched:.3e}")
    assert abs(value - untouched) <= fr.REG_TOL * untouched, (value, untouched)


# ---- stopping --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fr.MAX_EPOCHS))
def test_max_epochs_around_the_host_poll(ctx, name):
    """The host queues max(8, term_iter) iterations per look at the `done` flag and stops queuing at max_epochs, the
    device ends the loop at evaluation max_epochs: max_epochs = 0, 1 and around 8 and 16, the counter out of reach."""
    spec = fr.MAX_EPOCHS[name]
    case, got = compare_case(ctx, name, spec)
    assert got["epochs"] == spec["max_epochs"]
    if spec["max_epochs"] == 0:
        assert not got["A"].any()
        assert np.array_equal(got["beta"], np.full_like(got["beta"], (F(case["alpha0"]) - F(1)) * F(case["v0"])))
        assert np.array_equal(got["ssq"].view(np.uint32), fr.fresh_ssq(case).view(np.uint32))
        ssq = (1.0 + np.arange(case["L"] * case["K"], dtype=F).reshape(case["L"], case["K"])) * F(1e-3)
        again = run(ctx, case, ssq=ssq)
        assert np.array_equal(again["ssq"].view(np.uint32), ssq.view(np.uint32)) and again["epochs"] == 0


@pytest.mark.parametrize("name", list(fr.TERM_ITER))
def test_term_iter_on_a_trace_that_rises_and_recovers(ctx, name):
    """An oscillating run (rises, improvements past atol that reset the counter, a tail of rises): epochs_run and A_best
    -- which is not the last iterate -- for term_iter = 1, 3, 8, 9."""
    case, got = compare_case(ctx, name, fr.TERM_ITER[name])
    assert fr.norm_err(fr.last_iterate(case, got["epochs"]), got["A"]) > fr.A_BEST_GAP
    assert got["epochs"] < case["max_epochs"]


@pytest.mark.parametrize("name", ["strong_lambda", "strong_lambda_negative_atol"])
def test_strong_lambda_keeps_A_at_zero_and_counts_every_epoch(ctx, name):
    """A never leaves 0, so every loss equals the best one: not an improvement (new_loss < best_loss), whatever atol is --
    with atol < 0 an equal loss taken for an improvement would reset the counter and run to max_epochs."""
    case, got = compare_case(ctx, name, fr.STOP_RULES[name])
    assert got["epochs"] == case["term_iter"] < case["max_epochs"]
    assert not got["A"].any()
    rows = np.arange(case["L"]) != case["zero_row"]
    assert np.all(got["ssq"][rows] > fr.fresh_ssq(case)[rows])   # the accumulator still grows
    assert np.array_equal(got["ssq"][case["zero_row"]], fr.fresh_ssq(case)[case["zero_row"]])


def test_huge_atol_counts_every_improvement(ctx):
    case, got = compare_case(ctx, "atol_1e30", fr.STOP_RULES["atol_1e30"])
    assert got["epochs"] == case["term_iter"]
    assert fr.norm_err(got["A"], fr.last_iterate(case, got["epochs"])) <= fr.TOL["A"]       # A is the last iterate


def test_zero_atol(ctx):
    case, got = compare_case(ctx, "atol_0", fr.STOP_RULES["atol_0"])
    assert got["epochs"] == case["max_epochs"]


# ---- state -----------------------------------------------------------------------------------------------------------------
def test_second_call_starts_from_the_first_calls_accumulator(ctx):
    case = fr.make_case(**fr.STATE["two_calls"])
    load(ctx, case)
    o1 = fr.run_oracle(case)
    g1 = run(ctx, case)
    check("two_calls_1", g1, o1, fr.fresh_ssq(case))
    o2 = fr.run_oracle(case, ssq_in=o1["ssq"])
    g2 = run(ctx, case, ssq=g1["ssq"])
    check("two_calls_2", g2, o2, g1["ssq"], o1["ssq"])


def test_call_after_set_Y_reads_the_new_Y(ctx):
    a, b = fr.make_case(**fr.STATE["after_set_Y"]), fr.make_case(**fr.STATE["after_set_Y_second"])
    load(ctx, a)
    check("set_Y_before", run(ctx, a), fr.run_oracle(a), fr.fresh_ssq(a))
    ctx.set_Y(b["Y"])
    check("set_Y_after", run(ctx, a), fr.run_oracle(a, Y=b["Y"]), fr.fresh_ssq(a))


def test_larger_then_smaller_L_on_one_context(ctx):
    big, small = fr.make_case(**fr.STATE["L40"]), fr.make_case(**fr.STATE["L5"])
    load(ctx, big)
    check("L40", run(ctx, big), fr.run_oracle(big), fr.fresh_ssq(big))
    ctx.set_Y(small["Y"])
    check("L5", run(ctx, small), fr.run_oracle(small), fr.fresh_ssq(small))
    ctx.set_Y(big["Y"])
    check("L40_again", run(ctx, big), fr.run_oracle(big), fr.fresh_ssq(big))


# ---- reproducibility -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fr.REPRO))
def test_bitwise_reproducible(pkg, ctx, name):
    """A, ssq_grad, beta, the best loss and epochs_run are the same bits call to call and context to context."""
    case = fr.make_case(**fr.REPRO[name])
    load(ctx, case)
    a, b = run(ctx, case), run(ctx, case)
    other = pkg.Context(0)
    try:
        load(other, case)
        c = run(other, case)
    finally:
        other.close()
    check(name, a, fr.run_oracle(case), fr.fresh_ssq(case))
    for r in (b, c):
        for k in ("A", "ssq", "beta"):
            assert np.array_equal(a[k].view(np.uint32), r[k].view(np.uint32)), k
        assert np.float64(a["best"]).view(np.uint64) == np.float64(r["best"]).view(np.uint64) and a["epochs"] == r["epochs"]


# ---- refusals --------------------------------------------------------------------------------------------------------------
def _refusal_args(case, **over):
    a = dict(start1=case["c0"], stop1=case["c1"], L=case["L"], S=case["S"], alpha=case["alpha"], lam=case["lam"],
             max_epochs=case["max_epochs"], term_iter=case["term_iter"])
    a.update(over)
    return a


REFUSALS = {      # name -> (arguments, a word of the message)
    "LK_16385": (lambda c: _refusal_args(c, L=16385, S=np.zeros((16385, c["Nv"]), F)), "capacity"),          # K = 1 below
    "empty_range": (lambda c: _refusal_args(c, start1=5, stop1=4), "col_start1"),
    "reversed_range": (lambda c: _refusal_args(c, start1=10, stop1=5), "col_start1"),
    "start_0": (lambda c: _refusal_args(c, start1=0, stop1=c["Nv"] - 1), "col_start1"),
    "stop_past_N": (lambda c: _refusal_args(c, start1=2, stop1=c["N"] + 1), "col_stop1"),
    "L_0": (lambda c: _refusal_args(c, L=0), "L must"),
    "L_negative": (lambda c: _refusal_args(c, L=-3), "L must"),
    "term_iter_0": (lambda c: _refusal_args(c, term_iter=0), "term_iter"),
    "term_iter_negative": (lambda c: _refusal_args(c, term_iter=-1), "term_iter"),
    "max_epochs_negative": (lambda c: _refusal_args(c, max_epochs=-1), "max_epochs"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_name_the_argument_and_leave_the_context_usable(pkg, ctx, name):
    """Host-side argument checks: an error code and a message, no output touched, and a good call right after.
    term_iter <= 0 is refused (pinned): the reference would make one update before it looked at the counter, the device
    loop would end at "Iteration 0" -- neither is what a caller can mean."""
    spec = fr.REFUSAL_ROWS["good_after_refusal_K1" if name == "LK_16385" else "good_after_refusal"]
    good = fr.make_case(**spec)
    load(ctx, good)
    make, word = REFUSALS[name]
    a = make(good)
    rows = max(a["L"], good["L"], 1)
    ssq = np.full((rows, good["K"]), 0.25, F)
    A = np.full((rows, good["K"]), -1.0, F)
    beta = np.full((good["K"], good["Nv"] + 1), -2.0, F, order="F")
    if name == "LK_16385":
        assert a["L"] * good["K"] == fr.CAPACITY + 1
    rc, best, epochs, msg = raw_update_A(ctx, a["start1"], a["stop1"], a["L"], a["S"], a["alpha"], a["lam"], good["alpha0"],
                                         good["v0"], good["lr"], ssq, A, a["max_epochs"], a["term_iter"], good["atol"], beta)
    assert rc != 0 and "pmf_fsard_update_A" in msg and word in msg, (rc, msg)
    assert np.isnan(best) and epochs == -7
    assert np.all(ssq == F(0.25)) and np.all(A == F(-1.0)) and np.all(beta == F(-2.0))
    with pytest.raises(pkg.PMFError):
        ctx._chk(rc)
    check(name + "_then_good", run(ctx, good), fr.run_oracle(good), fr.fresh_ssq(good))

