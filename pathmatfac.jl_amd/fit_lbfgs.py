"""fit_lbfgs! (src/fit_lbfgs.jl): L-BFGS over the factors X and Y, run by the HIP library (pmf_fit_lbfgs).
Trailing underscore = the reference's `!`."""
from . import matfac as MF


def fit_lbfgs_(mf, ctx, m=10, max_iter=1000, rel_tol=1e-9, abs_tol=1e-6, backtrack_shrinkage=0.8, print_prefix="",
               print_iter=10, verbosity=1):
    """fit_lbfgs!(model::MatFacModel, D; ...) (src/fit_lbfgs.jl:170-243) with the reference's defaults.  Marshals the model
    with both regularizers, runs the loop on the device and copies X and Y back.  Returns a history dict with "term_code",
    "iters" and "loss" (the loss after every line search), plus the library's counters.  The data matrix is the context's.
    `print_prefix` is printed once by the caller's stage line only: the library's own progress lines carry no prefix."""
    MF.marshal(mf, ctx, with_xreg=True, with_yreg=True)
    h = ctx.fit_lbfgs(m=m, max_iter=max_iter, rel_tol=rel_tol, abs_tol=abs_tol, backtrack_shrinkage=backtrack_shrinkage,
                      verbosity=verbosity, print_iter=print_iter)
    MF.unmarshal(mf, ctx, True, True, False)
    return h
