"""MatFacModel and the replacement of `MF.fit!` (the un-vendored MatFac.jl inner loop, called at src/fit.jl:24).

`fit_(matfac, ctx, ...)` marshals the model through the C ABI (include/pmf_hip.h), runs pmf_fit on the GPU (or
the row-sharded loop of parallel.py when torch.distributed is initialised with more than one rank) and copies
the trained parameters back into the model's numpy arrays -- exactly what the Julia shim's `mf_fit!` does."""
import numpy as np

from .layers import BatchScale, BatchShift, ColScale, ColShift, FrozenLayer, Identity
from .optimizers import AdaGrad
from .regularizers import (BatchArrayReg, ColParamReg, FrozenRegularizer, SequenceReg, ZeroReg)
from .util import ids_to_ranges, unique

VALID_LOSSES = ["normal", "bernoulli", "bernoulli_sq_hinge", "poisson", "ordinal3", "ordinal_sq_hinge3"]  # util.jl:128
SUPPORTED_LOSSES = ("normal", "bernoulli", "poisson", "bernoulli_sq_hinge", "ordinal_sq_hinge3")
# thresholds (t0, t1, t2) of the two squared-hinge models (one kind of the library, include/pmf_hip.h).  SELF-SPECIFIED
# (DESIGN.md section 2): ordinal_sq_hinge3's default (-0.5, 0.5) is ours, MatFac's is not visible.
HINGE_THRESHOLDS = {"bernoulli_sq_hinge": (0.0, np.inf, np.inf), "ordinal_sq_hinge3": (-np.inf, -0.5, 0.5)}


class CompositeNoise:
    """MatFac's CompositeNoise{noises, col_ranges} as used at src/fit.jl:227, plus the per-column weights set by
    MF.set_weight! (src/fit.jl:157, 180).  `thresholds` has one entry per range: None, or the (t0, t1, t2) of a
    squared-hinge range (set_thresholds_): constants of the fit unless `train_thresholds` is on (train_thresholds_), in
    which case a fit called with update_noise_models=True trains them, one triple per range (DESIGN.md section 2,
    Deviation 5), and writes the trained triples back here."""

    def __init__(self, feature_distributions):
        dists = list(feature_distributions)
        self.col_ranges = tuple(ids_to_ranges(dists))
        self.noises = tuple(unique(dists))
        for d in self.noises:
            if d not in VALID_LOSSES:
                raise ValueError(f"unknown distribution {d!r}; valid: {VALID_LOSSES}")
            if d not in SUPPORTED_LOSSES:
                raise NotImplementedError(f"noise model {d!r} is not implemented by the HIP path "
                                          f"(supported: {SUPPORTED_LOSSES}); see DESIGN.md 'out of scope'")
        self.thresholds = [HINGE_THRESHOLDS.get(d) for d in self.noises]
        self.train_thresholds = False
        self.weights = np.ones(len(dists), dtype=np.float32)

    def train_thresholds_(self, on=True):
        """Lets the fits that are called with update_noise_models=True (mf_fit!'s default) train the thresholds."""
        self.train_thresholds = bool(on)
        return self

    def set_weight_(self, w):
        self.weights = np.asarray(w, dtype=np.float32).copy()

    def set_thresholds_(self, name_or_index, t):
        """Thresholds of one squared-hinge range, by its distribution name or its index among the ranges:
        bernoulli_sq_hinge takes one number (or (t0, inf, inf)), ordinal_sq_hinge3 two (t1, t2) (or (-inf, t1, t2))."""
        r = self.noises.index(name_or_index) if isinstance(name_or_index, str) else int(name_or_index)
        if self.thresholds[r] is None:
            raise ValueError(f"noise model {self.noises[r]!r} has no thresholds")
        t = [float(x) for x in np.atleast_1d(t)]
        if len(t) != 3:
            want = 1 if self.noises[r] == "bernoulli_sq_hinge" else 2
            if len(t) != want:
                raise ValueError(f"{self.noises[r]!r} takes {want} threshold(s) or the full triple, got {len(t)}")
            t = [t[0], np.inf, np.inf] if want == 1 else [-np.inf, t[0], t[1]]
        if not (t[0] <= t[1] <= t[2]):
            raise ValueError(f"thresholds must be ordered, got {t}")
        self.thresholds[r] = tuple(t)


class MatFacModel:
    """MatFacModel(M, N, K, feature_distributions; col_transform, X_reg, Y_reg, col_transform_reg) (src/model.jl:69-72).
    X is K x M, Y is K x N (column-major semantics; stored as Fortran-ordered float32).
    `row_shard` = (lo, hi, M_total) with M = hi - lo: X is drawn for all M_total samples and columns lo:hi are kept, so
    that the shards of one seed concatenate to the unsharded X and the draw of Y that follows is the same on every rank."""

    def __init__(self, M, N, K, feature_distributions, col_transform=None, X_reg=None, Y_reg=None,
                 col_transform_reg=None, rng=None, row_shard=None):
        rng = rng or np.random.default_rng()
        lo, hi, M_total = (0, M, M) if row_shard is None else row_shard
        # MatFac's own initialisation is not visible (un-vendored); self-specified: N(0,1)/sqrt(K)
        self.X = np.asfortranarray((rng.standard_normal((K, M_total)) / np.sqrt(K)).astype(np.float32)[:, lo:hi])
        self.Y = np.asfortranarray((rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32))
        self.col_transform = col_transform
        self.noise_model = CompositeNoise(feature_distributions)
        self.X_reg = X_reg if X_reg is not None else ZeroReg()
        self.Y_reg = Y_reg if Y_reg is not None else ZeroReg()
        self.col_transform_reg = col_transform_reg

    @property
    def K(self):
        return self.X.shape[0]


# --------------------------------------------------------------------------------------------------------
def _batch_views(col_transform):
    """The BatchArrays of layers 2 and 4 as the C ABI's per-view dicts (they share ranges and row batches by
    construction, layers.jl:247-248).  Returns ([], None, None) when the layers are the identity."""
    l2, l4 = col_transform.unwrapped(2), col_transform.unwrapped(4)
    ba2 = l2.logdelta if isinstance(l2, BatchScale) else None
    ba4 = l4.theta if isinstance(l4, BatchShift) else None
    ref = ba2 if ba2 is not None else ba4
    if ref is None:
        return [], None, None
    views = []
    for v, cr in enumerate(ref.col_ranges):
        nb, Nv = ref.values[v].shape
        ld = ba2.values[v] if ba2 is not None else np.zeros((nb, Nv))
        th = ba4.values[v] if ba4 is not None else np.zeros((nb, Nv))
        views.append(dict(start1=cr.start, stop1=cr.stop, batch_of_row=ref.row_batches[v], logdelta=ld, theta=th))
    return views, ba2, ba4


def marshal(mf, ctx, with_xreg=True, with_yreg=True):
    """Host model -> device (parameters, noise model, regularizers).  The data matrix is handled by the caller.
    A regularizer is only marshalled for a factor that is going to be updated: the loop never evaluates the others
    (and the reference keeps an X_reg of the wrong shape attached while regressing Y only, src/fit.jl:397-428)."""
    ctx.set_factors(mf.X, mf.Y)
    ct = mf.col_transform
    l1, l3 = ct.unwrapped(1), ct.unwrapped(3)
    ctx.set_col_params(l1.logsigma if isinstance(l1, ColScale) else np.zeros(ctx.N, np.float32),
                       l3.mu if isinstance(l3, ColShift) else np.zeros(ctx.N, np.float32))
    views, _, _ = _batch_views(ct)
    ctx.set_batch_views(views)
    nm = mf.noise_model
    ctx.set_noise([(r.start, r.stop) for r in nm.col_ranges], list(nm.noises), nm.weights)
    hinge = [(r, t) for r, t in zip(nm.col_ranges, nm.thresholds) if t is not None]
    if hinge:
        ctx.set_noise_thresholds([(r.start, r.stop) for r, _ in hinge], [t for _, t in hinge])
    ctx.clear_xreg()
    if with_xreg:
        mf.X_reg.add_to(ctx, "X")
    ctx.clear_yreg()
    if with_yreg:
        mf.Y_reg.add_to(ctx, "Y")
    sr = mf.col_transform_reg
    kw = {}
    if isinstance(sr, SequenceReg):
        regs = [r.reg if isinstance(r, FrozenRegularizer) else r for r in sr.regs]
        if isinstance(regs[0], ColParamReg) and isinstance(regs[2], ColParamReg):
            kw.update(ranges=[(r.start, r.stop) for r in regs[0].col_ranges],
                      w_logsigma=np.array(regs[0].weights, np.float32), c_logsigma=np.array(regs[0].centers, np.float32),
                      w_mu=np.array(regs[2].weights, np.float32), c_mu=np.array(regs[2].centers, np.float32))
        if views and isinstance(regs[1], BatchArrayReg) and isinstance(regs[3], BatchArrayReg):
            kw.update(w_logdelta=list(regs[1].weights), c_logdelta=list(regs[1].centers),
                      w_theta=list(regs[3].weights), c_theta=list(regs[3].centers))
    ctx.set_layer_regs(**kw)


def unmarshal(mf, ctx, update_X, update_Y, update_col_layers, update_thresholds=False):
    """Device -> host for the parameter groups that were trained."""
    if update_thresholds:
        nm, t = mf.noise_model, ctx.get_noise_thresholds()
        for r, cr in enumerate(nm.col_ranges):
            if nm.thresholds[r] is not None:
                nm.thresholds[r] = tuple(float(x) for x in t[cr.start - 1])
    if update_X or update_Y:
        X, Y = ctx.get_factors()
        if update_X:
            mf.X[...] = X
        if update_Y:
            mf.Y[...] = Y
    if update_col_layers:
        ct = mf.col_transform
        ls, mu = ctx.get_col_params()
        l1, l3 = ct.unwrapped(1), ct.unwrapped(3)
        if isinstance(l1, ColScale):
            l1.logsigma[...] = ls
        if isinstance(l3, ColShift):
            l3.mu[...] = mu
        views, ba2, ba4 = _batch_views(ct)
        for v in range(len(views)):
            ld, th = ctx.get_batch_view(v)
            if ba2 is not None:
                ba2.values[v][...] = ld
            if ba4 is not None:
                ba4.values[v][...] = th


def fit_(mf, ctx, opt=None, lr=0.01, update_X=False, update_Y=False, update_col_layers=False, max_epochs=1000,
         epoch=1, abs_tol=1e-9, rel_tol=1e-6, tol_max_iters=3, verbosity=0, print_iter=10, capacity=10 ** 8,
         keep_history=True, dist=None, group=None, update_noise_models=False, holdout_every=0, holdout_patience=0,
         holdout_min_delta=0.0, holdout_restore_best=False, **ignored):
    """MF.fit!(matfac, data; ...) -> history dict with "term_code", "epochs", "loss" (src/fit.jl:24-38, 61-69).
    holdout_every > 0: the fit tracks the loss of the context's hold-out set (holdout.set_holdout_) every so many epochs,
    ends with "holdout_increase" after holdout_patience > 0 evaluations without an improvement of more than
    holdout_min_delta, and with holdout_restore_best returns the factors of the best evaluation (the optimizer state is
    not rolled back); the history gains "holdout_loss", "holdout_epochs" and "best_epoch".  Not on a row-sharded fit.
    The options hold for this call: tracking that the caller set on the context itself is put back afterwards.
    update_noise_models is honoured only when the noise model says so (CompositeNoise.train_thresholds_): the squared-hinge
    thresholds then train inside pmf_fit and the trained triples are written into noise_model.thresholds.  The row-sharded
    loop of parallel.py runs on the step-level API, which keeps thresholds constant."""
    opt = opt if opt is not None else AdaGrad(lr)
    marshal(mf, ctx, with_xreg=update_X, with_yreg=update_Y)
    if opt._bound_ctx != id(ctx):          # a new optimizer object: fresh accumulators (src/fit.jl:55)
        ctx.set_optimizer(**opt.params())
        opt._bound_ctx = id(ctx)
    else:                                   # same object, possibly halved eta (src/fit.jl:64): keep the state
        ctx.set_lr(opt.eta)
    ct, sr = mf.col_transform, mf.col_transform_reg
    kw = dict(update_X=update_X, update_Y=update_Y, update_col_layers=update_col_layers,
              frozen_layers=ct.frozen_mask() | sum(1 << i for i, l in enumerate(ct.layers) if isinstance(l, Identity)),
              frozen_regs=sr.frozen_mask() if isinstance(sr, SequenceReg) else 0,
              max_epochs=max_epochs, epoch=epoch, abs_tol=abs_tol, rel_tol=rel_tol, tol_max_iters=tol_max_iters,
              verbosity=verbosity, print_iter=print_iter)
    if dist is not None and dist.is_initialized() and dist.get_world_size(group) > 1:
        if holdout_every:
            raise ValueError("hold-out tracking (holdout_every > 0) is not supported on a row-sharded fit: "
                             "score with holdout.holdout_scores between fits instead")
        from . import parallel
        h = parallel.fit_distributed(ctx, dist=dist, group=group, **kw)
        train_thr = False
    else:
        train_thr = bool(update_noise_models and mf.noise_model.train_thresholds)
        sticky = dict(ctx.holdout_tracking)
        if holdout_every:
            ctx.set_holdout_tracking(holdout_every, holdout_patience, holdout_min_delta, holdout_restore_best)
        try:
            h = ctx.fit(capacity=capacity, update_noise_models=train_thr, **kw)
        finally:
            if holdout_every:
                ctx.set_holdout_tracking(**sticky)
    unmarshal(mf, ctx, update_X, update_Y, update_col_layers, update_thresholds=train_thr)
    for reg, which, on in ((mf.X_reg, "X", update_X), (mf.Y_reg, "Y", update_Y)):
        if on and hasattr(reg, "read_back"):      # the network term's virtual nodes (NetworkRegularizer.x_virtual)
            reg.read_back(ctx, which)
    return h
