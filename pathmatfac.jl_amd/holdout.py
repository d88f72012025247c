"""Hold-out entries (not in the reference's library; DESIGN.md section 2, Deviation 7): a validation set that lives on the
device beside the resident data, its loss, and the early-stopping options of the fit (include/pmf_hip_holdout.h).

    rows, cols = sample_holdout(model, 0.1, seed=0)
    set_holdout_(model, rows, cols)
    h = mf_fit_adapt_lr_(model, update_X=True, update_Y=True, holdout_every=1, holdout_patience=5, holdout_restore_best=True)
    scores = holdout_scores(model)
    clear_holdout_(model)

Entries are 0-based numpy indices here (the library's are 1-based)."""
import numpy as np

from .impute import _context
from .util import unique


def _check_entries(rows, cols, M, N):
    r, c = np.asarray(rows, dtype=np.int64).ravel(), np.asarray(cols, dtype=np.int64).ravel()
    if r.shape != c.shape:
        raise ValueError(f"hold-out set: {r.size} rows but {c.size} columns")
    bad = np.flatnonzero((r < 0) | (r >= M) | (c < 0) | (c >= N))
    if bad.size:
        e = int(bad[0])
        raise ValueError(f"hold-out set: entry {e} = ({int(r[e])}, {int(c[e])}) is outside 0..{M - 1} x 0..{N - 1}")
    key = c * M + r
    order = np.argsort(key, kind="stable")
    rep = np.flatnonzero(key[order][1:] == key[order][:-1])
    if rep.size:
        e = int(order[rep + 1].min())                      # the first entry, in the caller's order, that repeats an earlier one
        raise ValueError(f"hold-out set: entry {e} = ({int(r[e])}, {int(c[e])}) is a duplicate of an earlier entry")
    return r[order], c[order]


def sample_holdout(model, frac, seed, min_train_per_column=2):
    """(rows, cols), sorted by (column, row): round(frac x observed) entries drawn uniformly without replacement among the
    observed (finite) entries of model.data by numpy's default_rng(seed).  A column of which fewer than
    min_train_per_column observed entries would remain for training loses its draws."""
    if not 0.0 <= frac <= 1.0:
        raise ValueError(f"frac={frac} is outside [0, 1]")
    D = np.asarray(model.data)
    M, N = D.shape
    obs = np.flatnonzero(np.isfinite(D).ravel(order="F"))                  # column-major positions j M + i, ascending
    rng = np.random.default_rng(seed)
    pick = np.sort(rng.choice(obs, size=int(round(frac * obs.size)), replace=False))
    rows, cols = pick % M, pick // M
    n_obs = np.isfinite(D).sum(0)
    n_held = np.bincount(cols, minlength=N)
    keep = (n_obs - n_held >= min_train_per_column)[cols]
    return rows[keep].astype(np.int64), cols[keep].astype(np.int64)


def set_holdout_(model, rows, cols, device=0):
    """Holds the entries out of the model's data: on the device (pmf_set_holdout) and, in place, in model.data, whose values
    are kept on model.holdout = dict(rows, cols, values), sorted by (column, row), for clear_holdout_.  The host array keeps
    its identity and shape, so the resident copy is not uploaded again and the stages="host" arithmetic sees what the device
    sees.  Entries that are missing already are dropped.  Returns the number of entries held."""
    if getattr(model, "sharded", False):
        raise ValueError("hold-out sets are not supported on a row-sharded model (include/pmf_hip_holdout.h: tracking needs "
                         "one rank); hold entries out before sharding, or score with impute_entries")
    if getattr(model, "holdout", None) is not None:
        raise ValueError("the model already has a hold-out set: clear_holdout_ first")
    D = model.data
    r, c = _check_entries(rows, cols, *D.shape)
    seen = np.isfinite(D[r, c])
    r, c = r[seen], c[seen]
    ctx = model.device_context(device)
    n = ctx.set_holdout(r + 1, c + 1)
    if n != r.size:
        ctx.clear_holdout(restore=True)
        raise RuntimeError(f"the device holds {n} entries but model.data has {r.size} observed ones: the resident copy is "
                           "not the model's data (model.invalidate_device_data() after an in-place edit)")
    model.holdout = dict(rows=r, cols=c, values=D[r, c].copy()) if n else None
    D[r, c] = np.nan
    return n


def ensure_device_holdout_(model, device=0):
    """The model's context, holding model.holdout.  The device loses its set with the resident data -- release_device,
    invalidate_device_data, simulate_data_(resident) -- while model.data stays masked: a new upload would then carry the NaN
    and no set.  In that case the values go back into model.data, the matrix is uploaded again and the set is taken anew."""
    h = getattr(model, "holdout", None)
    ctx = model.device_context(device)
    if h is None or ctx.holdout_count() == h["rows"].size:
        return ctx
    ctx.clear_holdout(restore=False)
    model.data[h["rows"], h["cols"]] = h["values"]
    model.invalidate_device_data()
    ctx = model.device_context(device)
    n = ctx.set_holdout(h["rows"] + 1, h["cols"] + 1)
    model.data[h["rows"], h["cols"]] = np.nan
    if n != h["rows"].size:
        raise RuntimeError(f"the device holds {n} of the model's {h['rows'].size} hold-out entries")
    return ctx


def clear_holdout_(model, restore=True, device=0):
    """Drops the model's hold-out set; restore=True writes the kept values back, on the device and into model.data.  If the
    device has lost its set (see ensure_device_holdout_) the resident copy is the masked matrix: it is marked stale, so the
    next device_context() uploads what model.data then holds."""
    h = getattr(model, "holdout", None)
    ctx = model.device_context(device)
    lost = h is not None and ctx.holdout_count() != h["rows"].size
    ctx.clear_holdout(restore=restore and not lost)
    if h is not None and restore:
        model.data[h["rows"], h["cols"]] = h["values"]
        if lost:
            model.invalidate_device_data()
    model.holdout = None


def holdout_scores(model, device=0):
    """dict(total, loss_col (N,), n_col (N,), mean_col (N,; NaN without a held entry), views, view_loss, view_n) at the
    model's current parameters: the hold-out loss of pmf_holdout_loss, per column, and summed over the columns of every
    view of unique(model.feature_views)."""
    ensure_device_holdout_(model, device)
    ctx = _context(model, device)
    total, loss_col, n_col = ctx.holdout_loss()
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_col = np.where(n_col > 0, loss_col / n_col, np.nan)
    views = unique(model.feature_views)
    fv = np.asarray(model.feature_views, dtype=object)
    masks = [np.array([x == name for x in fv], dtype=bool) for name in views]
    return dict(total=total, loss_col=loss_col, n_col=n_col, mean_col=mean_col, views=list(views),
                view_loss=np.array([loss_col[m].sum() for m in masks]), view_n=np.array([n_col[m].sum() for m in masks]))
