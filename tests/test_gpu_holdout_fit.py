"""Hold-out tracking inside pmf_fit (include/pmf_hip_holdout.h): a tracking fit is bitwise the fit it watches, its trace holds
pmf_holdout_loss at the parameters each epoch's data pass saw, early stopping follows the rule of tests/holdout_ref.py on the
device's own trace, restore_best returns the best epoch's factors, and the Python layer carries all of it."""
import numpy as np
import pytest

import hinge_ref as hr
import holdout_ref as ho

pytestmark = pytest.mark.gpu
EPOCHS = 7


@pytest.fixture()
def fresh(pkg):
    made = []

    def make(p, rows, cols, lr=0.05, chunks=0):
        c = pkg.Context(0)
        made.append(c)
        hr.to_context(p, c)
        c.set_optimizer("adagrad", lr=lr)
        c.comm_set_chunks(chunks)
        c.set_holdout(rows + 1, cols + 1)
        return c

    yield make
    for c in made:
        c.close()


def state(c):
    return [*c.get_factors(), *c.get_opt_state("X"), *c.get_opt_state("Y")]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 3. tracking only ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunks", [1, 3])
@pytest.mark.parametrize("ux,uy", [(True, False), (False, True), (True, True)])
def test_tracking_changes_nothing_and_records_the_loss_the_epoch_saw(fresh, ux, uy, chunks):
    p = ho.problem(33)
    rows, cols = ho.held_sets(p)["wide"]
    opts = dict(update_X=ux, update_Y=uy, abs_tol=0, rel_tol=0)
    plain = fresh(p, rows, cols, chunks=chunks)
    h0 = plain.fit(max_epochs=EPOCHS, **opts)
    assert "holdout_loss" not in h0 and (plain.comm_info()["n_chunks"] == chunks or not uy)
    tracked = fresh(p, rows, cols, chunks=chunks)
    tracked.set_holdout_tracking(every=1, patience=0)
    h1 = tracked.fit(max_epochs=EPOCHS, **opts)
    assert h1["term_code"] == h0["term_code"] == "max_epochs" and np.array_equal(h1["loss"], h0["loss"])
    assert same(state(tracked), state(plain))
    assert h1["holdout_epochs"].tolist() == list(range(1, EPOCHS + 1)) and np.isfinite(h1["holdout_loss"]).all()
    assert h1["best_epoch"] == int(np.argmin(h1["holdout_loss"])) + 1
    # the entry of epoch e: pmf_holdout_loss after a fit of e - 1 epochs from the same start (e = 1: the initial parameters)
    for e in (1, 2, 5):
        c = fresh(p, rows, cols, chunks=chunks)
        if e > 1:
            c.fit(max_epochs=e - 1, **opts)
        assert c.holdout_loss()[0] == h1["holdout_loss"][e - 1], e
    third = fresh(p, rows, cols, chunks=chunks)
    third.set_holdout_tracking(every=3, patience=0)
    h3 = third.fit(max_epochs=EPOCHS, **opts)
    assert h3["holdout_epochs"].tolist() == [1, 4, 7] and np.array_equal(h3["holdout_loss"], h1["holdout_loss"][[0, 3, 6]])
    assert np.array_equal(h3["loss"], h0["loss"]) and same(state(third), state(plain))
    # a second fit on the same context starts its own count at its own first epoch, and tracking is sticky
    h4 = third.fit(max_epochs=EPOCHS + 4, epoch=EPOCHS + 1, **opts)
    assert h4["holdout_epochs"].tolist() == [EPOCHS + 1, EPOCHS + 4]
    third.clear_holdout()
    assert "holdout_loss" not in third.fit(max_epochs=2, **opts)                  # no set: tracking has nothing to do


# ---- 4. early stopping ------------------------------------------------------------------------------------------------------------
def test_early_stopping_follows_the_rule_and_restores_the_best_epoch(fresh):
    o = ho.OVERFIT
    p, rows, cols = ho.overfit_problem(0)
    opts = dict(update_X=True, update_Y=True, abs_tol=0, rel_tol=0)
    watch = fresh(p, rows, cols, lr=o["lr"])
    watch.set_holdout_tracking(every=1, patience=0)
    hw = watch.fit(max_epochs=o["max_epochs"], **opts)
    assert hw["term_code"] == "max_epochs" and len(hw["holdout_loss"]) == o["max_epochs"]
    stop, best, best_loss, _ = ho.stopping_rule(hw["holdout_epochs"], hw["holdout_loss"], o["patience"])
    print(f"device trace: best epoch {best} (H = {best_loss:.4f}), stop at {stop}; H(1) = {hw['holdout_loss'][0]:.4f}")
    assert stop is not None and 3 <= best and stop == best + o["patience"] < o["max_epochs"]

    def run_to(n):
        c = fresh(p, rows, cols, lr=o["lr"])
        if n > 0:
            c.fit(max_epochs=n, **opts)
        return c

    stopped = fresh(p, rows, cols, lr=o["lr"])
    stopped.set_holdout_tracking(every=1, patience=o["patience"])
    hs = stopped.fit(max_epochs=o["max_epochs"], **opts)
    assert (hs["term_code"], hs["epochs"], hs["best_epoch"]) == ("holdout_increase", stop, best)
    assert np.array_equal(hs["holdout_loss"], hw["holdout_loss"][:stop]) and np.array_equal(hs["loss"], hw["loss"][:stop])
    assert same(state(stopped), state(run_to(stop)))                              # without restore: the ordinary final state
    restored = fresh(p, rows, cols, lr=o["lr"])
    restored.set_holdout_tracking(every=1, patience=o["patience"], restore_best=True)
    hr_ = restored.fit(max_epochs=o["max_epochs"], **opts)
    assert (hr_["term_code"], hr_["epochs"], hr_["best_epoch"]) == ("holdout_increase", stop, best)
    at_best = run_to(best - 1)                                                    # the parameters epoch `best` saw
    assert same(restored.get_factors(), at_best.get_factors())
    assert restored.holdout_loss()[0] == hw["holdout_loss"][best - 1] == restored.get_holdout_trace()["best_loss"]
    assert same(state(restored)[2:], state(stopped)[2:])                          # the optimizer state is NOT rolled back
    # only the factors the fit updates are restored; the others never moved
    only_y = fresh(p, rows, cols, lr=o["lr"])
    only_y.set_holdout_tracking(every=1, patience=2, min_delta=1e30, restore_best=True)   # nothing improves on epoch 1 by 1e30
    hy = only_y.fit(max_epochs=9, update_X=False, update_Y=True, abs_tol=0, rel_tol=0)
    assert (hy["term_code"], hy["epochs"], hy["best_epoch"]) == ("holdout_increase", 3, 1)
    assert same(only_y.get_factors(), (p["X"], p["Y"]))


# ---- 6. the Python layer ----------------------------------------------------------------------------------------------------------
def test_the_python_layer_masks_both_sides_and_reports_the_trace(pkg):
    p, _, _ = ho.overfit_problem(1)
    model = pkg.make_model(np.array(p["D"]), K=16, feature_views=[1] * 40 + [2] * 35, lambda_Y_l2=None, rng=np.random.default_rng(5))
    try:
        D0 = np.array(model.data)
        rows, cols = pkg.sample_holdout(model, 0.4, seed=3)
        ctx = model.device_context()
        pkg.matfac.marshal(model.matfac, ctx, with_xreg=False, with_yreg=False)    # (the statistics below need the model)
        key = model._ctx_data_id
        assert pkg.set_holdout_(model, rows, cols) == rows.size
        assert np.isnan(model.data[rows, cols]).all() and np.array_equal(model.holdout["values"], D0[rows, cols])
        assert model.device_context() is ctx and model._ctx_data_id == key        # no second upload
        gr, gc, gv = ctx.get_holdout()
        assert np.array_equal(gr, rows + 1) and np.array_equal(gc, cols + 1) and np.array_equal(gv, D0[rows, cols].astype(np.float32))
        assert np.array_equal(ctx.stats(False)["n"], np.isfinite(model.data).sum(0))   # the device and model.data agree
        with pytest.raises(ValueError, match="already has a hold-out set"):
            pkg.set_holdout_(model, rows[:3], cols[:3])
        kw = dict(lr=0.1, update_X=True, update_Y=True, abs_tol=0, rel_tol=0, verbosity=0)
        h = pkg.mf_fit_adapt_lr_(model, max_epochs=6, holdout_every=2, **kw)
        assert h["term_code"] == "max_epochs" and h["holdout_epochs"].tolist() == [1, 3, 5] and h["best_epoch"] in (1, 3, 5)
        assert ctx.get_holdout_trace()["epochs"].size == 3
        mf = model.matfac
        ct, w = mf.col_transform, mf.noise_model.weights
        q = dict(p, D=np.asfortranarray(D0.astype(np.float32)), X=np.asfortranarray(mf.X), Y=np.asfortranarray(mf.Y),
                 logsigma=np.asarray(ct.unwrapped(1).logsigma, np.float32), mu=np.asarray(ct.unwrapped(3).mu, np.float32),
                 col_weight=np.ones(75, np.float32) if w is None else np.asarray(w, np.float32))
        sc = pkg.holdout_scores(model)
        ho.check(sc["loss_col"], sc["n_col"], sc["total"], q, rows, cols)
        assert sc["views"] == [1, 2] and sc["view_n"].tolist() == [int((cols < 40).sum()), int((cols >= 40).sum())]
        assert np.allclose(sc["view_loss"].sum(), sc["total"], rtol=1e-12) and np.array_equal(sc["mean_col"] * sc["n_col"] > 0, sc["n_col"] > 0)
        h2 = pkg.mf_fit_adapt_lr_(model, max_epochs=10, holdout_every=1, holdout_patience=1, holdout_min_delta=1e30,
                                  holdout_restore_best=True, **kw)
        assert (h2["term_code"], h2["epochs"], h2["best_epoch"]) == ("holdout_increase", 2, 1)
        assert "holdout_loss" not in pkg.mf_fit_adapt_lr_(model, max_epochs=2, **kw)     # the switch does not outlive its fit
        pkg.clear_holdout_(model)
        assert model.holdout is None and np.array_equal(model.data, D0) and model._ctx_data_id == key
        assert np.array_equal(ctx.stats(False)["n"], np.isfinite(D0).sum(0)) and ctx.get_holdout()[0].size == 0
    finally:
        model.release_device()


def small_model(pkg):
    p, _, _ = ho.overfit_problem(2)
    model = pkg.make_model(np.array(p["D"]), K=4, feature_views=[1] * 40 + [2] * 35, rng=np.random.default_rng(6))
    rows, cols = pkg.sample_holdout(model, 0.2, seed=4)
    return model, np.array(model.data), rows, cols


def test_a_model_whose_device_lost_the_set_is_restored_on_both_sides(pkg):
    """release_device (or any new upload) drops the device's set while model.data stays masked: clear_holdout_ must not leave
    a masked resident copy behind the restored host array."""
    model, D0, rows, cols = small_model(pkg)
    try:
        pkg.set_holdout_(model, rows, cols)
        model.release_device()
        ctx = model.device_context()                                             # uploads the masked matrix, without a set
        assert ctx.holdout_count() == 0 and np.isnan(model.data[rows, cols]).all()
        pkg.clear_holdout_(model)
        assert model.holdout is None and np.array_equal(model.data, D0)
        ctx = model.device_context()                                             # ... marked stale: uploaded again, whole
        pkg.matfac.marshal(model.matfac, ctx, with_xreg=False, with_yreg=False)
        assert np.array_equal(ctx.stats(False)["n"], np.isfinite(D0).sum(0))
    finally:
        model.release_device()


def test_scores_and_fits_take_a_lost_set_again(pkg):
    model, D0, rows, cols = small_model(pkg)
    try:
        pkg.set_holdout_(model, rows, cols)
        before = pkg.holdout_scores(model)
        assert before["n_col"].sum() == rows.size and before["total"] > 0
        model.release_device()
        after = pkg.holdout_scores(model)                                        # a new context: the set is taken anew
        assert after["total"] == before["total"] and np.array_equal(after["loss_col"], before["loss_col"])
        assert np.isnan(model.data[rows, cols]).all() and model.device_context().holdout_count() == rows.size
        model.invalidate_device_data()
        h = pkg.mf_fit_(model, lr=0.05, update_X=True, update_Y=True, max_epochs=3, abs_tol=0, rel_tol=0, holdout_every=1)
        assert h["holdout_epochs"].tolist() == list(range(1, h["epochs"] + 1)) and h["holdout_loss"][0] == before["total"]
        pkg.clear_holdout_(model)
        assert np.array_equal(model.data, D0) and model.device_context().holdout_count() == 0
    finally:
        model.release_device()


def test_fit_options_leave_the_callers_sticky_tracking_as_it_was(pkg):
    model, _, rows, cols = small_model(pkg)
    try:
        pkg.set_holdout_(model, rows, cols)
        ctx = model.device_context()
        ctx.set_holdout_tracking(every=2, patience=0)                             # the caller's own switch
        kw = dict(lr=0.05, update_X=True, update_Y=True, abs_tol=0, rel_tol=0)
        h1 = pkg.mf_fit_(model, max_epochs=4, holdout_every=1, **kw)
        assert h1["holdout_epochs"].tolist() == list(range(1, h1["epochs"] + 1))
        assert ctx.holdout_tracking == dict(every=2, patience=0, min_delta=0.0, restore_best=False)
        h2 = pkg.mf_fit_(model, max_epochs=4, **kw)
        assert h2["holdout_epochs"].tolist() == list(range(1, h2["epochs"] + 1, 2)) and h2["epochs"] >= 3
    finally:
        model.release_device()
