"""The `stages` keyword of the closed-form stages, as far as it can be checked without a device: its values, and the refusal
on a row-sharded model whose reducer is not the library's communicator (tests/test_gpu_library_stages.py has the rest)."""
import inspect

import numpy as np
import pytest


def _model(pkg, row_shard=None):
    rng = np.random.default_rng(1)
    D = rng.standard_normal((12, 6)).astype(np.float32)
    kw = dict(K=2, sample_conditions=["a"] * 6 + ["b"] * 6, feature_views=[1] * 6, batch_dict={1: ["p"] * 4 + ["q"] * 8}, rng=rng)
    if row_shard is None:
        return pkg.make_model(D, **kw)
    lo, hi, _ = row_shard
    return pkg.make_model(D[lo:hi], row_shard=row_shard, **kw)


def test_unknown_value_is_refused_before_the_device_is_touched(pkg):
    model = _model(pkg)
    for call in (lambda: pkg.init_logsigma_(model, stages="device"), lambda: pkg.reweight_col_losses_(model, stages=None),
                 lambda: pkg.construct_minimal_regularizer(model, stages="lib"),
                 lambda: pkg.theta_delta_em(model, [], np.ones(6), stages="")):
        with pytest.raises(ValueError, match="'host' or 'library'"):
            call()
    assert model._ctx is None


def test_library_stages_refuse_a_replaced_reducer(pkg):
    model = _model(pkg, row_shard=(0, 7, 12))
    model.set_allreduce(lambda a: a)
    with pytest.raises(ValueError, match="set_allreduce.*no(ne)? "):
        pkg.init_logsigma_(model, stages="library")
    assert model._ctx is None


def test_every_driver_takes_the_keyword_and_defaults_to_host(pkg):
    for f in (pkg.init_logsigma_, pkg.reweight_col_losses_, pkg.construct_minimal_regularizer, pkg.theta_delta_em,
              pkg.init_batch_effects_, pkg.basic_fit_, pkg.fit_ard_, pkg.fit.basic_fit_reg_weight_eb_, pkg.fit_feature_set_ard_,
              pkg.fit_):
        assert inspect.signature(f).parameters["stages"].default == "host", f.__name__
