"""Row-sharded models on the host (no GPU): construction with `make_model(..., row_shard=...)`, the host arithmetic that the
stage drivers of pathmatfac.jl_amd/fit.py do between the device passes, and parallel.gather_factors.

The ranks of the arithmetic tests are threads; their reducer (given to model.set_allreduce) sums the ranks' buffers in rank
order behind a barrier, so every rank leaves with the same bits, as a real all-reduce guarantees."""
import threading

import numpy as np
import pytest

# ---- construction ---------------------------------------------------------------------------------------
M_TOTAL, N, K = 23, 12, 3
CONDS = ["a"] * 6 + ["b"] * 12 + ["c"] * 5          # b = rows 6..17 straddles row 8 and row 12; rows 8..15 lie inside b
BATCHES = ["x"] * 10 + ["y"] * 8 + ["z"] * 5        # z = rows 18..22: wholly in the last shard of both splits
VIEWS = [1] * 6 + [2] * 6


def _data(M=M_TOTAL, n=N, seed=0):
    return np.random.default_rng(seed).standard_normal((M, n)).astype(np.float32)


def _kw(**over):
    kw = dict(K=K, sample_ids=[f"s{i}" for i in range(M_TOTAL)], sample_conditions=CONDS, feature_views=VIEWS,
              batch_dict={1: BATCHES}, Y_ard=True)
    kw.update(over)
    return kw


def _shards(pkg, world, D=None, seed=1, **over):
    D = _data() if D is None else D
    out = []
    for r in range(world):
        lo, hi = pkg.parallel.shard_rows(D.shape[0], world, r)
        out.append(pkg.make_model(D[lo:hi], rng=np.random.default_rng(seed), row_shard=(lo, hi, D.shape[0]), **_kw(**over)))
    return out


class RecordingContext:
    """Stand-in for _lib.Context that records what a regularizer marshals (and refuses an empty range, as the library's
    add_quad_ranges does)."""

    def __init__(self):
        self.groups = []

    def add_reg_group(self, which, ranges, w, p=1.0):
        w = np.asarray(w)
        assert len(ranges) == w.shape[0]
        for a, b in ranges:
            assert b >= a, f"empty range {a}:{b}"
        self.groups.append((which, list(ranges), w, p))

    def add_reg_l2(self, which, w, p=1.0):
        pass


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_construction_is_consistent_across_ranks(pkg, world):
    D = _data()
    full = pkg.make_model(D, rng=np.random.default_rng(1), **_kw())
    shards = _shards(pkg, world, D)
    assert [s.row_shard for s in shards] == [(*pkg.parallel.shard_rows(M_TOTAL, world, r), M_TOTAL) for r in range(world)]
    assert [s.row_shard[1] - s.row_shard[0] for s in shards] == ([12, 11] if world == 2 else [8, 8, 7])
    assert not full.sharded and full.M_total == M_TOTAL and full.row_shard == (0, M_TOTAL, M_TOTAL)
    for s in shards:
        lo, hi, _ = s.row_shard
        assert s.sharded and s.M_total == M_TOTAL
        assert s.sample_ids == full.sample_ids[lo:hi] and s.sample_conditions == CONDS[lo:hi]
        assert s.conditions == ["a", "b", "c"] and [tuple(r) for r in s.condition_ranges] == [(1, 6), (7, 18), (19, 23)]
        assert s.data.shape == (hi - lo, N) and s.matfac.X.shape == (K, hi - lo)
        np.testing.assert_array_equal(s.matfac.Y, full.matfac.Y)
        np.testing.assert_array_equal(s.matfac.col_transform.unwrapped(3).mu, full.matfac.col_transform.unwrapped(3).mu)
    np.testing.assert_array_equal(np.concatenate([s.matfac.X for s in shards], axis=1), full.matfac.X)
    # batch layers: global numbering and table shapes on every rank, local row -> batch vectors
    for layer, attr in ((2, "logdelta"), (4, "theta")):
        fb = getattr(full.matfac.col_transform.unwrapped(layer), attr)
        sb = [getattr(s.matfac.col_transform.unwrapped(layer), attr) for s in shards]
        assert fb.row_batch_ids == (["x", "y", "z"],)
        for b in sb:
            assert b.row_batch_ids == fb.row_batch_ids and b.col_ranges == fb.col_ranges
            assert [v.shape for v in b.values] == [v.shape for v in fb.values] == [(3, 6)]
        np.testing.assert_array_equal(np.concatenate([b.row_batches[0] for b in sb]), fb.row_batches[0])
        assert 2 not in sb[0].row_batches[0] and set(sb[-1].row_batches[0]) >= {2}      # z: only in the last shard, slot kept
    # the layer regularizers are sized by the global tables
    for s in shards:
        assert [w.shape for w in s.matfac.col_transform_reg.regs[1].weights] == [(3,)]
    # X regularizer: global groups on the host, non-empty local intersections marshalled, tiling the local rows
    seen = []
    for s in shards:
        lo, hi, _ = s.row_shard
        reg = s.matfac.X_reg
        assert [tuple(g) for g in reg.group_idx] == [(1, 6), (7, 18), (19, 23)] and len(reg.group_weights) == 3
        rec = RecordingContext()
        reg.add_to(rec, "X")
        (which, ranges, w, p), = rec.groups
        assert which == "X" and w.shape == (len(ranges), K)
        assert ranges[0][0] == 1 and ranges[-1][1] == hi - lo
        assert all(b >= a for a, b in ranges) and all(ranges[i + 1][0] == ranges[i][1] + 1 for i in range(len(ranges) - 1))
        seen.append([i for i, _, _ in reg.local_groups()])
    assert seen == ([[0, 1], [1, 2]] if world == 2 else [[0, 1], [1], [1, 2]])            # b straddles; rows 8..15 inside b
    rec = RecordingContext()
    full.matfac.X_reg.add_to(rec, "X")
    assert rec.groups[0][1] == [(1, 6), (7, 18), (19, 23)]


def test_whole_range_shard_is_the_plain_model(pkg):
    D = _data()
    full = pkg.make_model(D, rng=np.random.default_rng(1), **_kw())
    one = pkg.make_model(D, rng=np.random.default_rng(1), row_shard=(0, M_TOTAL, M_TOTAL), **_kw())
    assert not one.sharded
    np.testing.assert_array_equal(one.matfac.X, full.matfac.X)
    np.testing.assert_array_equal(one.matfac.Y, full.matfac.Y)
    a = np.arange(4.0)
    assert one.allreduce(a) is a and np.array_equal(a, np.arange(4.0))       # a no-op without any reducer


def test_sharded_construction_refusals(pkg):
    D = _data()
    graphs = [[("s0", "s1", 1.0)]] * K
    with pytest.raises(ValueError, match="rows are sharded"):
        pkg.make_model(D[:12], rng=np.random.default_rng(1), row_shard=(0, 12, M_TOTAL), **_kw(sample_graphs=graphs, Y_ard=False))
    with pytest.raises(ValueError, match="rows"):
        pkg.make_model(D[:11], row_shard=(0, 12, M_TOTAL), **_kw())
    with pytest.raises(ValueError, match="lo < hi"):
        pkg.make_model(D[:0], row_shard=(5, 5, M_TOTAL), **_kw())
    with pytest.raises(AssertionError, match="sample_conditions"):               # per-sample arguments are passed whole
        pkg.make_model(D[:12], row_shard=(0, 12, M_TOTAL), **_kw(sample_conditions=CONDS[:12]))
    s = pkg.make_model(D[:12], rng=np.random.default_rng(1), row_shard=(0, 12, M_TOTAL), **_kw())
    with pytest.raises(ValueError, match="rows are sharded"):                    # no exchange recorded: no device context
        s.device_context()
    with pytest.raises(ValueError, match="exactly one"):
        s.attach_comm(0, 2)
    with pytest.raises(ValueError, match="float64"):
        s.set_allreduce(lambda a: None)
        s.allreduce(np.zeros(3, np.float32))


# ---- host arithmetic ------------------------------------------------------------------------------------
class ThreadRanks:
    """`world` ranks as threads.  reducer(rank) is that rank's all-reduce: the buffers are summed in rank order, so the
    result is the same bits on every rank.  A rank that raises breaks the barrier: nobody waits for a time limit."""

    def __init__(self, world):
        self.world = world
        self.barrier = threading.Barrier(world)
        self.slots = [None] * world
        self.calls = [0] * world

    def reducer(self, rank):
        def allreduce(arr):
            assert arr.dtype == np.float64 and arr.flags.c_contiguous
            self.calls[rank] += 1
            self.slots[rank] = arr
            self.barrier.wait()
            total = self.slots[0].copy()
            for a in self.slots[1:]:
                total += a
            self.barrier.wait()           # everyone has read every buffer
            arr[...] = total
            self.barrier.wait()
        return allreduce

    def run(self, fn):
        """fn(rank) on every rank; returns the list of results."""
        out, errs = [None] * self.world, []

        def target(r):
            try:
                out[r] = fn(r)
            except BaseException as e:    # noqa: BLE001 -- reported below
                errs.append(e)
                self.barrier.abort()
        threads = [threading.Thread(target=target, args=(r,)) for r in range(self.world)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        real = [e for e in errs if not isinstance(e, threading.BrokenBarrierError)]
        if real or errs:
            raise (real or errs)[0]
        return out


AM, AN, AK = 331, 10, 6
A_CONDS = ["g1"] * 100 + ["g2"] * 2 + ["g3"] * 120 + ["g4"] * 109      # g2 is two samples wide; g3 spans every boundary
A_VIEWS = [1] * 4 + [2] * 6


def _arith_models(pkg, world, **over):
    """The unsharded model and `world` shards in one seeded state: X rows scaled from 3 down to 1e-3."""
    rng = np.random.default_rng(5)
    D = np.zeros((AM, AN), np.float32)
    X = (np.logspace(np.log10(3.0), -3, AK)[:, None] * rng.standard_normal((AK, AM))).astype(np.float32)
    Y = rng.standard_normal((AK, AN)).astype(np.float32)
    ls = 0.1 * rng.standard_normal(AN)
    kw = dict(K=AK, sample_conditions=A_CONDS, feature_views=A_VIEWS, Y_ard=True)
    kw.update(over)
    full = pkg.make_model(D, rng=np.random.default_rng(1), **kw)
    shards = []
    for r in range(world):
        lo, hi = pkg.parallel.shard_rows(AM, world, r)
        shards.append(pkg.make_model(D[lo:hi], rng=np.random.default_rng(1), row_shard=(lo, hi, AM), **kw))
    for m in [full] + shards:
        lo, hi, _ = m.row_shard
        m.matfac.X[...] = X[:, lo:hi]
        m.matfac.Y[...] = Y
        m.matfac.col_transform.unwrapped(1).logsigma[...] = ls
    return full, shards


def _within_one_ulp(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape
    ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
    bad = np.abs(a.astype(np.float64) - b.astype(np.float64)) > ulp
    assert not bad.any(), (int(bad.sum()), a[bad][:3], b[bad][:3])


def _run_stage(pkg, world, stage, **over):
    """stage(model) on the unsharded model and on every rank.  Returns (full, shards, collectives per rank)."""
    full, shards = _arith_models(pkg, world, **over)
    stage(full)
    ranks = ThreadRanks(world)
    for r, s in enumerate(shards):
        s.set_allreduce(ranks.reducer(r))
    ranks.run(lambda r: stage(shards[r]))
    assert len(set(ranks.calls)) == 1
    return full, shards, ranks.calls[0]


def _replicated_bits_equal(shards):
    for s in shards[1:]:
        np.testing.assert_array_equal(s.matfac.Y, shards[0].matfac.Y)
        np.testing.assert_array_equal(s.matfac.col_transform.unwrapped(1).logsigma,
                                      shards[0].matfac.col_transform.unwrapped(1).logsigma)


def _gathered(shards):
    return np.concatenate([s.matfac.X for s in shards], axis=1)


@pytest.mark.parametrize("world", [2, 3])
def test_whiten_rotate_reorder_on_shards(pkg, world):
    full, shards, n = _run_stage(pkg, world, pkg.whiten_)
    assert n == 1
    _replicated_bits_equal(shards)
    _within_one_ulp(_gathered(shards), full.matfac.X)
    _within_one_ulp(shards[0].matfac.Y, full.matfac.Y)
    _within_one_ulp(shards[0].matfac.col_transform.unwrapped(1).logsigma.astype(np.float32),
                    full.matfac.col_transform.unwrapped(1).logsigma.astype(np.float32))
    ms = np.mean(_gathered(shards).astype(np.float64) ** 2, axis=1)
    np.testing.assert_allclose(ms, 1.0, rtol=1e-6)                           # unit mean square over ALL samples

    full, shards, n = _run_stage(pkg, world, pkg.rotate_by_svd_)
    assert n == 1
    _replicated_bits_equal(shards)
    _within_one_ulp(_gathered(shards), full.matfac.X)
    _within_one_ulp(shards[0].matfac.Y, full.matfac.Y)

    def reorder(m):                                  # (Y rows in rising order first, so that the permutation is not trivial)
        m.matfac.Y[...] = m.matfac.Y[np.argsort(np.sum(m.matfac.Y.astype(np.float64) ** 2, axis=1)), :]
        m.matfac.X_reg.group_weights = tuple(np.arange(AK, dtype=np.float32) + 10 * g for g in range(4))
        pkg.reorder_by_importance_(m)
    full, shards, n = _run_stage(pkg, world, reorder)
    assert n == 0                                    # replicated inputs: nothing to exchange
    _replicated_bits_equal(shards)
    np.testing.assert_array_equal(_gathered(shards), full.matfac.X)
    np.testing.assert_array_equal(shards[0].matfac.Y, full.matfac.Y)
    assert not np.array_equal(full.matfac.X_reg.group_weights[0], np.arange(AK, dtype=np.float32))
    for s in shards:
        for a, b in zip(s.matfac.X_reg.group_weights, full.matfac.X_reg.group_weights):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("world", [2, 3])
def test_reweight_eb_on_shards(pkg, world):
    R = pkg.regularizers

    def l2(m):
        m.matfac.X_reg = R.L2Regularizer(AK, 1.0)
        pkg.reweight_eb_(m.matfac.X_reg, m.matfac.X, model=m)
    full, shards, n = _run_stage(pkg, world, l2)
    assert n == 2                                    # the Gram matrix, then the root's eigenvalue
    for s in shards:
        np.testing.assert_array_equal(s.matfac.X_reg.weights, shards[0].matfac.X_reg.weights)
    _within_one_ulp(shards[0].matfac.X_reg.weights, full.matfac.X_reg.weights)
    assert full.matfac.X_reg.weights[0] != 1.0

    def group(m):
        assert isinstance(m.matfac.X_reg, R.GroupRegularizer)
        pkg.reweight_eb_(m.matfac.X_reg, m.matfac.X, mixture_p=0.7, model=m)
    full, shards, n = _run_stage(pkg, world, group)
    assert n == 2                                    # all groups' Grams in one buffer
    for s in shards:
        assert len(s.matfac.X_reg.group_weights) == 4
        for a, b in zip(s.matfac.X_reg.group_weights, shards[0].matfac.X_reg.group_weights):
            np.testing.assert_array_equal(a, b)
    for a, b in zip(shards[0].matfac.X_reg.group_weights, full.matfac.X_reg.group_weights):
        _within_one_ulp(a, b)
    assert len({float(w[0]) for w in full.matfac.X_reg.group_weights}) == 4

    def composite(m):
        reg = m.matfac.X_reg
        assert isinstance(reg, R.CompositeRegularizer) and isinstance(reg.regularizers[1], R.GroupRegularizer)
        pkg.reweight_eb_(reg, m.matfac.X, model=m)
    full, shards, n = _run_stage(pkg, world, composite, Y_ard=False, lambda_X_l2=0.7)
    assert n == 4
    for s in shards:
        np.testing.assert_array_equal(s.matfac.X_reg.regularizers[0].weights, shards[0].matfac.X_reg.regularizers[0].weights)
        for a, b in zip(s.matfac.X_reg.regularizers[1].group_weights, shards[0].matfac.X_reg.regularizers[1].group_weights):
            np.testing.assert_array_equal(a, b)
    _within_one_ulp(shards[0].matfac.X_reg.regularizers[0].weights, full.matfac.X_reg.regularizers[0].weights)
    for a, b in zip(shards[0].matfac.X_reg.regularizers[1].group_weights, full.matfac.X_reg.regularizers[1].group_weights):
        _within_one_ulp(a, b)
    assert full.matfac.X_reg.mixture_p[:2] == (0.5, 0.5)

    # a regularizer without a sharded update is refused, not silently computed from the local rows
    s = shards[0]
    with pytest.raises(NotImplementedError, match="rows are sharded"):
        pkg.reweight_eb_(R.L1Regularizer(AK, 1.0), s.matfac.X, model=s)


def test_condition_indicator_has_every_global_condition(pkg):
    _, shards = _arith_models(pkg, 3)
    mats = [pkg.fit._condition_ind_mat(s) for s in shards]
    assert [m.shape for m in mats] == [(111, 4), (110, 4), (110, 4)]
    np.testing.assert_array_equal(np.concatenate(mats), pkg.util.ids_to_ind_mat(A_CONDS))
    assert not mats[1][:, [0, 1, 3]].any()           # rows 111..220 lie inside g3: its column only, in slot 2


@pytest.mark.parametrize("world", [2, 3])
def test_gather_factors_and_saved_parameters(pkg, tmp_path, world):
    full, shards = _arith_models(pkg, world)
    ranks = ThreadRanks(world)
    for r, s in enumerate(shards):
        s.set_allreduce(ranks.reducer(r))

    def gather_and_save(r):
        X = pkg.parallel.gather_factors(shards[r])
        pkg.save_params_npz(shards[r], tmp_path / f"rank{r}.npz")
        return X
    for X in ranks.run(gather_and_save):
        assert X.dtype == np.float32 and X.flags.f_contiguous
        np.testing.assert_array_equal(X, full.matfac.X)
    np.testing.assert_array_equal(pkg.parallel.gather_factors(full), full.matfac.X)
    pkg.save_params_npz(full, tmp_path / "full.npz")
    want = np.load(tmp_path / "full.npz")
    for r in range(world):
        got = np.load(tmp_path / f"rank{r}.npz")
        assert sorted(got.files) == sorted(want.files)
        for k in want.files:
            np.testing.assert_array_equal(got[k], want[k])
    assert want["X"].shape == (AM, AK) and list(want["sample_ids"]) == [str(i) for i in range(1, AM + 1)]
