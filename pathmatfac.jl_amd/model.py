"""PathMatFacModel (src/model.jl): validating constructor, column permutation, model assembly."""
import numpy as np

from . import matfac as MF
from ._lib import Context
from .layers import BatchScale, BatchShift, construct_model_layers
from .regularizers import CompositeRegularizer, GroupRegularizer, construct_layer_reg, construct_X_reg, construct_Y_reg
from .util import ids_to_ranges, is_contiguous, unique


class PathMatFacModel:  # model.jl:6-28
    def __init__(self, matfac, data, sample_ids, sample_conditions, feature_ids, feature_views, data_idx):
        self.matfac = matfac
        self.data = data
        self.sample_ids = sample_ids
        self.sample_conditions = sample_conditions
        self.feature_ids = feature_ids
        self.feature_views = feature_views
        self.data_idx = data_idx          # 1-based permutation: model column j is raw column data_idx[j]
        self._ctx = None
        self._ctx_data_id = None
        # ---- row sharding.  The per-row attributes above hold the LOCAL rows; what a stage needs
        # of the whole sample axis is kept beside them.  assemble_model fills these in for a sharded model.
        M = 0 if data is None else data.shape[0]
        self.row_shard = (0, M, M)                                   # (lo, hi, M_total): 0-based, half-open
        self.sample_ids_total = sample_ids
        self.sample_conditions_total = sample_conditions
        self.conditions = None if sample_conditions is None else unique(sample_conditions)      # global, ordered
        self.condition_ranges = (tuple(ids_to_ranges(sample_conditions))                    # in global rows, 1-based
                                 if sample_conditions is not None and is_contiguous(sample_conditions) else None)
        self._comm = None                 # dict(rank, world, unique_id, host_allreduce) recorded by attach_comm
        self._comm_on_ctx = False
        self._allreduce_fn = None

    # ---- row shards
    @property
    def M_total(self):
        return self.row_shard[2]

    @property
    def sharded(self):
        lo, hi, M_total = self.row_shard
        return hi - lo < M_total

    @property
    def is_root(self):
        """True on the rank that owns row 0 (rank 0 under parallel.shard_rows): the one whose LAPACK results every rank
        takes (bcast_root_)."""
        return self.row_shard[0] == 0

    def attach_comm(self, rank, world, unique_id=None, host_allreduce=None):
        """Records the communicator of this rank; device_context() applies it when it creates the context (an existing
        context takes it at once).  `unique_id` (comm_unique_id() of rank 0, passed to every rank): RCCL, pmf_comm_init.
        `host_allreduce(array)`: the host-staged transport, pmf_comm_init_host -- a callable that sums a float32 or
        float64 numpy array in place over the ranks."""
        if (unique_id is None) == (host_allreduce is None):
            raise ValueError("attach_comm takes exactly one of `unique_id` (RCCL) and `host_allreduce` (host-staged)")
        if self._comm_on_ctx:
            self._ctx.comm_destroy()
            self._comm_on_ctx = False
        self._comm = dict(rank=int(rank), world=int(world), unique_id=unique_id, host_allreduce=host_allreduce)
        if self._ctx is not None:
            self._apply_comm()

    def _apply_comm(self):
        c = self._comm
        if c["unique_id"] is not None:
            self._ctx.comm_init(c["rank"], c["world"], c["unique_id"])
        else:
            self._ctx.comm_init_host(c["rank"], c["world"], c["host_allreduce"])
        self._comm_on_ctx = True

    def set_allreduce(self, fn):
        """Replaces the reducer of allreduce() by a plain callable `fn(float64 array)` (in-place sum over the ranks), so
        that the host arithmetic between the device passes can run without a device.  None: back to the communicator."""
        self._allreduce_fn = fn

    def allreduce(self, arr):
        """In-place sum over the ranks of a C-contiguous float64 numpy array: the ONE way host-side numbers cross ranks.
        A no-op for a model that is not sharded.  Collective: every rank calls it, in the same order."""
        if not self.sharded:
            return arr
        if not (isinstance(arr, np.ndarray) and arr.dtype == np.float64 and arr.flags.c_contiguous):
            raise ValueError("allreduce needs a C-contiguous float64 numpy array")
        if self._allreduce_fn is not None:
            self._allreduce_fn(arr)
        else:
            self.device_context().comm_allreduce(arr)
        return arr

    def bcast_root_(self, arr):
        """Every rank leaves with the root's `arr`: the other ranks contribute zeros to one sum (x + 0 is exact).  For
        what LAPACK computes from replicated inputs, so that a differing BLAS build or thread count cannot split ranks."""
        if self.sharded and not self.is_root:
            arr[...] = 0
        return self.allreduce(arr)

    # ---- gpu(model) / cpu(model)  (analyses/scripts/julia/fit_matfac.jl:325-340)
    def device_context(self, device=0):
        """The model's pmf_ctx; the data matrix is uploaded once and stays resident in HBM."""
        if self._ctx is None:
            if self.sharded and self._comm is None:
                raise ValueError("rows are sharded but no communicator is attached: call attach_comm() first "
                                 "(a fit of one shard alone would silently be a different model)")
            self._ctx = Context(device)
            if self._comm is not None:
                self._apply_comm()
        key = (id(self.data), None if self.data is None else self.data.shape)
        if self._ctx_data_id != key:
            if self.data is None:
                raise ValueError("model.data is nothing")
            self._ctx.set_data(self.data)
            self._ctx_data_id = key
        return self._ctx

    def invalidate_device_data(self):
        """Call after editing model.data IN PLACE: the HBM copy is keyed on the array's identity and shape, so an in-place
        edit is not seen; the next device_context() uploads the matrix again."""
        self._ctx_data_id = None

    def release_device(self):
        if self._ctx is not None:
            if self._comm_on_ctx:
                self._ctx.comm_destroy()
            self._ctx.close()
        self._ctx = None
        self._comm_on_ctx = False
        self._ctx_data_id = None


def assemble_model(D, K, sample_ids, sample_conditions, feature_ids, feature_views, feature_distributions, batch_dict,
                   feature_sets_dict, featureset_names, feature_graphs, sample_graphs, lambda_X_l2,
                   lambda_X_condition, lambda_X_graph, lambda_Y_l2, lambda_Y_selective_l1, lambda_Y_graph, Y_ard,
                   Y_feature_set_ard, alpha0, v0, lambda_layer, rng=None, row_shard=None):
    """model.jl:37-81.  Columns are permuted so that (distribution, view) pairs form contiguous blocks
    (stable sortperm of the zipped pairs, :50-54); `data_idx` keeps the permutation (1-based).
    With `row_shard` = (lo, hi, M_total), D holds rows lo:hi and every per-sample argument all M_total samples: layers
    and regularizers are built from the global metadata, so that their replicated tables agree on every rank, and then
    restricted to the local rows."""
    M, N = D.shape
    M_total = M if row_shard is None else row_shard[2]
    keys = list(zip(feature_distributions, feature_views))
    perm = sorted(range(N), key=lambda j: keys[j])          # Python's sort is stable, like Julia's sortperm
    data_idx = np.array(perm, dtype=np.int64) + 1
    feature_ids = [feature_ids[j] for j in perm]
    feature_views = [feature_views[j] for j in perm]
    feature_distributions = [feature_distributions[j] for j in perm]
    D = np.asfortranarray(np.asarray(D, dtype=np.float32)[:, perm])
    col_layers = construct_model_layers(feature_views, batch_dict, rng=rng)
    layer_reg = construct_layer_reg(feature_views, batch_dict, col_layers, lambda_layer)
    X_reg = construct_X_reg(K, M_total, sample_ids, sample_conditions, sample_graphs, lambda_X_l2, lambda_X_condition,
                            lambda_X_graph, Y_ard, Y_feature_set_ard)
    Y_reg = construct_Y_reg(K, N, feature_ids, feature_views, feature_sets_dict, feature_graphs, lambda_Y_l2,
                            lambda_Y_selective_l1, lambda_Y_graph, Y_ard, Y_feature_set_ard, featureset_names,
                            alpha0, v0)
    matfac = MF.MatFacModel(M, N, K, feature_distributions, col_transform=col_layers, X_reg=X_reg, Y_reg=Y_reg,
                            col_transform_reg=layer_reg, rng=rng, row_shard=row_shard)
    if row_shard is None:
        return PathMatFacModel(matfac, D, sample_ids, sample_conditions, feature_ids, feature_views, data_idx)
    lo, hi, _ = row_shard
    for i in (2, 4):                     # batch layers: global numbering and tables, local batch_of_row
        layer = col_layers.unwrapped(i)
        if isinstance(layer, (BatchScale, BatchShift)):
            col_layers.set_layer_(i, layer.view((lo + 1, hi), None))
    _shard_group_regs_(X_reg, lo, hi)
    model = PathMatFacModel(matfac, D, sample_ids[lo:hi], None if sample_conditions is None else sample_conditions[lo:hi],
                            feature_ids, feature_views, data_idx)
    model.row_shard = (lo, hi, M_total)
    model.sample_ids_total, model.sample_conditions_total = sample_ids, sample_conditions
    if sample_conditions is not None:
        model.conditions = unique(sample_conditions)
        model.condition_ranges = tuple(ids_to_ranges(sample_conditions))
    return model


def _shard_group_regs_(reg, lo, hi):
    """The GroupRegularizers of an X regularizer keep the global groups and weights; they marshal the non-empty
    intersections with rows lo:hi (GroupRegularizer.add_to)."""
    if isinstance(reg, GroupRegularizer):
        reg.row_shard = (lo, hi)
    elif isinstance(reg, CompositeRegularizer):
        for r in reg.regularizers:
            _shard_group_regs_(r, lo, hi)


def make_model(D, K=10, sample_ids=None, sample_conditions=None, feature_ids=None, feature_views=None,
               feature_distributions=None, batch_dict=None, sample_graphs=None, feature_sets_dict=None,
               featureset_names=None, feature_graphs=None, lambda_X_l2=None, lambda_X_condition=1.0,
               lambda_X_graph=1.0, lambda_Y_l2=1.0, lambda_Y_selective_l1=None, lambda_Y_graph=None,
               lambda_layer=1.0, Y_ard=False, Y_fsard=False, fsard_alpha0=np.float32(1.001),
               fsard_v0=np.float32(0.8), rng=None, row_shard=None):
    """PathMatFacModel(D; K=10, ...) -- the validating constructor of model.jl:92-196 (same keyword names).

    `row_shard` = (lo, hi, M_total), 0-based and half-open as parallel.shard_rows returns (lo, hi), makes one rank's part
    of a row-sharded model (no reference counterpart): D is rows lo:hi of the data, while `sample_ids`,
    `sample_conditions` and every value of `batch_dict` are passed whole, M_total long, on every rank.  The batch tables,
    their batch numbering, the condition groups and Y are then the same on all ranks; X, the row -> batch vectors, the
    sample ids and conditions of the model hold the local rows.  X is drawn for all M_total samples from `rng` and
    sliced -- K * M_total normals per rank -- so that with one seed the shards concatenate to the unsharded model's X and
    Y is equal on every rank.  The network term on X (`sample_graphs`) couples rows across shards and is refused."""
    D = np.asarray(D)
    M, N = D.shape
    if row_shard is not None:
        lo, hi, M_total = (int(x) for x in row_shard)
        if not (0 <= lo < hi <= M_total):
            raise ValueError(f"row_shard={row_shard!r}: needs 0 <= lo < hi <= M_total")
        if hi - lo != M:
            raise ValueError(f"row_shard={row_shard!r} names {hi - lo} rows but D has {M}")
        if sample_graphs is not None:
            raise ValueError("`sample_graphs` cannot be combined with `row_shard`: rows are sharded and the network "
                             "term on X couples samples of different shards")
        row_shard = (lo, hi, M_total)
        M = M_total                       # the per-sample arguments below are checked against the whole sample axis
    if feature_graphs is not None:
        K = len(feature_graphs)
        if sample_graphs is not None:
            assert K == len(sample_graphs), "`sample_graphs` and `feature_graphs` must have equal length; or one of them must be nothing"
    elif sample_graphs is not None:
        K = len(sample_graphs)
    if sample_ids is not None:
        assert len(sample_ids) == len(set(sample_ids)), "`sample_ids` must be unique"
        assert len(sample_ids) == M, "`sample_ids` must be nothing or have length equal to size(D,1)"
    else:
        sample_ids = list(range(1, M + 1))
    if sample_conditions is not None:
        assert len(sample_conditions) == M, "`sample_conditions` must be nothing or have length equal to size(D,1)"
        assert is_contiguous(sample_conditions), "`sample_conditions` must be contiguous; I.e., samples must be grouped by condition."
    if feature_ids is not None:
        assert len(feature_ids) == len(set(feature_ids)), "`feature_ids` must be left default, or set to a vector of unique identifiers"
        assert len(feature_ids) == N, "`feature_ids` must have length equal to dim(D,2)"
    else:
        feature_ids = list(range(1, N + 1))
    if batch_dict is not None:
        assert feature_views is not None, "`feature_views` must be provided whenever `batch_dict` is provided"
        assert sample_conditions is not None, "`sample_conditions` must be provided whenever `batch_dict` is provided"
        assert set(batch_dict.keys()) <= set(feature_views), "The `batch_dict` keys must be a subset of `feature_views`"
        for v in batch_dict.values():
            assert len(v) == M, "Each value of `batch_dict` must be a vector of length size(D,1)"
    if feature_views is not None:
        assert len(feature_views) == N, "`feature_views` must be nothing or have length equal to size(D,2)"
    else:
        feature_views = [1] * N
    if feature_distributions is not None:
        assert len(feature_distributions) == N, "`feature_distributions` must (a) be nothing or have length equal to size(D,2)"
        assert all(d in MF.VALID_LOSSES for d in feature_distributions), f"Each entry of `feature_distributions` must be one of {set(MF.VALID_LOSSES)}"
    else:
        feature_distributions = ["normal"] * N
    if Y_fsard:
        assert feature_sets_dict is not None, "`feature_sets_dict` must be provided whenever `Y_fsard` is true."
    return assemble_model(D, K, list(sample_ids), None if sample_conditions is None else list(sample_conditions),
                          list(feature_ids), list(feature_views), list(feature_distributions), batch_dict,
                          feature_sets_dict, featureset_names, feature_graphs, sample_graphs, lambda_X_l2,
                          lambda_X_condition, lambda_X_graph, lambda_Y_l2, lambda_Y_selective_l1, lambda_Y_graph,
                          Y_ard, Y_fsard, fsard_alpha0, fsard_v0, lambda_layer, rng=rng, row_shard=row_shard)
