"""Which kernel instance a fused data pass runs, per configuration, against a recorded table.

The instance of a pass -- kernel family, batch mode, register-resident X, plain tile loop -- is decided once on the host
(fused_geometry in pmf_pass.hip, by the rules of pmf_common.h) and the launchers select by that decision alone.  This test
runs one pass per configuration at 300 x 100 (ragged last row and column blocks; one row panel at 512 rows, two at 256),
reads pmf_debug_last_kernel / pmf_debug_last_path and compares (kernel, bmode, xreg, plain_tiles > 0) with
tests/golden/pass_instances.json.

The table was RECORDED from the library of the commit before the decision moved to one place, not written by hand and not
taken from the code under test:
    python tests/test_gpu_pass_instance.py --record path/to/that/libpmf_hip.so
A change that is meant to move a configuration to another instance re-records it from the library that does so and says
why; a refactor of the host code leaves it alone.

Factors, crossed where they can matter: K (every K-block count and both sides of its edges), precision, gradients (both, X
only, Y only, none = pmf_loss), batch layers (none; one view of 4 batches; one view of 20 scrambled batches, more than 15
in a row panel: the gather fallback), noise models (Gaussian; mixed), storage of D, and the switches PMF_XGEMM3=0,
PMF_XREG=0, PMF_PLAIN=0 (exact kernel at 32 < K <= 64), PMF_SB8=0 / 4 (split-bf16 products at K > 32), PMF_RBW=1 (K <= 32),
each with both gradients and with X only.  The table has one line per problem and storage of D.
PMF_SB2 is read once per process and stays out.  At this shape every workgroup gets one tile, and the first piece of a
segment visit has no plain run: plain_tiles is recorded as 0 throughout, PMF_PLAIN or not (tests/test_gpu_exact_plain.py
has the shapes that count plain tiles).  The only numerical claim is a finite loss: accuracy has its own suites.
"""
import json
import math
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "pass_instances.json"
M, N = 300, 100
KS = (16, 32, 48, 64, 96, 128)
PRECISIONS = ("f32", "bf16x3")
GRADS = {"both": (True, True), "x": (True, False), "y": (False, True), "none": (False, False)}
BATCHES = {"b0": dict(), "b4": dict(batch_views=1, n_batches=4, batch_order="sorted"),
           "b20": dict(batch_views=1, n_batches=20, batch_order="random")}
NOISES = {"gauss": dict(), "mixed": dict(bernoulli_frac=0.2, poisson_frac=0.1)}
STORES = ("f32", "bf16")


def switches_for(K, precision, grads):
    """The switch settings worth a pass at this K, precision and gradients: none, and those that the geometry can see.  All
    but PMF_RBW act on a pass with both gradients only: the switches are set for that one and for X only, the control."""
    sw = [None]
    if grads not in ("both", "x"):
        return sw
    if 32 < K <= 64:
        sw += [("PMF_XGEMM3", "0"), ("PMF_XREG", "0"), ("PMF_PLAIN", "0")]   # (bf16x3 too: what falls back to the exact kernel)
    if K > 32 and precision == "bf16x3":
        sw += [("PMF_SB8", "0"), ("PMF_SB8", "4")]
    if K <= 32:
        sw += [("PMF_RBW", "1")]
    return sw


def configurations(K):
    for batch in BATCHES:
        for noise in NOISES:
            for store in STORES:
                for precision in PRECISIONS:
                    for grads in GRADS:
                        for sw in switches_for(K, precision, grads):
                            yield batch, noise, store, precision, grads, sw


def key_of(K, batch, noise, store, precision, grads, sw):
    """(line of the table: problem and storage of D, entry of the line: the pass)"""
    return f"K{K}-{batch}-{noise}-D{store}", f"{precision}-{grads}-" + ("default" if sw is None else "=".join(sw))


def run_K(ctx, K, monkeypatch):
    """{line: {entry: [kernel, bmode, xreg, plain_tiles > 0]}} of every configuration at this K; asserts a finite loss."""
    from problems import make_problem, to_context
    out = {}
    state = None
    for batch, noise, store, precision, grads, sw in configurations(K):
        if state != (batch, noise, store):
            p = make_problem(M=M, N=N, K=K, seed=K, scale=0.3, col_params=True, weights=True, **BATCHES[batch], **NOISES[noise])
            to_context(p, ctx)
            if store == "bf16":
                ctx.set_data(p["D"], store="bf16")
            state = (batch, noise, store)
        ctx.set_precision(precision)
        if sw is not None:
            monkeypatch.setenv(*sw)
        try:
            gx, gy = GRADS[grads]
            if gx or gy:
                ctx.epoch_begin(ctx.make_opts(update_X=gx, update_Y=gy))
                loss, _ = ctx.epoch_loss()
            else:
                loss = ctx.loss()["data"]
        finally:
            if sw is not None:
                monkeypatch.delenv(sw[0])
        key = key_of(K, batch, noise, store, precision, grads, sw)
        assert math.isfinite(loss), (key, loss)
        path = ctx.last_path()
        out.setdefault(key[0], {})[key[1]] = [ctx.last_kernel(), path["bmode"], path["xreg"], int(path["plain_tiles"] > 0)]
    return out


@pytest.fixture(scope="module")
def own_ctx(pkg):
    """A context of this module's own: the passes change its precision mode and the storage of D."""
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def recorded():
    return json.loads(GOLDEN.read_text())


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_every_configuration_runs_the_recorded_instance(own_ctx, recorded, monkeypatch, K):
    got = run_K(own_ctx, K, monkeypatch)
    want = {k: v for k, v in recorded.items() if k.startswith(f"K{K}-")}
    assert {k: sorted(v) for k, v in got.items()} == {k: sorted(v) for k, v in want.items()}, \
        "the configurations of this file and of the recorded table differ: record again"
    wrong = {(k, e): (got[k][e], want[k][e]) for k in got for e in got[k] if got[k][e] != want[k][e]}
    assert not wrong, f"{len(wrong)} configurations ran another instance (got, recorded): {dict(list(wrong.items())[:8])}"


def test_recorded_table_covers_every_configuration(recorded):
    keys = {key_of(K, *cfg) for K in KS for cfg in configurations(K)}
    assert keys == {(k, e) for k, line in recorded.items() for e in line}
    values = [v for line in recorded.values() for v in line.values()]
    assert all(len(v) == 4 and all(isinstance(x, int) for x in v) for v in values)
    # the table is worth asserting against only if it tells instances apart
    assert {v[0] for v in values} == {0, 1, 2, 4, 8} and {v[1] for v in values} == {0, 1, 2} and {v[2] for v in values} == {0, 1}


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit("usage: python tests/test_gpu_pass_instance.py --record path/to/libpmf_hip.so")
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import pmf_import
    ctx = pmf_import.load().Context(0, lib_path=Path(sys.argv[2]).resolve())
    table = {}
    with pytest.MonkeyPatch.context() as mp:
        for K in KS:
            table.update(run_K(ctx, K, mp))
    ctx.close()
    GOLDEN.write_text("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(table[k], sort_keys=True)}" for k in sorted(table)) + "\n}\n")
    print(f"recorded {sum(len(v) for v in table.values())} configurations from {sys.argv[2]} into {GOLDEN}")
