"""bench.py's output contract on a small workload (the driver runs it with the defaults): exactly one line on stdout, a JSON
object with the contract's keys, `roofline`, and with --full `cpu_baseline` and `other_precision`; a plain run without them
whose --dump-outputs files are the same run to run; the full-model flavour; the one-rank RCCL path with a chunked data pass
(PMF_FORCE_DIST=1), whose losses must equal the plain run's (same arithmetic, same order)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
        "data", "config", "roofline"}


def run_bench(*args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--M", "3000", "--N", "1500", "--K", "64", "--steps", "4", "--warmup", "1",
                        *args], capture_output=True, text=True, env=e, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_line_contract_small():
    d = run_bench("--full", env={"PMF_BENCH_SKIP_OTHER_CPU": "1"})
    assert KEYS <= set(d), KEYS - set(d)
    assert d["metric"] == "fit_iters_per_sec" and d["unit"] == "iters/s" and d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"]
    rf = d["roofline"]
    assert rf["bound"] in ("mfma", "hbm") and 0.0 < rf["frac"] < 1.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert rf["launches"] == 4 and rf["kernel_ms"] > 0
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb
    assert d["other_precision"]["kernel_taken"] is True
    assert d["loss_last"] < d["loss_first"]


def test_bench_plain_run_is_headline_only_and_dumps_its_outputs(tmp_path):
    """No --full: no other arithmetic mode, no CPU baselines, exactly --steps timed steps.  --dump-outputs writes the timed
    steps' losses and the factors; X (70000 rows x K = 64 is past the dump's cap) as a fixed sample of its columns.  Two runs
    with the same arguments write the same files, bit for bit."""
    runs = []
    for tag in ("a", "b"):
        d = run_bench("--M", "70000", "--steps", "3", "--dump-outputs", str(tmp_path / tag))
        assert "other_precision" not in d and "cpu_baseline" not in d and "cpu_baseline_legs" not in d
        assert d["steps"] == 3 and d["roofline"]["launches"] == 3 and d["dtype"] == "f32"
        assert abs(d["value"] - 1e3 / d["ms_per_step"]) <= 1e-6 * d["value"]
        out = {f.stem: np.load(f) for f in sorted((tmp_path / tag).glob("*.npy"))}
        assert set(out) == {"loss", "X", "Y"}
        assert out["loss"].dtype == np.float64 and out["loss"].shape == (3,) and out["loss"][-1] == d["loss_last"]
        assert out["X"].dtype == np.float32 and out["X"].shape == (64, 65536) and np.isfinite(out["X"]).all()
        assert out["Y"].dtype == np.float32 and out["Y"].shape == (64, 1500) and np.isfinite(out["Y"]).all()
        assert np.abs(out["X"]).max() > 0 and np.abs(out["Y"]).max() > 0
        runs.append(out)
    for k in runs[0]:
        np.testing.assert_array_equal(runs[0][k], runs[1][k], err_msg=k)


def test_bench_full_model_and_one_rank_rccl(tmp_path):
    a = run_bench("--full-model", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "a"))
    assert a["config"]["full_model"] is True and "Bernoulli" in a["config"]["workload"]
    b = run_bench("--full-model", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "b"),
                  env={"PMF_FORCE_DIST": "1", "PMF_BENCH_CHUNKS": "3"})
    assert b["config"]["rccl_ranks"] == 1 and b["config"]["column_chunks"] == 3 and b["config"]["collectives_issued"] > 0
    # chunked + communicator: same arithmetic; the gY reduction order inside a chunk is the plain pass's
    assert abs(a["loss_last"] - b["loss_last"]) <= 1e-6 * abs(a["loss_last"]), (a["loss_last"], b["loss_last"])
    # the dump of a run with a communicator gathers X over it: the same factors as the plain run's
    for name in ("X", "Y"):
        xa, xb = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert xa.shape == xb.shape and np.abs(xa).max() > 0
        np.testing.assert_allclose(xb, xa, rtol=1e-4, atol=1e-5 * np.abs(xa).max(), err_msg=name)
    assert np.load(tmp_path / "b" / "loss.npy")[-1] == b["loss_last"]


def test_bench_under_the_drivers_launcher_one_rank_real_rccl():
    """The launch path of the N > 1 contract with N = 1: torch.distributed.run starts the rank, which reads RANK / LOCAL_RANK /
    WORLD_SIZE, maps LOCAL_RANK to its device, forms a (one-rank) RCCL communicator in the library and prints ONE JSON line."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    e = dict(os.environ, PMF_FORCE_DIST="1", PMF_BENCH_SKIP_OTHER_CPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), str(ROOT / "bench.py"), "--gpus", "1", "--M", "3000", "--N", "1500", "--K", "64", "--steps", "4",
                        "--warmup", "1", "--no-cpu-baseline"], capture_output=True, text=True, env=e, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip().startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert KEYS <= set(d) and d["n_gpus"] == 1 and d["config"]["rccl_ranks"] == 1 and d["config"]["collectives_issued"] > 0
    assert d["loss_last"] < d["loss_first"]


def test_bench_pinned_launcher_and_rank_failure():
    """A launcher that pins one device per rank leaves one visible device: LOCAL_RANK = 3 must run on device 0.  A rank that
    cannot get a device ends the job non-zero with its own message on stderr (no JSON line, no hang)."""
    args = ["--gpus", "1", "--M", "1000", "--N", "640", "--K", "32", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"]
    e3 = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="3")
    r3 = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], capture_output=True, text=True, env=e3, timeout=600)
    assert r3.returncode == 0, r3.stderr[-2000:]
    assert json.loads([ln for ln in r3.stdout.splitlines() if ln.strip()][0])["n_gpus"] == 1
    e0 = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0", HIP_VISIBLE_DEVICES="")
    r0 = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], capture_output=True, text=True, env=e0, timeout=600)
    assert r0.returncode != 0 and "[bench rank 0]" in r0.stderr, (r0.returncode, r0.stderr[-500:])
    assert not [ln for ln in r0.stdout.splitlines() if ln.strip()]
