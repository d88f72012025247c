"""End-to-end fit!(model) on a ROW-SHARDED synthetic model, with rank 0's per-stage time line (development aid).

python scripts/fit_e2e_sharded.py M N K --ranks P [--transport host|rccl] [--rank-timeout SECONDS]

The launcher starts P rank processes of this same file (never more than 16), each under its own time limit, and stops
everything at the first rank that fails.  Every rank builds its rows of the synthetic model of scripts/fit_e2e.py (same
low-rank signal, conditions, row batches and feature sets; the 2 % missing entries are drawn per rank), makes the sharded
model with make_model(..., row_shard=...), attaches the communicator and runs fit_.

  --transport host   the library's host-staged transport, gloo on the CPU moving the bytes, as the tests do; rank r uses
                     device r modulo the device count, so it is the only transport that runs on a one-GPU machine;
  --transport rccl   one GPU per rank, RCCL inside the library (rank 0's unique id travels through a file).

Two ranks sharing one device measure the path, not a speed-up: the numbers are no scaling figure."""
import argparse
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
MAX_RANKS, MAX_HW_QUEUES = 16, 32


def rank_main(a):
    sys.path.insert(0, str(ROOT))
    import pmf_import
    pkg = pmf_import.load()
    M, N, K, rank, world = a.M, a.N, a.K, a.rank, a.ranks
    lo, hi = pkg.parallel.shard_rows(M, world, rank)
    rng = np.random.default_rng(0)
    nrb, nsets = 4, 20
    Xt = rng.standard_normal((K, M)).astype(np.float32)
    Yt = rng.standard_normal((K, N)).astype(np.float32)
    Z = (Xt[:, lo:hi].T @ Yt).astype(np.float32)
    Z[np.random.default_rng([1, rank]).random((hi - lo, N)) < 0.02] = np.nan
    conds = [f"condition_{1 + (i * 2) // M}" for i in range(M)]
    fids = [f"x_{i}" for i in range(1, N + 1)]
    views = [1] * (N // 2) + [2] * (N - N // 2)
    batch_dict = {v: [f"rowbatch{1 + (i * nrb) // M}" for i in range(M)] for v in (1, 2)}
    fsets = {}
    for v, (c0, c1) in enumerate(((0, N // 2), (N // 2, N)), start=1):
        edges = np.linspace(c0, c1, nsets + 1).astype(int)
        fsets[v] = [[fids[j] for j in range(edges[s], edges[s + 1])] for s in range(nsets)]
    t0 = time.time()
    model = pkg.make_model(Z, K=K, sample_conditions=conds, feature_views=views, feature_ids=fids, batch_dict=batch_dict,
                           feature_sets_dict=fsets, Y_fsard=True, fsard_v0=0.5, rng=rng, row_shard=(lo, hi, M))
    say = print if rank == 0 else (lambda *x, **k: None)
    say(f"make_model rows {lo}:{hi} of {M} on each of {world} ranks, {time.time() - t0:.2f} s")
    device = 0
    if a.transport == "host":
        import torch
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(a.port), RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        device = rank % max(pkg._lib.device_count(), 1)
        model.attach_comm(rank, world, host_allreduce=lambda arr: dist.all_reduce(torch.from_numpy(arr)))
    else:
        device = rank
        id_file = Path(a.rendezvous) / "rccl_unique_id"
        if rank == 0:
            tmp = id_file.with_suffix(".tmp")
            tmp.write_bytes(bytes(pkg._lib.comm_unique_id()))
            tmp.rename(id_file)
        deadline = time.time() + 60
        while not id_file.exists():
            if time.time() > deadline:
                raise SystemExit(f"rank {rank}: no unique id from rank 0 after 60 s")
            time.sleep(0.05)
        model.attach_comm(rank, world, unique_id=id_file.read_bytes())
    model.device_context(device)
    t0 = time.time()
    hist = pkg.fit_(model, verbosity=0, lr=0.05, max_epochs=200, rel_tol=1e-5, abs_tol=1e-5, fsard_term_rtol=1e-3,
                    fsard_max_iter=2, fsard_max_A_iter=200, keep_history=True)
    tot = time.time() - t0
    info = model.device_context(device).comm_info()
    X = pkg.parallel.gather_factors(model)
    say(f"fit_ total {tot:.2f} s, {len(hist)} history entries, transport {info['transport']}, "
        f"{info['n_collectives']} collectives, gathered X {X.shape}")
    for d in hist:
        t = d.get("time", None)
        say(f"  {d.get('name')!s:38s} epochs={d.get('epochs', '')!s:6s} term={d.get('term_code', '')!s:14s} "
            f"t={t if t is None else round(t, 2)}")
    model.release_device()
    if a.transport == "host":
        dist.destroy_process_group()


def launch(a):
    if not 1 <= a.ranks <= MAX_RANKS:
        raise SystemExit(f"--ranks must be 1..{MAX_RANKS}")
    env = dict(os.environ)
    if int(env.get("GPU_MAX_HW_QUEUES", "0") or 0) > MAX_HW_QUEUES:
        env["GPU_MAX_HW_QUEUES"] = str(MAX_HW_QUEUES)
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    with tempfile.TemporaryDirectory() as rendezvous:
        base = [sys.executable, str(Path(__file__).resolve()), str(a.M), str(a.N), str(a.K), "--ranks", str(a.ranks),
                "--transport", a.transport, "--port", str(port), "--rendezvous", rendezvous]
        procs = [subprocess.Popen(base + ["--rank", str(r)], env=env) for r in range(a.ranks)]
        deadline = time.time() + a.rank_timeout          # (all ranks start together: one deadline is each rank's own limit)
        failed = None
        try:
            while failed is None and any(p.poll() is None for p in procs):
                for r, p in enumerate(procs):
                    if p.poll() not in (None, 0):
                        failed = f"rank {r} exited with status {p.returncode}"
                        break
                    if p.poll() is None and time.time() > deadline:
                        failed = f"rank {r} exceeded its time limit of {a.rank_timeout} s"
                        break
                time.sleep(0.2)
            for r, p in enumerate(procs):
                if failed is None and p.returncode != 0:
                    failed = f"rank {r} exited with status {p.returncode}"
        finally:
            for p in procs:                                # a rank left waiting in a collective must not outlive the launcher
                if p.poll() is None:
                    p.kill()
                    p.wait()
    if failed:
        raise SystemExit(f"fit_e2e_sharded: {failed}; the other ranks were stopped")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("M", type=int)
    ap.add_argument("N", type=int)
    ap.add_argument("K", type=int)
    ap.add_argument("--ranks", type=int, default=2)
    ap.add_argument("--transport", choices=("host", "rccl"), default="host")
    ap.add_argument("--rank-timeout", type=float, default=900.0)
    ap.add_argument("--rank", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--port", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--rendezvous", default="", help=argparse.SUPPRESS)
    args = ap.parse_args()
    rank_main(args) if args.rank is not None else launch(args)
