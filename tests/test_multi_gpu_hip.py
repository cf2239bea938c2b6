"""The N > 1 path on real hardware: runs whenever the box shows at least two GPUs (skipped on the one-GPU boxes).  One process per GPU,
torch.distributed backend "nccl" (= RCCL over xGMI):

  * ShardedVecEnv over the real ARCVecEnv, c4's flag set (step + fused packed row), an uneven global batch: the rows gathered by ONE
    all_gather_into_tensor per step — synchronously, overlapped on the side stream, in ping-pong groups, every K steps and replayed
    from a captured hipGraph — against the oracle stepping ALL global envs in one process, in global env order;
  * bench.py --gpus N --config c3 | c4 launched exactly as the driver does (torch.distributed.run): backend nccl, every rank counted,
    N x the per-GPU batch, the per-rank RCCL / device lines on stderr.
No 8-GPU run is claimed anywhere in this repo; this file exists so that the first contact with a node is a test run."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = W = 30
S = 12


def _n_gpus():
    import torch
    return min(8, torch.cuda.device_count()) if torch.cuda.is_available() else 0


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _inputs(G):
    import bench
    tasks = bench.make_tasks(G, 77)
    bb, op = bench.make_actions(S, G, 78)
    return tasks, bb, op


def _worker(rank, world, port, G, out_q):
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = torch.device(f"cuda:{rank}")
    torch.cuda.set_device(dev)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from arcle_amd.dist import ShardedVecEnv
    from arcle_amd.envs import ARCVecEnv, O2ARCv2Env
    from arcle_amd.loaders import SyntheticLoader
    tasks, bb_np, op_np = _inputs(G)
    bb, op = torch.from_numpy(bb_np).to(dev), torch.from_numpy(op_np).to(dev)

    def make(n, lo, hi):
        v = ARCVecEnv(O2ARCv2Env, n, SyntheticLoader(n_tasks=4, seed=1), device=dev, env_base=lo, autoreset=True)
        v.batch.set_tasks_padded(*(t[lo:hi] for t in tasks))  # the same tasks the oracle steps, by global env id
        v.batch.reset()
        return v
    out = {}
    env = ShardedVecEnv(G, make)
    assert env.fused and dist.get_backend() == "nccl"
    grids, rews = [], []
    for s in range(S):
        env.step_bbox(env.local_slice(bb[s]), env.local_slice(op[s]))
        g, gd, r, t = env.gather()
        grids.append(g.cpu().numpy().copy()), rews.append(r.cpu().numpy().copy())
    out["sync"] = (np.stack(grids), np.stack(rews))
    env = ShardedVecEnv(G, make)
    grids, pending = [], None
    for s in range(S):
        env.step_bbox(env.local_slice(bb[s]), env.local_slice(op[s]))
        work = env.gather_async()
        if pending is not None:
            grids.append(pending.wait()[0].cpu().numpy().copy())
            env.release(pending)
        pending = work
    grids.append(pending.wait()[0].cpu().numpy().copy())
    out["async"] = np.stack(grids)
    env = ShardedVecEnv(G, make, groups=2)
    per_group = [[], []]
    for s in range(S):
        works = []
        for g in range(2):
            env.step_bbox(env.local_slice(bb[s], g), env.local_slice(op[s], g), group=g)
            works.append(env.gather_async(g))
        for g in range(2):
            per_group[g].append(works[g].wait()[0].cpu().numpy().copy())
    out["groups"] = ([np.stack(x) for x in per_group], [env.group_global_ids(g).cpu().numpy() for g in range(2)])
    env = ShardedVecEnv(G, make, every=4)
    chunks = []
    for s in range(S):
        env.step_bbox(env.local_slice(bb[s]), env.local_slice(op[s]))
        if env.ready():
            chunks.append(env.gather()[0].cpu().numpy().copy())
    out["every"] = np.concatenate(chunks)
    # K steps + K all-gathers recorded into ONE hipGraph (RCCL collectives are capturable) — or the logged eager fallback
    env = ShardedVecEnv(G, make)
    try:
        lo, hi = env.lo, env.hi
        cap = env.capture(bb[:4, lo:hi].contiguous(), op[:4, lo:hi].contiguous())
        res = cap.replay()
        torch.cuda.synchronize(dev)
        out["captured"] = res[0][-1].cpu().numpy().copy() if isinstance(res, (tuple, list)) else None
        out["captured_mode"] = "hipGraph"
    except Exception as exc:  # noqa: BLE001 - the fallback is part of the contract being observed
        out["captured"], out["captured_mode"] = None, f"eager fallback: {type(exc).__name__}: {exc}"
    x = torch.ones(1, device=dev)
    dist.all_reduce(x)
    out["ranks_seen"] = int(x.item())
    print(f"rank {rank}/{world}: backend={dist.get_backend()} device={torch.cuda.get_device_name(dev)} shard [{env.lo}, {env.hi})", file=sys.stderr, flush=True)
    if rank == 0:
        out_q.put(out)
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_vec_env_over_rccl_vs_oracle_all_ranks():
    n = _n_gpus()
    if n < 2:
        pytest.skip("needs at least two GPUs (the driver's multi-GPU tier)")
    import torch.multiprocessing as mp
    import backends as B
    from oracle import oracle as O
    G = n * 2304 + 3  # uneven shards (the short ones are padded for the collective)
    ctx = mp.get_context("spawn")
    q, port = ctx.Queue(), _free_port()
    procs = [ctx.Process(target=_worker, args=(r, n, port, G, q)) for r in range(n)]
    for p in procs:
        p.start()
    out = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert out["ranks_seen"] == n
    tasks, bb_np, op_np = _inputs(G)
    O.set_threads(16)
    try:
        orc = B.OracleBackend(G, H, W, -1, "o2arc", O.o2arc_ops())
        orc.set_tasks(*tasks)
        orc.reset()
        want, rew = [], []
        for s in range(S):
            r, t = orc.step("bbox", bb_np[s], op_np[s], O.STEP_AUTORESET)
            want.append(orc.get("grid").copy()), rew.append(r.copy())
    finally:
        O.set_threads(1)
    want, rew = np.stack(want), np.stack(rew)
    assert np.array_equal(out["sync"][0], want) and np.array_equal(out["sync"][1], rew), "gathered rows differ from the oracle's global batch"
    assert np.array_equal(out["async"], want), "overlapped gathers differ"
    (ga, gb), (ia, ib) = out["groups"]
    assert sorted(ia.tolist() + ib.tolist()) == list(range(G))
    assert np.array_equal(ga, want[:, ia]) and np.array_equal(gb, want[:, ib]), "ping-pong groups differ"
    assert np.array_equal(out["every"], want), "every=4 gathers differ"
    print("captured gather:", out["captured_mode"], file=sys.stderr)
    if out["captured"] is not None:
        assert np.array_equal(out["captured"], want[3]), "graph-captured step + all-gather differs"


@pytest.mark.parametrize("cfg", ["c3", "c4"])
def test_bench_all_gpus_over_rccl_as_the_driver_launches_it(cfg):
    n = _n_gpus()
    if n < 2:
        pytest.skip("needs at least two GPUs (the driver's multi-GPU tier)")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "20", "--warmup", "5",
           "--config", cfg, "--full", "--no-cpu-baseline", "--no-extras"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    c = out["collective"]
    assert out["n_gpus"] == n and c["backend"] == "nccl" and c["world"] == n and c["ranks_seen"] == n and c["shared_gpu"] is False
    assert out["config"]["global_envs"] == n * out["config"]["envs_per_gpu"] and out["scaling"] == "weak" and out["value"] > 0
    rank_lines = [ln for ln in p.stderr.splitlines() if ln.startswith("bench: rank ")]
    assert len(rank_lines) == n and all("backend=nccl" in ln for ln in rank_lines), p.stderr[-2000:]
    assert all(" RCCL " in ln for ln in rank_lines), "every rank logs the RCCL version it runs"
    if cfg == "c3":  # BASELINE configs[3] / [4] over RCCL, on the same process group, inside the driver's own command
        m = out["multi"]
        assert "error" not in m, m
        assert m["c4_global_envs"] == 8192 * n and m["c5_global_envs"] == 4096 * n and m["transport"].startswith("RCCL")
        for k in ("c4_us_per_step", "c4_serial_us_per_step", "c4_gather_only_us", "gather_GBps", "gather_GBps_per_link_dir", "c5_us_per_step"):
            assert m[k] > 0, k
        assert m["c4_us_per_step"] <= m["c4_serial_us_per_step"] * 1.15, "the overlapped form must not be slower than step-then-gather"
