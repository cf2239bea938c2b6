#!/usr/bin/env python3
"""Research-env rollouts (arcle_rollout_ex) against graph-replayed research steps, in one process with the runs alternated.

The configuration is bench.py's research_env leg: 8192 envs, the Crop table (agents/env.py:23-28), autoreset="resample" with colour
permutation + rot90 augmentation, dense reward, TimeLimit 100, episodes desynchronised.  Timed, T = 32 and 128 steps per launch:
  rollout + filtered rows   every step's FilterO2ARC row into int8 [T, N, 2720]
  rollout + packed rows     every step's packed row into uint8 [T, N, 912]
  rollout, no rows          reward / terminated / truncated / dense pair per step only
  steps (graph), rows incr. T research step launches replayed as one hipGraph, incremental rows (what ARCVecEnv runs)
  steps (graph), rows full  the same with the rows rewritten in full (the rollout's row contract)
Prints us per step of 8192 envs (median over rounds) and the bytes a step moves by design: actions in, per-step outputs out and, for a
rollout, the planes read once and written once per launch (spread over its T steps).  One JSON line per configuration.
    python tools/research_rolloutbench.py [--rounds 7]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from arcle_amd import actions  # noqa: E402
from arcle_amd.engine import STEP_FLAT_OBS, STEP_PACK_OBS, STEP_ROWS_INCREMENTAL  # noqa: E402
from arcle_amd.envs import ARCVecEnv, O2ARCv2Env  # noqa: E402
from arcle_amd.loaders import SyntheticLoader  # noqa: E402


class Crop(O2ARCv2Env):  # agents/env.py:23-28
    def create_operations(self):
        ops = super().create_operations()
        ops[33] = actions.reset_sel(actions.crop_grid)
        return ops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--n", type=int, default=8192)
    a = ap.parse_args()
    dev, n = torch.device("cuda:0"), a.n
    v = ARCVecEnv(Crop, n, SyntheticLoader(n_tasks=400, seed=1, max_size=(30, 30)), device=dev, seed=7, autoreset="resample",
                  augment=("permute", "rot90"), dense_reward=True, max_episode_steps=100)
    v.reset()
    v.enable_flat_rows(filtered=True)
    b = v.batch
    b.cnt[:, 0] = torch.randint(0, 100, (n,), device=dev, dtype=torch.int32)  # desynchronised episodes (bench.py research_env_leg)
    K = 128
    bbox_np, op_np = bench.make_actions(K, n, 2000)
    bbox, op = torch.from_numpy(bbox_np).to(dev).contiguous(), torch.from_numpy(op_np).to(dev).contiguous()
    st = torch.cuda.current_stream(dev).cuda_stream
    for i in range(100):
        b.step_bbox_ptr(bbox[i % K].data_ptr(), op[(i * 7 + 3) % K].data_ptr(), v.flags, st)
    torch.cuda.synchronize(dev)
    base = v.flags & ~(STEP_FLAT_OBS | STEP_ROWS_INCREMENTAL | STEP_PACK_OBS)
    L = (b.flat_obs_size(True) + 15) & ~15
    R = b.packed_obs_size()
    P, planes = 900, len(b.planes)
    cfgs, bufs = [], {}
    for T in (32, 128):
        trunc = torch.zeros((T, n), dtype=torch.uint8, device=dev)
        dense = torch.zeros((T, n, 2), dtype=torch.int32, device=dev)
        rows = torch.zeros((T, n, L), dtype=torch.int8, device=dev)
        packed = torch.zeros((T, n, R), dtype=torch.uint8, device=dev)
        bufs[T] = (trunc, dense, rows, packed)
        outs = 4 + 1 + 1 + 8  # reward, terminated, truncated, dense pair
        state = (planes * 1024 + (planes - 1) * 1024 + 2 * 16 + 2 * 8) / T  # planes + record + counters in and out, once per launch
        for name, fl, kw, extra in (("rollout+filtered_rows", base | STEP_FLAT_OBS, dict(rows=rows, rows_filtered=True), L),
                                    ("rollout+packed_rows", base | STEP_PACK_OBS, dict(packed=packed), R),
                                    ("rollout_no_rows", base, {}, 0)):
            def run(T=T, fl=fl, kw=kw, trunc=trunc, dense=dense):
                b.rollout_ex(bbox[:T], op[:T], fl, "bbox", trunc=trunc, dense=dense, **kw)
            cfgs.append({"name": name, "T": T, "run": run, "launches": 1, "bytes_per_env_step": 20 + outs + extra + state})
        for name, fl in (("steps_graph_rows_incremental", v.flags), ("steps_graph_rows_full", v.flags & ~STEP_ROWS_INCREMENTAL)):
            def enqueue(sh, T=T, fl=fl):
                for i in range(T):
                    b.step_bbox_ptr(bbox[i].data_ptr(), op[i].data_ptr(), fl, sh)
            _, g = bench.graph_time(dev, enqueue, T, reps=1, warm=1)
            # (a step reads and writes the planes it touches; rows: 2710 B written (full) — the algorithmic figure is bench.py's roofline)
            cfgs.append({"name": name, "T": T, "run": g.replay, "launches": T, "graph": g, "bytes_per_env_step": None})
    times = {i: [] for i in range(len(cfgs))}
    for _ in range(a.rounds):  # alternated: every configuration once per round
        for i, c in enumerate(cfgs):
            c["run"]()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c["run"]()
            e1.record()
            torch.cuda.synchronize(dev)
            times[i].append(e0.elapsed_time(e1) * 1e3 / c["T"])
    assert b.status() == 0
    for i, c in enumerate(cfgs):
        t = times[i]
        rec = {"config": c["name"], "T": c["T"], "n_envs": n, "us_per_step": round(float(np.median(t)), 3),
               "us_per_step_min": round(float(np.min(t)), 3), "us_per_step_max": round(float(np.max(t)), 3), "launches": c["launches"]}
        if c["bytes_per_env_step"] is not None:
            mb = c["bytes_per_env_step"] * n / 1e6
            rec.update({"MB_per_step_by_design": round(mb, 2), "TB_per_s": round(mb * 1e6 / (rec["us_per_step"] * 1e-6) / 1e12, 2)})
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
