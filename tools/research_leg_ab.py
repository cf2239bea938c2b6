#!/usr/bin/env python3
"""The research-env leg of bench.py --full (bench.research_env_leg: 8192 envs, graph-replayed research steps, incremental and fully
rewritten rows) on two builds of libarcle_hip.so, alternated in one session:

  python tools/research_leg_ab.py LIB_A LIB_B [--rounds 3] [--envs 8192] [--out FILE]

Every run is a fresh child process (ARCLE_HIP_LIB picks its library) under a time limit of its own; the first child that fails ends the
session.  Prints, per library, every run's us per step batch and the band (min / median / max), and which plan the launches took."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(n):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    bb_np, op_np = bench.make_actions(400, n, 2000)
    bbox, op = torch.from_numpy(bb_np).to(dev), torch.from_numpy(op_np).to(dev)
    out = bench.research_env_leg(dev, n, bbox, op)
    print("RESULT " + json.dumps({k: out[k]["us_per_step_batch"] for k in ("rows_incremental", "rows_rewritten_in_full")}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a.envs)
    assert len(a.libs) == 2, "two libraries"
    runs = {lib: [] for lib in a.libs}
    for r in range(a.rounds):
        for lib in a.libs:
            env = dict(os.environ, ARCLE_HIP_LIB=os.path.abspath(lib))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--envs", str(a.envs)], env=env, capture_output=True, text=True, timeout=240)
            res = [line for line in p.stdout.splitlines() if line.startswith("RESULT ")]
            if p.returncode != 0 or not res:
                sys.exit(f"round {r} {lib}: exit status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
            runs[lib].append(json.loads(res[0][7:]))
            print(f"round {r} {lib}: {runs[lib][-1]}", flush=True)
    lines = [f"research_env leg of bench.py --full, {a.envs} envs, {a.rounds} alternated runs per library (us per step batch: min / median / max)"]
    for lib, rs in runs.items():
        for k in ("rows_incremental", "rows_rewritten_in_full"):
            v = sorted(x[k] for x in rs)
            lines.append(f"  {lib:40s} {k:24s} {v[0]:7.2f} / {v[len(v) // 2]:7.2f} / {v[-1]:7.2f}    runs: " + " ".join(f"{x[k]:.2f}" for x in rs))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
