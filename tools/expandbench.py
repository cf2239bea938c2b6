#!/usr/bin/env python3
"""Expanding a search frontier: K candidate actions for each of M state rows, three ways, at the project's own sizes (30 x 30 O2ARC,
states taken from 8192 envs after 10 random steps), alternating in one process, graph-replayed, HIP events around >= 0.5 s of work:

  (a) rows      the only route before arcle_expand_rows: index_select to [M*K] rows + out-of-place arcle_transition_rows (with the
                dense pair where M*K <= 8192 — the dense output is per env; without it beyond, i.e. given even less to do).  It
                produces NO hashes.
  (b) expand    arcle_expand_rows with one shared action set, and with a set per row: reward, terminated, status, dense pair and
                the (state_hash, grid_hash) of every child, ~38 bytes per child written
  (c) hash      arcle_hash_rows of the M rows alone

Prints us per launch (median and spread of three repeats), children/s and, for (b), the bytes the algorithm needs (M rows + actions
+ outputs) over the time as a share of 8 TB/s — the byte rate of a kernel that is bound by instruction issue, not by memory.
Usage: python tools/expandbench.py [--out profiles/expand_bench.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

HBM_PEAK = 8e12
SIZES = ((8192, 1), (1024, 32), (256, 256), (64, 1024))


def timed_graph(dev, enqueue, inner, min_s=0.5, warm=3):
    """`inner` launches of `enqueue` captured into one graph -> a function that replays it for >= min_s and returns seconds per launch."""
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        for _ in range(inner):
            enqueue()
    for _ in range(warm):
        g.replay()
    torch.cuda.synchronize(dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize(dev)
    reps = max(1, int(np.ceil(min_s / max(e0.elapsed_time(e1) * 1e-3, 1e-6))))

    def run():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            g.replay()
        b.record()
        torch.cuda.synchronize(dev)
        return a.elapsed_time(b) * 1e-3 / (reps * inner)
    return run, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "expand_bench.txt"))
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = 8192
    batch = bench.make_batch(dev, n)
    batch.set_dense_output()
    bbox, op = bench.make_actions(10, n, 2000)
    sh = torch.cuda.current_stream(dev).cuda_stream
    for i in range(10):
        bb, oo = torch.as_tensor(bbox[i], device=dev), torch.as_tensor(op[i], device=dev)
        batch.step_bbox_ptr(bb.data_ptr(), oo.data_ptr(), 0, sh)
        torch.cuda.synchronize(dev)
    all_rows = batch.get_state_rows().clone()
    L = batch.state_row_size()
    stride = (L + 15) & ~15
    lines = [f"expandbench: 30x30 O2ARC, rows of {L} B from {n} envs after 10 random steps; us per launch = median of {a.repeats} repeats "
             f"[min .. max], each >= 0.5 s of graph replays, legs alternating"]
    for M, K in SIZES:
        C = M * K
        src = torch.randperm(n, generator=torch.Generator().manual_seed(M))[:M].to(torch.int32).to(dev)
        rows = torch.zeros((M, stride), dtype=torch.int8, device=dev)  # (16-byte aligned rows: the row kernel's faster input form)
        rows[:, :L] = all_rows.index_select(0, src.long())
        pb, po = bench.make_actions(1, C, 77 + K)
        per_b, per_o = torch.as_tensor(pb[0], device=dev).reshape(M, K, 4).contiguous(), torch.as_tensor(po[0], device=dev).reshape(M, K).contiguous()
        sh_b, sh_o = per_b[0].contiguous(), per_o[0].contiguous()
        # (a) the row route over the shared set
        rep = torch.arange(M, device=dev).repeat_interleave(K)
        src_rep = src.index_select(0, rep).contiguous()
        pay_rep, op_rep = sh_b.repeat(M, 1).contiguous(), sh_o.repeat(M).contiguous()
        big = torch.empty((C, rows.shape[1]), dtype=torch.int8, device=dev)
        out = torch.empty((C, stride), dtype=torch.int8, device=dev)
        rw, tm = torch.empty(C, dtype=torch.int32, device=dev), torch.empty(C, dtype=torch.uint8, device=dev)
        fl = 16 if C <= n else 0

        def leg_rows():
            torch.index_select(rows, 0, rep, out=big)
            batch.transition_rows(big, "bbox", pay_rep, op_rep, src_rep, out=out, flags=fl, reward=rw, term=tm)
        ex_s = batch.expand_rows(rows, "bbox", sh_b, sh_o, src, dense=True)
        ex_p = batch.expand_rows(rows, "bbox", per_b, per_o, src, dense=True)
        hs = torch.empty((M, 2), dtype=torch.int64, device=dev)
        legs = [("rows" + ("+dense" if fl else ""), leg_rows), ("expand shared", lambda: batch.expand_rows(rows, "bbox", sh_b, sh_o, src, dense=True, out=ex_s)),
                ("expand per-row", lambda: batch.expand_rows(rows, "bbox", per_b, per_o, src, dense=True, out=ex_p)),
                ("hash", lambda: batch.hash_rows(rows, out=hs))]
        torch.cuda.synchronize(dev)
        inner = max(1, min(64, 65536 // C))
        runs = [(name, timed_graph(dev, fn, inner)) for name, fn in legs]
        times = {name: [] for name, _ in legs}
        for _ in range(a.repeats):
            for name, (run, _) in runs:
                times[name].append(run())
        lines.append(f"(M, K) = ({M}, {K}): {C} children per launch")
        for name, _ in legs:
            t = np.array(times[name])
            med = float(np.median(t))
            line = f"  {name:<15} {med * 1e6:10.2f} us  [{t.min() * 1e6:.2f} .. {t.max() * 1e6:.2f}]"
            if name != "hash":
                line += f"   {C / med / 1e9:7.3f} G children/s"
            if name.startswith("expand"):
                need = M * L + (K if "shared" in name else C) * 20 + C * (4 + 1 + 1 + 16 + 8) + M * 16
                line += f"   needs {need / 1e6:.2f} MB: {need / med / 1e9:.1f} GB/s = {100 * need / med / HBM_PEAK:.2f} % of 8 TB/s (issue-bound kernel's byte rate)"
            lines.append(line)
        ra, rb = np.array(times[legs[0][0]]), np.array(times["expand shared"])
        lines.append(f"  rows / expand shared = {np.median(ra) / np.median(rb):.2f}x  (slowest expand repeat vs fastest rows repeat: {ra.min() / rb.max():.2f}x)")
        del runs, big, out
        torch.cuda.empty_cache()
    assert batch.status(True) in (0, 2, 8, 10), "unexpected status bits"  # (the row route raises Rotate-domain / selection bits; expand never touches the word)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
