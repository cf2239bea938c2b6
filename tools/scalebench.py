#!/usr/bin/env python3
"""Is the answer the grid, or the input, zoomed, shrunk or tiled?  arcle_scale_rows beside the only route the library had before it:
every one of the 2 x 132 candidates as a host-built macro [resize_grid to the answer's dims, then one Color step per colour of the
candidate's child on that colour's cells] of up to 10 steps through arcle_expand_macros with the dense pair, then an arg-max per source
on the device.

Inputs: 1024 and 4096 freshly reset O2ARC state rows (grid = input) on a 30 x 30 plane whose source is 10 x 10 random colours 1 .. 9
and whose answer is that source under a planted candidate (zooms by (3, 3), (2, 2) and (2, 3), the four tilings, a shrink by (2, 2));
both sources, all three modes; row m is judged by env m.  The rows cycle through 16 distinct tasks: the macros of (b) are built once
per distinct task on the host (scale_numpy's children) and spread over the rows by one indexing pass on the device, so that (b) reads a
macro set per row, as a search that builds them per state would hand it over.  Building and uploading the macros is not timed.

  (a) scale_rows(sources = 3, modes = 7) with its bit rows: one launch
  (b) the same library: ALL 2 x 132 candidates per row — macros of 1 + (colours of the child) steps, a set per row — through
      expand_macros(dense), and per source the arg-max of correct, ties to the lowest index (torch, in the same captured graph)

Graph-replayed legs alternating in one process, HIP events around >= 0.5 s of work per repeat (3 warm replays).  Both legs must name
the same (cand, correct) for EVERY row and source; the tool says whether they do.  --size / --source run another plane, e.g. the flat
board at 16 x 33 with an 8 x 11 source.

Usage: python tools/scalebench.py [--out profiles/scale_bench.txt] [--repeats 5] [--rows 1024 4096] [--size 30 30] [--source 10 10]
       [--resources FILE] [--append]
(--resources: a text file with the kernels' register and scratch figures from the gfx950 compile, copied into the report; --append:
add to the report instead of replacing it)"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from expandbench import timed_graph  # noqa: E402
from turnbench import report  # noqa: E402
from arcle_amd import actions  # noqa: E402
from arcle_amd import search as S  # noqa: E402
from arcle_amd.engine import EnvBatch  # noqa: E402
from arcle_amd.envs import O2ARCv2Env  # noqa: E402
from arcle_amd.envs.vec import scales_of  # noqa: E402

RESIZE_OP, COLOR_OPS = 33, tuple(range(10))  # O2ARCv2Env's table: resize_grid, Color 0 .. 9
DISTINCT = 16
K1 = S.SCALE_CANDS


def tasks(H, W, sh, sw, seed=41):
    """DISTINCT (input, answer, answer_dim, planted candidate): the input sh x sw random colours 1 .. 9, the answer its child under a
    planted candidate, cut to the plane"""
    rng = np.random.default_rng(seed)
    plans = [8 * 2 + 2, 8 * 1 + 1, 8 * 1 + 2, 128, 129, 130, 131, 64 + 8 * 1 + 1]  # ZOOM (3, 3), (2, 2), (2, 3); TILE 0 .. 3; SHRINK (2, 2)
    inp, ans, adim, plan = np.zeros((DISTINCT, H, W), np.int8), np.zeros((DISTINCT, H, W), np.int8), np.zeros((DISTINCT, 2), np.int8), []
    for d in range(DISTINCT):
        cand = plans[d % len(plans)]
        mode, kx, ky = S.scale_candidates()[cand]
        inp[d, :sh, :sw] = rng.integers(1, 10, (sh, sw))
        ah, aw = (H, W) if mode == 2 else (min(H, sh * kx), min(W, sw * ky)) if mode == 0 else ((sh + kx - 1) // kx, (sw + ky - 1) // ky)
        adim[d] = (ah, aw)
        _, _, _, children = S.scale_numpy(inp[d], (sh, sw), inp[d], (sh, sw), ans[d], (ah, aw), 1, 7, full=True)
        ans[d] = children[0, cand]
        plan.append(cand)
    return inp, ans, adim, plan


def macro_sets(inp, ans, adim, sh, sw, H, W, dev):
    """All 2 x 132 candidates of every distinct task as macros, built from scale_numpy's children -> bits uint8 [D, 264, 10, 128], op
    int32 [D, 264, 10], length int32 [D, 264].  scale_macros does the packing: candidate c of task d is handed to it as the 'best' of a
    row of its own (base (-1, 1): nothing is dropped)."""
    D = len(inp)
    ch = np.stack([S.scale_numpy(inp[d], (sh, sw), inp[d], (sh, sw), ans[d], adim[d], 3, 7, full=True)[3] for d in range(D)])  # [D, 2, 132, H, W]
    ch = torch.as_tensor(ch, device=dev).permute(0, 2, 1, 3, 4).reshape(D * K1, 2, 1, H, W)
    c = torch.arange(1, 10, device=dev).reshape(1, 1, 9, 1, 1)
    cells = ch == c                                                                                       # [D * 132, 2, 9, H, W]
    colours = (cells.flatten(3).any(-1).to(torch.int32) << c.reshape(1, 1, 9).to(torch.int32)).sum(-1).to(torch.int32)
    one = torch.ones((D * K1, 2), dtype=torch.int32, device=dev)
    dims = torch.as_tensor(adim, device=dev).to(torch.int32).repeat_interleave(K1, 0).reshape(D * K1, 1, 2).expand(D * K1, 2, 2)
    fake = scales_of(torch.cat([torch.stack([one, one, one, colours], -1), dims, dims], -1), None, S.pack_bits(cells),
                     torch.tensor([[-1, 1]], dtype=torch.int32, device=dev).expand(D * K1, 2))
    mac = S.scale_macros(fake, RESIZE_OP, COLOR_OPS, H, W)
    # [D * 132, 2, ...] -> [D, 2 * 132, ...]: source-major, as scale's slots
    return tuple(mac[k].reshape((D, K1, 2) + tuple(mac[k].shape[2:])).transpose(1, 2).reshape((D, 2 * K1) + tuple(mac[k].shape[2:])).contiguous()
                 for k in ("bits", "operation", "length"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_bench.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--size", type=int, nargs=2, default=[30, 30])
    ap.add_argument("--source", type=int, nargs=2, default=[10, 10])
    ap.add_argument("--resources", default=None)
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    (H, W), (sh, sw) = a.size, a.source
    K = 2 * K1
    board = "flat board" if W > 32 or H > 64 else "row board"
    lines = [f"scalebench: {H}x{W} O2ARC ({board}), freshly reset rows (grid = input: {sh}x{sw} random colours 1 .. 9), the answer the source under a planted candidate; "
             f"both sources, all modes, row m judged by env m; the rows cycle through {DISTINCT} distinct tasks",
             f"command: python tools/scalebench.py --repeats {a.repeats} --rows {' '.join(str(r) for r in a.rows)} --size {H} {W} --source {sh} {sw}"
             f"{' --resources FILE' if a.resources else ''}{' --append' if a.append else ''}",
             f"us per call = median of {a.repeats} repeats [min .. max], each repeat >= 0.5 s of graph replays (3 warm replays), legs alternating; one library (ABI "
             f"{EnvBatch(1, H, W, 3, 'o2arc').L.arcle_abi_version()}) for both legs",
             f"(a) scale_rows(sources = 3, modes = 7, bits); (b) expand_macros(dense) over 2 x {K1} macros of up to 10 steps per row (a set per row, built and uploaded "
             f"beforehand) + arg-max per source"]
    head = open(a.out).read().rstrip("\n").split("\n") + [""] if a.append and os.path.exists(a.out) else []

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(head + lines) + "\n")
    inp, ans, adim, plan = tasks(H, W, sh, sw)
    sets = macro_sets(inp, ans, adim, sh, sw, H, W, dev)
    prio = (255 - torch.arange(K1, device=dev, dtype=torch.int64)).reshape(1, 1, K1)
    for M in a.rows:
        task = np.arange(M) % DISTINCT
        b = EnvBatch(M, H, W, 3, "o2arc")
        b.set_op_table(actions.table_descs(O2ARCv2Env.default_operations()))
        b.set_tasks_padded(inp[task], np.tile(np.array([[sh, sw]], np.int8), (M, 1)), ans[task], adim[task])
        b.reset()
        rows = b.get_state_rows().clone()
        src = torch.arange(M, dtype=torch.int32, device=dev)
        tid = torch.as_tensor(task, device=dev)
        bits, op, length = (t[tid].contiguous() for t in sets)  # a set per row
        out_a = b.scale_rows(rows, src)
        ex = b.expand_macros(rows, "bits", bits, op, length, src, dense=True)
        res_b = torch.zeros((M, 2, 2), dtype=torch.int64, device=dev)

        def leg_a():
            b.scale_rows(rows, src, out=out_a)

        def leg_b():
            b.expand_macros(rows, "bits", bits, op, length, src, dense=True, out=ex)
            dense0 = ex.dense[:, :, 0].to(torch.int64).reshape(M, 2, K1)
            key = torch.where((ex.status == 0).reshape(M, 2, K1), dense0 * 256 + prio, torch.full((), -1, dtype=torch.int64, device=dev))
            best = key.max(-1).values
            res_b[..., 0] = 255 - (best & 255)
            res_b[..., 1] = best >> 8
        leg_a()
        leg_b()
        torch.cuda.synchronize(dev)
        bad_status = int((ex.status != 0).sum())
        steps = int(length.sum())
        same = bool((res_b == out_a[0][..., :2].to(torch.int64)).all())
        want = torch.as_tensor(np.array(plan)[task], dtype=torch.int32).reshape(M, 1)
        planted = bool((out_a[0][..., 1] == out_a[0][..., 2]).all()) and bool((out_a[0][..., 0].cpu() == want).all())
        runs = [("(a) scale_rows", timed_graph(dev, leg_a, 8)), ("(b) expand_macros + arg-max", timed_graph(dev, leg_b, 1))]
        times = {name: [] for name, _ in runs}
        for _ in range(a.repeats):
            for name, (run, _) in runs:
                times[name].append(run())
        ta, tb = (np.array(times[name]) for name, _ in runs)
        lines.append(f"{M} rows ({M * K} macros, {steps} steps in all, {bad_status} macros refused); every row's planted candidate is the best of both sources and "
                     f"perfect: {planted}; both legs name the same (cand, correct) for every row and source: {same}")
        lines += report(times)
        spread = max(tb.max() - tb.min(), ta.max() - ta.min())
        lines.append(f"  (b) / (a) = {np.median(tb) / np.median(ta):.1f} x; (b) - (a) = {(np.median(tb) - np.median(ta)) * 1e6:.2f} us against run-to-run spreads of "
                     f"{(ta.max() - ta.min()) * 1e6:.2f} us (a) and {(tb.max() - tb.min()) * 1e6:.2f} us (b): (a) is "
                     f"{'faster' if np.median(tb) - np.median(ta) > spread else 'NOT faster'} by more than both spreads")
        flush()
        del b, ex, runs, out_a, res_b, bits, op, length
        torch.cuda.empty_cache()
    if a.resources:
        lines += ["", "kernel resources of the three arcle_scale_kernel instantiations:"]
        lines += ["  " + ln.rstrip() for ln in open(a.resources) if ln.strip()]
    flush()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
