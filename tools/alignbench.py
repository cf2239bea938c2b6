#!/usr/bin/env python3
"""At which offset does the grid, or the input, fit the answer's canvas?  arcle_align_rows beside the route the library had before it:
every offset of both sources as the three-step macro [Copy on the rectangle the canvas covers, resize_grid to the answer's dims, Paste at
the corner] through arcle_expand_macros with the dense pair, then an arg-max per source on the device.

Inputs: 1024 and 4096 freshly reset 30 x 30 O2ARC state rows (grid = input: random colours 1 .. 9) whose 10 x 10 answer is planted as a
window of the input; both sources, no distance limit; row m is judged by env m; under both Pastes (the default table's paste_blank, and
the same table with a Paste that writes positive cells only).

  (a) align_rows(sources = 3): one launch
  (b) the same library: ALL 39 x 39 offsets of both sources — 3042 macros of three steps per row, one set for every row (the dims are
      the same in every row, so the set is: the cheaper form of arcle_expand_macros) — through expand_macros(dense), and per source
      the arg-max of correct under the tie rule of arcle_align_rows (torch, in the same captured graph).  Building the macro set is
      not timed.

Graph-replayed legs alternating in one process, HIP events around >= 0.5 s of work per repeat (3 warm replays).  Both legs must name
the same (ox, oy, correct, total) for EVERY row and source; the tool says whether they do.  Only the row board is timed: the flat
board (W > 32) is checked for its answers by the tests.

Usage: python tools/alignbench.py [--out profiles/align_bench.txt] [--repeats 5] [--rows 1024 4096] [--resources FILE]
(--resources: a text file with the kernels' register and scratch figures from the gfx950 compile, copied into the report)"""
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

COPY_OPS, RESIZE_OP, PASTE_OP = (29, 28), 33, 30  # O2ARCv2Env's table: Copy_O, Copy_I, resize_grid, Paste
AH = AW = 10


def tasks(n, H, W, seed=31):
    """n (input, answer) pairs: the input random colours 1 .. 9, the answer a 10 x 10 window of it at a random place"""
    rng = np.random.default_rng(seed)
    inp = rng.integers(1, 10, (n, H, W)).astype(np.int8)
    ans = np.zeros((n, H, W), np.int8)
    at = np.stack([rng.integers(0, H - AH + 1, n), rng.integers(0, W - AW + 1, n)], 1)
    for m in range(n):
        ans[m, :AH, :AW] = inp[m, at[m, 0]:at[m, 0] + AH, at[m, 1]:at[m, 1] + AW]
    return inp, ans, at


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--resources", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H = W = 30
    cand = [(ox, oy) for ox in range(1 - AH, H) for oy in range(1 - AW, W)]
    K1 = len(cand)
    K = 2 * K1
    cox = torch.tensor([c[0] for c in cand], dtype=torch.int64, device=dev)
    coy = torch.tensor([c[1] for c in cand], dtype=torch.int64, device=dev)
    prio = (((127 - cox.abs() - coy.abs()) << 13) + ((63 - cox) << 6) + (31 - coy)).reshape(1, 1, K1)  # larger = preferred among equal counts
    zero = torch.zeros_like(cox)
    px, py = torch.maximum(-cox, zero), torch.maximum(-coy, zero)
    one = torch.stack([S._rect_bits(torch.maximum(cox, zero), torch.minimum(zero + H, AH + cox) - 1, torch.maximum(coy, zero), torch.minimum(zero + W, AW + coy) - 1, H, W),
                       S._rect_bits(zero, zero + AH - 1, zero, zero + AW - 1, H, W), S._rect_bits(px, px, py, py, H, W)], 1)  # [K1, 3, 128]
    bits = torch.cat([one, one]).contiguous()
    op = torch.tensor([[COPY_OPS[s], RESIZE_OP, PASTE_OP] for s in range(2) for _ in range(K1)], dtype=torch.int32, device=dev)
    length = torch.full((K,), 3, dtype=torch.int32, device=dev)
    default = O2ARCv2Env.default_operations()
    tables = {True: actions.table_descs(default), False: [d & ~0xff00 if (d & 0xff) == 7 else d for d in actions.table_descs(default)]}  # (OP_PASTE = 7; arg 0: no paste_blank)
    lines = [f"alignbench: {H}x{W} O2ARC, freshly reset rows (grid = input: random colours 1 .. 9), the {AH}x{AW} answer a window of the input; both sources, no distance "
             f"limit, row m judged by env m",
             f"command: python tools/alignbench.py --repeats {a.repeats} --rows {' '.join(str(r) for r in a.rows)}{' --resources FILE' if a.resources else ''}",
             f"us per call = median of {a.repeats} repeats [min .. max], each repeat >= 0.5 s of graph replays (3 warm replays), legs alternating; one library (ABI "
             f"{EnvBatch(1, H, W, 3, 'o2arc').L.arcle_abi_version()}) for both legs",
             f"(a) align_rows(sources = 3); (b) expand_macros(dense) over 2 x {K1} three-step macros per row (one set for every row) + arg-max per source",
             "the flat board (W > 32) was checked for its answers (tests/test_align_emu.py, tests/test_align_hip.py), not timed"]

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for M in a.rows:
        inp, ans, at = tasks(M, H, W)
        dims = np.tile(np.array([[H, W]], np.int8), (M, 1))
        adims = np.tile(np.array([[AH, AW]], np.int8), (M, 1))
        for blank in (True, False):
            b = EnvBatch(M, H, W, 3, "o2arc")
            b.set_op_table(tables[blank])
            b.set_tasks_padded(inp, dims, ans, adims)
            b.reset()
            rows = b.get_state_rows().clone()
            src = torch.arange(M, dtype=torch.int32, device=dev)
            out_a = b.align_rows(rows, src, None, 3, blank)
            ex = b.expand_macros(rows, "bits", bits, op, length, src, dense=True)
            res_b = torch.zeros((M, 2, 4), dtype=torch.int64, device=dev)

            def leg_a():
                b.align_rows(rows, src, None, 3, blank, out=out_a)

            def leg_b():
                b.expand_macros(rows, "bits", bits, op, length, src, dense=True, out=ex)
                dense0 = ex.dense[:, :, 0].to(torch.int64).reshape(M, 2, K1)
                key = torch.where((ex.status == 0).reshape(M, 2, K1), dense0 * (1 << 20) + prio, torch.full((), -1, dtype=torch.int64, device=dev))
                k = key.argmax(-1)
                res_b[..., 0] = cox[k]
                res_b[..., 1] = coy[k]
                res_b[..., 2] = key.gather(-1, k.unsqueeze(-1)).squeeze(-1) >> 20
                res_b[..., 3] = ex.dense[:, :, 1].to(torch.int64).reshape(M, 2, K1).gather(-1, k.unsqueeze(-1)).squeeze(-1)
            leg_a()
            leg_b()
            torch.cuda.synchronize(dev)
            bad_status = int((ex.status != 0).sum())
            same = bool((res_b == out_a[0][..., :4].to(torch.int64)).all())
            planted = bool((out_a[0][:, :, :2].cpu() == torch.as_tensor(at, dtype=torch.int32).reshape(M, 1, 2)).all()) and bool((out_a[0][..., 2] == AH * AW).all())
            runs = [("(a) align_rows", timed_graph(dev, leg_a, 8)), ("(b) expand_macros + arg-max", timed_graph(dev, leg_b, 1))]
            times = {name: [] for name, _ in runs}
            for _ in range(a.repeats):
                for name, (run, _) in runs:
                    times[name].append(run())
            ta, tb = (np.array(times[name]) for name, _ in runs)
            lines.append(f"{M} rows, blank = {int(blank)} ({M * K} macros of 3 steps, {bad_status} of them refused); every row's planted window found by both sources with "
                         f"{AH * AW} of {AH * AW} cells: {planted}; both legs name the same (ox, oy, correct, total) for every row and source: {same}")
            lines += report(times)
            spread = max(tb.max() - tb.min(), ta.max() - ta.min())
            lines.append(f"  (b) / (a) = {np.median(tb) / np.median(ta):.1f} x; (b) - (a) = {(np.median(tb) - np.median(ta)) * 1e6:.2f} us against run-to-run spreads of "
                         f"{(ta.max() - ta.min()) * 1e6:.2f} us (a) and {(tb.max() - tb.min()) * 1e6:.2f} us (b): (a) is "
                         f"{'faster' if np.median(tb) - np.median(ta) > spread else 'NOT faster'} by more than both spreads")
            flush()
            del b, ex, runs, out_a, res_b
            torch.cuda.empty_cache()
    if a.resources:
        lines += ["", "kernel resources (-Rpass-analysis=kernel-resource-usage of the gfx950 compile of arcle_amd/csrc/arcle_hip.hip):"]
        lines += ["  " + ln.rstrip() for ln in open(a.resources) if ln.strip()]
    flush()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
