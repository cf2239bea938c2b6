#!/usr/bin/env python3
"""Where does a COPY of each object belong?  arcle_stamp_rows beside the route the library had before it: every paste position of every
object as a two-step CopyO + Paste macro through arcle_expand_macros with the dense pair, then an arg-max on the device.

Inputs: 1024 and 4096 freshly reset 30 x 30 O2ARC state rows with 16 objects each (one 2-4 cell two-colour shape in every cell of a
4 x 4 lattice) whose answer holds, besides the objects, one copy of each somewhere in the grid (later copies may cover earlier ones);
no distance limit; row m is judged by env m.  Both Pastes: blank = 1 (the default table) and blank = 0 (the same table with the
Paste's arg byte 0).

  (a) objects_rows(any_color, diagonal, bits) + stamp_rows: two launches
  (b) the same library: objects_rows as in (a), then ALL 900 cells (px, py) of the grid for every object as macros [CopyO on the
      object's cells, Paste on the one cell] — 16 x 900 macros of two steps per row — through expand_macros(dense), and per object
      the arg-max of correct under the tie rule of arcle_stamp_rows (torch, in the same captured graph).  Building the macro set is not
      timed.

Graph-replayed legs alternating in one process, HIP events around >= 0.5 s of work per repeat (3 warm replays).  Both legs must name
the same position and count for EVERY object; the tool says whether they do.

Usage: python tools/stampbench.py [--out profiles/stamp_bench.txt] [--repeats 5] [--rows 1024 4096] [--resources FILE]
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
from placebench import SHAPES  # noqa: E402
from arcle_amd import actions  # noqa: E402
from arcle_amd.engine import EnvBatch  # noqa: E402
from arcle_amd.envs import O2ARCv2Env  # noqa: E402

H = W = 30
C = 16
COPY_OP, PASTE_OP = 29, 30  # O2ARCv2Env's table: CopyO, Paste


def tasks(n, seed=23):
    """n (input, answer) pairs: 16 shapes, one per 7 x 7 lattice cell (a free border keeps them apart, also diagonally), each of two
    colours; the answer is the input with the clip of every shape's box pasted once at a random cell (cut at the grid's edge)."""
    rng = np.random.default_rng(seed)
    inp = np.zeros((n, H, W), np.int8)
    ans = np.zeros((n, H, W), np.int8)
    for m in range(n):
        shapes = []
        for i in range(4):
            for j in range(4):
                sh = np.array(SHAPES[rng.integers(0, len(SHAPES))])
                x, y = 1 + 7 * i + int(rng.integers(0, 3)), 1 + 7 * j + int(rng.integers(0, 3))
                cols = rng.integers(1, 10, 2)[(np.arange(len(sh)) >= len(sh) // 2).astype(int)]
                inp[m, x + sh[:, 0], y + sh[:, 1]] = cols
                shapes.append((sh, cols))
        ans[m] = inp[m]
        for sh, cols in shapes:
            px, py = int(rng.integers(0, H)), int(rng.integers(0, W))
            box = np.zeros(sh.max(0) + 1, np.int8)
            box[sh[:, 0] - sh[:, 0].min(), sh[:, 1] - sh[:, 1].min()] = cols
            box = box[:H - px, :W - py]
            ans[m, px:px + box.shape[0], py:py + box.shape[1]] = box
    return inp, ans


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stamp_bench.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--resources", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    K1 = H * W
    cell = torch.arange(K1, device=dev)
    px, py = (cell // W).reshape(1, 1, K1), (cell % W).reshape(1, 1, K1)
    one = torch.zeros((K1, 128), dtype=torch.uint8, device=dev)
    one[cell, cell >> 3] = (torch.ones((), dtype=torch.int64, device=dev) << (cell & 7)).to(torch.uint8)
    lines = [f"stampbench: {H}x{W} O2ARC, freshly reset rows with {C} objects each (two-colour shapes of 2-4 cells on a 4 x 4 lattice; the answer holds one copy of "
             f"each somewhere in the grid), no distance limit, row m judged by env m",
             f"command: python tools/stampbench.py --repeats {a.repeats} --rows {' '.join(str(r) for r in a.rows)}{' --resources FILE' if a.resources else ''}",
             f"us per call = median of {a.repeats} repeats [min .. max], each repeat >= 0.5 s of graph replays (3 warm replays), legs alternating; one library (ABI "
             f"{EnvBatch(1, H, W, 3, 'o2arc').L.arcle_abi_version()}) for both legs",
             f"(a) objects_rows(any_color, diagonal, bits) + stamp_rows; (b) objects_rows + expand_macros(dense) over {C} x {K1} CopyO + Paste macros of two steps per row "
             f"+ arg-max"]
    table = actions.table_descs(O2ARCv2Env.default_operations())
    for M in a.rows:
        inp, ans = tasks(M)
        dims = np.tile(np.array([[H, W]], np.int8), (M, 1))
        for blank in (1, 0):
            b = EnvBatch(M, H, W, 3, "o2arc")
            b.set_op_table(table if blank else [d & ~0xff00 if (d & 0xff) == 7 else d for d in table])  # (OP_PASTE = 7; arg byte = paste_blank)
            b.set_tasks_padded(inp, dims, ans, dims)
            b.reset()
            rows = b.get_state_rows().clone()
            src = torch.arange(M, dtype=torch.int32, device=dev)
            # ---- (a)
            objs_a = b.objects_rows(rows, C, 0, True, True, True)
            out_a = b.stamp_rows(rows, objs_a[0], objs_a[2], src, None, bool(blank))

            def leg_a():
                b.objects_rows(rows, C, 0, True, True, True, out=objs_a)
                b.stamp_rows(rows, objs_a[0], objs_a[2], src, None, bool(blank), out=out_a)
            # ---- (b): the macro set of every row, built once from the objects' boxes and bit rows
            objs_b = b.objects_rows(rows, C, 0, True, True, True)
            torch.cuda.synchronize(dev)
            assert int(objs_b[0][:, 0].min()) == C and int(objs_b[0][:, 1].max()) == 0, "every row holds exactly 16 objects"
            box = objs_b[1][:, :, 0:4].to(torch.int64)  # x0, y0, x1, y1
            dx, dy = px - box[:, :, 0:1], py - box[:, :, 1:2]
            prio = ((127 - dx.abs() - dy.abs()) << 13) + ((63 - dx) << 6) + (31 - dy)  # larger = preferred among equal counts
            op = torch.tensor([COPY_OP, PASTE_OP], dtype=torch.int32, device=dev).reshape(1, 1, 2).expand(M, C * K1, 2).contiguous()
            length = torch.full((M, C * K1), 2, dtype=torch.int32, device=dev)
            bits = torch.empty((M, C, K1, 2, 128), dtype=torch.uint8, device=dev)
            bits[:, :, :, 0] = objs_b[2].reshape(M, C, 1, 128)
            bits[:, :, :, 1] = one.reshape(1, 1, K1, 128)
            bits = bits.reshape(M, C * K1, 2, 128)
            ex = b.expand_macros(rows, "bits", bits, op, length, src, dense=True)
            best_b = torch.zeros((M, C), dtype=torch.int64, device=dev)
            corr_b = torch.zeros((M, C), dtype=torch.int64, device=dev)

            def leg_b():
                b.objects_rows(rows, C, 0, True, True, True, out=objs_b)
                b.expand_macros(rows, "bits", bits, op, length, src, dense=True, out=ex)
                key = torch.where(ex.status.reshape(M, C, K1) == 0, ex.dense[:, :, 0].to(torch.int64).reshape(M, C, K1) * (1 << 20) + prio,
                                  torch.full((), -1, dtype=torch.int64, device=dev))
                k = key.argmax(-1)
                best_b.copy_(k)
                corr_b.copy_(key.gather(-1, k.unsqueeze(-1)).squeeze(-1) >> 20)
            leg_a()
            leg_b()
            torch.cuda.synchronize(dev)
            bad_status = int((ex.status != 0).sum())
            same = bool(((best_b // W == out_a[0][:, :, 0]) & (best_b % W == out_a[0][:, :, 1]) & (corr_b == out_a[0][:, :, 2])).all())
            gain = int((out_a[0][:, :, 2] > out_a[1][:, 0:1]).sum())
            runs = [("(a) objects_rows + stamp_rows", timed_graph(dev, leg_a, 8)), ("(b) objects_rows + expand_macros + arg-max", timed_graph(dev, leg_b, 1))]
            times = {name: [] for name, _ in runs}
            for _ in range(a.repeats):
                for name, (run, _) in runs:
                    times[name].append(run())
            ta, tb = (np.array(times[name]) for name, _ in runs)
            lines.append(f"{M} rows, blank = {blank} ({M * C} objects, {M * C * K1} two-step macros, {bad_status} of them refused); {gain} objects gain by a stamp; both "
                         f"legs name the same position and count for every object: {same}")
            for name, t in zip(times, (ta, tb)):
                lines.append(f"  {name:<60} {np.median(t) * 1e6:10.2f} us  [{t.min() * 1e6:.2f} .. {t.max() * 1e6:.2f}]  spread {100 * (t.max() - t.min()) / np.median(t):.1f} %")
            lines.append(f"  (b) / (a) = {np.median(tb) / np.median(ta):.1f} x; (b) - (a) = {(np.median(tb) - np.median(ta)) * 1e6:.2f} us against (b)'s run-to-run spread of "
                         f"{(tb.max() - tb.min()) * 1e6:.2f} us: (a) is {'faster' if np.median(tb) - np.median(ta) > tb.max() - tb.min() else 'NOT faster'} by more than the spread")
            del b, bits, ex, runs, objs_a, objs_b, out_a, prio, op, length
            torch.cuda.empty_cache()
    if a.resources:
        lines += ["", "kernel resources (gfx950 compile of arcle_amd/csrc/arcle_hip.hip with -Rpass-analysis=kernel-resource-usage):"]
        lines += ["  " + ln.rstrip() for ln in open(a.resources) if ln.strip()]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
