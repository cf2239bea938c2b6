#!/usr/bin/env python3
"""Where does each object belong?  arcle_place_rows beside the only route the PARENT commit's library has: every translation of every
object as a Move macro through arcle_expand_macros with the dense pair, then an arg-max on the device.

Inputs: 1024 and 4096 freshly reset 30 x 30 O2ARC state rows with 16 objects each (one 2-4 cell two-colour shape in every cell of a
4 x 4 lattice) whose answer holds every object somewhere else, at most 4 + 4 cells away; max_dist = 8; row m is judged by env m.

  (a) objects_rows(any_color, diagonal, bits) + place_rows on this library: two launches
  (b) on the library at --baseline-lib (built at the parent commit, loaded with _lib.load): objects_rows as in (a), then the 145
      translations with |dx| + |dy| <= 8 of every object as macros of |dx| vertical and |dy| horizontal Moves — 16 x 145 macros of up to
      8 steps per row; a translation that would leave the grid, and (0, 0), is padding (operation -1) — through expand_macros(dense),
      and per object the arg-max of correct under the tie rule of arcle_place_rows (torch, in the same captured graph).  Building the
      macro set is not timed.

Graph-replayed legs alternating in one process, HIP events around >= 0.5 s of work per repeat.  Both legs must name the same
translation and count for every object that gains by moving; the tool says whether they do.

Usage: python tools/placebench.py --baseline-lib PATH [--out profiles/place_bench.txt] [--repeats 5] [--rows 1024 4096]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from expandbench import timed_graph  # noqa: E402
from expandbitsbench import other_library  # noqa: E402
from arcle_amd import actions  # noqa: E402
from arcle_amd.engine import EnvBatch  # noqa: E402
from arcle_amd.envs import O2ARCv2Env  # noqa: E402

H = W = 30
C, DIST, T = 16, 8, 8
MOVE_OPS = (20, 21, 22, 23)  # O2ARCv2Env's table: Move up, down, right, left
SHAPES = (((0, 0), (0, 1)), ((0, 0), (1, 1), (2, 2)), ((0, 0), (0, 1), (1, 0)), ((0, 1), (1, 0), (1, 1), (2, 1)), ((0, 0), (1, 0), (1, 1), (2, 2)))


def tasks(n, seed=17):
    """n (input, answer) pairs: 16 shapes, one per 7 x 7 lattice cell (a free border keeps them apart, also diagonally), each of two
    colours; the answer holds every shape moved by up to +-4 rows and columns, clipped to the grid."""
    rng = np.random.default_rng(seed)
    inp, ans = np.zeros((n, H, W), np.int8), np.zeros((n, H, W), np.int8)
    for m in range(n):
        for i in range(4):
            for j in range(4):
                sh = np.array(SHAPES[rng.integers(0, len(SHAPES))])
                x, y = 1 + 7 * i + int(rng.integers(0, 3)), 1 + 7 * j + int(rng.integers(0, 3))
                cols = rng.integers(1, 10, 2)[(np.arange(len(sh)) >= len(sh) // 2).astype(int)]
                xs, ys = x + sh[:, 0], y + sh[:, 1]
                inp[m, xs, ys] = cols
                dx = int(np.clip(rng.integers(-4, 5), -xs.min(), H - 1 - xs.max()))
                dy = int(np.clip(rng.integers(-4, 5), -ys.min(), W - 1 - ys.max()))
                ans[m, xs + dx, ys + dy] = cols
    return inp, ans


def diamond():
    """The 145 translations with |dx| + |dy| <= 8 -> (dxdy int64 [145, 2], op int32 [145, T] (-1 beyond the macro's length), length
    int32 [145], prio int64 [145]: larger = preferred among equal counts (nearer, then the smaller dx, then the smaller dy))."""
    up, down, right, left = MOVE_OPS
    pts = [(dx, dy) for dx in range(-DIST, DIST + 1) for dy in range(-DIST, DIST + 1) if abs(dx) + abs(dy) <= DIST]
    op = np.full((len(pts), T), -1, np.int32)
    for k, (dx, dy) in enumerate(pts):
        op[k, :abs(dx)] = up if dx < 0 else down
        op[k, abs(dx):abs(dx) + abs(dy)] = right if dy > 0 else left
    pts = np.array(pts, np.int64)
    dist = np.abs(pts).sum(1)
    prio = (63 - dist) * 4096 + (31 - pts[:, 0]) * 64 + (31 - pts[:, 1])
    return pts, op, np.maximum(dist, 1).astype(np.int32), prio


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "place_bench.txt"))
    ap.add_argument("--baseline-lib", required=True, help="libarcle_hip.so built at the parent commit")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="+", default=[1024, 4096])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    pts_np, op_np, len_np, prio_np = diamond()
    K1 = len(pts_np)
    pts, op1, len1, prio = (torch.as_tensor(x, device=dev) for x in (pts_np, op_np, len_np, prio_np))
    lines = [f"placebench: {H}x{W} O2ARC, freshly reset rows with {C} objects each (two-colour shapes of 2-4 cells on a 4 x 4 lattice; the answer holds each up to "
             f"4 + 4 cells away), max_dist = {DIST}, row m judged by env m",
             f"command: python tools/placebench.py --baseline-lib <libarcle_hip.so of the parent commit> --repeats {a.repeats} --rows {' '.join(str(r) for r in a.rows)}",
             f"us per call = median of {a.repeats} repeats [min .. max], each repeat >= 0.5 s of graph replays (3 warm replays), legs alternating",
             f"(a) objects_rows(any_color, diagonal, bits) + place_rows, this library; (b) objects_rows + expand_macros(dense) over {C} x {K1} Move macros of up to {T} steps "
             f"per row + arg-max, the parent commit's library"]
    for M in a.rows:
        inp, ans = tasks(M)
        dims = np.tile(np.array([[H, W]], np.int8), (M, 1))
        with other_library(a.baseline_lib) as Lb:
            old = EnvBatch(M, H, W, 3, "o2arc")
            abi_old = Lb.arcle_abi_version()
        new = EnvBatch(M, H, W, 3, "o2arc")
        assert old.L is not new.L
        for b in (old, new):
            b.set_op_table(actions.table_descs(O2ARCv2Env.default_operations()))
            b.set_tasks_padded(inp, dims, ans, dims)
            b.reset()
        rows = new.get_state_rows().clone()
        assert torch.equal(rows, old.get_state_rows())
        src = torch.arange(M, dtype=torch.int32, device=dev)
        # ---- (a)
        objs_a = new.objects_rows(rows, C, 0, True, True, True)
        out_a = new.place_rows(rows, objs_a[0], objs_a[2], src, DIST)

        def leg_a():
            new.objects_rows(rows, C, 0, True, True, True, out=objs_a)
            new.place_rows(rows, objs_a[0], objs_a[2], src, DIST, out=out_a)
        # ---- (b): the macro set of every row, built once from the objects' boxes and bit rows
        objs_b = old.objects_rows(rows, C, 0, True, True, True)
        torch.cuda.synchronize(dev)
        assert int(objs_b[0][:, 0].min()) == C and int(objs_b[0][:, 1].max()) == 0, "every row holds exactly 16 objects"
        box = objs_b[1][:, :, 0:4].to(torch.int64)  # x0, y0, x1, y1
        dx, dy = pts[:, 0].reshape(1, 1, K1), pts[:, 1].reshape(1, 1, K1)
        fits = (box[:, :, 0:1] + dx >= 0) & (box[:, :, 2:3] + dx <= H - 1) & (box[:, :, 1:2] + dy >= 0) & (box[:, :, 3:4] + dy <= W - 1) & ((dx != 0) | (dy != 0))
        op = torch.where(fits.reshape(M, C, K1, 1), op1.reshape(1, 1, K1, T), torch.full((), -1, dtype=torch.int32, device=dev)).reshape(M, C * K1, T).contiguous()
        length = torch.where(fits, len1.reshape(1, 1, K1), torch.ones((), dtype=torch.int32, device=dev)).reshape(M, C * K1).contiguous()
        bits = torch.zeros((M, C * K1, T, 128), dtype=torch.uint8, device=dev)
        bits[:, :, 0] = objs_b[2].reshape(M, C, 1, 128).expand(M, C, K1, 128).reshape(M, C * K1, 128)
        ex = old.expand_macros(rows, "bits", bits, op, length, src, dense=True)
        best_b = torch.zeros((M, C), dtype=torch.int64, device=dev)
        corr_b = torch.zeros((M, C), dtype=torch.int64, device=dev)

        def leg_b():
            old.objects_rows(rows, C, 0, True, True, True, out=objs_b)
            old.expand_macros(rows, "bits", bits, op, length, src, dense=True, out=ex)
            key = torch.where(ex.status == 0, ex.dense[:, :, 0].to(torch.int64) * (1 << 20) + prio.repeat(C).reshape(1, C * K1), torch.full((), -1, dtype=torch.int64, device=dev))
            k = key.reshape(M, C, K1).argmax(-1)
            best_b.copy_(k)
            corr_b.copy_(key.reshape(M, C, K1).gather(-1, k.unsqueeze(-1)).squeeze(-1) >> 20)
        leg_a()
        leg_b()
        torch.cuda.synchronize(dev)
        gain = out_a[0][:, :, 2] > out_a[0][:, :, 3]
        same = bool(((pts[best_b][:, :, 0] == out_a[0][:, :, 0]) & (pts[best_b][:, :, 1] == out_a[0][:, :, 1]) & (corr_b == out_a[0][:, :, 2]))[gain].all())
        runs = [("(a) objects_rows + place_rows", timed_graph(dev, leg_a, 8)), ("(b) objects_rows + expand_macros + arg-max, parent library", timed_graph(dev, leg_b, 1))]
        times = {name: [] for name, _ in runs}
        for _ in range(a.repeats):
            for name, (run, _) in runs:
                times[name].append(run())
        ta, tb = (np.array(times[name]) for name, _ in runs)
        lines.append(f"{M} rows ({M * C} objects, {M * C * K1} macro slots, {int(fits.sum())} of them Move macros; parent library ABI {abi_old}, this library ABI "
                     f"{new.L.arcle_abi_version()}); {int(gain.sum())} objects gain by moving, both legs name the same translation and count for them: {same}")
        for name, t in zip(times, (ta, tb)):
            lines.append(f"  {name:<60} {np.median(t) * 1e6:10.2f} us  [{t.min() * 1e6:.2f} .. {t.max() * 1e6:.2f}]  spread {100 * (t.max() - t.min()) / np.median(t):.1f} %")
        lines.append(f"  (b) / (a) = {np.median(tb) / np.median(ta):.1f} x; (b) - (a) = {(np.median(tb) - np.median(ta)) * 1e6:.2f} us against (b)'s run-to-run spread of "
                     f"{(tb.max() - tb.min()) * 1e6:.2f} us: (a) is {'faster' if np.median(tb) - np.median(ta) > tb.max() - tb.min() else 'NOT faster'} by more than the spread")
        del old, new, bits, ex
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
