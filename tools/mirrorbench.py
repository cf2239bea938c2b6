#!/usr/bin/env python3
"""What belongs in each object's box by symmetry?  arcle_mirror_rows beside the only route the library had before it: every (slot, source
rectangle) of every object as a macro — CopyO on the rectangle, Paste at the box's corner, the Flip(s) of the box — through
arcle_expand_macros with the dense pair, then an arg-max per slot on the device.

Inputs: 1024 and 4096 freshly reset 30 x 30 O2ARC state rows with 16 objects each (one filled 3 x 3 block of random colours in every
cell of a 4 x 4 lattice) whose answer holds, in every block's place, the mirror image of another block: under a random slot — left-right
(a block of the same lattice row), up-down (of the same lattice column) or the point reflection (any block).  No distance limit; row m is
judged by env m.  O2ARCv2Env's op table.

  (a) objects_rows(any_color, diagonal, bits) + mirror_rows with all three slots: two launches
  (b) the same library: objects_rows as in (a), then ALL 28 + 28 + 784 source rectangles of every object (slot H: the 28 columns, slot V:
      the 28 rows, slot point: all 28 x 28 corners) as macros of 3 (H, V) or 4 (point) steps — 16 x 840 macros per row — through
      expand_macros(dense), and per object and slot the arg-max of correct under the tie rule of arcle_mirror_rows (torch, in the same
      captured graph).  Building the macro set is not timed.
  also timed: mirror_rows alone (all three slots, and the point slot alone), and the flat board: objects_rows + mirror_rows on 1024 rows
  of 16 x 33.

Graph-replayed legs alternating in one process, HIP events around >= 0.5 s of work per repeat (3 warm replays).  Both legs must name
the same (dx, dy, correct, valid) for EVERY object and slot; the tool says whether they do.

Usage: python tools/mirrorbench.py [--out profiles/mirror_bench.txt] [--repeats 5] [--rows 1024 4096] [--resources FILE]
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
from arcle_amd import actions  # noqa: E402
from arcle_amd import search as S  # noqa: E402
from arcle_amd.engine import EnvBatch  # noqa: E402
from arcle_amd.envs import O2ARCv2Env  # noqa: E402

C = 16
BOX = 3
COPY_OP, PASTE_OP, FLIP_H, FLIP_V = 29, 30, 26, 27  # O2ARCv2Env's table


def flipped(box, s):
    return (box[:, ::-1], box[::-1], box[::-1, ::-1])[s]


def tasks(n, H, W, seed=31):
    """n (input, answer) pairs: a filled 3 x 3 block of random colours at (2 + 7 i, 2 + 7 j) for every lattice cell that fits; the answer
    holds in every block's place the mirror image of a partner block under a random slot (H: a block of the same lattice row, V: of
    the same lattice column, point: any)."""
    rng = np.random.default_rng(seed)
    ni, nj = (H - 2) // 7, (W - 2) // 7
    inp = np.zeros((n, H, W), np.int8)
    ans = np.zeros((n, H, W), np.int8)
    for m in range(n):
        blocks = rng.integers(1, 10, (ni, nj, BOX, BOX))
        for i in range(ni):
            for j in range(nj):
                inp[m, 2 + 7 * i:5 + 7 * i, 2 + 7 * j:5 + 7 * j] = blocks[i, j]
                s = int(rng.integers(0, 3))
                pi, pj = (i if s == 0 else int(rng.integers(0, ni))), (j if s == 1 else int(rng.integers(0, nj)))
                ans[m, 2 + 7 * i:5 + 7 * i, 2 + 7 * j:5 + 7 * j] = flipped(blocks[pi, pj], s)
    return inp, ans


def report(times):
    out = []
    for name, t in times.items():
        t = np.array(t)
        out.append(f"  {name:<60} {np.median(t) * 1e6:10.2f} us  [{t.min() * 1e6:.2f} .. {t.max() * 1e6:.2f}]  spread {100 * (t.max() - t.min()) / np.median(t):.1f} %")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mirror_bench.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--resources", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H = W = 30
    n1 = H - BOX + 1  # corners per axis
    K1, T = 2 * n1 + n1 * n1, 4
    # candidate j of an object: (slot, sx, sy); -1 = the box's own coordinate
    slot = np.array([0] * n1 + [1] * n1 + [2] * (n1 * n1))
    csx = np.array([-1] * n1 + list(range(n1)) + [v for v in range(n1) for _ in range(n1)])
    csy = np.array(list(range(n1)) + [-1] * n1 + list(range(n1)) * n1)
    seg = ((0, n1), (n1, 2 * n1), (2 * n1, K1))
    op1 = np.full((K1, T), -1, np.int32)
    op1[:, 0], op1[:, 1], op1[:, 2] = COPY_OP, PASTE_OP, np.where(slot == 1, FLIP_V, FLIP_H)
    op1[slot == 2, 3] = FLIP_V
    len1 = np.where(slot == 2, 4, 3).astype(np.int32)
    table = actions.table_descs(O2ARCv2Env.default_operations())
    lines = [f"mirrorbench: {H}x{W} O2ARC, freshly reset rows with {C} objects each (filled 3 x 3 blocks of random colours on a 4 x 4 lattice; the answer holds in each "
             f"block's place the mirror image of a partner block under a random slot), no distance limit, blank = 1, row m judged by env m",
             f"command: python tools/mirrorbench.py --repeats {a.repeats} --rows {' '.join(str(r) for r in a.rows)}{' --resources FILE' if a.resources else ''}",
             f"us per call = median of {a.repeats} repeats [min .. max], each repeat >= 0.5 s of graph replays (3 warm replays), legs alternating; one library (ABI "
             f"{EnvBatch(1, H, W, 3, 'o2arc').L.arcle_abi_version()}) for both legs",
             f"(a) objects_rows(any_color, diagonal, bits) + mirror_rows(all three slots); (b) objects_rows + expand_macros(dense) over {C} x ({n1} + {n1} + {n1 * n1}) macros of "
             f"3 or 4 steps per row + arg-max per slot"]

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for M in a.rows:
        inp, ans = tasks(M, H, W)
        dims = np.tile(np.array([[H, W]], np.int8), (M, 1))
        b = EnvBatch(M, H, W, 3, "o2arc")
        b.set_op_table(table)
        b.set_tasks_padded(inp, dims, ans, dims)
        b.reset()
        rows = b.get_state_rows().clone()
        src = torch.arange(M, dtype=torch.int32, device=dev)
        # ---- (a)
        objs_a = b.objects_rows(rows, C, 0, True, True, True)
        out_a = b.mirror_rows(rows, objs_a[0], objs_a[2], src, None, 7)
        out_1 = b.mirror_rows(rows, objs_a[0], objs_a[2], src, None, 4)

        def leg_a():
            b.objects_rows(rows, C, 0, True, True, True, out=objs_a)
            b.mirror_rows(rows, objs_a[0], objs_a[2], src, None, 7, out=out_a)

        def leg_mirror():
            b.mirror_rows(rows, objs_a[0], objs_a[2], src, None, 7, out=out_a)

        def leg_point():
            b.mirror_rows(rows, objs_a[0], objs_a[2], src, None, 4, out=out_1)
        # ---- (b): the macro set of every row, built once from the objects' boxes
        objs_b = b.objects_rows(rows, C, 0, True, True, True)
        torch.cuda.synchronize(dev)
        assert int(objs_b[0][:, 0].min()) == C and int(objs_b[0][:, 1].max()) == 0, "every row holds exactly 16 objects"
        box = objs_b[1][:, :, 0:4].to(torch.int64)  # x0, y0, x1, y1
        assert bool(((box[..., 2] - box[..., 0] == BOX - 1) & (box[..., 3] - box[..., 1] == BOX - 1)).all())
        x0, y0 = box[:, :, 0].reshape(M, C, 1), box[:, :, 1].reshape(M, C, 1)
        tsx, tsy = torch.as_tensor(csx, device=dev).reshape(1, 1, K1), torch.as_tensor(csy, device=dev).reshape(1, 1, K1)
        sx, sy = torch.where(tsx < 0, x0, tsx), torch.where(tsy < 0, y0, tsy)  # [M, C, K1]
        cdx, cdy = sx - x0, sy - y0
        prio = ((127 - cdx.abs() - cdy.abs()) << 13) + ((63 - cdx) << 6) + (31 - cdy)  # larger = preferred among equal counts
        # (arcle_expand_macros takes n_rows * n_actions * max_len < 2^28 steps per call: the rows go through it in equal chunks, all in leg (b)'s graph)
        nchunk = 1
        while (M // nchunk) * C * K1 * T >= 1 << 28 or M % nchunk:
            nchunk += 1
        Mc = M // nchunk
        op = torch.as_tensor(op1, device=dev).reshape(1, 1, K1, T).expand(Mc, C, K1, T).reshape(Mc, C * K1, T).contiguous()
        length = torch.as_tensor(len1, device=dev).reshape(1, 1, K1).expand(Mc, C, K1).reshape(Mc, C * K1).contiguous()
        bits, ex = [], []
        for i in range(nchunk):
            bt = torch.zeros((Mc, C, K1, T, 128), dtype=torch.uint8, device=dev)
            for r0 in range(0, Mc, 64):  # (the rectangles' bit rows in slices: pack_bits goes through one byte per cell)
                sl = slice(i * Mc + r0, i * Mc + min(r0 + 64, Mc))
                bt[r0:r0 + 64, :, :, 0] = S._rect_bits(sx[sl], sx[sl] + BOX - 1, sy[sl], sy[sl] + BOX - 1, H, W)
            sl = slice(i * Mc, (i + 1) * Mc)
            bx = box[sl]
            bt[:, :, :, 1] = S._rect_bits(bx[..., 0], bx[..., 0], bx[..., 1], bx[..., 1], H, W).reshape(Mc, C, 1, 128)
            bt[:, :, :, 2] = S._rect_bits(bx[..., 0], bx[..., 2], bx[..., 1], bx[..., 3], H, W).reshape(Mc, C, 1, 128)
            bits.append(bt.reshape(Mc, C * K1, T, 128))
            ex.append(b.expand_macros(rows[sl], "bits", bits[i], op, length, src[sl], dense=True))
        res_b = torch.zeros((M, C, 3, 4), dtype=torch.int64, device=dev)

        def leg_b():
            b.objects_rows(rows, C, 0, True, True, True, out=objs_b)
            for i in range(nchunk):
                b.expand_macros(rows[i * Mc:(i + 1) * Mc], "bits", bits[i], op, length, src[i * Mc:(i + 1) * Mc], dense=True, out=ex[i])
            status = torch.cat([e.status for e in ex]).reshape(M, C, K1)
            dense0 = torch.cat([e.dense[:, :, 0] for e in ex]).to(torch.int64).reshape(M, C, K1)
            key = torch.where(status == 0, dense0 * (1 << 20) + prio, torch.full((), -1, dtype=torch.int64, device=dev))
            for s, (lo, hi) in enumerate(seg):
                k = key[..., lo:hi].argmax(-1, keepdim=True)
                best = key[..., lo:hi].gather(-1, k).squeeze(-1)
                any_ok = best >= 0
                res_b[:, :, s, 0] = torch.where(any_ok, cdx[..., lo:hi].gather(-1, k).squeeze(-1), 0)
                res_b[:, :, s, 1] = torch.where(any_ok, cdy[..., lo:hi].gather(-1, k).squeeze(-1), 0)
                res_b[:, :, s, 2] = torch.where(any_ok, best >> 20, 0)
                res_b[:, :, s, 3] = any_ok.to(torch.int64)
        leg_a()
        leg_b()
        torch.cuda.synchronize(dev)
        bad_status = sum(int((e.status != 0).sum()) for e in ex)
        same = bool((res_b == out_a[0].to(torch.int64)).all())
        best_slot = (out_a[0][..., 2] * out_a[0][..., 3]).max(-1).values
        gain = int((best_slot > out_a[1][:, 0:1]).sum())
        runs = [("(a) objects_rows + mirror_rows", timed_graph(dev, leg_a, 8)), ("(b) objects_rows + expand_macros + arg-max", timed_graph(dev, leg_b, 1)),
                ("mirror_rows alone, all three slots", timed_graph(dev, leg_mirror, 8)), ("mirror_rows alone, the point slot only", timed_graph(dev, leg_point, 8))]
        times = {name: [] for name, _ in runs}
        for _ in range(a.repeats):
            for name, (run, _) in runs:
                times[name].append(run())
        ta, tb = (np.array(times[name]) for name, _ in runs[:2])
        lines.append(f"{M} rows ({M * C} objects, {M * C * K1} macros of 3 or 4 steps in {nchunk} expand_macros call(s), {bad_status} of them refused); {gain} objects gain by a "
                     f"mirror image; both legs name the same (dx, dy, correct, valid) for every object and slot: {same}")
        lines += report(times)
        lines.append(f"  (b) / (a) = {np.median(tb) / np.median(ta):.1f} x; (b) - (a) = {(np.median(tb) - np.median(ta)) * 1e6:.2f} us against (b)'s run-to-run spread of "
                     f"{(tb.max() - tb.min()) * 1e6:.2f} us: (a) is {'faster' if np.median(tb) - np.median(ta) > tb.max() - tb.min() else 'NOT faster'} by more than the spread")
        flush()
        del b, bits, ex, runs, objs_a, objs_b, out_a, out_1, op, length, res_b, prio, cdx, cdy, sx, sy
        torch.cuda.empty_cache()
    # ---- the flat board: 16 x 33 (W > 32), leg (a) only
    FH, FW, M = 16, 33, 1024
    inp, ans = tasks(M, FH, FW)
    dims = np.tile(np.array([[FH, FW]], np.int8), (M, 1))
    b = EnvBatch(M, FH, FW, 3, "o2arc")
    b.set_op_table(table)
    b.set_tasks_padded(inp, dims, ans, dims)
    b.reset()
    rows = b.get_state_rows().clone()
    src = torch.arange(M, dtype=torch.int32, device=dev)
    objs_f = b.objects_rows(rows, C, 0, True, True, True)
    out_f = b.mirror_rows(rows, objs_f[0], objs_f[2], src, None, 7)
    torch.cuda.synchronize(dev)
    nobj = int(objs_f[0][:, 0].sum())

    def leg_f():
        b.objects_rows(rows, C, 0, True, True, True, out=objs_f)
        b.mirror_rows(rows, objs_f[0], objs_f[2], src, None, 7, out=out_f)

    def leg_fm():
        b.mirror_rows(rows, objs_f[0], objs_f[2], src, None, 7, out=out_f)
    runs = [("(a) objects_rows + mirror_rows", timed_graph(dev, leg_f, 4)), ("mirror_rows alone, all three slots", timed_graph(dev, leg_fm, 4))]
    times = {name: [] for name, _ in runs}
    for _ in range(a.repeats):
        for name, (run, _) in runs:
            times[name].append(run())
    lines.append(f"flat board: {M} rows of {FH}x{FW} ({nobj} objects, {nobj / M:.1f} per row: the lattice cells that fit), no distance limit, all three slots (answers: the device tests)")
    lines += report(times)
    if a.resources:
        lines += ["", "kernel resources (code-object notes of the gfx950 build of arcle_amd/csrc/arcle_hip.hip):"]
        lines += ["  " + ln.rstrip() for ln in open(a.resources) if ln.strip()]
    flush()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
