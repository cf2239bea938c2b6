#!/usr/bin/env python3
"""Where does each object belong once it is rotated or mirrored?  arcle_turn_rows beside the route the library had before it: every
(turn, dx, dy) of every object as a macro — the turn's op on the object's cells, then |dx| + |dy| Moves — through arcle_expand_macros
with the dense pair, then an arg-max per turn on the device.

Inputs: 1024 and 4096 freshly reset 30 x 30 O2ARC state rows with 16 objects each (one 2-4 cell two-colour shape in every cell of a
4 x 4 lattice) whose answer holds every object turned (a random one of the five turns) and moved up to 4 cells from where the turn
leaves it; max_dist = 8; row m is judged by env m.  The op table is O2ARCv2Env's with gen_rotate(2) appended.

  (a) objects_rows(any_color, diagonal, bits) + turn_rows with all five turns: two launches
  (b) the same library: objects_rows as in (a), then ALL 5 x 145 (turn, dx, dy) with |dx| + |dy| <= 8 for every object as macros of
      1 + |dx| + |dy| <= 9 steps — 16 x 725 macros per row — through expand_macros(dense), and per object and turn the arg-max of
      correct under the tie rule of arcle_turn_rows over the candidates that keep the turned tile inside the grid (torch, in the same
      captured graph; arcle_expand_macros takes fewer than 2^28 steps per call, so 4096 rows go through it in two calls).  Building the
      macro set is not timed.
  also timed: turn_rows alone (all five turns, and Rotate 90 alone), for the comparison with place_rows in profiles/place_bench.txt,
  and the flat board: objects_rows + turn_rows on 1024 rows of 16 x 33.

Graph-replayed legs alternating in one process, HIP events around >= 0.5 s of work per repeat (3 warm replays).  Both legs must name
the same (dx, dy, correct, valid) for EVERY object and turn; the tool says whether they do.

Usage: python tools/turnbench.py [--out profiles/turn_bench.txt] [--repeats 5] [--rows 1024 4096] [--resources FILE]
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

C = 16
D = 8
MOVE_OPS = (20, 21, 22, 23)          # O2ARCv2Env's table: Move up, down, right, left
TURN_OPS = (24, 35, 25, 26, 27)      # Rotate 90, (appended) Rotate 180, Rotate 270, Flip H, Flip V


def turned(box, t):
    return (np.rot90(box, 1), np.rot90(box, 2), np.rot90(box, 3), box[:, ::-1], box[::-1])[t]


def tasks(n, H, W, seed=29):
    """n (input, answer) pairs: up to 16 shapes, one per 7 x 7 lattice cell that fits (a free border keeps them apart, also diagonally),
    each of two colours; the answer holds every shape turned by a random turn and moved up to 4 cells from where the turn leaves it
    (kept inside the grid; later shapes may cover earlier ones)."""
    rng = np.random.default_rng(seed)
    inp = np.zeros((n, H, W), np.int8)
    ans = np.zeros((n, H, W), np.int8)
    for m in range(n):
        for i in range((H - 2) // 7):
            for j in range((W - 2) // 7):
                sh = np.array(SHAPES[rng.integers(0, len(SHAPES))])
                sh = sh - sh.min(0)
                x, y = 1 + 7 * i + int(rng.integers(0, 3)), 1 + 7 * j + int(rng.integers(0, 3))
                cols = rng.integers(1, 10, 2)[(np.arange(len(sh)) >= len(sh) // 2).astype(int)]
                inp[m, x + sh[:, 0], y + sh[:, 1]] = cols
                h, w = (int(v) for v in sh.max(0) + 1)
                box = np.zeros((h, w), np.int8)
                box[sh[:, 0], sh[:, 1]] = cols
                t = int(rng.integers(0, 5))
                tile = turned(box, t)
                nx, ny = ((2 * x + h - w) // 2, (2 * y + w - h) // 2) if t in (0, 2) else (x, y)
                a = int(rng.integers(-4, 5))
                b_ = int(rng.integers(-(4 - abs(a)), 4 - abs(a) + 1))
                px, py = min(max(nx + a, 0), H - tile.shape[0]), min(max(ny + b_, 0), W - tile.shape[1])
                dst = ans[m, px:px + tile.shape[0], py:py + tile.shape[1]]
                dst[...] = np.where(tile > 0, tile, dst)
    return inp, ans


def report(times):
    out = []
    for name, t in times.items():
        t = np.array(t)
        out.append(f"  {name:<60} {np.median(t) * 1e6:10.2f} us  [{t.min() * 1e6:.2f} .. {t.max() * 1e6:.2f}]  spread {100 * (t.max() - t.min()) / np.median(t):.1f} %")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "turn_bench.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--resources", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H = W = 30
    cand = [(dx, dy) for dx in range(-D, D + 1) for dy in range(-D, D + 1) if abs(dx) + abs(dy) <= D]
    K1, T = len(cand), 1 + D
    K = 5 * K1
    up, down, right, left = MOVE_OPS
    op1 = np.full((5, K1, T), -1, np.int32)
    for t in range(5):
        for j, (dx, dy) in enumerate(cand):
            op1[t, j, 0] = TURN_OPS[t]
            op1[t, j, 1:1 + abs(dx)] = up if dx < 0 else down
            op1[t, j, 1 + abs(dx):1 + abs(dx) + abs(dy)] = right if dy > 0 else left
    len1 = np.array([1 + abs(dx) + abs(dy) for dx, dy in cand], np.int32)
    cdx = torch.tensor([c[0] for c in cand], dtype=torch.int64, device=dev).reshape(1, 1, 1, K1)
    cdy = torch.tensor([c[1] for c in cand], dtype=torch.int64, device=dev).reshape(1, 1, 1, K1)
    prio = ((127 - cdx.abs() - cdy.abs()) << 13) + ((63 - cdx) << 6) + (31 - cdy)  # larger = preferred among equal counts
    table = actions.table_descs(O2ARCv2Env.default_operations() + [actions.gen_rotate(2)])
    lines = [f"turnbench: {H}x{W} O2ARC (the table with gen_rotate(2) appended), freshly reset rows with {C} objects each (two-colour shapes of 2-4 cells on a 4 x 4 "
             f"lattice; the answer holds each turned and moved up to 4 cells), max_dist = {D}, row m judged by env m",
             f"command: python tools/turnbench.py --repeats {a.repeats} --rows {' '.join(str(r) for r in a.rows)}{' --resources FILE' if a.resources else ''}",
             f"us per call = median of {a.repeats} repeats [min .. max], each repeat >= 0.5 s of graph replays (3 warm replays), legs alternating; one library (ABI "
             f"{EnvBatch(1, H, W, 3, 'o2arc').L.arcle_abi_version()}) for both legs",
             f"(a) objects_rows(any_color, diagonal, bits) + turn_rows(all five turns); (b) objects_rows + expand_macros(dense) over {C} x 5 x {K1} macros of up to {T} steps "
             f"per row + arg-max per turn"]

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
        out_a = b.turn_rows(rows, objs_a[0], objs_a[2], src, D, 31)
        out_1 = b.turn_rows(rows, objs_a[0], objs_a[2], src, D, 1)

        def leg_a():
            b.objects_rows(rows, C, 0, True, True, True, out=objs_a)
            b.turn_rows(rows, objs_a[0], objs_a[2], src, D, 31, out=out_a)

        def leg_turn():
            b.turn_rows(rows, objs_a[0], objs_a[2], src, D, 31, out=out_a)

        def leg_one():
            b.turn_rows(rows, objs_a[0], objs_a[2], src, D, 1, out=out_1)
        # ---- (b): the macro set of every row, built once from the objects' boxes and bit rows
        objs_b = b.objects_rows(rows, C, 0, True, True, True)
        torch.cuda.synchronize(dev)
        assert int(objs_b[0][:, 0].min()) == C and int(objs_b[0][:, 1].max()) == 0, "every row holds exactly 16 objects"
        box = objs_b[1][:, :, 0:4].to(torch.int64)  # x0, y0, x1, y1
        x0, y0 = box[:, :, 0].reshape(M, C, 1, 1), box[:, :, 1].reshape(M, C, 1, 1)
        h, w = box[:, :, 2].reshape(M, C, 1, 1) - x0 + 1, box[:, :, 3].reshape(M, C, 1, 1) - y0 + 1
        quarter = torch.tensor([True, False, True, False, False], device=dev).reshape(1, 1, 5, 1)
        th, tw = torch.where(quarter, w, h), torch.where(quarter, h, w)
        nx, ny = torch.where(quarter, (2 * x0 + h - w) >> 1, x0), torch.where(quarter, (2 * y0 + w - h) >> 1, y0)
        inside = (nx + cdx >= 0) & (nx + cdx + th <= H) & (ny + cdy >= 0) & (ny + cdy + tw <= W)  # [M, C, 5, K1]
        # (arcle_expand_macros takes n_rows * n_actions * max_len < 2^28 steps per call: the rows go through it in equal chunks, all in leg (b)'s graph)
        nchunk = 1
        while (M // nchunk) * C * K * T >= 1 << 28 or M % nchunk:
            nchunk += 1
        Mc = M // nchunk
        op = torch.as_tensor(op1, device=dev).reshape(1, 1, K, T).expand(Mc, C, K, T).reshape(Mc, C * K, T).contiguous()
        length = torch.as_tensor(np.tile(len1, 5), device=dev).reshape(1, 1, K).expand(Mc, C, K).reshape(Mc, C * K).contiguous()
        bits, ex = [], []
        for i in range(nchunk):
            bt = torch.zeros((Mc, C, K, T, 128), dtype=torch.uint8, device=dev)
            bt[:, :, :, 0] = objs_b[2][i * Mc:(i + 1) * Mc].reshape(Mc, C, 1, 128)
            bits.append(bt.reshape(Mc, C * K, T, 128))
            ex.append(b.expand_macros(rows[i * Mc:(i + 1) * Mc], "bits", bits[i], op, length, src[i * Mc:(i + 1) * Mc], dense=True))
        res_b = torch.zeros((M, C, 5, 4), dtype=torch.int64, device=dev)

        def leg_b():
            b.objects_rows(rows, C, 0, True, True, True, out=objs_b)
            for i in range(nchunk):
                b.expand_macros(rows[i * Mc:(i + 1) * Mc], "bits", bits[i], op, length, src[i * Mc:(i + 1) * Mc], dense=True, out=ex[i])
            status = torch.cat([e.status for e in ex]).reshape(M, C, 5, K1)
            dense0 = torch.cat([e.dense[:, :, 0] for e in ex]).to(torch.int64).reshape(M, C, 5, K1)
            key = torch.where(inside & (status == 0), dense0 * (1 << 20) + prio, torch.full((), -1, dtype=torch.int64, device=dev))
            k = key.argmax(-1, keepdim=True)
            best = key.gather(-1, k).squeeze(-1)
            any_ok = best >= 0
            res_b[..., 0] = torch.where(any_ok, cdx.expand(M, C, 5, K1).gather(-1, k).squeeze(-1), 0)
            res_b[..., 1] = torch.where(any_ok, cdy.expand(M, C, 5, K1).gather(-1, k).squeeze(-1), 0)
            res_b[..., 2] = torch.where(any_ok, best >> 20, 0)
            res_b[..., 3] = any_ok.to(torch.int64)
        leg_a()
        leg_b()
        torch.cuda.synchronize(dev)
        bad_status = sum(int((e.status != 0).sum()) for e in ex)
        same = bool((res_b == out_a[0].to(torch.int64)).all())
        best_turn = (out_a[0][..., 2] * out_a[0][..., 3]).max(-1).values
        gain = int((best_turn > out_a[1][:, 0:1]).sum())
        runs = [("(a) objects_rows + turn_rows", timed_graph(dev, leg_a, 8)), ("(b) objects_rows + expand_macros + arg-max", timed_graph(dev, leg_b, 1)),
                ("turn_rows alone, all five turns", timed_graph(dev, leg_turn, 8)), ("turn_rows alone, Rotate 90 only", timed_graph(dev, leg_one, 8))]
        times = {name: [] for name, _ in runs}
        for _ in range(a.repeats):
            for name, (run, _) in runs:
                times[name].append(run())
        ta, tb = (np.array(times[name]) for name, _ in runs[:2])
        lines.append(f"{M} rows ({M * C} objects, {M * C * K} macros of up to {T} steps in {nchunk} expand_macros call(s), {bad_status} of them refused; {int((~inside).sum())} leave the grid and are not "
                     f"candidates); {gain} objects gain by a turn; both legs name the same (dx, dy, correct, valid) for every object and turn: {same}")
        lines += report(times)
        lines.append(f"  (b) / (a) = {np.median(tb) / np.median(ta):.1f} x; (b) - (a) = {(np.median(tb) - np.median(ta)) * 1e6:.2f} us against (b)'s run-to-run spread of "
                     f"{(tb.max() - tb.min()) * 1e6:.2f} us: (a) is {'faster' if np.median(tb) - np.median(ta) > tb.max() - tb.min() else 'NOT faster'} by more than the spread")
        flush()
        del b, bits, ex, runs, objs_a, objs_b, out_a, out_1, op, length, inside, res_b
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
    out_f = b.turn_rows(rows, objs_f[0], objs_f[2], src, D, 31)
    torch.cuda.synchronize(dev)
    nobj = int(objs_f[0][:, 0].sum())

    def leg_f():
        b.objects_rows(rows, C, 0, True, True, True, out=objs_f)
        b.turn_rows(rows, objs_f[0], objs_f[2], src, D, 31, out=out_f)

    def leg_ft():
        b.turn_rows(rows, objs_f[0], objs_f[2], src, D, 31, out=out_f)
    runs = [("(a) objects_rows + turn_rows", timed_graph(dev, leg_f, 4)), ("turn_rows alone, all five turns", timed_graph(dev, leg_ft, 4))]
    times = {name: [] for name, _ in runs}
    for _ in range(a.repeats):
        for name, (run, _) in runs:
            times[name].append(run())
    lines.append(f"flat board: {M} rows of {FH}x{FW} ({nobj} objects, {nobj / M:.1f} per row: the lattice cells that fit), max_dist = {D}, all five turns (answers: the device tests)")
    lines += report(times)
    if a.resources:
        lines += ["", "kernel resources (code-object notes of the gfx950 build of arcle_amd/csrc/arcle_hip.hip):"]
        lines += ["  " + ln.rstrip() for ln in open(a.resources) if ln.strip()]
    flush()
    print("\n".join(lines))


if __name__ == "__main__":
    main()
