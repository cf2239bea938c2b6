#!/usr/bin/env python3
"""Which lines does each object cast?  arcle_ray_rows beside the only route the library had to the same answers: every candidate's
cells built on the HOST and uploaded as bit rows, one child per (object, set, colour) through arcle_expand_rows with the dense pair,
then an arg-max on the device.

Inputs: 1024 and 4096 freshly reset 30 x 30 O2ARC state rows with 16 objects each (one-cell seeds of random colours, one per cell of a
4 x 4 lattice, so every ray is stopped by the edge or by another seed) whose answer holds, for every seed, the rays of one randomly
drawn set of the 13 default sets; row m is judged by env m; the rows repeat 256 distinct tasks.

  (a) objects_rows(any_color, diagonal, bits) + ray_rows(13 default sets, free_color 0, best_bits): two launches
  (b) the same library: objects_rows as in (a), then the 13 masks of every object — built beforehand by ray_numpy and uploaded, NOT
      timed, which favours (b) — times the ten Colour ops, 16 x 13 x 10 children per row through expand_rows(dense), and per object the
      arg-max under the tie rules of arcle_ray_rows (torch, in the same captured graph)

Graph-replayed legs alternating in one process, HIP events around >= 0.5 s of work per repeat (3 warm replays).  Both legs must name the
same (set, colour, correct) for EVERY object: the tool asserts it before it times anything (and that no child of a non-empty candidate
was refused, and that the flat board's first row equals ray_numpy).  The flat board (1024 rows of 16 x 33, leg (a) only) is
timed once and reported as what it is: the slow path.

Usage: python tools/raybench.py [--out profiles/ray_bench.txt] [--repeats 5] [--rows 1024 4096] [--resources FILE]
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
from arcle_amd import actions, search  # noqa: E402
from arcle_amd.engine import EnvBatch  # noqa: E402
from arcle_amd.envs import O2ARCv2Env  # noqa: E402

C = 16
SETS = tuple(search.RAY_SETS)
NS = len(SETS)
DISTINCT = 256


def tasks(n, H, W, seed=29):
    """n (input, answer) pairs: 16 one-cell seeds, one per cell of a 4 x 4 lattice (jittered, never adjacent); the answer is the input
    with every seed's rays of one randomly drawn default set, in the seed's colour, drawn in seed order while the cells are free."""
    rng = np.random.default_rng(seed)
    inp = np.zeros((n, H, W), np.int8)
    ans = np.zeros((n, H, W), np.int8)
    sh, sw = H // 4, W // 4
    for m in range(n):
        seeds = []
        for i in range(4):
            for j in range(4):
                x, y = sh * i + int(rng.integers(0, sh - 1)), sw * j + int(rng.integers(0, sw - 1))
                inp[m, x, y] = int(rng.integers(1, 10))
                seeds.append((x, y))
        ans[m] = inp[m]
        for x, y in seeds:
            dirs = SETS[int(rng.integers(0, NS))]
            for d, (dx, dy) in enumerate(search.RAY_DIRS):
                if (dirs >> d) & 1:
                    a, b = x + dx, y + dy
                    while 0 <= a < H and 0 <= b < W and inp[m, a, b] == 0:
                        ans[m, a, b] = inp[m, x, y]
                        a, b = a + dx, b + dy
    return inp, ans


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_bench.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--resources", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H = W = 30
    table = actions.table_descs(O2ARCv2Env.default_operations())
    sets_t = torch.as_tensor(np.array(SETS, np.uint8), device=dev)
    lines = [f"raybench: {H}x{W} O2ARC, freshly reset rows with {C} objects each (one-cell seeds on a 4 x 4 lattice; the answer holds every seed's rays of one of the "
             f"{NS} default sets), free_color 0, through 0, row m judged by env m; the rows repeat {DISTINCT} distinct tasks",
             f"command: python tools/raybench.py --repeats {a.repeats} --rows {' '.join(str(r) for r in a.rows)}{' --resources FILE' if a.resources else ''}",
             f"us per call = median of {a.repeats} repeats [min .. max], each repeat >= 0.5 s of graph replays (3 warm replays), legs alternating; one library (ABI "
             f"{EnvBatch(1, H, W, 3, 'o2arc').L.arcle_abi_version()}) for both legs",
             f"(a) objects_rows(any_color, diagonal, bits) + ray_rows({NS} sets, best_bits); (b) objects_rows + expand_rows(dense) over {C} x {NS} x 10 Colour children per "
             f"row, masks built by ray_numpy on the host and uploaded beforehand (not timed) + arg-max"]
    inp0, ans0 = tasks(DISTINCT, H, W)
    for M in a.rows:
        pick = np.arange(M) % DISTINCT
        inp, ans = inp0[pick], ans0[pick]
        dims = np.tile(np.array([[H, W]], np.int8), (M, 1))
        b = EnvBatch(M, H, W, 3, "o2arc")
        b.set_op_table(table)
        b.set_tasks_padded(inp, dims, ans, dims)
        b.reset()
        rows = b.get_state_rows().clone()
        src = torch.arange(M, dtype=torch.int32, device=dev)
        # ---- (a)
        objs_a = b.objects_rows(rows, C, 0, True, True, True)
        out_a = b.ray_rows(rows, objs_a[0], objs_a[2], sets_t, 0, False, src, True)

        def leg_a():
            b.objects_rows(rows, C, 0, True, True, True, out=objs_a)
            b.ray_rows(rows, objs_a[0], objs_a[2], sets_t, 0, False, src, True, out=out_a)
        # ---- (b): every candidate's cells from the host mirror, for the objects in the device's order
        objs_b = b.objects_rows(rows, C, 0, True, True, True)
        torch.cuda.synchronize(dev)
        assert int(objs_b[0][:, 0].min()) == C and int(objs_b[0][:, 1].max()) == 0, "every row holds exactly 16 objects"
        obits = objs_b[2][:DISTINCT].cpu().numpy()
        omasks = np.unpackbits(obits, axis=-1, bitorder="little")[..., :H * W].reshape(-1, C, H, W)
        cand = np.zeros((min(M, DISTINCT), C, NS, 128), np.uint8)
        for m in range(cand.shape[0]):
            cells = search.ray_numpy(inp0[m], (H, W), ans0[m], (H, W), omasks[m], SETS, 0, False, full=True)[3]
            flat = np.zeros((C, NS, 1024), np.uint8)
            flat[..., :H * W] = cells.reshape(C, NS, H * W)
            cand[m] = np.packbits(flat, axis=-1, bitorder="little")
        cand_t = torch.as_tensor(cand, device=dev)[torch.as_tensor(pick % cand.shape[0], device=dev)]  # [M, C, NS, 128]
        ncell = torch.as_tensor(np.unpackbits(cand, axis=-1).sum(-1).astype(np.int64), device=dev)[torch.as_tensor(pick % cand.shape[0], device=dev)]  # [M, C, NS]
        pay = cand_t.reshape(M, C, NS, 1, 128).expand(M, C, NS, 10, 128).reshape(M, C * NS * 10, 128).contiguous()
        op = torch.arange(10, dtype=torch.int32, device=dev).reshape(1, 1, 10).expand(M, C * NS, 10).reshape(M, C * NS * 10).contiguous()
        del cand_t
        ex = b.expand_rows(rows, "bits", pay, op, src, dense=True)
        set_b = torch.zeros((M, C), dtype=torch.int64, device=dev)
        col_b = torch.zeros((M, C), dtype=torch.int64, device=dev)
        cor_b = torch.zeros((M, C), dtype=torch.int64, device=dev)
        sidx = torch.arange(NS, device=dev).reshape(1, 1, NS)
        cidx = torch.arange(10, device=dev).reshape(1, 1, 1, 10)

        def leg_b():
            b.objects_rows(rows, C, 0, True, True, True, out=objs_b)
            b.expand_rows(rows, "bits", pay, op, src, dense=True, out=ex)
            cor = ex.dense[:, :, 0].to(torch.int64).reshape(M, C, NS, 10)
            kc = (cor * 16 + (15 - cidx)).max(-1).values  # per set: the most correct, the smaller colour on a tie
            per_cor, per_col = kc >> 4, 15 - (kc & 15)
            key = torch.where(ncell > 0, (per_cor << 20) + ((1023 - ncell) << 4) + (15 - sidx), torch.full((), -1, dtype=torch.int64, device=dev))
            k = key.argmax(-1, keepdim=True)
            none = key.gather(-1, k).squeeze(-1) < 0
            set_b.copy_(torch.where(none, torch.full((), -1, dtype=torch.int64, device=dev), k.squeeze(-1)))
            col_b.copy_(torch.where(none, torch.zeros((), dtype=torch.int64, device=dev), per_col.gather(-1, k).squeeze(-1)))
            cor_b.copy_(per_cor.gather(-1, k).squeeze(-1))
        leg_a()
        leg_b()
        torch.cuda.synchronize(dev)
        best = out_a[1].to(torch.int64)
        live = (ncell > 0).reshape(M, C * NS, 1).expand(M, C * NS, 10).reshape(M, -1)
        bad_status = int(((ex.status != 0) & live).sum())
        # (an object without a candidate: leg (b) has no child to read `correct` from; arcle_ray_rows reports the row's base correct)
        cor_w = torch.where(set_b >= 0, cor_b, out_a[3][:, 0:1].to(torch.int64).expand(M, C))
        same = bool(((best[..., 0] == set_b) & (best[..., 1] == col_b) & (best[..., 2] == cor_w)).all())
        assert bad_status == 0, f"{M} rows: {bad_status} children of non-empty candidates were refused by expand_rows"
        assert same, f"{M} rows: the two routes name different (set, colour, correct) for {int((~((best[..., 0] == set_b) & (best[..., 1] == col_b) & (best[..., 2] == cor_w))).sum())} objects"
        gain = int((best[..., 2] > out_a[3][:, 0:1]).sum())
        runs = [("(a) objects_rows + ray_rows", timed_graph(dev, leg_a, 8)), ("(b) objects_rows + expand_rows + arg-max", timed_graph(dev, leg_b, 1))]
        times = {name: [] for name, _ in runs}
        for _ in range(a.repeats):
            for name, (run, _) in runs:
                times[name].append(run())
        ta, tb = (np.array(times[name]) for name, _ in runs)
        lines.append(f"{M} rows ({M * C} objects, {M * C * NS * 10} children, {bad_status} of those with cells refused); {gain} objects gain by a ray step; both legs name the "
                     f"same (set, colour, correct) for every object: {same}")
        for name, t in zip(times, (ta, tb)):
            lines.append(f"  {name:<60} {np.median(t) * 1e6:10.2f} us  [{t.min() * 1e6:.2f} .. {t.max() * 1e6:.2f}]  spread {100 * (t.max() - t.min()) / np.median(t):.1f} %")
        lines.append(f"  (b) / (a) = {np.median(tb) / np.median(ta):.1f} x; (b) - (a) = {(np.median(tb) - np.median(ta)) * 1e6:.2f} us against (b)'s run-to-run spread of "
                     f"{(tb.max() - tb.min()) * 1e6:.2f} us: (a) is {'faster' if np.median(tb) - np.median(ta) > tb.max() - tb.min() else 'NOT faster'} by more than the spread")
        del b, pay, op, ex, runs, objs_a, objs_b, out_a
        torch.cuda.empty_cache()
    # ---- the flat board, leg (a) only
    H, W, M = 16, 33, 1024
    inp, ans = tasks(DISTINCT, H, W, seed=31)
    pick = np.arange(M) % DISTINCT
    dims = np.tile(np.array([[H, W]], np.int8), (M, 1))
    b = EnvBatch(M, H, W, 3, "o2arc")
    b.set_op_table(table)
    b.set_tasks_padded(inp[pick], dims, ans[pick], dims)
    b.reset()
    rows = b.get_state_rows().clone()
    src = torch.arange(M, dtype=torch.int32, device=dev)
    objs = b.objects_rows(rows, C, 0, True, True, True)
    out = b.ray_rows(rows, objs[0], objs[2], sets_t, 0, False, src, True)

    def leg_flat():
        b.objects_rows(rows, C, 0, True, True, True, out=objs)
        b.ray_rows(rows, objs[0], objs[2], sets_t, 0, False, src, True, out=out)
    leg_flat()
    torch.cuda.synchronize(dev)
    want = search.ray_numpy(inp[0], (H, W), ans[0], (H, W), np.unpackbits(objs[2][0].cpu().numpy(), axis=-1, bitorder="little")[:, :H * W].reshape(C, H, W), SETS)
    ok = bool(np.array_equal(out[0][0].cpu().numpy(), want[0]) and np.array_equal(out[1][0].cpu().numpy(), want[1]))
    assert ok, "flat board: arcle_ray_rows and ray_numpy differ on row 0"
    run, _ = timed_graph(dev, leg_flat, 4)
    t = np.array([run() for _ in range(a.repeats)])
    lines.append(f"flat board: {M} rows of {H} x {W}, {int(objs[0][:, 0].sum())} objects, (a) only; row 0 equals ray_numpy: {ok}")
    lines.append(f"  {'(a) objects_rows + ray_rows':<60} {np.median(t) * 1e6:10.2f} us  [{t.min() * 1e6:.2f} .. {t.max() * 1e6:.2f}]")
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
