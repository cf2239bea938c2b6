#!/usr/bin/env python3
"""Which cells around or inside each object should be painted?  arcle_region_rows beside the only route the library had to the same
answers: every candidate's cells built on the HOST and uploaded as bit rows, one child per (object, kind, colour) through
arcle_expand_rows with the dense pair, then an arg-max on the device.

Inputs: 1024 and 4096 freshly reset 30 x 30 O2ARC state rows with 16 objects each (a cell, a domino, an L, a T or a 3 x 3 ring of a random
colour, one per cell of a 4 x 4 lattice with a free cell around it) whose answer paints, for every object, the region of one randomly drawn
kind of the seven defaults; row m is judged by env m; the rows repeat 256 distinct tasks.

  (a) objects_rows(any_color, diagonal, bits) + region_rows(7 default kinds, free_color 0, best_bits): two launches
  (b) the same library: objects_rows as in (a), then the 7 masks of every object — built beforehand by region_numpy and uploaded, NOT
      timed, which favours (b) — times the ten Colour ops, 16 x 7 x 10 children per row through expand_rows(dense), and per object the
      arg-max under the tie rules of arcle_region_rows (torch, in the same captured graph)

Graph-replayed legs alternating in one process, HIP events around >= 0.5 s of work per repeat (3 warm replays).  Both legs must name the
same (kind, colour, correct) for EVERY object: the tool asserts it before it times anything (and that no child of a non-empty candidate
was refused, and that the flat board's first row equals region_numpy).  The flat board (1024 rows of 16 x 33, leg (a) only) is
timed once and reported as what it is: the slow path.

Usage: python tools/regionbench.py [--out profiles/region_bench.txt] [--repeats 5] [--rows 1024 4096] [--resources FILE]
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
KINDS = tuple(search.REGION_KINDS)
NS = len(KINDS)
DISTINCT = 256
SHAPES = (np.ones((1, 1), bool), np.ones((1, 2), bool), np.array([[1, 0], [1, 1]], bool), np.array([[1, 1, 1], [0, 1, 0]], bool),
          np.array([[1, 1, 1], [1, 0, 1], [1, 1, 1]], bool))


def tasks(n, H, W, seed=37):
    """n (input, answer) pairs: 16 objects, one shape of SHAPES per cell of a 4 x 4 lattice (jittered, a free cell all round inside its
    lattice cell, so no two are 8-connected); the answer is the input with, per object, the region of one randomly drawn default kind
    (region_numpy's cells, through = 0) painted in a random colour."""
    rng = np.random.default_rng(seed)
    inp = np.zeros((n, H, W), np.int8)
    ans = np.zeros((n, H, W), np.int8)
    sh, sw = H // 4, W // 4
    for m in range(n):
        masks = []
        for i in range(4):
            for j in range(4):
                shp = SHAPES[int(rng.integers(0, len(SHAPES)))]
                h, w = shp.shape
                x, y = sh * i + 1 + int(rng.integers(0, max(sh - h - 1, 1))), sw * j + 1 + int(rng.integers(0, max(sw - w - 1, 1)))
                full = np.zeros((H, W), bool)
                full[x:x + h, y:y + w] = shp
                inp[m][full] = int(rng.integers(1, 10))
                masks.append(full)
        ans[m] = inp[m]
        for k, full in enumerate(masks):
            cells = search.region_numpy(inp[m], (H, W), inp[m], (H, W), full[None], [KINDS[int(rng.integers(0, NS))]], 0, False, full=True)[3]
            ans[m][cells[0, 0]] = int(rng.integers(1, 10))
    return inp, ans


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_bench.txt"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--resources", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    H = W = 30
    table = actions.table_descs(O2ARCv2Env.default_operations())
    kinds_t = torch.as_tensor(np.array(KINDS, np.uint8), device=dev)
    lines = [f"regionbench: {H}x{W} O2ARC, freshly reset rows with {C} objects each (small shapes on a 4 x 4 lattice; the answer paints every object's region of one of the "
             f"{NS} default kinds), free_color 0, through 0, row m judged by env m; the rows repeat {DISTINCT} distinct tasks",
             f"command: python tools/regionbench.py --repeats {a.repeats} --rows {' '.join(str(r) for r in a.rows)}{' --resources FILE' if a.resources else ''}",
             f"us per call = median of {a.repeats} repeats [min .. max], each repeat >= 0.5 s of graph replays (3 warm replays), legs alternating; one library (ABI "
             f"{EnvBatch(1, H, W, 3, 'o2arc').L.arcle_abi_version()}) for both legs",
             f"(a) objects_rows(any_color, diagonal, bits) + region_rows({NS} kinds, best_bits); (b) objects_rows + expand_rows(dense) over {C} x {NS} x 10 Colour children per "
             f"row, masks built by region_numpy on the host and uploaded beforehand (not timed) + arg-max"]
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
        out_a = b.region_rows(rows, objs_a[0], objs_a[2], kinds_t, 0, False, src)

        def leg_a():
            b.objects_rows(rows, C, 0, True, True, True, out=objs_a)
            b.region_rows(rows, objs_a[0], objs_a[2], kinds_t, 0, False, src, out=out_a)
        # ---- (b): every candidate's cells from the host mirror, for the objects in the device's order
        objs_b = b.objects_rows(rows, C, 0, True, True, True)
        torch.cuda.synchronize(dev)
        assert int(objs_b[0][:, 0].min()) == C and int(objs_b[0][:, 1].max()) == 0, "every row holds exactly 16 objects"
        obits = objs_b[2][:DISTINCT].cpu().numpy()
        omasks = np.unpackbits(obits, axis=-1, bitorder="little")[..., :H * W].reshape(-1, C, H, W)
        cand = np.zeros((min(M, DISTINCT), C, NS, 128), np.uint8)
        for m in range(cand.shape[0]):
            cells = search.region_numpy(inp0[m], (H, W), ans0[m], (H, W), omasks[m], KINDS, 0, False, full=True)[3]
            flat = np.zeros((C, NS, 1024), np.uint8)
            flat[..., :H * W] = cells.reshape(C, NS, H * W)
            cand[m] = np.packbits(flat, axis=-1, bitorder="little")
        cand_t = torch.as_tensor(cand, device=dev)[torch.as_tensor(pick % cand.shape[0], device=dev)]  # [M, C, NS, 128]
        ncell = torch.as_tensor(np.unpackbits(cand, axis=-1).sum(-1).astype(np.int64), device=dev)[torch.as_tensor(pick % cand.shape[0], device=dev)]  # [M, C, NS]
        pay = cand_t.reshape(M, C, NS, 1, 128).expand(M, C, NS, 10, 128).reshape(M, C * NS * 10, 128).contiguous()
        op = torch.arange(10, dtype=torch.int32, device=dev).reshape(1, 1, 10).expand(M, C * NS, 10).reshape(M, C * NS * 10).contiguous()
        del cand_t
        ex = b.expand_rows(rows, "bits", pay, op, src, dense=True)
        kind_b = torch.zeros((M, C), dtype=torch.int64, device=dev)
        col_b = torch.zeros((M, C), dtype=torch.int64, device=dev)
        cor_b = torch.zeros((M, C), dtype=torch.int64, device=dev)
        sidx = torch.arange(NS, device=dev).reshape(1, 1, NS)
        cidx = torch.arange(10, device=dev).reshape(1, 1, 1, 10)

        def leg_b():
            b.objects_rows(rows, C, 0, True, True, True, out=objs_b)
            b.expand_rows(rows, "bits", pay, op, src, dense=True, out=ex)
            cor = ex.dense[:, :, 0].to(torch.int64).reshape(M, C, NS, 10)
            kc = (cor * 16 + (15 - cidx)).max(-1).values  # per kind: the most correct, the smaller colour on a tie
            per_cor, per_col = kc >> 4, 15 - (kc & 15)
            key = torch.where(ncell > 0, (per_cor << 20) + ((1023 - ncell) << 4) + (15 - sidx), torch.full((), -1, dtype=torch.int64, device=dev))
            k = key.argmax(-1, keepdim=True)
            none = key.gather(-1, k).squeeze(-1) < 0
            kind_b.copy_(torch.where(none, torch.full((), -1, dtype=torch.int64, device=dev), k.squeeze(-1)))
            col_b.copy_(torch.where(none, torch.zeros((), dtype=torch.int64, device=dev), per_col.gather(-1, k).squeeze(-1)))
            cor_b.copy_(per_cor.gather(-1, k).squeeze(-1))
        leg_a()
        leg_b()
        torch.cuda.synchronize(dev)
        best = out_a[1].to(torch.int64)
        live = (ncell > 0).reshape(M, C * NS, 1).expand(M, C * NS, 10).reshape(M, -1)
        bad_status = int(((ex.status != 0) & live).sum())
        # (an object without a candidate: leg (b) has no child to read `correct` from; arcle_region_rows reports the row's base correct)
        cor_w = torch.where(kind_b >= 0, cor_b, out_a[3][:, 0:1].to(torch.int64).expand(M, C))
        same = bool(((best[..., 0] == kind_b) & (best[..., 1] == col_b) & (best[..., 2] == cor_w)).all())
        assert bad_status == 0, f"{M} rows: {bad_status} children of non-empty candidates were refused by expand_rows"
        assert same, f"{M} rows: the two routes name different (kind, colour, correct) for {int((~((best[..., 0] == kind_b) & (best[..., 1] == col_b) & (best[..., 2] == cor_w))).sum())} objects"
        gain = int((best[..., 2] > out_a[3][:, 0:1]).sum())
        runs = [("(a) objects_rows + region_rows", timed_graph(dev, leg_a, 8)), ("(b) objects_rows + expand_rows + arg-max", timed_graph(dev, leg_b, 1))]
        times = {name: [] for name, _ in runs}
        for _ in range(a.repeats):
            for name, (run, _) in runs:
                times[name].append(run())
        ta, tb = (np.array(times[name]) for name, _ in runs)
        lines.append(f"{M} rows ({M * C} objects, {M * C * NS * 10} children, {bad_status} of those with cells refused); {gain} objects gain by a region step; both legs name the "
                     f"same (kind, colour, correct) for every object: {same}")
        for name, t in zip(times, (ta, tb)):
            lines.append(f"  {name:<60} {np.median(t) * 1e6:10.2f} us  [{t.min() * 1e6:.2f} .. {t.max() * 1e6:.2f}]  spread {100 * (t.max() - t.min()) / np.median(t):.1f} %")
        lines.append(f"  (b) / (a) = {np.median(tb) / np.median(ta):.1f} x; (b) - (a) = {(np.median(tb) - np.median(ta)) * 1e6:.2f} us against (b)'s run-to-run spread of "
                     f"{(tb.max() - tb.min()) * 1e6:.2f} us: (a) is {'faster' if np.median(tb) - np.median(ta) > tb.max() - tb.min() else 'NOT faster'} by more than the spread")
        del b, pay, op, ex, runs, objs_a, objs_b, out_a
        torch.cuda.empty_cache()
    # ---- the flat board, leg (a) only
    H, W, M = 16, 33, 1024
    inp, ans = tasks(DISTINCT, H, W, seed=41)
    pick = np.arange(M) % DISTINCT
    dims = np.tile(np.array([[H, W]], np.int8), (M, 1))
    b = EnvBatch(M, H, W, 3, "o2arc")
    b.set_op_table(table)
    b.set_tasks_padded(inp[pick], dims, ans[pick], dims)
    b.reset()
    rows = b.get_state_rows().clone()
    src = torch.arange(M, dtype=torch.int32, device=dev)
    objs = b.objects_rows(rows, C, 0, True, True, True)
    out = b.region_rows(rows, objs[0], objs[2], kinds_t, 0, False, src)

    def leg_flat():
        b.objects_rows(rows, C, 0, True, True, True, out=objs)
        b.region_rows(rows, objs[0], objs[2], kinds_t, 0, False, src, out=out)
    leg_flat()
    torch.cuda.synchronize(dev)
    want = search.region_numpy(inp[0], (H, W), ans[0], (H, W), np.unpackbits(objs[2][0].cpu().numpy(), axis=-1, bitorder="little")[:, :H * W].reshape(C, H, W), KINDS)
    ok = bool(np.array_equal(out[0][0].cpu().numpy(), want[0]) and np.array_equal(out[1][0].cpu().numpy(), want[1]))
    assert ok, "flat board: arcle_region_rows and region_numpy differ on row 0"
    run, _ = timed_graph(dev, leg_flat, 4)
    t = np.array([run() for _ in range(a.repeats)])
    lines.append(f"flat board: {M} rows of {H} x {W}, {int(objs[0][:, 0].sum())} objects, (a) only; row 0 equals region_numpy: {ok}")
    lines.append(f"  {'(a) objects_rows + region_rows':<60} {np.median(t) * 1e6:10.2f} us  [{t.min() * 1e6:.2f} .. {t.max() * 1e6:.2f}]")
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
