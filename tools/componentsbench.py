#!/usr/bin/env python3
"""Labelling the objects of a search frontier: arcle_components_rows over the project's own states (30 x 30 O2ARC, the state rows of
8192 envs after 10 random steps), graph-replayed legs alternating in one process, HIP events around >= 0.5 s of work, three repeats.

  yardstick    a kernel the library already ships, timed in the same run: arcle_transition_rows IN PLACE with one FloodFill per row,
               seeded at each row's first cell, over the same 8192 rows — one closure per row, the whole step body, a plane stored
  components   rows and resident forms; C = 16 and 64; with and without bits; skip_color 0 and -1

and three worst-case batches (every row the same grid): one 900-cell component, the 1-wide spiral corridor of
tests/golden/flood_30.npz (two interleaved arms of ~450 cells: the closure with the most passes), and a checkerboard cut at C = 64.

Beside every time: the mean number of components written per row (n), and the expectation it is held against — a components launch
takes no longer than n yardstick launches (per component it runs the same closure, does less memory work and none of the step body).
Usage: python tools/componentsbench.py [--out profiles/components_bench.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from expandbench import timed_graph  # noqa: E402
from arcle_amd import search as S  # noqa: E402

FLOODFILL5 = 15  # O2ARCv2Env's table: FloodFill0-9 are ops 10-19


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_bench.txt"))
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = 8192
    batch = bench.make_batch(dev, n)
    bbox, op = bench.make_actions(10, n, 2000)
    sh = torch.cuda.current_stream(dev).cuda_stream
    for i in range(10):
        bb, oo = torch.as_tensor(bbox[i], device=dev), torch.as_tensor(op[i], device=dev)
        batch.step_bbox_ptr(bb.data_ptr(), oo.data_ptr(), 0, sh)
        torch.cuda.synchronize(dev)
    batch.status(True)
    L = batch.state_row_size()
    stride = (L + 15) & ~15
    P = 900
    goff = sum(ln for f, ln in S.row_layout("o2arc", P)[:[f for f, _ in S.row_layout("o2arc", P)].index("grid")])
    states = torch.zeros((n, stride), dtype=torch.int8, device=dev)
    states[:, :L] = batch.get_state_rows()
    src = torch.arange(n, dtype=torch.int32, device=dev)
    first = torch.zeros((n, 2), dtype=torch.int32, device=dev)
    fill = torch.full((n,), FLOODFILL5, dtype=torch.int32, device=dev)
    rw, tm = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    lines = [f"componentsbench: 30x30 O2ARC, {n} rows of {L} B (stride {stride}); us per launch = median of {a.repeats} repeats [min .. max], each "
             f">= 0.5 s of graph replays, legs alternating; n = mean components written per row; bound = n x the yardstick of the same batch"]

    def with_grid(g):
        """The states with every row's grid replaced by g (grid_dim 30 x 30)."""
        r = states.clone()
        r[:, goff:goff + P] = torch.as_tensor(g.reshape(-1), device=dev)
        r[:, goff + P:goff + P + 2] = 30
        return r

    spiral = np.load(os.path.join(ROOT, "tests", "golden", "flood_30.npz"))["input"][2].astype(np.int8)
    i, j = np.indices((30, 30))
    batches = [("states after 10 random steps", states, [(f, C, b, s) for f in ("rows", "resident") for C in (16, 64) for b in (False, True) for s in (0, -1)]),
               ("worst case: one 900-cell component", with_grid(np.full((30, 30), 3, np.int8)), [("rows", 16, False, -1), ("rows", 16, True, -1)]),
               ("worst case: spiral corridor (two 1-wide arms, 451 + 449 cells)", with_grid(spiral), [("rows", 16, False, -1), ("rows", 16, True, -1)]),
               ("worst case: checkerboard (900 components) cut at C = 64", with_grid((1 + (i + j) % 2).astype(np.int8)), [("rows", 64, False, -1), ("rows", 64, True, -1)])]
    for title, rows, legs_spec in batches:
        yard = rows.clone()  # (in place: the fill rewrites the yardstick's own copy)
        legs = [("yardstick: transition_rows in place, FloodFill at (0, 0)", None,
                 lambda yard=yard: batch.transition_rows(yard, "point", first, fill, src, out=yard, reward=rw, term=tm))]
        if any(f == "resident" for f, _, _, _ in legs_spec):
            batch.set_state_rows(rows)
        for form, C, bits, skip in legs_spec:
            r = rows if form == "rows" else None
            out = batch.components_rows(r, C, skip, bits)
            torch.cuda.synchronize(dev)
            nbar = float(out[0][:, 0].float().mean())
            left = float((out[0][:, 1] > 0).float().mean())
            legs.append((f"{form:<8} C={C:<3} skip={skip:<2} {'bits' if bits else '    '}", (nbar, left),
                         lambda r=r, C=C, skip=skip, bits=bits, out=out: batch.components_rows(r, C, skip, bits, out=out)))
        runs = [(name, info, timed_graph(dev, fn, 8)) for name, info, fn in legs]
        times = {name: [] for name, _, _ in legs}
        for _ in range(a.repeats):
            for name, _, (run, _) in runs:
                times[name].append(run())
        lines.append(title)
        ty = float(np.median(times[legs[0][0]]))
        for name, info, _ in legs:
            t = np.array(times[name])
            med = float(np.median(t))
            line = f"  {name:<58} {med * 1e6:9.2f} us  [{t.min() * 1e6:.2f} .. {t.max() * 1e6:.2f}]"
            if info:
                nbar, left = info
                bound = nbar * ty
                line += (f"   n = {nbar:6.2f} ({100 * left:.0f} % of the rows cut)   bound {bound * 1e6:9.2f} us: {med / bound:.3f} of it"
                         f"{'' if med <= bound else '   MISSES the expectation'}   {med / max(nbar, 1e-9) / n * 1e9:.2f} ns per component")
            lines.append(line)
        del runs
        torch.cuda.empty_cache()
    batch.status(True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
