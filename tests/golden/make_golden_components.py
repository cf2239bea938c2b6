#!/usr/bin/env python3
"""Connected-component golden vectors: the reference's OWN `arcle.actions.color.dfs` (color.py:8-30; unmodified reference, imported
through oracle/stubs) called from every not-yet-covered cell of each grid in row-major order — the definition arcle_components_rows
and arcle_amd.search.components_numpy are pinned against.  Build-container only; the output tests/golden/components/components.npz (a folder
of its own: every .npz directly under tests/golden/ is replayed as a trace fixture by tests/backends.py) holds data alone:

    names            JSON list of the case names; case i has
    grid_i           int8 [H, W]      the grid plane (cells outside grid_dim included)
    dim_i            int8 [2]         grid_dim
    comp_i_s / label_i_s  for s in SKIPS (skip_color -1, 0, 3), written as m1 / 0 / 3:
                     int16 [n, 8]     x0, y0, x1, y1, sx, sy, colour, cells of every component, in order
                     int16 [H, W]     the index of the component each cell belongs to, -1 = none (the masks, compactly)

    python tests/golden/make_golden_components.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import refdriver as RD  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SKIPS = (-1, 0, 3)


def skip_tag(s):
    return "m1" if s < 0 else str(s)


def _rand(rng, H, W, ncol):
    return np.array([[rng.below(ncol) for _ in range(W)] for _ in range(H)], np.int8)


def _sparse(rng, H, W):
    """Non-zero cells (15 %) on background 0: small objects."""
    return np.array([[1 + rng.below(9) if rng.chance(15, 100) else 0 for _ in range(W)] for _ in range(H)], np.int8)


def _checker(H, W):
    i, j = np.indices((H, W))
    return (1 + (i + j) % 2).astype(np.int8)


def _wrap(H, W):
    """(i, W-1) and (i+1, 0) share a colour no neighbour of either has: two components, whatever a flat board's shifts say."""
    g = np.full((H, W), 1, np.int8)
    for i in range(0, H - 1, 3):
        g[i, W - 1] = 5
        g[i + 1, 0] = 5
    return g


def _diagonal(H, W):
    g = np.zeros((H, W), np.int8)
    for k in range(min(H, W) - 1):
        g[k, k] = 4          # a diagonal chain: every cell its own component
    g[H - 2:, :2] = 7
    g[H - 4:H - 2, 2:4] = 7  # two blocks touching at one corner only
    return g


def cases():
    """-> list of (name, grid int8 [H, W], grid_dim): the smallest shapes at which each code path of the kernel can go wrong."""
    rng = RD.SplitMix64(0xC0C0)
    out = []
    flood = np.load(os.path.join(OUT, "flood_30.npz"))
    H = W = 30
    contents = {"one": np.full((H, W), 3, np.int8), "checker": _checker(H, W), "rand3": _rand(rng, H, W, 3), "rand10": _rand(rng, H, W, 10),
                "sparse": _sparse(rng, H, W)}
    for dim in ((30, 30), (7, 9), (1, 1), (30, 1), (1, 30)):
        for name, g in contents.items():
            out.append((f"30x30 {name} dim {dim[0]}x{dim[1]}", g, dim))
    out.append(("30x30 spiral", flood["input"][2].astype(np.int8), (30, 30)))
    out.append(("30x30 diagonal", _diagonal(30, 30), (30, 30)))
    out.append(("30x30 wrap", _wrap(30, 30), (30, 30)))
    g = _rand(rng, 30, 30, 2)   # cells outside grid_dim carrying the colour of their inside neighbours: they join nothing
    g[:, 9:12] = g[:, 8:9]
    g[7:10, :] = g[6:7, :]
    out.append(("30x30 outside dim 7x9", g, (7, 9)))
    for H, W, dims in ((32, 32, ((32, 32), (20, 31))), (12, 12, ((12, 12), (5, 11))), (5, 5, ((5, 5), (3, 4))), (64, 16, ((64, 16), (33, 15))),
                       (40, 20, ((40, 20), (39, 7))), (127, 8, ((127, 8), (70, 5))), (100, 10, ((100, 10), (65, 10))),
                       (8, 127, ((8, 127), (5, 100))), (25, 40, ((25, 40), (24, 33)))):
        alt = np.tile(np.array([1, 2], np.int8)[np.arange(W) % 2], (H, 1))  # alternating columns
        contents = {"one": np.full((H, W), 3, np.int8), "altcols": alt, "rand3": _rand(rng, H, W, 3), "rand10": _rand(rng, H, W, 10),
                    "sparse": _sparse(rng, H, W), "wrap": _wrap(H, W), "diagonal": _diagonal(H, W)}
        if (H, W) in ((32, 32), (8, 127)):  # a component per cell on a full row board and on the flat board (1016 <= ARCLE_MAX_CELLS)
            contents["checker"] = _checker(H, W)
        for name, g in contents.items():
            if name != "rand10":
                out.append((f"{H}x{W} {name} dim {dims[0][0]}x{dims[0][1]}", g, dims[0]))
        for name in ("rand3", "rand10", "sparse", "wrap"):
            out.append((f"{H}x{W} {name} dim {dims[1][0]}x{dims[1][1]}", contents[name], dims[1]))
    out.append(("1x1 one", np.full((1, 1), 3, np.int8), (1, 1)))
    out.append(("1x1 zero", np.zeros((1, 1), np.int8), (1, 1)))
    return out


def label(dfs, grid, dim, skip):
    H, W = grid.shape
    lab = np.full((H, W), -1, np.int16)
    comp = []
    gd = np.array(dim, np.int8)
    for x in range(dim[0]):
        for y in range(dim[1]):
            if lab[x, y] >= 0 or (skip >= 0 and grid[x, y] == skip):
                continue
            m = np.asarray(dfs(grid, gd, (x, y))) != 0
            xs, ys = np.nonzero(m)
            assert (lab[m] < 0).all()
            lab[m] = len(comp)
            comp.append((xs.min(), ys.min(), xs.max(), ys.max(), x, y, int(grid[x, y]), int(m.sum())))
    return np.array(comp, np.int16).reshape(-1, 8), lab


def main():
    sys.setrecursionlimit(20000)  # dfs recurses once per cell: a 900-cell component overflows the default limit
    import threading
    threading.stack_size(512 * 1024 * 1024)
    RD.import_reference()
    from arcle.actions.color import dfs
    arrays, names = {}, []

    def run():
        for i, (name, g, dim) in enumerate(cases()):
            names.append(name)
            arrays[f"grid_{i}"] = g
            arrays[f"dim_{i}"] = np.array(dim, np.int8)
            for s in SKIPS:
                comp, lab = label(dfs, g, dim, s)
                arrays[f"comp_{i}_{skip_tag(s)}"] = comp
                arrays[f"label_{i}_{skip_tag(s)}"] = lab
            print(f"{name}: {[len(arrays[f'comp_{i}_{skip_tag(s)}']) for s in SKIPS]} components (skip -1, 0, 3)")
    t = threading.Thread(target=run)  # (a deep C stack for the recursion)
    t.start()
    t.join()
    arrays["names"] = np.array(json.dumps(names))
    os.makedirs(os.path.join(OUT, "components"), exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "components", "components.npz"), **arrays)
    print("wrote", os.path.join(OUT, "components", "components.npz"), os.path.getsize(os.path.join(OUT, "components", "components.npz")), "bytes")


if __name__ == "__main__":
    main()
