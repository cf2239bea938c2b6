#!/usr/bin/env python3
"""arcle_objects_rows in each of its four modes beside arcle_components_rows of the PARENT commit's library, on the same rows: the
30 x 30 grids of tests/golden/components/components.npz tiled to 4096 O2ARC state rows, C = 16, skip_color 0, bits written.
Graph-replayed legs alternating in one process, HIP events around >= 0.5 s of work per repeat.

  baseline   components_rows of the library at --baseline-lib (built at the parent commit; loaded with _lib.load)
  mode 0     objects_rows(any_color=False, diagonal=False): expected to BE the old kernel — a difference beyond the spread of the
             repeats means the dispatch is wrong
  the rest   no target; per leg the mean objects written per row and the time per object written, beside the baseline's

Usage: python tools/objectsbench.py --baseline-lib PATH [--out profiles/objects_bench.txt] [--repeats 5]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from expandbench import timed_graph  # noqa: E402
from expandbitsbench import other_library  # noqa: E402
from arcle_amd import search as S  # noqa: E402
from arcle_amd.engine import EnvBatch  # noqa: E402

N_ROWS, C, SKIP = 4096, 16, 0


def fixture_rows(dev):
    """4096 O2ARC state rows at the library's stride whose grid / grid_dim are the fixture's 30 x 30 cases in turn; other bytes zero."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "components", "components.npz"))
    idx = [i for i in range(len([k for k in z.files if k.startswith("grid_")])) if z[f"grid_{i}"].shape == (30, 30)]
    P = 900
    lay = S.row_layout("o2arc", P)
    L = sum(ln for _, ln in lay)
    goff = sum(ln for f, ln in lay[:[f for f, _ in lay].index("grid")])
    rows = np.zeros((N_ROWS, (L + 15) & ~15), np.int8)
    for m in range(N_ROWS):
        i = idx[m % len(idx)]
        rows[m, goff:goff + P] = z[f"grid_{i}"].reshape(-1)
        rows[m, goff + P:goff + P + 2] = z[f"dim_{i}"]
    return torch.as_tensor(rows, device=dev)[:, :L], len(idx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "objects_bench.txt"))
    ap.add_argument("--baseline-lib", required=True, help="libarcle_hip.so built at the parent commit")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows, n_grids = fixture_rows(dev)
    with other_library(a.baseline_lib) as Lb:
        old = EnvBatch(2, 30, 30, 3, "o2arc")
        abi_old = Lb.arcle_abi_version()
    new = EnvBatch(2, 30, 30, 3, "o2arc")
    legs = []
    out_old = old.components_rows(rows, C, SKIP, True)
    legs.append((f"baseline: components_rows, parent library (ABI {abi_old})", out_old, lambda: old.components_rows(rows, C, SKIP, True, out=out_old)))
    out_cur = new.components_rows(rows, C, SKIP, True)
    legs.append(("components_rows, this library", out_cur, lambda: new.components_rows(rows, C, SKIP, True, out=out_cur)))
    for any_color, diagonal in ((False, False), (True, False), (False, True), (True, True)):
        for colors in (False, True):
            out = new.objects_rows(rows, C, SKIP, any_color, diagonal, True, colors)
            name = f"objects_rows mode {int(any_color) | 2 * int(diagonal)} ({'any_color' if any_color else 'one colour'}, {'8' if diagonal else '4'}-connected)" \
                   f"{' + colors' if colors else ''}"
            legs.append((name, out, lambda o=out, ac=any_color, dg=diagonal, cl=colors: new.objects_rows(rows, C, SKIP, ac, dg, True, cl, out=o)))
    torch.cuda.synchronize(dev)
    same = all(torch.equal(x, y) for x, y in zip(out_old, legs[2][1][:3])) and all(torch.equal(x, y) for x, y in zip(out_old, out_cur))
    runs = [(name, out, timed_graph(dev, fn, 8)) for name, out, fn in legs]
    times = {name: [] for name, _, _ in legs}
    for _ in range(a.repeats):
        for name, _, (run, _) in runs:
            times[name].append(run())
    lines = [f"objectsbench: 30x30 O2ARC, {N_ROWS} rows = the {n_grids} 30x30 grids of tests/golden/components tiled, C = {C}, skip_color = {SKIP}, bits = True",
             f"command: python tools/objectsbench.py --baseline-lib <libarcle_hip.so of the parent commit> --repeats {a.repeats}",
             f"us per launch = median of {a.repeats} repeats [min .. max], each repeat >= 0.5 s of graph replays (8 launches per graph, 3 warm replays), legs alternating",
             f"mode 0 outputs equal the parent library's byte for byte: {same}"]
    base = float(np.median(times[legs[0][0]]))
    nb = float(out_old[0][:, 0].float().mean())
    for name, out, _ in legs:
        t = np.array(times[name])
        med = float(np.median(t))
        n = float(out[0][:, 0].float().mean())
        cut = float((out[0][:, 1] > 0).float().mean())
        lines.append(f"  {name:<66} {med * 1e6:8.2f} us  [{t.min() * 1e6:.2f} .. {t.max() * 1e6:.2f}]  spread {100 * (t.max() - t.min()) / med:.1f} %   "
                     f"{med / base:.3f} x baseline   n = {n:5.2f} objects per row ({100 * cut:.0f} % of the rows cut)   "
                     f"{med / n / N_ROWS * 1e9:.2f} ns per object = {(med / n) / (base / nb):.2f} x baseline's")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
