#!/usr/bin/env python3
"""Expanding a search frontier on the objects' exact cells: K = 16 components x K/16 ops for each of M state rows (30 x 30 O2ARC,
states taken from 8192 envs after 10 random steps; masks and boxes from arcle_components_rows with C = 16), the protocol of
tools/expandbench.py — graph-replayed, legs alternating in one process, three repeats of >= 0.5 s:

  (a) rows+hash     the only route to these verdicts before arcle_expand_rows took bit rows: index_select to [M*K] rows + out-of-place
                    arcle_transition_rows with the UNPACKED int8 masks + arcle_hash_rows of the rows it wrote.  With --baseline-lib it
                    runs on that library (one built from the commit before this form existed), loaded next to the current one; the
                    unpacking itself is not timed, which favours this leg.  No dense pair (M*K > n_envs: the dense output is per env)
  (b) expand bits   arcle_expand_rows with the bit rows: reward, terminated, status, dense pair, both hashes of every child
  (c) expand bbox   arcle_expand_rows with the same components' bounding boxes: what the mask ingest and the non-rectangular op paths cost
  (d) rows bits / rows mask   arcle_transition_rows alone on the same M*K pairs, bit rows against int8 masks (report only)

Usage: python tools/expandbitsbench.py [--baseline-lib PATH] [--out profiles/expand_bits_bench.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench  # noqa: E402
from expandbench import timed_graph  # noqa: E402
from arcle_amd import _lib, search as S  # noqa: E402
from arcle_amd.envs.vec import Components  # noqa: E402

SIZES = ((1024, 32), (256, 256))
C = 16
OPS = [22, 3, 20, 21, 23, 24, 25, 26, 27, 1, 2, 4, 5, 6, 7, 8]  # MoveR, Color3, the other moves, Rotate, Flip, colours: K / 16 of them


class other_library:
    """Inside the block `_lib.lib()` hands out the library at `path` (loaded through `_lib.load`, its own ABI version accepted), so an
    EnvBatch made there calls into it for life; outside, the current library is back."""

    def __init__(self, path):
        self.L = _lib.load(os.path.abspath(path))

    def __enter__(self):
        self.saved, _lib._lib = _lib.lib(), self.L
        return self.L

    def __exit__(self, *exc):
        _lib._lib = self.saved


def warmed_batch(dev, n):
    batch = bench.make_batch(dev, n)
    bbox, op = bench.make_actions(10, n, 2000)
    sh = torch.cuda.current_stream(dev).cuda_stream
    for i in range(10):
        bb, oo = torch.as_tensor(bbox[i], device=dev), torch.as_tensor(op[i], device=dev)
        batch.step_bbox_ptr(bb.data_ptr(), oo.data_ptr(), 0, sh)
        torch.cuda.synchronize(dev)
    batch.status(True)
    return batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expand_bits_bench.txt"))
    ap.add_argument("--baseline-lib", default=None, help="libarcle_hip.so of the commit before bit rows: leg (a) runs on it")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = 8192
    batch = warmed_batch(dev, n)
    if a.baseline_lib:
        with other_library(a.baseline_lib) as Lb:
            base = warmed_batch(dev, n)
            base_abi = Lb.arcle_abi_version()
        assert base.L is not batch.L and torch.equal(base.get_state_rows(), batch.get_state_rows())
    else:
        base, base_abi = batch, batch.L.arcle_abi_version()
    all_rows = batch.get_state_rows().clone()
    L = batch.state_row_size()
    stride = (L + 15) & ~15
    lines = [f"expandbitsbench: 30x30 O2ARC, rows of {L} B from {n} envs after 10 random steps; actions = the {C} first components of every row "
             f"(skip_color 0) x K/{C} ops; us per launch = median of {a.repeats} repeats [min .. max], each >= 0.5 s of graph replays, legs alternating",
             f"leg (a) on {'the baseline library (ABI %d), current library ABI %d' % (base_abi, batch.L.arcle_abi_version()) if a.baseline_lib else 'the current library'}"]
    ok = True
    for M, K in SIZES:
        Cn = M * K
        src = torch.randperm(n, generator=torch.Generator().manual_seed(M))[:M].to(torch.int32).to(dev)
        rows = torch.zeros((M, stride), dtype=torch.int8, device=dev)
        rows[:, :L] = all_rows.index_select(0, src.long())
        count, comp, cbits = batch.components_rows(rows, C, 0, bits=True)
        comps = Components(count[:, 0], count[:, 1], comp[:, :, 0:4], comp[:, :, 4:6], comp[:, :, 6], comp[:, :, 7], cbits)
        ops = OPS[:K // C]
        am, ab = S.object_actions(comps, ops, [], masks=True), S.object_actions(comps, ops, [])
        bits, boxes, op = am["bits"], ab["bbox"], am["operation"]
        assert tuple(bits.shape) == (M, K, 128) and torch.equal(op, ab["operation"])
        masks = S.unpack_bits(bits, 30, 30).to(torch.int8).reshape(Cn, 30, 30).contiguous()  # (not timed)
        xs, ys = torch.arange(30, device=dev).reshape(1, 1, 30, 1), torch.arange(30, device=dev).reshape(1, 1, 1, 30)
        x0, y0, x1, y1 = (boxes[..., i, None, None] for i in range(4))
        filled = S.pack_bits((xs >= x0) & (xs <= x1) & (ys >= y0) & (ys <= y1))
        nonrect = float((filled != bits).any(-1)[op >= 0].float().mean())
        rep = torch.arange(M, device=dev).repeat_interleave(K)
        src_rep = src.index_select(0, rep).contiguous()
        bits_rep, op_rep = bits.reshape(Cn, 128), op.reshape(Cn)
        big = torch.empty((Cn, stride), dtype=torch.int8, device=dev)
        out = torch.empty((Cn, stride), dtype=torch.int8, device=dev)
        rw, tm = torch.empty(Cn, dtype=torch.int32, device=dev), torch.empty(Cn, dtype=torch.uint8, device=dev)
        hs = torch.empty((Cn, 2), dtype=torch.int64, device=dev)

        def leg_a():
            torch.index_select(rows, 0, rep, out=big)
            base.transition_rows(big, "mask", masks, op_rep, src_rep, out=out, reward=rw, term=tm)
            base.hash_rows(out[:, :L], out=hs)
        ex_b = batch.expand_rows(rows, "bits", bits, op, src, dense=True)
        ex_c = batch.expand_rows(rows, "bbox", boxes, op, src, dense=True)
        torch.index_select(rows, 0, rep, out=big)
        # the stated equality, at this size: (b) against the row route
        leg_a()
        torch.cuda.synchronize(dev)
        assert torch.equal(ex_b.reward.reshape(-1), rw) and torch.equal(ex_b.term.reshape(-1), tm) and torch.equal(ex_b.hash.reshape(Cn, 2), hs), "expand_rows(bits) != the row route"
        changed = float((ex_b.hash[:, :, 0] != ex_b.parent_hash[:, None, 0]).float().mean())
        differ = float((ex_b.hash[:, :, 0] != ex_c.hash[:, :, 0]).float().mean())
        legs = [("(a) rows+hash", leg_a),
                ("(b) expand bits", lambda: batch.expand_rows(rows, "bits", bits, op, src, dense=True, out=ex_b)),
                ("(c) expand bbox", lambda: batch.expand_rows(rows, "bbox", boxes, op, src, dense=True, out=ex_c)),
                ("(d) rows bits", lambda: batch.transition_rows(big, "bits", bits_rep, op_rep, src_rep, out=out, reward=rw, term=tm)),
                ("(d) rows mask", lambda: batch.transition_rows(big, "mask", masks, op_rep, src_rep, out=out, reward=rw, term=tm))]
        torch.cuda.synchronize(dev)
        runs = [(name, timed_graph(dev, fn, max(1, min(64, 65536 // Cn)))) for name, fn in legs]
        times = {name: [] for name, _ in legs}
        for _ in range(a.repeats):
            for name, (run, _) in runs:
                times[name].append(run())
        lines.append(f"(M, K) = ({M}, {K}): {Cn} children per launch; {changed:.2f} of them differ from their parent, {nonrect:.2f} of the masks are not their "
                     f"filled box, {differ:.2f} of the children differ between mask and box")
        for name, _ in legs:
            t = np.array(times[name])
            med = float(np.median(t))
            lines.append(f"  {name:<16} {med * 1e6:10.2f} us  [{t.min() * 1e6:.2f} .. {t.max() * 1e6:.2f}]   {Cn / med / 1e9:7.3f} G children/s")
        ta, tb, tc = np.array(times["(a) rows+hash"]), np.array(times["(b) expand bits"]), np.array(times["(c) expand bbox"])
        td = np.array(times["(d) rows bits"]), np.array(times["(d) rows mask"])
        good = tb.max() < ta.min()
        ok = ok and good
        lines.append(f"  (a) / (b) = {np.median(ta) / np.median(tb):.2f}x  (fastest (a) repeat over slowest (b) repeat: {ta.min() / tb.max():.2f}x — acceptance "
                     f"{'met' if good else 'MISSED'});  (b) / (c) = {np.median(tb) / np.median(tc):.2f}x;  rows bits / rows mask = {np.median(td[0]) / np.median(td[1]):.2f}x")
        del runs, big, out, masks
        torch.cuda.empty_cache()
    batch.status(True), base.status(True)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
