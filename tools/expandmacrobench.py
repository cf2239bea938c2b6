#!/usr/bin/env python3
"""Scoring two-step candidates for a search frontier: K macros [op_a on one object's box, op_b on another's] for each of M state rows
(30 x 30 O2ARC, states taken from 8192 envs after 10 random steps; boxes from arcle_components_rows with C = 16), the protocol of
tools/expandbench.py — graph-replayed, legs alternating in one process on ONE library, three repeats of >= 0.5 s:

  (a) rows route     what served these verdicts before arcle_expand_macros: index_select to [M*K] rows, in-place arcle_transition_rows for
                     step 0, arcle_expand_rows with ONE action per row for step 1 (reward, terminated, status, dense pair, hashes)
  (b) expand macros  arcle_expand_macros, T = 2, with the lengths array: the same verdicts, no child row written anywhere
  (c) expand 1 step  arcle_expand_rows with step 0 alone (report only: what the second step and the macro loop add)

Before timing, (b)'s reward, terminated, dense pair and hashes are checked against (a)'s at that size.  No ratio is an acceptance
condition: the figures are reported as measured.  --resource-log: a file holding the remarks of
`hipcc ... -Rpass-analysis=kernel-resource-usage -c arcle_amd/csrc/arcle_hip.hip` (flags of arcle_amd/_lib.py; needs no GPU); the
registers and scratch of every expand instantiation are appended to the report.

Usage: python tools/expandmacrobench.py [--resource-log FILE] [--out profiles/expand_macros_bench.txt]"""
import argparse
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from expandbench import timed_graph  # noqa: E402
from expandbitsbench import warmed_batch  # noqa: E402

SIZES = ((1024, 32), (256, 256))
C, T = 16, 2
PAIRS = [(29, 30), (22, 3), (20, 24), (5, 23), (29, 30), (25, 21), (2, 22), (28, 30), (23, 7), (26, 20), (29, 30), (21, 1), (24, 22), (4, 20), (27, 23), (6, 21)]


def resource_lines(path):
    """-Rpass-analysis=kernel-resource-usage remarks -> one line per arcle_expand*_kernel instantiation."""
    blocks = re.split(r"(?=remark: [^\n]*Function Name:)", open(path).read())
    out = ["registers of the expand kernels (hipcc ... -Rpass-analysis=kernel-resource-usage -c arcle_amd/csrc/arcle_hip.hip; <ingress, width class>: "
           "ingress 1 bbox, 2 point, 4 bits; width 1 = 16 <= W <= 32):"]
    for b in blocks:
        m = re.search(r"Function Name: _Z\d+(arcle_expand\w*?_kernel)ILi(\d)ELi(\d)EE", b)
        if not m:
            continue
        get = lambda k: re.search(k + r": (\S+)", b).group(1)  # noqa: E731
        scratch, occ, lds = get(r"ScratchSize \[bytes/lane\]"), get(r"Occupancy \[waves/SIMD\]"), get(r"LDS Size \[bytes/block\]")
        out.append(f"{m.group(1)}<{m.group(2)}, {m.group(3)}> SGPR {get('SGPRs')} VGPR {get('VGPRs')} AGPR {get('AGPRs')} sgpr-spill {get('SGPRs Spill')} "
                   f"vgpr-spill {get('VGPRs Spill')} scratch B/lane {scratch} waves/SIMD {occ} LDS {lds}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expand_macros_bench.txt"))
    ap.add_argument("--resource-log", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    n = 8192
    batch = warmed_batch(dev, n)
    all_rows = batch.get_state_rows().clone()
    L = batch.state_row_size()
    stride = (L + 15) & ~15
    lines = [f"expandmacrobench: 30x30 O2ARC, rows of {L} B from {n} envs after 10 random steps; macros of T = {T} steps on the boxes of the {C} first "
             f"components of every row (skip_color 0): macro k = [op_a on box k % {C}, op_b on box (k % {C} + 1 + k // {C}) % {C}], slots of absent "
             f"components: op -1, length 1; us per launch = median of {a.repeats} repeats [min .. max], each >= 0.5 s of graph replays, legs alternating"]
    for M, K in SIZES:
        Cn = M * K
        src = torch.randperm(n, generator=torch.Generator().manual_seed(M))[:M].to(torch.int32).to(dev)
        rows = torch.zeros((M, stride), dtype=torch.int8, device=dev)
        rows[:, :L] = all_rows.index_select(0, src.long())
        count, comp, _ = batch.components_rows(rows, C, 0)
        box = comp[:, :, 0:4].to(torch.int32)
        k = torch.arange(K, device=dev)
        i, j = k % C, (k % C + 1 + k // C) % C
        pair = torch.as_tensor(PAIRS, dtype=torch.int32, device=dev)[(k // C) % len(PAIRS)]          # [K, 2]
        there = (i.reshape(1, K) < count[:, :1]) & (j.reshape(1, K) < count[:, :1]) & (i != j).reshape(1, K)  # [M, K]
        pay = torch.stack([box.index_select(1, i), box.index_select(1, j)], 2)                        # [M, K, 2, 4]
        pay = torch.where(there.reshape(M, K, 1, 1), pay, torch.zeros((), dtype=torch.int32, device=dev)).contiguous()
        op = torch.where(there.reshape(M, K, 1), pair.reshape(1, K, 2), torch.full((), -1, dtype=torch.int32, device=dev)).contiguous()
        length = torch.where(there, 2, 1).to(torch.int32).contiguous()
        rep = torch.arange(M, device=dev).repeat_interleave(K)
        src_rep = src.index_select(0, rep).contiguous()
        pay0, op0 = pay[:, :, 0].reshape(Cn, 4).contiguous(), op[:, :, 0].reshape(Cn).contiguous()
        # (a)'s second step: one action per row; a macro of length 1 gets an out-of-range op there (the step does not happen)
        pay1, op1 = pay[:, :, 1].reshape(Cn, 1, 4).contiguous(), op[:, :, 1].reshape(Cn, 1).contiguous()
        big = torch.empty((Cn, stride), dtype=torch.int8, device=dev)
        rw, tm = torch.empty(Cn, dtype=torch.int32, device=dev), torch.empty(Cn, dtype=torch.uint8, device=dev)
        ex_a = batch.expand_rows(rows.index_select(0, rep), "bbox", pay1, op1, src_rep, dense=True)
        ex_b = batch.expand_macros(rows, "bbox", pay, op, length, src, dense=True)
        ex_c = batch.expand_rows(rows, "bbox", pay[:, :, 0].contiguous(), op[:, :, 0].contiguous(), src, dense=True)

        def leg_a():
            torch.index_select(rows, 0, rep, out=big)
            batch.transition_rows(big, "bbox", pay0, op0, src_rep, out=big, reward=rw, term=tm)
            batch.expand_rows(big, "bbox", pay1, op1, src_rep, dense=True, out=ex_a)
        leg_a()
        torch.cuda.synchronize(dev)
        batch.status(True)  # (the row kernel's status bits are sticky: the padding slots)
        two = (length == 2).reshape(-1)
        assert torch.equal(ex_b.hash.reshape(Cn, 2), ex_a.hash.reshape(Cn, 2)), "expand_macros' hashes != the row route's"
        assert torch.equal(ex_b.reward.reshape(-1)[two], (rw + ex_a.reward.reshape(-1))[two]) and torch.equal(ex_b.term.reshape(-1)[two], ex_a.term.reshape(-1)[two])
        assert torch.equal(ex_b.dense.reshape(Cn, 2)[two], ex_a.dense.reshape(Cn, 2)[two]), "expand_macros' dense pairs != the row route's"
        changed = float((ex_b.hash[:, :, 0] != ex_b.parent_hash[:, None, 0]).float().mean())
        second = float((ex_b.hash[:, :, 0] != ex_c.hash[:, :, 0]).float().mean())
        p0, o0 = pay[:, :, 0].contiguous(), op[:, :, 0].contiguous()
        legs = [("(a) rows route", leg_a),
                ("(b) expand macros", lambda: batch.expand_macros(rows, "bbox", pay, op, length, src, dense=True, out=ex_b)),
                ("(c) expand 1 step", lambda: batch.expand_rows(rows, "bbox", p0, o0, src, dense=True, out=ex_c))]
        torch.cuda.synchronize(dev)
        runs = [(name, timed_graph(dev, fn, max(1, min(64, 65536 // Cn)))) for name, fn in legs]
        times = {name: [] for name, _ in legs}
        for _ in range(a.repeats):
            for name, (run, _) in runs:
                times[name].append(run())
        lines.append(f"(M, K) = ({M}, {K}): {Cn} macros per launch, {float(two.float().mean()):.2f} of them of 2 steps; {changed:.2f} of the children differ from "
                     f"their parent, {second:.2f} from the child of their first step alone")
        for name, _ in legs:
            t = np.array(times[name])
            med = float(np.median(t))
            lines.append(f"  {name:<18} {med * 1e6:10.2f} us  [{t.min() * 1e6:.2f} .. {t.max() * 1e6:.2f}]   {Cn / med / 1e9:7.3f} G macros/s")
        ta, tb, tc = (np.array(times[name]) for name, _ in legs)
        lines.append(f"  (a) / (b) = {np.median(ta) / np.median(tb):.2f}x  (fastest (a) repeat over slowest (b) repeat: {ta.min() / tb.max():.2f}x);  "
                     f"(b) / (c) = {np.median(tb) / np.median(tc):.2f}x;  child rows the rows route writes and reads back: {Cn * stride / 2**20:.0f} MiB per launch")
        del runs, big
        torch.cuda.empty_cache()
    batch.status(True)
    if a.resource_log:
        lines += [""] + resource_lines(a.resource_log)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
