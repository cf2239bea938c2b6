"""The host side of arcle_stamp_rows: stamp_numpy against the oracle's own CopyO + Paste (copy the object, paste on a one-cell
selection, count the correct cells) under both Pastes, stamp_macros / propose_stamps on an oracle-backed stub vec env (torch CPU
tensors; no GPU), and the search demonstration: planted tasks whose one object is stamped once or twice into empty space."""
import numpy as np
import pytest
import torch

import components as CP
import objects as OB
import search_bits as SB
import stamp as ST
from arcle_amd import search as S
from arcle_amd.envs.vec import Stamps


@pytest.mark.parametrize("blank", [True, False])
@pytest.mark.parametrize("H,W", ST.ORACLE_SIZES)
def test_mirror_equals_the_oracle(H, W, blank):
    """The whole correct(px, py) table of stamp_numpy(full=True) against the chained oracle (mask ingress) for EVERY cell of grid_dim
    of every object of every case — blank False on a table whose Paste descriptor has arg byte 0 — and `stamp` is the table's arg-max
    under the tie rule, `base` the dense pair of the grid."""
    total = 0
    for c in ST.cases_of(H, W):
        want, grid = ST.oracle_table(c, blank)
        stamp, base, table = S.stamp_numpy(grid, c["dim"], c["answer"], c["adim"], c["masks"], None, blank, full=True)
        assert np.array_equal(table, want), (c["name"], np.argwhere(table != want)[:3].tolist())
        gh, gw = int(c["dim"][0]), int(c["dim"][1])
        for k, m in enumerate(c["masks"]):
            xs, ys = np.nonzero(m[:gh, :gw])
            if not len(xs):
                assert stamp[k].tolist() == [0, 0, base[0], 0] and (table[k] == -1).all()
                continue
            x0, y0 = int(xs.min()), int(ys.min())
            cand = np.argwhere(table[k] >= 0)
            assert len(cand) == gh * gw
            total += len(cand)
            best = min((-int(table[k, px, py]), abs(px - x0) + abs(py - y0), px - x0, py - y0) for px, py in cand.tolist())
            assert stamp[k].tolist() == [x0 + best[2], y0 + best[3], -best[0], len(xs)], (c["name"], k)
    assert total > 300, total


def test_max_dist_cuts_the_candidates_to_the_diamond():
    c = [c for c in ST.cases_of(7, 6) if c["name"].endswith("moved")][0]
    _, _, full = S.stamp_numpy(c["grid"], c["dim"], c["answer"], c["adim"], c["masks"], None, True, full=True)
    for D in (0, 1, 3):
        stamp, _, table = S.stamp_numpy(c["grid"], c["dim"], c["answer"], c["adim"], c["masks"], D, True, full=True)
        for k, m in enumerate(c["masks"]):
            xs, ys = np.nonzero(m)
            if not len(xs):
                continue
            px, py = np.mgrid[0:7, 0:6]
            inside = (abs(px - xs.min()) + abs(py - ys.min())) <= D
            assert np.array_equal(table[k], np.where(inside, full[k], -1))
            assert stamp[k, 2] == table[k].max() and table[k, stamp[k, 0], stamp[k, 1]] == stamp[k, 2]


def test_the_tie_rule_level_by_level():
    """One-cell object at the centre, two equally good cells in the answer: the nearer wins, then the smaller dx, then the smaller dy."""
    seen = set()
    for H, W in ((7, 6), (30, 30), (16, 33)):
        for c in ST.cases_of(H, W):
            name = c["name"].split(" ", 1)[1]
            if name in ST.TIE_WANT:
                for blank in (True, False):
                    stamp, _, table = S.stamp_numpy(c["grid"], c["dim"], c["answer"], c["adim"], c["masks"], None, blank, full=True)
                    assert (int(stamp[0, 0]) - H // 2, int(stamp[0, 1]) - W // 2) == ST.TIE_WANT[name], (c["name"], stamp[0])
                    assert (table[0] == stamp[0, 2]).sum() == 2, c["name"]  # two positions score the best count
                seen.add(name)
    assert seen == set(ST.TIE_WANT)


def _objs_and_stamps():
    cases = [c for c in ST.cases_of(7, 6) if c["dim"].tolist() == [7, 6]]
    grids, dims = np.stack([c["grid"] for c in cases]), np.stack([c["dim"] for c in cases])
    objs = OB.objects_numpy(grids, dims, 6, 0, True, True, True, False)
    st = ST.stamp_numpy_rows(grids, dims, np.stack([c["answer"] for c in cases]), np.stack([c["adim"] for c in cases]), objs, None)
    return cases, objs, st


def test_stamp_macros_shapes_padding_and_drop_rule():
    cases, objs, st = _objs_and_stamps()
    assert isinstance(st, Stamps) and Stamps._fields == ("px", "py", "correct", "cells", "base")
    M, C, W = len(cases), 6, 6
    mac = S.stamp_macros(objs, st, ST.COPY_OP, ST.PASTE_OP, W)
    assert tuple(mac["bits"].shape) == (M, C, 2, 128) and mac["bits"].dtype == torch.uint8
    assert tuple(mac["operation"].shape) == (M, C, 2) and mac["operation"].dtype == torch.int32
    assert tuple(mac["length"].shape) == (M, C) and mac["length"].dtype == torch.int32
    real = 0
    for m in range(M):
        for k in range(C):
            px, py, cor = (int(getattr(st, f)[m, k]) for f in ("px", "py", "correct"))
            ops, ln = mac["operation"][m, k].tolist(), int(mac["length"][m, k])
            if k >= int(objs.count[m]) or cor <= int(st.base[m, 0]):
                assert ops == [-1, -1] and ln == 1 and not mac["bits"][m, k].any(), (m, k)
                continue
            real += 1
            assert ops == [ST.COPY_OP, ST.PASTE_OP] and ln == 2
            assert torch.equal(mac["bits"][m, k, 0], objs.bits[m, k])
            one = S.unpack_bits(mac["bits"][m, k, 1], 7, 6)
            assert int(one.sum()) == 1 and bool(one[px, py]) and int(mac["bits"][m, k, 1].to(torch.int32).sum()) == 1 << ((px * W + py) & 7)
    assert real >= 4 and real < M * C


def test_propose_stamps_singles_first_then_the_macros():
    inputs, dims, answers, spots = ST.planted_stamp_tasks(3)
    rows = torch.from_numpy(CP.clean_rows("o2arc", inputs, dims, answers, dims)[0])
    venv = ST.stamp_venv(answers, dims)
    prop = S.propose_stamps(ST.COPY_OP, ST.PASTE_OP, box_ops=[3, 25], seed_ops=[12], max_components=4, any_color=True, diagonal=True)
    assert prop.wants_src is True
    cand = prop(venv, rows, torch.arange(3, dtype=torch.int32))
    objs = venv.objects(rows, max_components=4, skip_color=0, any_color=True, diagonal=True, bits=True)
    single = S.object_actions(objs, [3, 25], [12], masks=True)
    K1 = 4 * 3
    assert tuple(cand["bits"].shape) == (3, K1 + 4, 2, 128) and tuple(cand["operation"].shape) == (3, K1 + 4, 2) and tuple(cand["length"].shape) == (3, K1 + 4)
    assert torch.equal(cand["bits"][:, :K1, 0], single["bits"]) and torch.equal(cand["operation"][:, :K1, 0], single["operation"])
    assert bool((cand["operation"][:, :K1, 1:] == -1).all()) and bool((cand["length"][:, :K1] == 1).all()) and not cand["bits"][:, :K1, 1:].any()
    for i, targets in enumerate(spots):  # the one object's macro pastes at a planted position
        assert int(cand["length"][i, K1]) == 2 and bool((cand["operation"][i, K1 + 1:, 0] == -1).all())
        one = S.unpack_bits(cand["bits"][i, K1, 1], 12, 12)
        assert int(one.sum()) == 1 and tuple(np.argwhere(one.numpy())[0]) in targets
    only = S.propose_stamps(ST.COPY_OP, ST.PASTE_OP, max_components=4, any_color=True, diagonal=True)(venv, rows, None)
    assert all(torch.equal(only[k], cand[k][:, K1:]) for k in only)
    near = S.propose_stamps(ST.COPY_OP, ST.PASTE_OP, max_dist=0, max_components=4, any_color=True, diagonal=True)(venv, rows, None)
    assert bool((near["operation"] == -1).all())  # (within distance 0 the copy lands on the object: nothing to gain)


def test_beam_search_stamps_copies_into_empty_space():
    """Eight planted 12 x 12 tasks, one object of three or four cells stamped once (four tasks) or twice (four tasks) into empty
    space: propose_stamps at width 1, depth = the number of stamps solves all eight and the primitive steps it returns — CopyO on the
    object's cells, Paste on one cell — replay to the answer on the oracle; the macros the library had before (Moves, and CopyO +
    Paste at ANOTHER OBJECT's box: there is no other object where the copy belongs) solve ST.BEFORE_SOLVES of them."""
    inputs, dims, answers, spots = ST.planted_stamp_tasks(8)
    assert [len(s) for s in spots] == [1] * 4 + [2] * 4
    rows = torch.from_numpy(CP.clean_rows("o2arc", inputs, dims, answers, dims)[0])
    venv = ST.stamp_venv(answers, dims)
    before, stamped = ST.stamp_searches(venv, rows, 8, [len(s) for s in spots])
    assert sum(r.sequence is not None for r in stamped) == 8
    assert sum(r.sequence is not None for r in before) == ST.BEFORE_SOLVES < 8
    for i, (r, targets) in enumerate(zip(stamped, spots)):
        assert r.root == 0 and [op for _, op in r.sequence] == [ST.COPY_OP, ST.PASTE_OP] * len(targets), i
        pasted = sorted(tuple(np.argwhere(sel)[0]) for sel, op in r.sequence if op == ST.PASTE_OP)
        assert all(sel.sum() == 1 for sel, op in r.sequence if op == ST.PASTE_OP) and pasted == sorted(targets), i
        assert SB.replay_masks_on_oracle(inputs[i], dims[i], answers[i], r.sequence) == 1, i
