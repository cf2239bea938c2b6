"""The host side of arcle_mirror_rows: mirror_numpy against the oracle's own CopyO + Paste + Flip (both Pastes, every candidate of every
slot, by grid and dense pair), the max_dist cut and the tie rule, mirror_macros / propose_mirrors on an oracle-backed stub vec env (torch
CPU tensors; no GPU), and the search demonstration: planted symmetric patterns with rectangles punched out."""
import numpy as np
import pytest
import torch

import components as CP
import mirror as MI
import objects as OB
from arcle_amd import search as S
from arcle_amd.envs.vec import Mirrors
from oracle import oracle as O


@pytest.mark.parametrize("blank", (True, False))
@pytest.mark.parametrize("H,W", MI.ORACLE_SIZES)
def test_mirror_equals_the_oracle(H, W, blank):
    """Every candidate (s, dx, dy) of every object of every case as the oracle's own macro (the chained oracle, mask ingress, O2ARCv2Env's
    table; blank False: the same table with a Paste that writes positive cells only) — CopyO on the source rectangle, Paste at the box's
    corner, Flip H / Flip V of the box, and Flip V on the empty selection for the point reflection: the grid the oracle leaves is the
    child of the definition, its dense pair is (the table's entry, base total); at least 100 candidates per slot; `mirror` is the
    table's arg-max under the tie rule and `base` the dense pair of the grid."""
    per = np.zeros(3, np.int64)
    for c in MI.cases_of(H, W):
        grids, dense, want, cand, owner, grid = MI.oracle_children(c, blank)
        mir, base, table = S.mirror_numpy(grid, c["dim"], c["answer"], c["adim"], c["masks"], None, MI.ALL, blank, full=True)
        assert np.array_equal(dense[:, 0], want), (c["name"], cand[dense[:, 0] != want][:3].tolist())
        assert (dense[:, 1] == base[1]).all(), c["name"]
        for j in range(len(cand)):
            child = MI.child_numpy(grid, c["masks"][owner[j]], c["dim"], *cand[j], blank)
            assert np.array_equal(child, grids[j]), (c["name"], cand[j].tolist())
        per += np.bincount(cand[:, 0], minlength=3) if len(cand) else 0
        gh, gw = int(c["dim"][0]), int(c["dim"][1])
        mh, mw = min(gh, int(c["adim"][0])), min(gw, int(c["adim"][1]))
        assert base[0] == int((grid[:mh, :mw] == c["answer"][:mh, :mw]).sum())
        for k, m in enumerate(c["masks"]):
            for s in range(3):
                cd = np.argwhere(table[k, s] >= 0) - (H - 1, W - 1)
                if not (m[:gh, :gw] != 0).any():
                    assert mir[k, s].tolist() == [0, 0, base[0], 1] and not len(cd)
                else:
                    assert len(cd) and (s != 0 or not cd[:, 0].any()) and (s != 1 or not cd[:, 1].any())  # (0, 0) is always one; dx = 0 under H, dy = 0 under V
                    best = min((-int(table[k, s, dx + H - 1, dy + W - 1]), abs(dx) + abs(dy), dx, dy) for dx, dy in cd.tolist())
                    assert mir[k, s].tolist() == [best[2], best[3], -best[0], 1], (c["name"], k, s)
    assert (per >= 100).all(), per


def test_the_arc_table_has_no_flip():
    """ARCEnv's table carries Copy and Paste but no Flip: the macro cannot be run there, and propose_mirrors refuses a table without one."""
    assert not any((d & 0xff) == O.OP_FLIP for d in O.arc_ops()) and sum((d & 0xff) == O.OP_FLIP for d in O.o2arc_ops()) == 2
    assert [O.o2arc_ops()[i] & 0xff for i in (MI.COPY_OP, MI.PASTE_OP) + MI.FLIP_OPS] == [O.OP_COPY, O.OP_PASTE, O.OP_FLIP, O.OP_FLIP]
    with pytest.raises(AssertionError):
        S.propose_mirrors(22, 24, (-1, -1))


def test_unrequested_slots_stay_zero_and_requested_ones_do_not_change():
    c = [c for c in MI.cases_of(7, 6) if c["name"].endswith("pt central")][0]
    for blank in (True, False):
        full, base = S.mirror_numpy(c["grid"], c["dim"], c["answer"], c["adim"], c["masks"], 3, MI.ALL, blank)
        for mirrors in range(1, 7):
            part, b = S.mirror_numpy(c["grid"], c["dim"], c["answer"], c["adim"], c["masks"], 3, mirrors, blank)
            asked = np.array([(mirrors >> s) & 1 for s in range(3)], bool)
            assert b == base and np.array_equal(part[:, asked], full[:, asked]) and not part[:, ~asked].any()


def test_max_dist_cuts_the_candidates_to_the_diamond():
    for c in [c for c in MI.cases_of(7, 6) if c["name"].endswith(("moved", "pt off", "wide"))]:
        _, _, full = S.mirror_numpy(c["grid"], c["dim"], c["answer"], c["adim"], c["masks"], None, MI.ALL, True, full=True)
        dx, dy = np.mgrid[-6:7, -5:6]
        for D in (0, 1, 3):
            mir, _, table = S.mirror_numpy(c["grid"], c["dim"], c["answer"], c["adim"], c["masks"], D, MI.ALL, True, full=True)
            assert np.array_equal(table, np.where((abs(dx) + abs(dy) <= D)[None, None], full, -1))
            for k in range(len(c["masks"])):
                for s in range(3):
                    if c["masks"][k].any():
                        assert mir[k, s, 3] == 1 and mir[k, s, 2] == table[k, s].max() == table[k, s, mir[k, s, 0] + 6, mir[k, s, 1] + 5]
                        assert D > 0 or mir[k, s, :2].tolist() == [0, 0]


def test_the_cases_are_what_they_claim():
    """Per size (H, W >= 4): the holes of the symmetric cases are restored in full by the slot they are named for and by no candidate
    at (0, 0); an edge case has candidates on one side only; every source rectangle of `wide` overlaps its box; `lshape` has a
    non-rectangular object and its best child differs from the answer in the cell that was right; `odd bytes` has sources below 0 and
    above 9 and `show through` scores differently under the two Pastes; grid_dim is shrunk with answer_dim larger and smaller per axis
    and object cells outside grid_dim; there are an empty mask, the whole-grid object (one candidate per slot) and one tie case per
    level of the tie rule, each with exactly two best sources in the point slot."""
    for H, W in MI.SIZES:
        cases = MI.cases_of(H, W)
        by = {c["name"].split(" ", 1)[1]: c for c in cases}
        assert any(not (c["masks"][k][:c["dim"][0], :c["dim"][1]]).any() for c in cases for k in range(len(c["masks"]))), "an empty mask"
        whole = by["bytes"]
        assert whole["masks"][0].all()
        _, _, table = S.mirror_numpy(whole["grid"], whole["dim"], whole["answer"], whole["adim"], whole["masks"][:1], None, MI.ALL, True, full=True)
        assert [(table[0, s] >= 0).sum() for s in range(3)] == [1, 1, 1]
        if H < 4 or W < 4:
            continue
        shrunk = [c for c in cases if c["dim"].tolist() != [H, W]]
        assert any(c["adim"][0] > c["dim"][0] and c["adim"][1] < c["dim"][1] for c in shrunk) and any(c["adim"][0] < c["dim"][0] and c["adim"][1] > c["dim"][1] for c in shrunk)
        assert all(c["masks"][:, c["dim"][0]:].any() or c["masks"][:, :, c["dim"][1]:].any() for c in shrunk), "object cells outside grid_dim"
        for s, tag in enumerate(("lr", "ud", "pt")):
            for name in ("central", "off"):
                c = by[f"{tag} {name}"]
                mir, base = MI.mirror(c, MI.LARGE, True)
                assert mir[0, s, 2] == H * W > base[0] and (mir[0, s, 0], mir[0, s, 1]) != (0, 0), c["name"]
        for name, s, side in (("edge top", 1, lambda dx, dy: dx >= 0), ("edge bottom", 1, lambda dx, dy: dx <= 0 or 2 * (H // 2) < H),
                              ("edge left", 0, lambda dx, dy: dy >= 0), ("edge right", 0, lambda dx, dy: dy <= 0 or 2 * (W // 2) < W)):
            c = by[name]
            _, _, table = S.mirror_numpy(c["grid"], c["dim"], c["answer"], c["adim"], c["masks"], None, MI.ALL, True, full=True)
            cd = np.argwhere(table[0, s] >= 0) - (H - 1, W - 1)
            assert len(cd) > 1 and all(side(dx, dy) for dx, dy in cd.tolist()), c["name"]
            assert MI.mirror(c, MI.LARGE, True)[0][0, s, 2] == H * W, c["name"]
        c = by["wide"]
        ys = np.nonzero(c["masks"][0])[1]
        assert 2 * (ys.max() - ys.min() + 1) > W
        c = by["lshape"]
        xs, ys = np.nonzero(c["masks"][0])
        assert len(xs) < (xs.max() - xs.min() + 1) * (ys.max() - ys.min() + 1)
        c = by["odd bytes"]
        assert (c["grid"] < 0).any() and (c["grid"] > 9).any()
        c = by["show through"]
        assert not np.array_equal(MI.mirror(c, MI.LARGE, True)[0], MI.mirror(c, MI.LARGE, False)[0])
        ties = [c for c in cases if " mtie" in c["name"]]
        assert len(ties) == 7
        for c in ties:
            mir, _, table = S.mirror_numpy(c["grid"], c["dim"], c["answer"], c["adim"], c["masks"], None, MI.ALL, True, full=True)
            assert (table[0, 2] == mir[0, 2, 2]).sum() == 2, c["name"]
    assert {MI.tie_want(n, 2) for n in MI.TIE_SPOTS} == {(-1, 0), (0, -1), (1, 0), (0, 1), (-1, 1)}


def test_the_tie_rule_level_by_level():
    """A one-cell hole at the centre, two equally good source cells: the nearer wins, then the smaller dx, then the smaller dy — in the
    point slot among both spots, in the H slot among those with dx = 0, in the V slot among those with dy = 0."""
    seen = set()
    for H, W in ((7, 6), (30, 30), (16, 33)):
        for c in MI.cases_of(H, W):
            name = c["name"].split(" ", 1)[1]
            if name in MI.TIE_SPOTS:
                for blank in (True, False):
                    mir, _ = MI.mirror(c, MI.LARGE, blank)
                    for s in range(3):
                        assert (int(mir[0, s, 0]), int(mir[0, s, 1])) == MI.tie_want(name, s), (c["name"], s, mir[0, s])
                seen.add(name)
    assert seen == set(MI.TIE_SPOTS)


def _objs_and_mirrors(max_dist=None, mirrors=MI.ALL):
    cases = [c for c in MI.cases_of(7, 6) if c["dim"].tolist() == [7, 6]]
    grids, dims = np.stack([c["grid"] for c in cases]), np.stack([c["dim"] for c in cases])
    objs = OB.objects_numpy(grids, dims, 8, -1, False, False, True, False)
    mn = MI.mirror_numpy_rows(grids, dims, np.stack([c["answer"] for c in cases]), np.stack([c["adim"] for c in cases]), objs, max_dist, mirrors)
    return cases, objs, mn


def test_mirror_macros_shapes_padding_and_drop_rule():
    cases, objs, mn = _objs_and_mirrors()
    assert isinstance(mn, Mirrors) and Mirrors._fields == ("dx", "dy", "correct", "valid", "base")
    M, C, T, H, W = len(cases), 8, 4, 7, 6
    assert tuple(mn.dx.shape) == (M, C, 3) and tuple(mn.base.shape) == (M, 2)
    real = point = dropped = 0
    for flip_ops in (MI.FLIP_OPS, (MI.FLIP_OPS[0], -1), (-1, MI.FLIP_OPS[1])):
        mac = S.mirror_macros(objs, mn, MI.COPY_OP, MI.PASTE_OP, flip_ops, H, W)
        assert tuple(mac["bits"].shape) == (M, C, T, 128) and mac["bits"].dtype == torch.uint8
        assert tuple(mac["operation"].shape) == (M, C, T) and mac["operation"].dtype == torch.int32
        assert tuple(mac["length"].shape) == (M, C) and mac["length"].dtype == torch.int32
        has = (flip_ops[0] >= 0, flip_ops[1] >= 0, min(flip_ops) >= 0)
        sel = S.unpack_bits(mac["bits"], H, W).numpy()
        for m in range(M):
            for k in range(C):
                usable = [s for s in range(3) if int(mn.valid[m, k, s]) and has[s]]
                best = min(((-int(mn.correct[m, k, s]), (3, 3, 4)[s], s) for s in usable), default=None)
                ops, ln = mac["operation"][m, k].tolist(), int(mac["length"][m, k])
                if k >= int(objs.count[m]) or best is None or -best[0] <= int(mn.base[m, 0]):
                    assert ops == [-1] * T and ln == 1 and not mac["bits"][m, k].any(), (m, k)
                    dropped += 1
                    continue
                real += 1
                s = best[2]
                point += s == 2
                dx, dy = int(mn.dx[m, k, s]), int(mn.dy[m, k, s])
                x0, y0, x1, y1 = (int(v) for v in objs.box[m, k])
                want = [MI.COPY_OP, MI.PASTE_OP, flip_ops[1] if s == 1 else flip_ops[0]] + ([flip_ops[1]] if s == 2 else [])
                assert ln == len(want) and ops == want + [-1] * (T - ln), (m, k, ops, want)
                rect = np.zeros((4, H, W), bool)
                rect[0, x0 + dx:x1 + dx + 1, y0 + dy:y1 + dy + 1] = True
                rect[1, x0, y0] = True
                rect[2, x0:x1 + 1, y0:y1 + 1] = True
                assert np.array_equal(sel[m, k], rect), (m, k)
    assert real >= 8 and point >= 1 and dropped >= 8, (real, point, dropped)


def test_propose_mirrors_singles_first_then_the_macros():
    inputs, dims, answers, plans = MI.planted_mirror_tasks(3)
    rows = torch.from_numpy(CP.clean_rows("o2arc", inputs, dims, answers, dims)[0])
    venv = MI.mirror_venv(answers, dims)
    asked = []
    inner = venv.mirror
    venv.mirror = lambda rows, objs, src_env=None, max_dist=None, mirrors=7, blank=True: (asked.append((max_dist, mirrors, blank)), inner(rows, objs, src_env, max_dist, mirrors, blank))[1]
    C = MI.MAX_OBJECTS
    prop = S.propose_mirrors(MI.COPY_OP, MI.PASTE_OP, MI.FLIP_OPS, box_ops=[3, 29], seed_ops=[12], max_dist=9, max_components=C, skip_color=-1)
    assert prop.wants_src is True
    cand = prop(venv, rows, torch.arange(3, dtype=torch.int32))
    objs = venv.components(rows, max_components=C, skip_color=-1, bits=True)
    single = S.object_actions(objs, [3, 29], [12], masks=True)
    K1, T = C * 3, 4
    assert tuple(cand["bits"].shape) == (3, K1 + C, T, 128) and tuple(cand["operation"].shape) == (3, K1 + C, T) and tuple(cand["length"].shape) == (3, K1 + C)
    assert torch.equal(cand["bits"][:, :K1, 0], single["bits"]) and torch.equal(cand["operation"][:, :K1, 0], single["operation"])
    assert bool((cand["operation"][:, :K1, 1:] == -1).all()) and bool((cand["length"][:, :K1] == 1).all()) and not cand["bits"][:, :K1, 1:].any()
    for i, (s, boxes) in enumerate(plans):  # the hole's macro is there, with the Flips of a slot that restores it
        k = [j for j in range(int(objs.count[i])) if tuple(int(v) for v in objs.box[i, j]) == boxes[0] and int(objs.color[i, j]) == 0]
        assert len(k) == 1 and int(cand["length"][i, K1 + k[0]]) in (3, 4) and int(cand["operation"][i, K1 + k[0], 0]) == MI.COPY_OP
    only = S.propose_mirrors(MI.COPY_OP, MI.PASTE_OP, MI.FLIP_OPS, max_dist=9, max_components=C, skip_color=-1)(venv, rows, None)
    assert all(torch.equal(only[k], cand[k][:, K1:]) for k in only)
    S.propose_mirrors(MI.COPY_OP, MI.PASTE_OP, (-1, MI.FLIP_OPS[1]), max_components=C, skip_color=-1, blank=False)(venv, rows, None)
    assert asked == [(9, 7, True), (9, 7, True), (None, 2, False)]  # only the slots whose Flips the table has are asked for; max_dist and blank are passed on


def test_beam_search_restores_symmetric_patterns():
    """Eight planted 12 x 12 tasks — a left-right-, up-down- or point-symmetric pattern (all three occur, the axis off-centre in five) with
    one or two rectangular holes of at least 6 cells whose true content has at least 3 colours and is not itself symmetric under the
    slot: propose_mirrors at width 1 and depth = the number of holes solves all eight and the primitive steps it returns — CopyO, Paste,
    Flip(s) per hole — replay to the answer on the oracle; the six earlier proposers at the same width and depth solve MI.BEFORE_SOLVES."""
    inputs, dims, answers, plans = MI.planted_mirror_tasks(8)
    assert {s for s, _ in plans} == {0, 1, 2} and {len(b) for _, b in plans} == {1, 2}
    for (s, boxes), g, a in zip(plans, inputs, answers):
        for x0, y0, x1, y1 in boxes:
            content = a[x0:x1 + 1, y0:y1 + 1]
            assert content.size >= 6 and len(set(content.ravel().tolist())) >= 3 and not (g[x0:x1 + 1, y0:y1 + 1] != 0).any()
            assert not np.array_equal(content, S._flipped(content, s))
    rows = torch.from_numpy(CP.clean_rows("o2arc", inputs, dims, answers, dims)[0])
    venv = MI.mirror_venv(answers, dims)
    depths = [len(b) for _, b in plans]
    mirrored, before = MI.searches(venv, rows, 8, depths)
    assert sum(r.sequence is not None for r in mirrored) == 8
    assert set(before) == {"objects", "placements", "stamps", "turns", "alignments", "rays"}
    assert sum(r.sequence is not None for rs in before.values() for r in rs) == MI.BEFORE_SOLVES == 0
    for i, (r, (s, boxes)) in enumerate(zip(mirrored, plans)):
        ops = [op for _, op in r.sequence]
        assert r.root == 0 and ops.count(MI.COPY_OP) == ops.count(MI.PASTE_OP) == len(boxes) and 3 * len(boxes) <= len(ops) <= 4 * len(boxes), (i, ops)
        assert MI.replay_on_oracle(inputs[i], dims[i], answers[i], r.sequence) == 1, i
