"""arcle_amd.search.region_numpy — the mirror every region test compares against — pinned on the oracle's own Color step and on a
brute-force restatement (a per-cell BFS for INSIDE, a neighbour loop for the halos), the rules on hand-made grids, region_actions /
propose_regions, and the planted tasks on the oracle-backed stub vec env.  No GPU."""
import collections

import numpy as np
import pytest
import torch

import align as AL
import components as CP
import objects as OB
import regions as RG
from arcle_amd import search as S
from arcle_amd.envs.vec import Regions

NONE, HALO4, HALO8, BOX_REST, BOX_FRAME, INSIDE, BOX, SELF = range(8)
ALL = (1, 2, 3, 4, 5, 6, 7)


def regions_of(grid, mask, kinds=ALL, answer=None, dim=None, adim=None, free_color=0, through=False):
    grid = np.asarray(grid, np.int8)
    answer = grid if answer is None else np.asarray(answer, np.int8)
    reg, best, base, cells = S.region_numpy(grid, grid.shape if dim is None else dim, answer, answer.shape if adim is None else adim, np.asarray(mask)[None], kinds,
                                            free_color, through, full=True)
    return reg[0], best[0], base, cells[0]


def test_the_constants():
    assert (S.REGION_NONE, S.REGION_HALO4, S.REGION_HALO8, S.REGION_BOX_REST, S.REGION_BOX_FRAME, S.REGION_INSIDE, S.REGION_BOX, S.REGION_SELF) == tuple(range(8))
    assert S.REGION_KINDS == ALL
    from arcle_amd import _lib
    assert (_lib.REGION_NONE, _lib.REGION_HALO4, _lib.REGION_HALO8, _lib.REGION_BOX_REST, _lib.REGION_BOX_FRAME, _lib.REGION_INSIDE, _lib.REGION_BOX,
            _lib.REGION_SELF) == tuple(range(8)) and _lib.ABI_VERSION == 18 and "arcle_region_rows" in _lib.EXPORTS and len(_lib.EXPORTS) == 61


@pytest.mark.parametrize("through,free_color", [(False, 0), (False, 5), (False, -1), (True, 0), (True, 5), (True, -1)])
@pytest.mark.parametrize("H,W", RG.ORACLE_SIZES)
def test_mirror_equals_the_oracles_color_step(H, W, through, free_color):
    """Every case of the size (grid_dim below the plane in the shrunk cases and in `edges`), every object, each of the seven kinds, all
    ten colours: the oracle runs `Color c` on the mirror's cells of the candidate; the dense pair's first number for the reported colour
    is `correct`, the reported colour is the first arg-max over the ten children, and the children's differences are the differences
    of the answer's colour counts under the cells (`right`)."""
    seen = 0
    for case in RG.cases_of(H, W):
        gh, gw = (int(v) for v in case["dim"])
        mh, mw = min(gh, int(case["adim"][0])), min(gw, int(case["adim"][1]))
        dense, (reg, best, base, cells) = RG.oracle_children(case, ALL, through, "o2arc", free_color)
        for k in range(len(reg)):
            for s in range(len(ALL)):
                color, correct, n, right = (int(v) for v in reg[k, s])
                if n == 0:
                    assert (dense[k, s] == -1).all() and (color, correct, right) == (0, base[0], 0), (case["name"], k, s)
                    continue
                assert not cells[k, s][gh:].any() and not cells[k, s][:, gw:].any() and int(cells[k, s].sum()) == n
                d = dense[k, s]
                assert correct == d[color] and color == int(np.argmax(d)), (case["name"], through, k, s, reg[k, s], d)
                under = case["answer"][:mh, :mw][cells[k, s][:mh, :mw]]
                freq = np.array([(under == c).sum() for c in range(10)])
                assert right == freq[color] and np.array_equal(d - d[color], freq - right), (case["name"], through, k, s)
                seen += 1
    assert seen > 100


def test_mirror_equals_the_oracles_color_step_on_arc_rows():
    """The same on the ARC env kind's rows at one size."""
    for case in RG.cases_of(7, 6)[::3]:
        dense, (reg, best, base, cells) = RG.oracle_children(case, ALL, True, "arc")
        for k in range(len(reg)):
            for s in range(len(ALL)):
                if reg[k, s, 2]:
                    assert reg[k, s, 1] == dense[k, s][reg[k, s, 0]] and reg[k, s, 0] == int(np.argmax(dense[k, s]))


def brute(grid, dim, mask, free_color, through):
    """The seven regions straight from their sentences, one cell at a time: -> bool [8, H, W] (index = code)"""
    H, W = grid.shape
    gh, gw = dim
    B = np.zeros((H, W), bool)
    B[:gh, :gw] = mask[:gh, :gw] != 0
    out = np.zeros((8, H, W), bool)
    if not B.any():
        return out
    xs, ys = np.nonzero(B)
    x0, x1, y0, y1 = xs.min(), xs.max(), ys.min(), ys.max()
    for i in range(gh):
        for j in range(gw):
            near = [(i + a, j + b) for a in (-1, 0, 1) for b in (-1, 0, 1) if (a or b) and 0 <= i + a < gh and 0 <= j + b < gw]
            in_box = x0 <= i <= x1 and y0 <= j <= y1
            if not B[i, j]:
                out[HALO4, i, j] = any(B[p] for p in near if p[0] == i or p[1] == j)
                out[HALO8, i, j] = any(B[p] for p in near)
                out[BOX_REST, i, j] = in_box
                out[BOX_FRAME, i, j] = not in_box and x0 - 1 <= i <= x1 + 1 and y0 - 1 <= j <= y1 + 1
                # INSIDE: a BFS from THIS cell that never meets the edge
                seen, queue, free = {(i, j)}, collections.deque([(i, j)]), False
                while queue and not free:
                    a, b = queue.popleft()
                    if a in (0, gh - 1) or b in (0, gw - 1):
                        free = True
                    for p in ((a - 1, b), (a + 1, b), (a, b - 1), (a, b + 1)):
                        if 0 <= p[0] < gh and 0 <= p[1] < gw and not B[p] and p not in seen:
                            seen.add(p)
                            queue.append(p)
                out[INSIDE, i, j] = not free
            out[BOX, i, j] = in_box
            out[SELF, i, j] = B[i, j]
    keep = B.copy()
    keep[:gh, :gw] |= True if through else (grid[:gh, :gw] == free_color)
    return out & keep


def test_mirror_equals_the_brute_force_on_random_boards():
    rng = np.random.default_rng(11)
    n = 0
    for H, W, gh, gw in ((6, 7, 6, 7), (9, 8, 8, 6), (10, 10, 10, 10), (5, 12, 5, 11)):
        for trial in range(6):
            grid = (rng.integers(0, 4, (H, W)) * (rng.random((H, W)) < 0.55)).astype(np.int8)
            masks = [grid == c for c in (1, 2, 3)] + [rng.random((H, W)) < 0.45, np.zeros((H, W), bool)]
            for through, fc in ((False, 0), (True, 0), (False, 2)):
                cells = S.region_numpy(grid, (gh, gw), grid, (gh, gw), np.stack(masks), range(8), fc, through, full=True)[3]
                for k, m in enumerate(masks):
                    want = brute(grid, (gh, gw), m, fc, through)
                    assert np.array_equal(cells[k], want), (H, W, trial, through, fc, k, np.argwhere((cells[k] != want).any((1, 2))).ravel())
                    n += int(want[INSIDE].any())
    assert n > 10  # (the random boards do enclose something)


def test_halos_boxes_and_frames_on_a_hand_made_grid():
    g = np.zeros((6, 7), np.int8)
    g[2, 2] = g[3, 2] = g[3, 3] = 4  # an L
    reg, best, base, cells = regions_of(g, g == 4)
    assert sorted(np.argwhere(cells[0]).tolist()) == sorted([[1, 2], [2, 1], [2, 3], [3, 1], [3, 4], [4, 2], [4, 3]])
    assert int(cells[1].sum()) == 12 and cells[1][1, 1] and cells[1][4, 4] and cells[1][1, 3] and not cells[1][1, 4]
    assert np.argwhere(cells[2]).tolist() == [[2, 3]] and int(cells[3].sum()) == 12 and not cells[3][2, 3] and cells[3][1, 4]
    assert not cells[4].any() and int(cells[5].sum()) == 4 and np.array_equal(cells[6], g == 4)
    # at the corner everything is clipped to grid_dim; a code above 7 and code 0 are empty candidates, not errors
    reg, best, base, cells = regions_of(g, g == 4, kinds=[HALO8, BOX_FRAME, 0, 9, SELF], dim=(4, 4), adim=(4, 4))
    assert not cells[:, 4:].any() and not cells[:, :, 4:].any() and int(cells[0].sum()) == 6 and int(cells[1].sum()) == 5
    assert reg[2].tolist() == reg[3].tolist() == [0, base[0], 0, 0] and int(cells[4].sum()) == 3


def test_inside_rules():
    g = np.zeros((7, 7), np.int8)
    g[1:6, 1:6] = 5
    g[2:5, 2:5] = 0
    g[3, 3] = 9
    reg, best, base, cells = regions_of(g, g == 5, [INSIDE])
    assert int(cells[0].sum()) == 8 and not cells[0][3, 3]  # the 9 is spared under through = 0 ...
    _, _, _, cells = regions_of(g, g == 5, [INSIDE], through=True)
    assert int(cells[0].sum()) == 9 and cells[0][3, 3]  # ... and covered under through = 1
    _, _, _, cells = regions_of(g, g == 5, [INSIDE], free_color=9)
    assert np.argwhere(cells[0]).tolist() == [[3, 3]]
    # the grid's edge does not close a shape: a ring cut by grid_dim is open
    _, _, _, cells = regions_of(g, g == 5, [INSIDE], dim=(5, 7), adim=(5, 7), through=True)
    assert not cells.any()
    # a gap in the ring opens it; a diagonal gap does not (the flood is 4-connected)
    g2 = g.copy()
    g2[1, 3] = 0
    assert not regions_of(g2, g2 == 5, [INSIDE], through=True)[3].any()
    d = np.zeros((5, 5), np.int8)
    for x, y in ((0, 2), (1, 1), (1, 3), (2, 0), (2, 4), (3, 1), (3, 3), (4, 2)):
        d[x, y] = 2
    assert int(regions_of(d, d == 2, [INSIDE])[3].sum()) == 5


def test_free_filter_spares_the_objects_own_cells_and_tie_rules():
    g = np.full((5, 5), 5, np.int8)
    g[1:4, 1:4] = 2
    g[2, 2] = 0
    reg, best, base, cells = regions_of(g, g == 2, [BOX, SELF, HALO4, BOX_REST], free_color=0)
    assert int(cells[0].sum()) == 9 and int(cells[1].sum()) == 8 and np.argwhere(cells[2]).tolist() == [[2, 2]] and np.argwhere(cells[3]).tolist() == [[2, 2]]
    reg, best, base, cells = regions_of(g, g == 2, [BOX, HALO4], free_color=5)
    assert int(cells[0].sum()) == 8 and int(cells[1].sum()) == 12  # the hole (byte 0) is no longer free
    reg, best, base, cells = regions_of(g, g == 2, [HALO4], free_color=5 + 256)
    assert int(cells[0].sum()) == 12
    # colour ties go to the smaller colour; best: more correct, then fewer cells, then the lower index
    g = np.zeros((3, 5), np.int8)
    g[1, 2] = 1
    ans = g.copy()
    ans[1, 1], ans[1, 3], ans[0, 2], ans[2, 2] = 7, 7, 4, 4
    reg, best, base, _ = regions_of(g, g == 1, [HALO4, HALO8, HALO4], answer=ans, through=True)
    assert reg[0].tolist() == [4, base[0] + 2, 4, 2] and reg[1].tolist() == [0, base[0], 8, 4] and best.tolist() == [0, 4, base[0] + 2, 4]
    reg, best, base, _ = regions_of(g, np.zeros_like(g), ALL, answer=ans)
    assert (reg == np.array([0, base[0], 0, 0])).all() and best.tolist() == [-1, 0, base[0], 0]


def _objs_and_regions(kinds=None):
    cases = [c for c in RG.cases_of(7, 6) if c["dim"].tolist() == [7, 6]]
    grids, dims = np.stack([c["grid"] for c in cases]), np.stack([c["dim"] for c in cases])
    objs = OB.objects_numpy(grids, dims, 6, 0, True, True, True, False)
    regs = RG.region_numpy_rows(grids, dims, np.stack([c["answer"] for c in cases]), np.stack([c["adim"] for c in cases]), objs, kinds, 0, False)
    return cases, objs, regs


def test_region_actions_shapes_padding_and_drop_rule():
    cases, objs, regs = _objs_and_regions()
    assert isinstance(regs, Regions) and Regions._fields == ("color", "correct", "cells", "right", "best_kind", "best_color", "best_correct", "best_cells", "best_bits", "base")
    M, C = len(cases), 6
    assert tuple(regs.color.shape) == (M, C, 7) and tuple(regs.best_kind.shape) == (M, C) and tuple(regs.best_bits.shape) == (M, C, 128)
    ops = [40 + c for c in range(10)]
    act = S.region_actions(objs, regs, ops)
    assert set(act) == {"bits", "operation"} and tuple(act["bits"].shape) == (M, C, 128) and act["bits"].dtype == torch.uint8
    assert tuple(act["operation"].shape) == (M, C) and act["operation"].dtype == torch.int32
    real = 0
    for m in range(M):
        for k in range(C):
            if k >= int(objs.count[m]) or int(regs.best_kind[m, k]) < 0 or int(regs.best_correct[m, k]) <= int(regs.base[m, 0]):
                assert int(act["operation"][m, k]) == -1 and not act["bits"][m, k].any(), (m, k)
                continue
            real += 1
            assert int(act["operation"][m, k]) == 40 + int(regs.best_color[m, k]) and torch.equal(act["bits"][m, k], regs.best_bits[m, k])
            assert int(S.unpack_bits(act["bits"][m, k], 7, 6).sum()) == int(regs.best_cells[m, k]) > 0
    assert 2 <= real < M * C


def test_propose_regions_singles_first_then_the_regions():
    inputs, dims, answers, depths, kinds = RG.planted_region_tasks(3)
    rows = torch.from_numpy(CP.clean_rows("o2arc", inputs, dims, answers, dims)[0])
    venv = RG.region_venv(answers, dims)
    prop = S.propose_regions(range(10), through=True, box_ops=[3, 25], seed_ops=[12], max_components=8)
    assert prop.wants_src is True
    cand = prop(venv, rows, torch.arange(3, dtype=torch.int32))
    objs = venv.components(rows, max_components=8, skip_color=0, bits=True)
    single = S.object_actions(objs, [3, 25], [12], masks=True)
    K1 = 8 * 3
    assert set(cand) == {"bits", "operation"} and tuple(cand["bits"].shape) == (3, K1 + 8, 128) and tuple(cand["operation"].shape) == (3, K1 + 8)
    assert torch.equal(cand["bits"][:, :K1], single["bits"]) and torch.equal(cand["operation"][:, :K1], single["operation"])
    for i in range(3):
        n = int(objs.count[i])
        assert bool((cand["operation"][i, K1 + n:] == -1).all()) and not cand["bits"][i, K1 + n:].any()
        planted = [k for k in range(n) if int(objs.color[i, k]) != 9]
        assert len(planted) == depths[i] and all(int(cand["operation"][i, K1 + k]) in (7, 8) for k in planted)  # Color <the answer's paint>
    only = S.propose_regions(range(10), through=True, max_components=8)(venv, rows, None)
    assert all(torch.equal(only[k], cand[k][:, K1:]) for k in only)
    none = S.propose_regions(range(10), kinds=[0, 0], max_components=8)(venv, rows, None)
    assert bool((none["operation"] == -1).all()) and not none["bits"].any()


def test_the_planted_tasks_follow_their_rule():
    inputs, dims, answers, depths, kinds = RG.planted_region_tasks(8)
    assert sorted(kinds) == sorted([HALO8, HALO8, HALO4, HALO4, INSIDE, INSIDE, BOX_REST, BOX_FRAME]) and set(depths) == {1, 2, 3}
    again = RG.planted_region_tasks(8)
    assert np.array_equal(again[0], inputs) and np.array_equal(again[2], answers)  # fixed by the seed
    for g, a, n, kind in zip(inputs, answers, depths, kinds):
        cnt, _, comp, masks = S.components_numpy(g, (12, 12), 16, 0)
        planted = [k for k in range(cnt) if comp[k][6] != 9]
        assert len(planted) == n and ((g != 0) <= (a != 0)).all()
        for k in planted:
            x0, y0, x1, y1 = (int(v) for v in comp[k][:4])
            assert x0 >= RG.GAP and y0 >= RG.GAP and x1 < 12 - RG.GAP and y1 < 12 - RG.GAP
            grown = np.zeros((12, 12), bool)
            grown[x0 - RG.GAP:x1 + 1 + RG.GAP, y0 - RG.GAP:y1 + 1 + RG.GAP] = True
            box = np.zeros((12, 12), bool)
            box[x0:x1 + 1, y0:y1 + 1] = True
            assert not ((g != 0) & grown & ~box).any()  # at least GAP free cells to anything else
        assert int(((a != g)).sum()) >= 4 * n
        assert ((kind == INSIDE) == bool((g == 9).any())) and (kind != INSIDE or 1 <= int((g == 9).sum()) <= 2) and not (a == 9).any()


def test_beam_search_paints_the_planted_regions():
    """Eight planted 12 x 12 tasks — 1 to 3 objects whose 8-halo, 4-halo, inside, box rest or box frame the answer paints:
    propose_regions(range(10), through=True) at width 1 and depth = the number of objects solves all eight, one Color step per object,
    and the steps replay to the answer on the oracle.  The seven proposers the library had (objects with the Colour ops among their box
    ops, placements, stamps, turns, alignments, rays, mirrors) solve RG.BEFORE_SOLVES = 0 at the same width and depth."""
    inputs, dims, answers, depths, kinds = RG.planted_region_tasks(8)
    rows_np = CP.clean_rows("o2arc", inputs, dims, answers, dims)[0]
    rows = torch.from_numpy(rows_np)
    venv = RG.region_venv(answers, dims)
    painted, before = RG.searches(venv, rows, 8, depths)
    solved = {name: sum(r.sequence is not None for r in res) for name, res in before.items()}
    print("planted region tasks: propose_regions solves", sum(r.sequence is not None for r in painted), "of 8; the earlier proposers:", solved)
    assert sum(r.sequence is not None for r in painted) == 8
    assert set(before) == {"objects", "placements", "stamps", "turns", "alignments", "rays", "mirrors"}
    assert sum(solved.values()) == RG.BEFORE_SOLVES == 0, solved
    for i, r in enumerate(painted):
        assert r.root == 0 and len(r.sequence) == depths[i], i
        assert all(op in (7, 8) for _, op in r.sequence), i
        assert AL.replay_on_oracle(rows_np[i], answers[i], dims[i], r.sequence) == 1, i
