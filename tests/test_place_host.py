"""The host side of arcle_place_rows: place_numpy against the oracle's own Moves (select the object, Move |dx| + |dy| times, count the
correct cells), the tie rule, placement_macros / propose_placements on an oracle-backed stub vec env (torch CPU tensors; no GPU), and
the search demonstration: planted tasks whose one object sits 5 to 8 cells from its place."""
import numpy as np
import pytest
import torch

import components as CP
import objects as OB
import place as PL
import search_bits as SB
from arcle_amd import search as S
from arcle_amd.envs.vec import Placements


@pytest.mark.parametrize("H,W", PL.ORACLE_SIZES)
def test_mirror_equals_the_oracle(H, W):
    """The whole correct(dx, dy) table of place_numpy(full=True) against the chained oracle: every translation of T at 5 x 5 and 7 x 6, a
    random tenth of them (for the first four objects of every case) at 30 x 30; and `place` is the table's arg-max under the tie rule,
    `base` the dense pair of the grid."""
    rng = np.random.default_rng(H * 100 + W)
    total = 0
    for c in PL.cases_of(H, W):
        pick = (lambda k, cand: cand) if H < 30 else (lambda k, cand: cand[rng.random(len(cand)) < 0.1] if k < 4 else cand[:0])
        got, grid, table = PL.oracle_table(c, pick)
        place, base = S.place_numpy(grid, c["dim"], c["answer"], c["adim"], c["masks"])
        for k, res in enumerate(got):
            for (dx, dy), v in res.items():
                assert table[k, dx + H - 1, dy + W - 1] == v, (c["name"], k, dx, dy)
            total += len(res)
            cand = np.argwhere(table[k] >= 0) - (H - 1, W - 1)
            best = min((-int(table[k, dx + H - 1, dy + W - 1]), abs(dx) + abs(dy), dx, dy) for dx, dy in cand.tolist())
            assert place[k].tolist() == [best[2], best[3], -best[0], int(table[k, H - 1, W - 1])], (c["name"], k)
        gh, gw, ah, aw = int(c["dim"][0]), int(c["dim"][1]), int(c["adim"][0]), int(c["adim"][1])
        mh, mw = min(gh, ah), min(gw, aw)
        assert base == (int((grid[:mh, :mw] == c["answer"][:mh, :mw]).sum()),
                        mh * mw + (abs(ah * aw - gh * gw) if (gh <= ah) == (gw <= aw) else abs(gh - ah) * mw + abs(gw - aw) * mh)), c["name"]
    assert total > 300, total


def test_the_cases_are_what_the_issue_lists():
    for H, W in PL.ORACLE_SIZES + ((20, 7), (16, 33)):
        by = {c["name"].split(" ", 1)[1].split(" grid")[0]: c for c in PL.cases_of(H, W)}
        a, b = by["shrunk a"], by["shrunk b"]
        for c in (a, b):
            assert c["dim"][0] < H and c["dim"][1] < W and c["masks"][:, c["dim"][0]:].any()  # grid_dim below (H, W), mask cells outside it
        assert a["adim"][0] > a["dim"][0] and a["adim"][1] < a["dim"][1] and b["adim"][0] < b["dim"][0] and b["adim"][1] > b["dim"][1]
        two = by["twocolour"]
        assert len(np.unique(two["grid"][two["masks"][0] != 0])) == 2
        byt = by["bytes"]
        assert byt["masks"][0].all() and not byt["masks"][1].any()  # the whole grid (T = {(0, 0)}); an empty bit row
        assert any((byt["grid"][m != 0] < 0).any() and (byt["grid"][m != 0] == 0).any() for m in byt["masks"][2:])  # bytes <= 0 in an object
        place, base, table = S.place_numpy(byt["grid"], byt["dim"], byt["answer"], byt["adim"], byt["masks"][:2], full=True)
        assert (table[0] >= 0).sum() == 1 and (table[1] >= 0).sum() == 1 and place[1].tolist() == [0, 0, base[0], base[0]]
        assert any(n.startswith("tie") for n in by)


def test_the_tie_rule_level_by_level():
    """One-cell object at the centre, two equally good cells in the answer: the nearer wins, then the smaller dx, then the smaller dy."""
    want = {"tie dx": (-1, 0), "tie dy": (0, -1), "tie distance": (1, 0), "tie distance y": (0, 1), "tie dx before dy": (-1, 0),
            "tie dx before dy 2": (0, 1), "tie diagonal": (-1, 1)}
    seen = set()
    for H, W in ((7, 6), (30, 30), (16, 33)):
        for c in PL.cases_of(H, W):
            name = c["name"].split(" ", 1)[1]
            if name in want:
                place, _, table = S.place_numpy(c["grid"], c["dim"], c["answer"], c["adim"], c["masks"], full=True)
                assert tuple(place[0, :2]) == want[name], (c["name"], place[0])
                assert (table[0] == place[0, 2]).sum() == 2, c["name"]  # two placements score the best count
                seen.add(name)
    assert seen == set(want)
    c = [c for c in PL.cases_of(7, 6) if c["name"].endswith("tie distance")][0]
    assert tuple(S.place_numpy(c["grid"], c["dim"], c["answer"], c["adim"], c["masks"], max_dist=0)[0][0, :2]) == (0, 0)


def _objs_and_places():
    cases = [c for c in PL.cases_of(7, 6) if c["dim"].tolist() == [7, 6]]
    grids, dims = np.stack([c["grid"] for c in cases]), np.stack([c["dim"] for c in cases])
    objs = OB.objects_numpy(grids, dims, 6, 0, True, True, True, False)
    pl = PL.place_numpy_rows(grids, dims, np.stack([c["answer"] for c in cases]), np.stack([c["adim"] for c in cases]), objs, None)
    return cases, objs, pl


def test_placement_macros_shapes_padding_and_step_order():
    cases, objs, pl = _objs_and_places()
    assert isinstance(pl, Placements) and Placements._fields == ("dx", "dy", "correct", "stay", "base")
    M, C, T = len(cases), 6, 4
    up, down, right, left = PL.MOVE_OPS
    mac = S.placement_macros(objs, pl, PL.MOVE_OPS, T)
    assert tuple(mac["bits"].shape) == (M, C, T, 128) and mac["bits"].dtype == torch.uint8
    assert tuple(mac["operation"].shape) == (M, C, T) and mac["operation"].dtype == torch.int32
    assert tuple(mac["length"].shape) == (M, C) and mac["length"].dtype == torch.int32
    real = 0
    for m in range(M):
        for k in range(C):
            dx, dy, cor, stay = (int(getattr(pl, f)[m, k]) for f in ("dx", "dy", "correct", "stay"))
            ops, ln = mac["operation"][m, k].tolist(), int(mac["length"][m, k])
            if k >= int(objs.count[m]) or (dx, dy) == (0, 0) or cor <= stay or abs(dx) + abs(dy) > T:
                assert ops[0] == -1 and ln == 1 and not mac["bits"][m, k].any(), (m, k)
                continue
            real += 1
            assert ln == abs(dx) + abs(dy)
            assert ops[:abs(dx)] == [up if dx < 0 else down] * abs(dx) and ops[abs(dx):ln] == [right if dy > 0 else left] * abs(dy)
            assert all(o == -1 for o in ops[ln:])
            assert torch.equal(mac["bits"][m, k, 0], objs.bits[m, k]) and not mac["bits"][m, k, 1:].any()
    assert real >= 4
    far = S.placement_macros(objs, pl, PL.MOVE_OPS, 1)  # T = 1: every farther placement is padding
    assert int((far["operation"][:, :, 0] >= 0).sum()) == int((((pl.dx.abs() + pl.dy.abs()) == 1) & (pl.correct > pl.stay)).sum())


def test_propose_placements_singles_first_then_the_macros():
    inputs, dims, answers, moves = PL.planted_far_tasks(3)
    rows = torch.from_numpy(CP.clean_rows("o2arc", inputs, dims, answers, dims)[0])
    venv = PL.place_venv(answers, dims)
    prop = S.propose_placements(PL.MOVE_OPS, box_ops=[3, 25], seed_ops=[12], max_dist=8, max_components=4, any_color=True, diagonal=True)
    assert prop.wants_src is True
    cand = prop(venv, rows, torch.arange(3, dtype=torch.int32))
    objs = venv.objects(rows, max_components=4, skip_color=0, any_color=True, diagonal=True, bits=True)
    single = S.object_actions(objs, [3, 25], [12], masks=True)
    K1 = 4 * 3
    assert tuple(cand["bits"].shape) == (3, K1 + 4, 8, 128) and tuple(cand["operation"].shape) == (3, K1 + 4, 8) and tuple(cand["length"].shape) == (3, K1 + 4)
    assert torch.equal(cand["bits"][:, :K1, 0], single["bits"]) and torch.equal(cand["operation"][:, :K1, 0], single["operation"])
    assert bool((cand["operation"][:, :K1, 1:] == -1).all()) and bool((cand["length"][:, :K1] == 1).all()) and not cand["bits"][:, :K1, 1:].any()
    for i, (dx, dy) in enumerate(moves):  # the one object's macro is the planted move
        assert int(cand["length"][i, K1]) == abs(dx) + abs(dy) and bool((cand["operation"][i, K1 + 1:, 0] == -1).all())
    only = S.propose_placements(PL.MOVE_OPS, max_components=4, any_color=True, diagonal=True)(venv, rows, None)
    assert all(torch.equal(only[k], cand[k][:, K1:]) for k in only)


def test_an_existing_proposer_still_receives_two_arguments():
    inputs, dims, answers, _ = PL.planted_far_tasks(2)
    rows = torch.from_numpy(CP.clean_rows("o2arc", inputs, dims, answers, dims)[0])
    venv = PL.place_venv(answers, dims)
    calls = []
    inner = S.propose_objects(list(PL.MOVE_OPS), [], masks=True, any_color=True, diagonal=True)

    def old(*args):
        calls.append(len(args))
        return inner(*args)
    S.beam_search(venv, rows[:1], None, width=1, depth=2, propose=old)
    new_inner = S.propose_placements(PL.MOVE_OPS, any_color=True, diagonal=True)

    def new(*args):
        calls.append(len(args))
        assert args[2].dtype == torch.int32 and args[2].tolist() == [1]
        return new_inner(*args)
    new.wants_src = True
    r = S.beam_search(venv, rows[1:2], None, width=1, depth=1, src_env=torch.tensor([1]), propose=new)
    assert calls == [2, 2, 3] and r.sequence is not None


def test_beam_search_places_far_objects_in_one_depth():
    """Eight planted 12 x 12 tasks, one diagonal line 5 to 8 cells from its place: propose_placements at width 1, depth 1 solves all
    eight and the primitive steps it returns replay to the answer on the oracle; the single-step beam on the same objects' exact
    cells, width 1 and depth = the distance, solves PL.SINGLE_STEP_SOLVES of them (no one-cell shift overlaps the target: the first
    moves score alike and the width cut keeps the lowest child index)."""
    inputs, dims, answers, moves = PL.planted_far_tasks(8)
    assert all(5 <= abs(dx) + abs(dy) <= 8 and dx and dy for dx, dy in moves)
    rows = torch.from_numpy(CP.clean_rows("o2arc", inputs, dims, answers, dims)[0])
    venv = PL.place_venv(answers, dims)
    single, placed = PL.placement_searches(venv, rows, 8, [abs(dx) + abs(dy) for dx, dy in moves])
    assert sum(r.sequence is not None for r in placed) == 8
    assert sum(r.sequence is not None for r in single) == PL.SINGLE_STEP_SOLVES < 8
    up, down, right, left = PL.MOVE_OPS
    for i, (r, (dx, dy)) in enumerate(zip(placed, moves)):
        assert r.root == 0 and [op for _, op in r.sequence] == [up if dx < 0 else down] * abs(dx) + [right if dy > 0 else left] * abs(dy), i
        assert np.array_equal(r.sequence[0][0], inputs[i] != 0) and not any(sel.any() for sel, _ in r.sequence[1:]), i
        assert SB.replay_masks_on_oracle(inputs[i], dims[i], answers[i], r.sequence) == 1, i
