"""The host side of arcle_turn_rows: turn_numpy against the oracle's own select + turn + Moves (which settles the rule for the corner
at which a quarter turn leaves an object), the max_dist cut and the tie rule, turn_macros / propose_turns on an oracle-backed stub vec
env (torch CPU tensors; no GPU), and the search demonstration: planted tasks whose one object is turned and moved."""
import numpy as np
import pytest
import torch

import components as CP
import objects as OB
import turn as TU
from arcle_amd import search as S
from arcle_amd.envs.vec import Turns


@pytest.mark.parametrize("H,W", TU.ORACLE_SIZES)
def test_mirror_equals_the_oracle(H, W):
    """The whole correct(t, dx, dy) table of turn_numpy(full=True) against the chained oracle (mask ingress, the table with
    gen_rotate(2) appended) running select + turn + |dx| vertical + |dy| horizontal Moves, for EVERY candidate of every object of every
    case; at least 100 candidates per turn, so that no turn is silently empty; `turn` is the table's arg-max under the tie rule and
    `base` the dense pair of the grid."""
    per = np.zeros(5, np.int64)
    for c in TU.cases_of(H, W):
        want, got, cand = TU.oracle_table(c)
        assert np.array_equal(want, got), (c["name"], cand[want != got][:3].tolist(), want[want != got][:3].tolist(), got[want != got][:3].tolist())
        per += np.bincount(cand[:, 0], minlength=5) if len(cand) else 0
        turn, base, table = S.turn_numpy(c["grid"], c["dim"], c["answer"], c["adim"], c["masks"], None, TU.ALL, full=True)
        gh, gw = int(c["dim"][0]), int(c["dim"][1])
        assert base[0] == int((c["grid"][:min(gh, c["adim"][0]), :min(gw, c["adim"][1])] == c["answer"][:min(gh, c["adim"][0]), :min(gw, c["adim"][1])]).sum())
        for k, m in enumerate(c["masks"]):
            for t in range(5):
                cd = np.argwhere(table[k, t] >= 0) - (H - 1, W - 1)
                if not (m[:gh, :gw] != 0).any():
                    assert turn[k, t].tolist() == [0, 0, base[0], 1] and not len(cd)
                elif not len(cd):
                    assert turn[k, t].tolist() == [0, 0, 0, 0]
                else:
                    best = min((-int(table[k, t, dx + H - 1, dy + W - 1]), abs(dx) + abs(dy), dx, dy) for dx, dy in cd.tolist())
                    assert turn[k, t].tolist() == [best[2], best[3], -best[0], 1], (c["name"], k, t)
    assert (per >= 100).all(), per


def test_unrequested_turns_stay_zero_and_requested_ones_do_not_change():
    c = [c for c in TU.cases_of(7, 6) if c["name"].endswith("moved")][0]
    full, base = S.turn_numpy(c["grid"], c["dim"], c["answer"], c["adim"], c["masks"], 3)
    for turns in (1, 2, 4, 8, 16, 21):
        part, b = S.turn_numpy(c["grid"], c["dim"], c["answer"], c["adim"], c["masks"], 3, turns)
        asked = np.array([(turns >> t) & 1 for t in range(5)], bool)
        assert b == base and np.array_equal(part[:, asked], full[:, asked]) and not part[:, ~asked].any()


def test_max_dist_cuts_the_candidates_to_the_diamond():
    for c in [c for c in TU.cases_of(7, 6) if c["name"].endswith(("moved", "over left", "parity 2x3"))]:
        _, _, full = S.turn_numpy(c["grid"], c["dim"], c["answer"], c["adim"], c["masks"], None, TU.ALL, full=True)
        dx, dy = np.mgrid[-6:7, -5:6]
        for D in (0, 1, 3):
            turn, _, table = S.turn_numpy(c["grid"], c["dim"], c["answer"], c["adim"], c["masks"], D, TU.ALL, full=True)
            assert np.array_equal(table, np.where((abs(dx) + abs(dy) <= D)[None, None], full, -1))
            for k in range(len(c["masks"])):
                for t in range(5):
                    if (table[k, t] >= 0).any():
                        assert turn[k, t, 3] == 1 and turn[k, t, 2] == table[k, t].max() == table[k, t, turn[k, t, 0] + 6, turn[k, t, 1] + 5]
                    elif c["masks"][k].any():
                        assert turn[k, t].tolist() == [0, 0, 0, 0]
    over = [c for c in TU.cases_of(7, 6) if c["name"].endswith("over left")][0]
    t0, _ = S.turn_numpy(over["grid"], over["dim"], over["answer"], over["adim"], over["masks"], 0)
    assert t0[0, :, 3].tolist() == [0, 1, 0, 1, 1]  # (the quarter turns leave the line hanging over the edge: no candidate within 0 Moves)


def test_the_tie_rule_level_by_level():
    """One-cell object at the centre (every turn leaves it there), two equally good cells in the answer: the nearer wins, then the
    smaller dx, then the smaller dy."""
    seen = set()
    for H, W in ((7, 6), (30, 30), (16, 33)):
        for c in TU.cases_of(H, W):
            name = c["name"].split(" ", 1)[1]
            if name in TU.TIE_WANT:
                turn, _, table = S.turn_numpy(c["grid"], c["dim"], c["answer"], c["adim"], c["masks"], None, TU.ALL, full=True)
                for t in range(5):
                    assert (int(turn[0, t, 0]), int(turn[0, t, 1])) == TU.TIE_WANT[name], (c["name"], t, turn[0, t])
                    assert (table[0, t] == turn[0, t, 2]).sum() == 2, c["name"]  # two translations score the best count
                seen.add(name)
    assert seen == set(TU.TIE_WANT)


def _objs_and_turns(max_dist=None, turns=TU.ALL):
    cases = [c for c in TU.cases_of(7, 6) if c["dim"].tolist() == [7, 6]]
    grids, dims = np.stack([c["grid"] for c in cases]), np.stack([c["dim"] for c in cases])
    objs = OB.objects_numpy(grids, dims, 6, 0, True, True, True, False)
    tn = TU.turn_numpy_rows(grids, dims, np.stack([c["answer"] for c in cases]), np.stack([c["adim"] for c in cases]), objs, max_dist, turns)
    return cases, objs, tn


def test_turn_macros_shapes_padding_and_drop_rule():
    cases, objs, tn = _objs_and_turns()
    assert isinstance(tn, Turns) and Turns._fields == ("dx", "dy", "correct", "valid", "base")
    M, C, T = len(cases), 6, 6
    assert tuple(tn.dx.shape) == (M, C, 5) and tuple(tn.base.shape) == (M, 2)
    up, down, right, left = TU.MOVE_OPS
    real = dropped_long = rot180 = 0
    for turn_ops in (TU.TURN_OPS, TU.TURN_OPS_ALL):
        mac = S.turn_macros(objs, tn, turn_ops, TU.MOVE_OPS, T)
        assert tuple(mac["bits"].shape) == (M, C, T, 128) and mac["bits"].dtype == torch.uint8
        assert tuple(mac["operation"].shape) == (M, C, T) and mac["operation"].dtype == torch.int32
        assert tuple(mac["length"].shape) == (M, C) and mac["length"].dtype == torch.int32
        for m in range(M):
            for k in range(C):
                usable = [t for t in range(5) if int(tn.valid[m, k, t]) and turn_ops[t] >= 0]
                best = min(((-int(tn.correct[m, k, t]), abs(int(tn.dx[m, k, t])) + abs(int(tn.dy[m, k, t])), t) for t in usable), default=None)
                ops, ln = mac["operation"][m, k].tolist(), int(mac["length"][m, k])
                if k >= int(objs.count[m]) or best is None or -best[0] <= int(tn.base[m, 0]) or 1 + best[1] > T:
                    assert ops == [-1] * T and ln == 1 and not mac["bits"][m, k].any(), (m, k)
                    dropped_long += best is not None and k < int(objs.count[m]) and -best[0] > int(tn.base[m, 0])
                    continue
                real += 1
                t = best[2]
                rot180 += t == 1
                dx, dy = int(tn.dx[m, k, t]), int(tn.dy[m, k, t])
                want = [turn_ops[t]] + [up if dx < 0 else down] * abs(dx) + [right if dy > 0 else left] * abs(dy)
                assert ln == len(want) and ops == want + [-1] * (T - ln), (m, k, ops, want)
                assert torch.equal(mac["bits"][m, k, 0], objs.bits[m, k]) and not mac["bits"][m, k, 1:].any()
    assert real >= 8 and dropped_long >= 1 and rot180 >= 1, (real, dropped_long, rot180)


def test_propose_turns_singles_first_then_the_macros():
    inputs, dims, answers, plans = TU.planted_turn_tasks(3)
    rows = torch.from_numpy(CP.clean_rows("o2arc", inputs, dims, answers, dims)[0])
    venv = TU.turn_venv(answers, dims)
    asked = []
    inner = venv.turn
    venv.turn = lambda rows, objs, src_env=None, max_dist=8, turns=31: (asked.append((max_dist, turns)), inner(rows, objs, src_env, max_dist, turns))[1]
    prop = S.propose_turns(TU.TURN_OPS_ALL, TU.MOVE_OPS, box_ops=[3, 29], seed_ops=[12], max_dist=4, max_components=4, any_color=True, diagonal=True)
    assert prop.wants_src is True
    cand = prop(venv, rows, torch.arange(3, dtype=torch.int32))
    objs = venv.objects(rows, max_components=4, skip_color=0, any_color=True, diagonal=True, bits=True)
    single = S.object_actions(objs, [3, 29], [12], masks=True)
    K1, T = 4 * 3, 5
    assert tuple(cand["bits"].shape) == (3, K1 + 4, T, 128) and tuple(cand["operation"].shape) == (3, K1 + 4, T) and tuple(cand["length"].shape) == (3, K1 + 4)
    assert torch.equal(cand["bits"][:, :K1, 0], single["bits"]) and torch.equal(cand["operation"][:, :K1, 0], single["operation"])
    assert bool((cand["operation"][:, :K1, 1:] == -1).all()) and bool((cand["length"][:, :K1] == 1).all()) and not cand["bits"][:, :K1, 1:].any()
    for i, (t, dx, dy) in enumerate(plans):  # the one object's macro is the planted turn and its Moves
        assert int(cand["length"][i, K1]) == 1 + abs(dx) + abs(dy) and int(cand["operation"][i, K1, 0]) == TU.TURN_OPS_ALL[t]
        assert bool((cand["operation"][i, K1 + 1:, 0] == -1).all())
    only = S.propose_turns(TU.TURN_OPS_ALL, TU.MOVE_OPS, max_dist=4, max_components=4, any_color=True, diagonal=True)(venv, rows, None)
    assert all(torch.equal(only[k], cand[k][:, K1:]) for k in only)
    S.propose_turns(TU.TURN_OPS, TU.MOVE_OPS, max_components=4, any_color=True, diagonal=True)(venv, rows, None)
    assert asked == [(4, 31), (4, 31), (8, 29)]  # only the turns that have an op are asked for; max_dist is passed on


def test_beam_search_turns_and_moves_in_one_candidate():
    """Eight planted 12 x 12 tasks, one two-colour L-tetromino (no symmetry: no translation of it equals any turn of it) turned — every
    one of the five turns at least once — and moved 0 to 4 cells from where the turn leaves it: propose_turns at width 1 and depth 1
    solves all eight and the primitive steps it returns — the turn on the object's cells, then Moves on the empty selection — replay to
    the answer on the oracle; propose_placements at the same width and depth solves TU.BEFORE_SOLVES of them."""
    inputs, dims, answers, plans = TU.planted_turn_tasks(8)
    assert {t for t, _, _ in plans} == set(range(5)) and {abs(dx) + abs(dy) for _, dx, dy in plans} == {0, 1, 2, 3, 4}
    rows = torch.from_numpy(CP.clean_rows("o2arc", inputs, dims, answers, dims)[0])
    venv = TU.turn_venv(answers, dims)
    before, turned = TU.turn_searches(venv, rows, 8)
    assert sum(r.sequence is not None for r in turned) == 8
    assert sum(r.sequence is not None for r in before) == TU.BEFORE_SOLVES < 8
    for i, (r, (t, dx, dy)) in enumerate(zip(turned, plans)):
        assert r.root == 0 and len(r.sequence) == 1 + abs(dx) + abs(dy) and r.sequence[0][1] == TU.TURN_OPS_ALL[t], (i, [op for _, op in r.sequence])
        assert r.sequence[0][0].sum() == 4 and not any(sel.any() for sel, _ in r.sequence[1:])
        assert TU.replay_on_oracle(inputs[i], dims[i], answers[i], r.sequence) == 1, i
