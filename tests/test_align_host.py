"""The host side of arcle_align_rows: align_numpy against the oracle's own Copy + resize_grid + Paste for every offset (which pins the
closed form: the child's grid, its grid_dim and its dense pair), the max_dist cut and the unrequested sources, align_macros replayed
step by step on the oracle, propose_alignments' padding rules on an oracle-backed stub vec env (torch CPU tensors; no GPU), and the
search demonstration: planted tasks whose answer has another size than the grid."""
import numpy as np
import pytest
import torch

import align as AL
import macros as MC
import search_bits as SB
from arcle_amd import search as S
from arcle_amd.envs.vec import Alignments


@pytest.mark.parametrize("H,W", AL.ORACLE_SIZES)
def test_mirror_equals_the_oracle(H, W):
    """EVERY candidate (source, ox, oy) of every case as the three-step macro [Copy_src on R, resize_grid on the canvas rectangle, Paste
    on P] on the chained oracle, O2ARC and ARC tables, both Pastes: the grid it leaves is the mirror's child on the whole plane, its
    grid_dim is the answer's dims, its dense pair is (the mirror's count, ah * aw); `align` is the table's arg-max under the tie rule."""
    seen = {0: 0, 1: 0}
    for kind in ("o2arc", "arc"):
        for blank in (True, False):
            for c in AL.cases_of(H, W):
                ah, aw = int(c["adim"][0]), int(c["adim"][1])
                for cand, grid, gdim, dense, child, count in AL.oracle_children(c, kind, blank):
                    assert np.array_equal(grid, child), (c["name"], kind, blank, cand)
                    assert gdim.tolist() == [ah, aw] and dense.tolist() == [count, ah * aw], (c["name"], kind, blank, cand, gdim, dense, count)
                    seen[cand[0]] += 1
                al, base, table, _ = S.align_numpy(c["grid"], c["dim"], c["inp"], c["idim"], c["answer"], c["adim"], None, 3, blank, full=True)
                for s in range(2):
                    cd = np.argwhere(table[s] >= 0) - (H - 1, W - 1)
                    if not len(cd):
                        assert al[s, :4].tolist() == [0, 0, 0, 0]
                    else:
                        best = min((-int(table[s, ox + H - 1, oy + W - 1]), abs(ox) + abs(oy), ox, oy) for ox, oy in cd.tolist())
                        assert al[s, :4].tolist() == [best[2], best[3], -best[0], ah * aw], (c["name"], s)
    assert min(seen.values()) >= 1000, seen


def test_unrequested_sources_stay_zero_and_max_dist_cuts_to_the_diamond():
    H, W = 7, 6
    ox, oy = np.mgrid[-(H - 1):H, -(W - 1):W]
    for c in AL.cases_of(H, W):
        args = (c["grid"], c["dim"], c["inp"], c["idim"], c["answer"], c["adim"])
        both, base, full, _ = S.align_numpy(*args, None, 3, True, full=True)
        for sources in (1, 2):
            part, b = S.align_numpy(*args, None, sources, True)
            assert b == base and np.array_equal(part[sources - 1], both[sources - 1]) and not part[2 - sources].any()
        for D in (0, 1, 3):
            al, _, table, _ = S.align_numpy(*args, D, 3, True, full=True)
            assert np.array_equal(table, np.where((abs(ox) + abs(oy) <= D)[None], full, -1))
            for s in range(2):
                if (table[s] >= 0).any():
                    assert al[s, 2] == table[s].max() == table[s, al[s, 0] + H - 1, al[s, 1] + W - 1] and abs(al[s, 0]) + abs(al[s, 1]) <= D


def _stub(H, W, cases, blank=True, sources=3):
    rows = np.concatenate([AL.case_rows(c) for c in cases])
    answers, adims = np.stack([c["answer"] for c in cases]), np.stack([c["adim"] for c in cases])
    venv = AL.align_venv(answers, adims, H, W)
    return rows, answers, adims, venv, venv.align(torch.from_numpy(rows), None, None, sources, blank)


def test_align_macros_replayed_step_by_step_on_the_oracle():
    """The three steps of every macro align_macros builds, one oracle step at a time: the child is the one the mirror names (its count
    and total are the slot's), and a dropped slot is operation -1 at step 0, length 1 and zero bits."""
    H, W = 7, 6
    cases = AL.cases_of(H, W)
    real = dropped = 0
    for blank in (True, False):
        rows, answers, adims, venv, al = _stub(H, W, cases, blank)
        assert isinstance(al, Alignments) and Alignments._fields == ("ox", "oy", "correct", "total", "src_dim", "ans_dim", "base")
        M = len(cases)
        assert tuple(al.ox.shape) == (M, 2) and tuple(al.src_dim.shape) == (M, 2, 2) and tuple(al.ans_dim.shape) == (M, 2, 2) and tuple(al.base.shape) == (M, 2)
        copy_ops, resize_op, paste_op = AL.ALIGN_OPS["o2arc"]
        mac = S.align_macros(al, copy_ops, resize_op, paste_op, H, W)
        assert tuple(mac["bits"].shape) == (M, 2, 3, 128) and mac["bits"].dtype == torch.uint8
        assert tuple(mac["operation"].shape) == (M, 2, 3) and mac["operation"].dtype == torch.int32
        assert tuple(mac["length"].shape) == (M, 2) and mac["length"].dtype == torch.int32
        masks = S.unpack_bits(mac["bits"], H, W).numpy().astype(np.int8)
        for m, c in enumerate(cases):
            bc, bt = int(al.base[m, 0]), int(al.base[m, 1])
            for s in range(2):
                cor, tot = int(al.correct[m, s]), int(al.total[m, s])
                ops, ln = mac["operation"][m, s].tolist(), int(mac["length"][m, s])
                if tot == 0 or cor * bt <= bc * tot:
                    assert ops == [-1, -1, -1] and ln == 1 and not mac["bits"][m, s].any(), (c["name"], s)
                    dropped += 1
                    continue
                real += 1
                assert ops == [copy_ops[s], resize_op, paste_op] and ln == 3
                ox, oy = int(al.ox[m, s]), int(al.oy[m, s])
                assert masks[m, s, 1].sum() == tot and masks[m, s, 2].sum() == 1 and masks[m, s, 2][max(-ox, 0), max(-oy, 0)] == 1
                cur = rows[m:m + 1]
                for t in range(3):
                    cur, _, _, st, dense = MC.oracle_step_rows(cur, answers[m:m + 1], adims[m:m + 1], "o2arc", H, W, 3, AL.ops_for("o2arc", blank), "mask",
                                                               masks[m, s, t].reshape(1, -1), np.array([ops[t]], np.int32))
                    assert not st.any(), (c["name"], s, t)
                grid, gdim = SB._grids_of(cur, "o2arc", H, W)
                sh, sw = (int(v) for v in al.src_dim[m, s])
                want = AL.child_of(c["inp"] if s else c["grid"], sh, sw, int(c["adim"][0]), int(c["adim"][1]), ox, oy, blank)
                assert np.array_equal(grid[0], want) and gdim[0].tolist() == c["adim"].tolist() and dense[0].tolist() == [cor, tot], (c["name"], s)
    assert real >= 20 and dropped >= 8, (real, dropped)


def test_the_identity_is_dropped():
    """A row whose grid already has the answer's dims and is its own best fit at (0, 0): the grid's macro does not beat the row's own
    ratio and is padding; the input's macro stays if it scores more."""
    H, W = 7, 6
    g = np.random.default_rng(3).integers(1, 10, (H, W)).astype(np.int8)
    a = g.copy()
    a[0, 0] = 0
    case = {"name": "identity", "H": H, "W": W, "grid": g, "dim": np.array((H, W), np.int8), "inp": a, "idim": np.array((H, W), np.int8),
            "answer": a, "adim": np.array((H, W), np.int8), "want": {}}
    _, _, _, _, al = _stub(H, W, [case])
    assert al.ox[0].tolist() == [0, 0] and al.correct[0].tolist() == [H * W - 1, H * W] and al.base[0].tolist() == [H * W - 1, H * W]
    mac = S.align_macros(al, (29, 28), 33, 30, H, W)
    assert mac["operation"][0].tolist() == [[-1, -1, -1], [28, 33, 30]] and mac["length"][0].tolist() == [1, 3]


def test_propose_alignments_padding_rules():
    inputs, idims, answers, adims, kinds, plans = AL.planted_align_tasks()
    rows = torch.from_numpy(AL.planted_rows(inputs, idims, answers, adims, kinds))
    venv = AL.align_venv(answers, adims)
    asked = []
    inner = venv.align
    venv.align = lambda rows, src_env=None, max_dist=None, sources=3, blank=True: (asked.append((max_dist, sources, blank)), inner(rows, src_env, max_dist, sources, blank))[1]
    prop = S.propose_alignments((29, 28), 33, 30, box_ops=[3, 29], seed_ops=[12], max_components=4)
    assert prop.wants_src is True
    src = torch.arange(8, dtype=torch.int32)
    cand = prop(venv, rows, src)
    objs = venv.components(rows, max_components=4, skip_color=0, bits=True)
    single = S.object_actions(objs, [3, 29], [12], masks=True)
    K1 = 4 * 3
    assert tuple(cand["bits"].shape) == (8, K1 + 2, 3, 128) and tuple(cand["operation"].shape) == (8, K1 + 2, 3) and tuple(cand["length"].shape) == (8, K1 + 2)
    assert torch.equal(cand["bits"][:, :K1, 0], single["bits"]) and torch.equal(cand["operation"][:, :K1, 0], single["operation"])
    assert bool((cand["operation"][:, :K1, 1:] == -1).all()) and bool((cand["length"][:, :K1] == 1).all()) and not cand["bits"][:, :K1, 1:].any()
    only = S.propose_alignments((29, 28), 33, 30)(venv, rows, src)
    assert all(torch.equal(only[k], cand[k][:, K1:]) for k in only)
    for i, (s, ox, oy) in enumerate(plans):  # the planted source's macro is there, three steps long
        assert only["operation"][i, s].tolist() == [(29, 28)[s], 33, 30] and int(only["length"][i, s]) == 3, (i, only["operation"][i].tolist())
    one = S.propose_alignments((29, 28), 33, 30, blank=False, sources=2, max_dist=5)(venv, rows, src)
    assert bool((one["operation"][:, 0] == -1).all()) and bool((one["length"][:, 0] == 1).all()) and not one["bits"][:, 0].any()  # (not asked for: total 0)
    assert asked == [(None, 3, True), (None, 3, True), (5, 2, False)]


def test_beam_search_solves_tasks_whose_answer_has_another_size():
    """Eight planted 12 x 12 tasks — three windows of the grid among distractors, three inputs on a larger blank canvas, two windows of
    the input after reset_grid has wiped the grid — each with ONE perfect offset (checked here with the mirror, so that solving them is
    a property of the tasks): a beam of width 1 and depth 1 over propose_alignments solves all eight, and the three primitive steps it
    returns replay to the answer, dims included, on the oracle."""
    inputs, idims, answers, adims, kinds, plans = AL.planted_align_tasks()
    assert kinds == ["window"] * 3 + ["embed"] * 3 + ["wiped"] * 2
    rows = AL.planted_rows(inputs, idims, answers, adims, kinds)
    grids, gdims = SB._grids_of(rows, "o2arc", 12, 12)
    for i in range(8):
        assert gdims[i].tolist() != adims[i].tolist()  # (no proposer that keeps grid_dim can reach the answer)
        assert (not grids[i].any()) == (kinds[i] == "wiped") and gdims[i].tolist() == idims[i].tolist()
        perfect = AL.perfect_offsets(inputs[i], idims[i], grids[i], gdims[i], answers[i], adims[i])
        want = {plans[i]} | ({(1,) + plans[i][1:]} if kinds[i] != "wiped" else set())  # (grid == input before any step: both sources fit)
        assert set(perfect) == want, (i, perfect, plans[i])
    venv = AL.align_venv(answers, adims)
    aligned, _ = AL.searches(venv, torch.from_numpy(rows), 8, before=False)
    assert sum(r.sequence is not None for r in aligned) == 8
    for i, r in enumerate(aligned):
        s, ox, oy = plans[i]
        assert r.root == 0 and [op for _, op in r.sequence] == [(29, 28)[s], 33, 30], (i, [op for _, op in r.sequence])
        assert r.sequence[1][0].sum() == int(adims[i][0]) * int(adims[i][1]) and r.sequence[2][0].sum() == 1
        assert AL.replay_on_oracle(rows[i], answers[i], adims[i], r.sequence) == 1, i
