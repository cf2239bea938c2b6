"""The host side of arcle_objects_rows: components_numpy in its four modes against an independent union-find labelling
(tests/objects.py::uf_objects) and, in mode 0, against the reference's dfs (tests/golden/components/components.npz); object_actions on
an Objects tuple; and the search demonstration on a stub vec env backed by the oracle (torch CPU tensors; no GPU): planted tasks whose
answer moves a two-colour shape or a diagonal line as ONE object."""
import numpy as np
import pytest
import torch

import components as CP
import macros as MC
import objects as OB
import search_bits as SB
from arcle_amd import search as S
from arcle_amd.envs.vec import Components, Objects
from oracle import oracle as O


def _all_cases():
    seen, out = set(), []
    for c in CP.fixture() + [c for hw in OB.SIZES for c in OB.cases_of(*hw)]:
        if (c["name"], c["H"], c["W"]) not in seen:
            seen.add((c["name"], c["H"], c["W"]))
            out.append(c)
    return out


@pytest.mark.parametrize("mode", OB.MODES)
def test_components_numpy_equals_the_union_find(mode):
    """Descriptors, order, masks, `left` and the colour words of every fixture grid and every generated grid, skip_color in {-1, 0, 3};
    a cut list (C = 5) is the prefix, and `left` the cells of the rest."""
    any_color, diagonal = bool(mode & OB.ANY), bool(mode & OB.DIAG)
    for c in _all_cases():
        for skip in OB.SKIPS:
            want, wmasks, wcolors = OB.uf_objects(c["grid"], c["dim"], skip, any_color, diagonal)
            n, left, comp, masks = S.components_numpy(c["grid"], c["dim"], 1024, skip, any_color, diagonal)
            assert (n, left) == (len(want), 0), (c["name"], skip)
            assert np.array_equal(comp[:n], want) and np.array_equal(masks[:n], wmasks), (c["name"], skip)
            assert not comp[n:].any() and not masks[n:].any()
            colors = S.component_colors_numpy(c["grid"], masks[:n])
            assert colors.dtype == np.uint32 and np.array_equal(colors, wcolors), (c["name"], skip)
            if not any_color:
                assert np.array_equal(colors, np.uint32(1) << (want[:, 6].astype(np.uint32) & 31)), (c["name"], skip)
            n5, left5, comp5, masks5 = S.components_numpy(c["grid"], c["dim"], 5, skip, any_color, diagonal)
            assert n5 == min(5, len(want)) and np.array_equal(comp5[:n5], want[:n5]) and left5 == int(want[n5:, 7].sum()), (c["name"], skip)
            assert np.array_equal(masks5[:n5], wmasks[:n5])
            assert (want[:, 0] == want[:, 4]).all()  # the seed lies in the box's first row


@pytest.mark.parametrize("skip", OB.SKIPS)
def test_mode_0_equals_the_reference_dfs(skip):
    """The union-find labelling, the mirror of the device tests, on the golden comp / label arrays; and the defaults of components_numpy
    are mode 0."""
    for c in CP.fixture():
        want, label = c["want"][skip]
        comp, masks, _ = OB.uf_objects(c["grid"], c["dim"], skip)
        assert np.array_equal(comp, want), c["name"]
        got_label = np.full(label.shape, -1, np.int16)
        for k in range(len(comp)):
            got_label[masks[k] != 0] = k
        assert np.array_equal(got_label, label), c["name"]
        n, left, comp0, _ = S.components_numpy(c["grid"], c["dim"], 1024, skip, any_color=False, diagonal=False)
        assert (n, left) == (len(want), 0) and np.array_equal(comp0[:n], want), c["name"]


def test_the_generated_grids_are_what_the_issue_lists():
    for H, W in OB.SIZES:
        by = {c["name"].split(" gen ", 1)[1]: c for c in OB.cases_of(H, W) if " gen " in c["name"]}
        assert {"noise3", "checker35", "diagonal", "antidiagonal", "zigzag", "bytes"} <= set(by) and ("wrap2" in by) == (H >= 3)
        n = [len(OB.uf_objects(by["checker35"]["grid"], (H, W), -1, bool(m & OB.ANY), bool(m & OB.DIAG))[0]) for m in OB.MODES]
        assert n[0] == H * W and n[1] == 1 and n[2] == (2 if min(H, W) > 1 else H * W) and n[3] == 1, (H, W, n)
        for name in ("diagonal", "antidiagonal"):
            n = [len(OB.uf_objects(by[name]["grid"], (H, W), 0, False, d)[0]) for d in (False, True)]
            assert n == [min(H, W), 1], (H, W, name, n)
        if H > 1 and W > 1:
            n = [len(OB.uf_objects(by["zigzag"]["grid"], (H, W), 0, a, True)[0]) for a in (False, True)]
            assert n[1] == 1 and n[0] == (H + 2) // 3, (H, W, n)
        if H >= 3 and W > 2:  # (r, W - 1) and (r + 2, 0): never one object
            comp = OB.uf_objects(by["wrap2"]["grid"], (H, W), 0, True, True)[0]
            assert (comp[:, 7] == 1).all() and len(comp) == 2 * len(range(0, H - 2, 3)), (H, W)
        c = [c for k, c in by.items() if k.startswith("shrunk")][0]
        gh, gw = (int(v) for v in c["dim"])
        comp, masks, _ = OB.uf_objects(c["grid"], c["dim"], -1, True, True)
        assert (gh, gw) == (max(1, H - 2), max(1, W - 3)) and len(comp) == 1 and comp[0, 7] == gh * gw and not masks[0][gh:].any() and not masks[0][:, gw:].any()
    assert max(c["H"] for c in OB.cases_of(20, 7)) > 8 and (16, 33) in OB.SIZES  # the staircase is taller than the 8-row jump


def test_plan_covers_every_axis():
    for H, W in OB.SIZES:
        runs = OB.plan(H, W)
        assert {r[0] for r in runs} == {"o2arc", "arc", "raw"} and {r[1] for r in runs} == {1, 5, 1024} and {r[2] for r in runs} == set(OB.SKIPS)
        assert {r[3] for r in runs} == {"lib", "dense", "odd", "resident"} and {1, 37} <= {r[6] for r in runs}
        assert {r[4] for r in runs} == {True, False} and {r[5] for r in runs} == {True, False}
    assert {(r[1], r[2]) for r in OB.plan(30, 30) if r[3] == "lib"} >= {(C, s) for C in (1, 5, 1024) for s in OB.SKIPS}


def test_object_actions_take_an_objects_tuple_like_a_components_tuple():
    cases = [c for c in OB.cases_of(5, 5)]
    grids, dims = np.stack([c["grid"] for c in cases]), np.stack([c["dim"] for c in cases])
    C, box_ops, seed_ops = 6, [20, 21, 3], [10, 15]
    obj = OB.objects_numpy(grids, dims, C, 0, False, False, True, True)
    assert isinstance(obj, Objects) and Objects._fields == Components._fields + ("colors",)
    comp = Components(*obj[:7])
    for masks in (False, True):
        a, b = S.object_actions(obj, box_ops, seed_ops, masks=masks), S.object_actions(comp, box_ops, seed_ops, masks=masks)
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)
    m1, m2 = S.object_macros(obj, box_ops, seed_ops, [(29, 30)]), S.object_macros(comp, box_ops, seed_ops, [(29, 30)])
    assert all(torch.equal(m1[k], m2[k]) for k in m1)
    # ... and with the wider notion the layout is the same: component k's exact cells with every box op, then its seed's bit
    wide = OB.objects_numpy(grids, dims, C, 0, True, True, True, True)
    a = S.object_actions(wide, box_ops, seed_ops, masks=True)
    M, per = len(cases), 5
    bits, op = a["bits"].reshape(M, C, per, 128).numpy(), a["operation"].reshape(M, C, per).numpy()
    for m, c in enumerate(cases):
        n, _, desc, masks = S.components_numpy(c["grid"], c["dim"], C, 0, True, True)
        assert int(wide.count[m]) == n and (op[m, n:] == -1).all() and not bits[m, n:].any() and (op[m, :n] == np.array(box_ops + seed_ops)).all()
        for k in range(n):
            cells = np.unpackbits(bits[m, k], axis=-1, bitorder="little")[:, :25].reshape(per, 5, 5)
            seed = np.zeros((5, 5), np.uint8)
            seed[desc[k, 4], desc[k, 5]] = 1
            assert (cells[:3] == masks[k]).all() and (cells[3:] == seed).all()


class ObjectsVenv(MC.MacroVenv):
    """The oracle-backed stub vec env of the stamp tasks + `objects`, from components_numpy."""

    def objects(self, rows, max_components=32, skip_color=-1, any_color=False, diagonal=False, bits=False, colors=False):
        grids, gdims = SB._grids_of(rows.numpy(), self.kind, self.H, self.W)
        return OB.objects_numpy(grids, gdims, max_components, skip_color, any_color, diagonal, bits, colors)


def test_the_proposers_call_objects_only_when_asked():
    calls = []

    class Spy(ObjectsVenv):
        def objects(self, *a, **k):
            calls.append(("objects", k.get("any_color"), k.get("diagonal")))
            return super().objects(*a, **k)

        def components(self, *a, **k):
            calls.append(("components",))
            return super().components(*a, **k)
    inputs, dims, answers, _ = OB.planted_whole_object_tasks(2)
    rows, _ = CP.clean_rows("o2arc", inputs, dims, answers, dims)
    venv = Spy("o2arc", 12, 12, 3, O.o2arc_ops(), answers, dims)
    r = torch.from_numpy(rows)
    S.propose_objects(OB.MOVE_OPS, [])(venv, r)
    S.propose_object_macros(OB.MOVE_OPS, [], [])(venv, r)
    S.propose_objects(OB.MOVE_OPS, [], diagonal=True)(venv, r)
    S.propose_object_macros(OB.MOVE_OPS, [], [], any_color=True)(venv, r)
    assert calls == [("components",), ("components",), ("objects", False, True), ("objects", True, False)]


def test_planted_tasks_have_objects_their_parts_are_not():
    inputs, dims, answers, steps = OB.planted_whole_object_tasks(8)
    for i, (g, (mask, op)) in enumerate(zip(inputs, steps)):
        n, _, comp, masks = S.components_numpy(g, (12, 12), 16, 0)
        assert n == (2 if i % 2 == 0 else 3) and all(not np.array_equal(masks[k] != 0, mask) for k in range(n)), i
        n, _, comp, masks = S.components_numpy(g, (12, 12), 16, 0, True, True)
        assert n == 1 and np.array_equal(masks[0] != 0, mask) and op in OB.MOVE_OPS, i
        if i % 2 == 0:  # the two colour parts are 4-adjacent: multi-colour 4-connected is enough
            assert S.components_numpy(g, (12, 12), 16, 0, True, False)[0] == 1 and len(np.unique(g[mask])) == 2


def test_beam_search_moves_whole_objects_only_with_the_wider_notion():
    """width 1, depth 1, Move ops on exact cells: the 4-connected one-colour components solve none of the eight planted tasks (moving
    a strict subset leaves the rest where it was), multi-colour 8-connected objects solve all eight, and the returned step replayed
    on the oracle gives the answer."""
    inputs, dims, answers, steps = OB.planted_whole_object_tasks(8)
    rows, _ = CP.clean_rows("o2arc", inputs, dims, answers, dims)
    venv = ObjectsVenv("o2arc", 12, 12, 3, O.o2arc_ops(), answers, dims)
    narrow, wide = OB.whole_object_searches(venv, torch.from_numpy(rows), 8)
    assert sum(r.sequence is not None for r in narrow) == 0, [r.sequence for r in narrow]
    assert sum(r.sequence is not None for r in wide) == 8
    for i, r in enumerate(wide):
        assert len(r.sequence) == 1 and r.root == 0
        sel, op = r.sequence[0]
        assert sel.dtype == bool and np.array_equal(sel, steps[i][0]) and op == steps[i][1], i
        assert SB.replay_masks_on_oracle(inputs[i], dims[i], answers[i], r.sequence) == 1, i
