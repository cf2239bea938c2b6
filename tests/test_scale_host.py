"""The host side of arcle_scale_rows: scale_numpy against the oracle's own resize_grid + Color macro for every candidate (which pins the
closed form: the child's grid, its grid_dim and its dense pair), the modes and the unrequested sources, what the generated cases reach,
scale_macros against scale_numpy and replayed step by step on the oracle, propose_scales' padding rules on an oracle-backed stub vec
env (torch CPU tensors; no GPU), and the search demonstration: planted tasks whose answer is the input zoomed, shrunk or tiled."""
import os

import numpy as np
import pytest
import torch

import align as AL
import macros as MC
import scales as SC
import search_bits as SB
from arcle_amd import search as S
from arcle_amd.envs.vec import Scales


def test_the_constants():
    from arcle_amd import _lib
    assert (S.SCALE_ZOOM, S.SCALE_SHRINK, S.SCALE_TILE, S.SCALE_CANDS) == (1, 2, 4, 132) == (_lib.SCALE_ZOOM, _lib.SCALE_SHRINK, _lib.SCALE_TILE, _lib.SCALE_CANDS)
    # (an extension of ABI 18: the version and the 61 entry points of include/arcle_hip.h stay, the new one is listed beside them)
    assert _lib.EXTENSIONS == ["arcle_scale_rows"] and "arcle_scale_rows" not in _lib.EXPORTS
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    hdr = open(os.path.join(inc, "arcle_scale_rows.h")).read()
    assert "int arcle_scale_rows(arcle_env* env" in hdr and "#define ARCLE_HAS_SCALE_ROWS 1" in hdr and "#define ARCLE_SCALE_CANDS 132" in hdr
    assert '#include "arcle_scale_rows.h"' in open(os.path.join(inc, "arcle_hip.h")).read()
    L = _lib.lib()
    assert hasattr(L, "arcle_scale_rows") and L.arcle_abi_version() == _lib.ABI_VERSION
    cands = S.scale_candidates()
    assert len(cands) == 132 and cands[0] == (0, 1, 1) and cands[63] == (0, 8, 8) and cands[64] == (1, 1, 1) and cands[64 + 8 * 2 + 4] == (1, 3, 5)
    assert cands[128:] == [(2, 0, 0), (2, 0, 1), (2, 1, 0), (2, 1, 1)]  # bit 0 of t: the tile columns, bit 1: the tile rows
    assert all(SC.cand_of(*c) == i for i, c in enumerate(cands))


@pytest.mark.parametrize("kind", ("o2arc", "arc"))
@pytest.mark.parametrize("H,W", SC.ORACLE_SIZES)
def test_mirror_equals_the_oracle(H, W, kind):
    """EVERY candidate of every case and both sources as the macro [resize_grid on the canvas rectangle, Color c on the child's cells of
    colour c for each colour present, ascending] on the chained oracle, O2ARC and ARC tables: the grid it leaves is the mirror's child
    on the whole plane, its grid_dim is the answer's dims, its dense pair is (the mirror's count, ah * aw); `scale` is the table's
    first arg-max, with the colours of that child."""
    seen = 0
    for c in SC.cases_of(H, W):
        ah, aw = int(c["adim"][0]), int(c["adim"][1])
        scale, _, table, children = SC.mirror(c)
        for s in range(2):
            got = SC.oracle_children(c, kind, s)
            assert (len(got) == 132) == (scale[s, 0] >= 0), (c["name"], s)
            for cand, grid, gdim, dense, child, count in got:
                assert np.array_equal(grid, child), (c["name"], kind, s, cand)
                assert gdim.tolist() == [ah, aw] and dense.tolist() == [count, ah * aw], (c["name"], kind, s, cand, gdim, dense, count)
                seen += 1
            if scale[s, 0] >= 0:
                best = int(np.argmax(table[s]))  # (the first of the maxima: the lowest index)
                colours = sum(1 << int(v) for v in np.unique(children[s, best]) if v)
                assert scale[s].tolist()[:4] == [best, int(table[s, best]), ah * aw, colours], (c["name"], s)
            else:
                assert scale[s].tolist()[:4] == [-1, 0, 0, 0] and (table[s] == -1).all() and not children[s].any()
    assert seen >= 132 * 2 * 14, seen


def _one(cases, suffix):
    return [c for c in cases if c["name"].endswith(suffix)][0]


@pytest.mark.parametrize("H,W", SC.SIZES)
def test_the_cases_reach_what_they_are_built_for(H, W):
    """What tests/scales.py::cases_of promises, from the cases themselves and from the mirror."""
    cases = SC.cases_of(H, W)
    names = [c["name"].split(" ", 1)[1] for c in cases]
    assert len(set(names)) == len(names) == 19
    for c in cases:
        scale, _, table, children = SC.mirror(c)
        for s, want in c["want"].items():  # the candidate a case was built for is the mirror's, and perfect
            assert int(scale[s, 0]) == want and scale[s, 1] == scale[s, 2] > 0, (c["name"], s, scale[s].tolist())
        for s in c["unique"]:
            assert (table[s] == scale[s, 2]).sum() == 1, (c["name"], s)
        for s in c["short"]:
            assert 0 <= scale[s, 1] < scale[s, 2], (c["name"], s)
    kinds = {SC.CANDS[w][0] for c in cases for s, w in c["want"].items() if s in c["unique"]}
    assert kinds == {SC.ZOOM, SC.SHRINK, SC.TILE}, "a unique perfect candidate of each mode"
    an = _one(cases, "zoom aniso")
    _, kx, ky = SC.CANDS[an["want"][1]]
    assert kx != ky and not an["grid"].any()
    zs = _one(cases, "zoom short")
    assert 2 * int(zs["dim"][0]) < H and 2 * int(zs["dim"][1]) < W and zs["adim"].tolist() == [H, W] and not zs["answer"][H - 1].any() and not zs["answer"][:, W - 1].any()
    sp = _one(cases, "shrink past")
    sh, sw = (int(v) for v in sp["idim"])
    assert (int(sp["adim"][0]) - 1) * 2 >= sh and (int(sp["adim"][1]) - 1) * 2 >= sw, "the last canvas row and column read past the source"
    one = _one(cases, "1x1 source")
    assert one["dim"].tolist() == [1, 1] and one["adim"].tolist() == [min(8, H), min(8, W)]
    assert SC.mirror(one)[2][0, SC.cand_of(SC.ZOOM, 8, 8)] == SC.mirror(one)[0][0, 2], "factor 8 is among the perfect candidates"
    fr, fc = _one(cases, "tile flat row"), _one(cases, "tile flat column")
    assert fr["dim"].tolist() == [1, 3] and fc["dim"].tolist() == [2, 1]
    for c, a, b in ((fr, 1, 3), (fc, 2, 3)):  # the mirror bit of the axis of extent 1 cannot matter; the other one does
        scale, _, table, _ = SC.mirror(c)
        assert table[0, 128 + a] == table[0, 128 + b] == scale[0, 2] and table[0, 128] < scale[0, 2] and scale[0, 0] == 128 + a, c["name"]
    rg = _one(cases, "tile ragged")
    assert H % int(rg["dim"][0]) and W % int(rg["dim"][1]) and rg["want"] == {0: 128}
    assert _one(cases, "tile mirrored")["want"] == {1: 131}
    j = _one(cases, "junk")
    sh, sw = (int(v) for v in j["dim"])
    assert (sh, sw) == (H - 1, W - 1) and j["grid"][sh:].all() and j["grid"][:, sw:].all()
    assert np.array_equal(SC.child_of(j["grid"], H, W, H, W, 0), j["answer"]), "reading the junk would complete the answer"
    bb = _one(cases, "bad bytes")
    assert {-128, -1, 10, 127} <= set(bb["grid"].reshape(-1).tolist()) and not bb["answer"][(bb["grid"] < 1) | (bb["grid"] > 9)].any()
    ab = _one(cases, "answer byte")
    odd = (ab["answer"] < 0) | (ab["answer"] > 9)
    assert {-1, 10, 127} <= set(ab["answer"].reshape(-1).tolist()) and np.array_equal(ab["answer"], ab["grid"])
    assert SC.mirror(ab)[0][0, :3].tolist() == [0, H * W - int(odd.sum()), H * W], "equal bytes outside 0..9 do not match"
    z = SC.mirror(_one(cases, "zero source"))
    assert z[0][:, 0].tolist() == [0, 0] and z[0][:, 3].tolist() == [0, 0] and (z[2] == z[2][:, :1]).all()
    for suffix, s in (("zero dim a", 0), ("zero dim b", 1), ("zero dim c", 0), ("zero dim c", 1)):
        scale = SC.mirror(_one(cases, suffix))[0]
        assert scale[s, :4].tolist() == [-1, 0, 0, 0] and 0 in scale[s, 4:].tolist(), suffix
    ti = _one(cases, "tie identity")
    scale, _, table, _ = SC.mirror(ti)
    assert table[0, 0] == table[0, 64] == H * W and (table[0, 128:] == H * W).all() and scale[0, 0] == 0
    assert [int(SC.mirror(ti, m)[0][0, 0]) for m in (1, 2, 3, 4, 5, 6, 7)] == [0, 64, 0, 128, 0, 64, 0]
    co = SC.mirror(_one(cases, "constant"))
    assert (co[2][0, :64] == H * W).all() and co[0][0, 0] == 0 and co[0][0, 3] == 1 << 4


def test_modes_cut_the_table_and_unrequested_sources_stay_zero():
    H, W = 7, 6
    mode_of = np.array([c[0] for c in SC.CANDS])
    for c in SC.cases_of(H, W):
        args = (c["grid"], c["dim"], c["inp"], c["idim"], c["answer"], c["adim"])
        both, base, full, _ = S.scale_numpy(*args, 3, 7, full=True)
        for sources in (1, 2):
            part, b = S.scale_numpy(*args, sources, 7)
            assert b == base and np.array_equal(part[sources - 1], both[sources - 1]) and not part[2 - sources].any()
        for modes in range(1, 7):
            sc, _, table, _ = S.scale_numpy(*args, 3, modes, full=True)
            assert np.array_equal(table, np.where(((modes >> mode_of) & 1 != 0)[None], full, -1))
            for s in range(2):
                if sc[s, 0] >= 0:
                    assert sc[s, 1] == table[s].max() == table[s, sc[s, 0]] and sc[s, 0] == int(np.argmax(table[s]))


def _stub(H, W, cases, sources=3, modes=7):
    rows = np.concatenate([SC.case_rows(c) for c in cases])
    answers, adims = np.stack([c["answer"] for c in cases]), np.stack([c["adim"] for c in cases])
    venv = SC.scale_venv(answers, adims, H, W)
    return rows, answers, adims, venv, venv.scale(torch.from_numpy(rows), None, sources, modes, table=True)


def test_scale_macros_equal_the_mirror_and_replay_on_the_oracle():
    """Every macro scale_macros builds against scale_numpy — resize_grid on the canvas, then the colours present, ascending, packed to
    the front, each on the mirror's cells of that colour — and one oracle step at a time: the child is the one the mirror names (its
    count and total are the slot's); a dropped slot is operation -1 at every step, length 1 and zero bits."""
    H, W = 7, 6
    cases = SC.cases_of(H, W)
    rows, answers, adims, venv, sc = _stub(H, W, cases)
    M = len(cases)
    assert isinstance(sc, Scales) and Scales._fields == ("cand", "correct", "total", "colours", "kind", "kx", "ky", "src_dim", "ans_dim", "bits", "table", "base")
    assert tuple(sc.cand.shape) == (M, 2) and tuple(sc.src_dim.shape) == (M, 2, 2) and tuple(sc.bits.shape) == (M, 2, 9, 128) and tuple(sc.table.shape) == (M, 2, 132)
    resize_op, color_ops = SC.SCALE_OPS["o2arc"]
    mac = S.scale_macros(sc, resize_op, color_ops, H, W)
    assert tuple(mac["bits"].shape) == (M, 2, 10, 128) and mac["bits"].dtype == torch.uint8
    assert tuple(mac["operation"].shape) == (M, 2, 10) and mac["operation"].dtype == torch.int32
    assert tuple(mac["length"].shape) == (M, 2) and mac["length"].dtype == torch.int32
    masks = S.unpack_bits(mac["bits"], H, W).numpy().astype(np.int8)
    real = dropped = 0
    for m, c in enumerate(cases):
        scale, base, _, children = SC.mirror(c)
        bc, bt = base
        for s in range(2):
            cand, cor, tot, colours = (int(v) for v in scale[s, :4])
            assert (int(sc.cand[m, s]), int(sc.correct[m, s]), int(sc.total[m, s]), int(sc.colours[m, s])) == (cand, cor, tot, colours)
            want_kind = (-1, 0, 0) if cand < 0 else SC.CANDS[cand]
            assert (int(sc.kind[m, s]), int(sc.kx[m, s]), int(sc.ky[m, s])) == want_kind, (c["name"], s)
            ops, ln = mac["operation"][m, s].tolist(), int(mac["length"][m, s])
            if tot == 0 or cor * bt <= bc * tot:
                assert ops == [-1] * 10 and ln == 1 and not mac["bits"][m, s].any(), (c["name"], s)
                dropped += 1
                continue
            real += 1
            present = [k for k in range(1, 10) if (colours >> k) & 1]
            assert ops == [resize_op] + [color_ops[k] for k in present] + [-1] * (9 - len(present)) and ln == 1 + len(present), (c["name"], s, ops)
            ah, aw = int(c["adim"][0]), int(c["adim"][1])
            assert masks[m, s, 0].sum() == tot and masks[m, s, 0][:ah, :aw].all() and not masks[m, s, ln:].any()
            for t, k in enumerate(present):
                assert np.array_equal(masks[m, s, 1 + t] != 0, children[s, cand] == k), (c["name"], s, k)
            cur = rows[m:m + 1]
            for t in range(ln):
                cur, _, _, st, dense = MC.oracle_step_rows(cur, answers[m:m + 1], adims[m:m + 1], "o2arc", H, W, 3, SC.CP.OPS["o2arc"](), "mask",
                                                           masks[m, s, t].reshape(1, -1), np.array([ops[t]], np.int32))
                assert not st.any(), (c["name"], s, t)
            grid, gdim = SB._grids_of(cur, "o2arc", H, W)
            assert np.array_equal(grid[0], children[s, cand]) and gdim[0].tolist() == c["adim"].tolist() and dense[0].tolist() == [cor, tot], (c["name"], s)
    assert real >= 14 and dropped >= 8, (real, dropped)
    zero = [n for n, c in enumerate(cases) if c["name"].endswith("zero source")][0]
    assert sc.cand[zero].tolist() == [0, 0] and sc.colours[zero].tolist() == [0, 0]
    if int(sc.correct[zero, 0]) * int(sc.base[zero, 1]) > int(sc.base[zero, 0]) * int(sc.total[zero, 0]):
        assert int(mac["length"][zero, 0]) == 1 and mac["operation"][zero, 0].tolist() == [resize_op] + [-1] * 9


def test_an_all_zero_source_is_one_resize_step():
    """All-zero sources under an answer of another size: candidate 0, no colour, and a macro of length 1 — the resize alone."""
    H, W = 7, 6
    zero = np.zeros((H, W), np.int8)
    a = zero.copy()
    a[1, 1] = 3
    case = {"name": "zero", "H": H, "W": W, "grid": zero, "dim": np.array((H, W), np.int8), "inp": zero, "idim": np.array((H, W), np.int8),
            "answer": a, "adim": np.array((4, 3), np.int8), "want": {}}
    _, _, _, _, sc = _stub(H, W, [case])
    assert sc.cand[0].tolist() == [0, 0] and sc.colours[0].tolist() == [0, 0] and sc.correct[0].tolist() == [11, 11] and sc.total[0].tolist() == [12, 12]
    mac = S.scale_macros(sc, 33, range(10), H, W)
    assert mac["length"][0].tolist() == [1, 1] and mac["operation"][0].tolist() == [[33] + [-1] * 9] * 2 and not mac["bits"][0, :, 1:].any()


def test_the_identity_is_dropped():
    """A row whose grid already has the answer's dims and is its own best candidate (ZOOM(1, 1)): the grid's macro does not beat the
    row's own ratio and is padding; the input's macro stays if it scores more."""
    H, W = 7, 6
    g = np.random.default_rng(3).integers(1, 10, (H, W)).astype(np.int8)
    a = g.copy()
    a[0, 0] = 0
    case = {"name": "identity", "H": H, "W": W, "grid": g, "dim": np.array((H, W), np.int8), "inp": a, "idim": np.array((H, W), np.int8),
            "answer": a, "adim": np.array((H, W), np.int8), "want": {}}
    _, _, _, _, sc = _stub(H, W, [case])
    assert sc.cand[0].tolist() == [0, 0] and sc.correct[0].tolist() == [H * W - 1, H * W] and sc.base[0].tolist() == [H * W - 1, H * W]
    mac = S.scale_macros(sc, 33, range(10), H, W)
    assert mac["operation"][0, 0].tolist() == [-1] * 10 and mac["operation"][0, 1, 0] == 33 and mac["length"][0].tolist() == [1, 1 + bin(int(sc.colours[0, 1])).count("1")]


def test_propose_scales_padding_rules():
    inputs, idims, answers, adims, names, plans = SC.planted_scale_tasks()
    rows = torch.from_numpy(SC.planted_rows(inputs, idims, answers, adims))
    venv = SC.scale_venv(answers, adims)
    asked = []
    inner = venv.scale
    venv.scale = lambda rows, src_env=None, sources=3, modes=7, table=False, bits=True: (asked.append((sources, modes)), inner(rows, src_env, sources, modes, table, bits))[1]
    prop = S.propose_scales(33, range(10), box_ops=[3, 29], seed_ops=[12], max_components=4)
    assert prop.wants_src is True
    src = torch.arange(8, dtype=torch.int32)
    cand = prop(venv, rows, src)
    objs = venv.components(rows, max_components=4, skip_color=0, bits=True)
    single = S.object_actions(objs, [3, 29], [12], masks=True)
    K1 = 4 * 3
    assert tuple(cand["bits"].shape) == (8, K1 + 2, 10, 128) and tuple(cand["operation"].shape) == (8, K1 + 2, 10) and tuple(cand["length"].shape) == (8, K1 + 2)
    assert torch.equal(cand["bits"][:, :K1, 0], single["bits"]) and torch.equal(cand["operation"][:, :K1, 0], single["operation"])  # the singles come first
    assert bool((cand["operation"][:, :K1, 1:] == -1).all()) and bool((cand["length"][:, :K1] == 1).all()) and not cand["bits"][:, :K1, 1:].any()
    only = S.propose_scales(33, range(10))(venv, rows, src)
    assert all(torch.equal(only[k], cand[k][:, K1:]) for k in only)
    for i in range(8):  # the macro of either source (grid == input before any step) is there: the resize, then the colours
        n = len(np.unique(answers[i][answers[i] > 0]))
        assert only["operation"][i, 0, 0] == 33 and only["length"][i].tolist() == [1 + n, 1 + n], i
    one = S.propose_scales(33, range(10), sources=2, modes=4)(venv, rows, src)
    assert bool((one["operation"][:, 0] == -1).all()) and bool((one["length"][:, 0] == 1).all()) and not one["bits"][:, 0].any()  # (not asked for: total 0)
    assert asked == [(3, 7), (3, 7), (2, 4)]


def test_beam_search_solves_zoomed_shrunk_and_tiled_tasks():
    """Eight planted 12 x 12 tasks — x2, x3 and (2, 3) zooms of 4 x 4, /2 and /3 shrinks of a block-uniform 12 x 12, a plain 2 x 3
    tiling of 4 x 4, a 2 x 2 tiling of 5 x 5 mirrored on both axes, a 1 x 2 tiling of 6 x 6 with mirrored columns; every source has
    at least 3 colours and no symmetry — each with its planted candidate perfect (checked with the mirror): a beam of width 1 and depth
    1 over propose_scales solves all eight, and the steps it returns replay to the answer, dims included, on the oracle.
    propose_alignments and the object proposers solve none, for a reason asserted here: every answer's dims differ from the input's
    (no proposer that keeps grid_dim can reach it), and no window or embedding of the input equals the answer (align's table holds no
    perfect offset)."""
    inputs, idims, answers, adims, names, plans = SC.planted_scale_tasks()
    assert len(names) == 8
    rows = SC.planted_rows(inputs, idims, answers, adims)
    grids, gdims = SB._grids_of(rows, "o2arc", 12, 12)
    for i in range(8):
        sh, sw = (int(v) for v in idims[i])
        src = inputs[i][:sh, :sw]
        assert len(np.unique(src)) >= 3 and not any(np.array_equal(src, t) for t in (src[::-1], src[:, ::-1], src[::-1, ::-1], src.T if sh == sw else None) if t is not None)
        assert gdims[i].tolist() == idims[i].tolist() != adims[i].tolist() and np.array_equal(grids[i], inputs[i])
        scale, _, table, _ = S.scale_numpy(grids[i], gdims[i], inputs[i], idims[i], answers[i], adims[i], full=True)
        for s in range(2):
            # (one tile row: whether every second tile ROW is mirrored cannot matter, 129 ties with 131; every other plan is unique)
            perfect = [129, 131] if names[i] == "tile 1 x 2 mirrored columns" else [plans[i]]
            assert scale[s, 0] == plans[i] and scale[s, 1] == scale[s, 2] and np.flatnonzero(table[s] == scale[s, 2]).tolist() == perfect, (names[i], scale[s].tolist())
        assert AL.perfect_offsets(inputs[i], idims[i], grids[i], gdims[i], answers[i], adims[i]) == [], names[i]
    venv = SC.scale_venv(answers, adims)
    scaled, before = SC.searches(venv, torch.from_numpy(rows), 8, before=("alignments", "objects", "placements"))  # (what the stub env serves)
    assert sum(r.sequence is not None for r in scaled) == 8
    assert {k: sum(r.sequence is not None for r in v) for k, v in before.items()} == {"alignments": 0, "objects": 0, "placements": 0}
    for i, r in enumerate(scaled):
        present = sorted(int(v) for v in np.unique(answers[i]) if v)
        assert r.root == 0 and [op for _, op in r.sequence] == [33] + present, (names[i], [op for _, op in r.sequence])
        assert r.sequence[0][0].sum() == int(adims[i][0]) * int(adims[i][1])
        assert SC.replay_on_oracle(rows[i], answers[i], adims[i], r.sequence) == 1, names[i]
