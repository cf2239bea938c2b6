"""arcle_scale_rows on the MI355X: EnvBatch.scale_rows against arcle_amd.search.scale_numpy over the emulator test's plan (and every
case with every mode in the remaining kinds), the device's own macros through arcle_expand_macros with the dense pair, under a
caller-chosen plane stride, graph capture, the refusals, the untouched handle, and beam search solving tasks whose answer is the input
zoomed, shrunk or tiled."""
import numpy as np
import pytest
import torch

import align as AL
import scales as SC
import search as SR
import search_bits as SB
import strides as STR
from arcle_amd import _lib
from arcle_amd import search as S

pytestmark = pytest.mark.gpu

_HIP = []


def hip():
    if not _HIP:
        _HIP.append(SC.HipScale())
    return _HIP[0]


@pytest.mark.parametrize("H,W", SC.SIZES)
def test_device_equals_the_mirror(H, W):
    """The emulator test's plan through the product — plus every case with every mode under the ARC rows and 37 rows of the raw kind:
    every word of scale, table, bits and base exact; slots not asked for and the words around every output untouched."""
    errs = SC.run_size(hip(), H, W, full=True)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("H,W", ((7, 6), (30, 30), (16, 33)))
def test_the_devices_macros_report_the_slots_pair(H, W):
    """The device's best candidates as macros (scale_macros on the device's own bit rows) through expand_macros with the dense pair: a
    macro that was kept runs without a status bit and reports (correct, total) of its slot; a dropped one is one ARCLE_ST_BAD_OP
    child."""
    from arcle_amd.engine import EnvBatch
    from arcle_amd.envs.vec import scales_of
    dev = torch.device("cuda:0")
    cases = SC.cases_of(H, W)
    M = len(cases)
    b = EnvBatch(M, H, W, 3, "o2arc")
    b.set_op_table(SC.CP.OPS["o2arc"]())
    b.plane("answer").copy_(torch.as_tensor(np.stack([c["answer"] for c in cases]), device=dev))
    b.field("answer_dim").copy_(torch.as_tensor(np.stack([c["adim"] for c in cases]), device=dev))
    rows = torch.as_tensor(np.concatenate([SC.case_rows(c) for c in cases]), device=dev)
    sc = scales_of(*b.scale_rows(rows))
    resize_op, color_ops = SC.SCALE_OPS["o2arc"]
    mac = S.scale_macros(sc, resize_op, color_ops, H, W)
    ex = b.expand_macros(rows, "bits", mac["bits"], mac["operation"], mac["length"], dense=True)
    dense, status, length = ex.dense.cpu().numpy(), ex.status.cpu().numpy(), mac["length"].cpu().numpy()
    cor, tot, colours, base = sc.correct.cpu().numpy(), sc.total.cpu().numpy(), sc.colours.cpu().numpy(), sc.base.cpu().numpy()
    kept = 0
    for m, c in enumerate(cases):
        for s in range(2):
            if tot[m, s] == 0 or int(cor[m, s]) * int(base[m, 1]) <= int(base[m, 0]) * int(tot[m, s]):
                assert status[m, s] == SR.ST_BAD_OP and length[m, s] == 1, (c["name"], s)
                continue
            kept += 1
            assert status[m, s] == 0 and length[m, s] == 1 + bin(int(colours[m, s])).count("1"), (c["name"], s)
            assert dense[m, s].tolist() == [cor[m, s], tot[m, s]], (c["name"], s, dense[m, s].tolist(), cor[m, s], tot[m, s])
    assert kept >= 14, kept
    b.status(True)


def test_a_caller_chosen_plane_stride():
    """30 x 30 at plane stride 912 (57 live lanes, the last holding 4 cells and 12 padding bytes; rows never line-aligned): the plan's
    answers, zero padding and the slack behind every plane untouched."""
    inst, check = STR.family_with_stride(SC.HipScale, 912)
    errs = SC.run_size(inst, 30, 30) + check()
    assert not errs, "\n".join(errs[:10])


def test_scale_in_a_captured_graph_replays_with_new_rows():
    H, W = 20, 7
    cases = SC.cases_of(H, W)
    M = len(cases)
    rng = np.random.default_rng(1)
    b = hip().batch("o2arc", H, W, M)
    dev = b.device
    b.plane("answer").copy_(torch.as_tensor(np.stack([c["answer"] for c in cases]), device=dev))
    b.field("answer_dim").copy_(torch.as_tensor(np.stack([c["adim"] for c in cases]), device=dev))
    order = [np.arange(M), np.arange(M)[::-1].copy(), np.roll(np.arange(M), 3)]
    buf = torch.as_tensor(SC.make_rows("o2arc", cases, rng), device=dev)
    src = torch.arange(M, dtype=torch.int32, device=dev)
    b.scale_rows(buf, src)  # (warm: the module is loaded before the capture)
    out = (torch.full((M, 2, 8), SC.SENTINEL, dtype=torch.int32, device=dev), torch.full((M, 2, 132), SC.SENTINEL, dtype=torch.int32, device=dev),
           torch.full((M, 2, 9, 128), SC.SENTINEL8, dtype=torch.uint8, device=dev), torch.full((M, 2), SC.SENTINEL, dtype=torch.int32, device=dev))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        b.scale_rows(buf, src, 2, 5, out=out)
    for perm in order:
        cs = [cases[i] for i in perm]
        buf.copy_(torch.as_tensor(SC.make_rows("o2arc", cs, rng), device=dev))
        src.copy_(torch.as_tensor(perm.astype(np.int32), device=dev))
        for t in out:
            t.fill_(SC.SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        errs = SC.compare("graph", tuple(t.cpu().numpy() for t in out) + ([],), cs, True, 2, 5, True, True)
        assert not errs, "\n".join(errs[:10])


def test_refusals_return_their_codes_and_write_nothing():
    from arcle_amd.engine import EnvBatch
    L = _lib.lib()
    dev = torch.device("cuda:0")
    b = hip().batch("o2arc", 12, 12, 4)
    rows = b.get_state_rows().clone()
    scale = torch.full((8, 2, 8), 77, dtype=torch.int32, device=dev)
    table = torch.full((8, 2, 132), 77, dtype=torch.int32, device=dev)
    bits = torch.full((8, 2, 9, 128), 77, dtype=torch.uint8, device=dev)
    base = torch.full((8, 2), 77, dtype=torch.int32, device=dev)
    src = torch.zeros(8, dtype=torch.int32, device=dev)
    ERR_ARG, ERR_CONFIG = -1, -2

    def call(h, n_rows, rows_t, stride, sources=3, modes=7, scale_t=scale, src_t=None, bits_off=0):
        return L.arcle_scale_rows(h, n_rows, None if rows_t is None else rows_t.data_ptr(), stride, None if src_t is None else src_t.data_ptr(), sources, modes,
                                  None if scale_t is None else scale_t.data_ptr(), table.data_ptr(), bits.data_ptr() + bits_off, base.data_ptr(), None)
    Lrow = b.state_row_size()
    assert call(b._h, 0, rows, rows.stride(0)) == ERR_ARG and call(b._h, -3, rows, rows.stride(0)) == ERR_ARG  # n_rows <= 0
    assert call(b._h, 4, rows, Lrow - 1) == ERR_ARG                                  # stride below the row length
    assert call(b._h, 4, rows, rows.stride(0), scale_t=None) == ERR_ARG              # NULL scale
    assert call(b._h, 4, rows, rows.stride(0), sources=0) == ERR_ARG                 # no source asked for
    assert call(b._h, 4, rows, rows.stride(0), sources=4) == ERR_ARG and call(b._h, 4, rows, rows.stride(0), sources=3 | 8) == ERR_ARG  # a bit above INPUT
    assert call(b._h, 4, rows, rows.stride(0), modes=0) == ERR_ARG                   # no mode asked for
    assert call(b._h, 4, rows, rows.stride(0), modes=8) == ERR_ARG and call(b._h, 4, rows, rows.stride(0), modes=7 | 16) == ERR_ARG  # a bit above TILE
    assert call(b._h, 4, rows, rows.stride(0), bits_off=1) == ERR_ARG                # an odd bits address
    assert call(b._h, 5, None, 0) == ERR_ARG                                         # resident form with more rows than envs
    assert call(b._h, 5, None, 0, src_t=src) == ERR_ARG                              # (a src_env does not help: row m's grid is env m's)
    assert call(None, 4, rows, rows.stride(0)) == ERR_ARG
    big = EnvBatch(4, 40, 40, 3, "o2arc")
    big_rows = big.get_state_rows()
    assert call(big._h, 4, big_rows, big_rows.stride(0)) == ERR_CONFIG  # more than ARCLE_MAX_CELLS cells
    with pytest.raises(_lib.ArcleHipError, match="1024"):
        big.scale_rows(big_rows)
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in (scale, table, bits, base))
    assert call(b._h, 4, rows, rows.stride(0), sources=2, modes=4) == 0  # (and served when asked properly)
    torch.cuda.synchronize()
    assert bool((base[:4] != 77).all()) and bool((base[4:] == 77).all()) and bool((scale[4:] == 77).all()) and bool((table[4:] == 77).all()) and bool((bits[4:] == 77).all())
    assert bool((scale[:4, 0] == 77).all()) and bool((table[:4, 0] == 77).all()) and bool((bits[:4, 0] == 77).all())  # the slot asked for, and only it
    assert bool((scale[:4, 1, 4:] != 77).all()) and bool((table[:4, 1, :128] == -1).all()) and bool((table[:4, 1, 128:] != 77).all()) and bool((bits[:4, 1] != 77).all())
    assert call(b._h, 4, None, 0, sources=1) == 0
    torch.cuda.synchronize()
    assert bool((scale[:4, 0, 4:] != 77).all()) and bool((scale[4:] == 77).all())
    b.status(True)


def test_handle_is_untouched():
    """State rows, status word, counters and the installed reward / term buffers are byte-identical before and after the calls."""
    be, orc, rng, ops = SR.case_pair(SR.HipSearchBackend, "o2arc", 12, 12, 1)
    b = be.b
    pay, op = SR.draw_actions(rng, "bbox", b.N, 12, 12, len(ops))
    op[0] = len(ops) + 3  # a sticky status bit to keep
    be.step("bbox", pay, op)

    def snapshot():
        torch.cuda.synchronize()
        return (b.get_state_rows().cpu().numpy().copy(), b.status(False), b.cnt.cpu().numpy().copy(), b.reward.cpu().numpy().copy(),
                b.term.cpu().numpy().copy(), {k: v.cpu().numpy().copy() for k, v in b.planes.items()}, b.rec.cpu().numpy().copy())
    before = snapshot()
    assert before[1] != 0
    rows = b.get_state_rows().clone()
    b.scale_rows(None, table=True)
    b.scale_rows(rows, torch.arange(b.N, dtype=torch.int32, device=b.device).flip(0).contiguous(), 2, 5)
    b.scale_rows(rows, None, 1, 2, bits=False)
    after = snapshot()
    for x, y in zip(before[:5], after[:5]):
        assert np.array_equal(x, y)
    assert all(np.array_equal(before[5][k], after[5][k]) for k in before[5]) and np.array_equal(before[6], after[6])
    b.status(True)


# ---- planted tasks whose answer is the input zoomed, shrunk or tiled, end to end ------------------------------------------------------
def test_beam_search_solves_zoomed_shrunk_and_tiled_tasks():
    """The demonstration of tests/test_scale_host.py through ARCVecEnv: each of the eight planted tasks has its planted candidate
    perfect (checked here on the CPU with the mirror, and the oracle replays the sequences); propose_scales at width 1 and depth 1
    solves 8 of 8; propose_alignments, propose_objects, propose_placements, propose_stamps and propose_turns at the same width and
    depth solve 0 of 8 — every answer's dims differ from the input's, and no window or embedding of the input equals the answer;
    `scale` equals the host mirror."""
    from arcle_amd.envs import ARCVecEnv, O2ARCv2Env
    from arcle_amd.envs.vec import Scales
    from arcle_amd.loaders import SyntheticLoader
    inputs, idims, answers, adims, names, plans = SC.planted_scale_tasks()
    rows_np = SC.planted_rows(inputs, idims, answers, adims)
    grids, gdims = SB._grids_of(rows_np, "o2arc", 12, 12)
    for i in range(8):
        assert gdims[i].tolist() != adims[i].tolist()
        assert AL.perfect_offsets(inputs[i], idims[i], grids[i], gdims[i], answers[i], adims[i]) == [], names[i]
    venv = ARCVecEnv(O2ARCv2Env, 8, SyntheticLoader(n_tasks=2, max_size=(12, 12)), max_grid_size=(12, 12), max_trial=3)
    venv.batch.set_tasks_padded(inputs, idims, answers, adims)
    venv.batch.reset()
    assert np.array_equal(venv.state_rows().cpu().numpy(), rows_np)
    rows = torch.as_tensor(rows_np, device=venv.device)
    for sources, modes in ((3, 7), (2, 5)):
        got = venv.scale(rows, None, sources, modes, table=True)
        want = SC.scale_numpy_rows(grids, gdims, inputs, idims, answers, adims, sources, modes, table=True)
        assert isinstance(got, Scales)
        for f in Scales._fields:
            assert np.array_equal(getattr(got, f).cpu().numpy(), getattr(want, f).numpy()), f
    got = venv.scale(rows)
    assert got.table is None
    for i, cand in enumerate(plans):
        for s in range(2):
            assert (int(got.cand[i, s]), int(got.correct[i, s])) == (cand, int(got.total[i, s])), (names[i], s)
    scaled, before = SC.searches(venv, rows, 8)
    assert sum(r.sequence is not None for r in scaled) == 8
    assert {k: sum(r.sequence is not None for r in v) for k, v in before.items()} == {"alignments": 0, "objects": 0, "placements": 0, "stamps": 0, "turns": 0}
    for i, r in enumerate(scaled):
        present = sorted(int(v) for v in np.unique(answers[i]) if v)
        assert r.root == 0 and [op for _, op in r.sequence] == [33] + present, names[i]
        assert SC.replay_on_oracle(rows_np[i], answers[i], adims[i], r.sequence) == 1, names[i]
    venv.check_errors()
