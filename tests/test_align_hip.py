"""arcle_align_rows on the MI355X: EnvBatch.align_rows against arcle_amd.search.align_numpy over the emulator test's plan (and every
case without a distance limit under both Pastes), against the product's own Copy + resize_grid + Paste macros (arcle_expand_macros with
the dense pair), under a caller-chosen plane stride, graph capture, the refusals, the untouched handle, the slots of sources that were
not asked for, and beam search solving tasks whose answer has another size than the grid."""
import numpy as np
import pytest
import torch

import align as AL
import search as SR
import search_bits as SB
import strides as STR
from arcle_amd import _lib
from arcle_amd import search as S

pytestmark = pytest.mark.gpu

_HIP = []


def hip():
    if not _HIP:
        _HIP.append(AL.HipAlign())
    return _HIP[0]


def _creatable(H, W):
    """arcle_create serves the one-wavefront kernels where the reciprocal multiply divides every flat cell index by W exactly
    (tests/test_objects_hip.py)."""
    magic = 65536 // W + 1
    return all((n * magic) >> 16 == n // W for n in range(1024 + 16))


@pytest.mark.parametrize("H,W", AL.SIZES)
def test_device_equals_the_mirror(H, W):
    """The emulator test's plan through the product — plus every case without a distance limit under both Pastes, where the emulator's
    plan takes few cases: every word of every slot asked for and base exact; slots not asked for and the words around both outputs
    untouched."""
    if not _creatable(H, W):
        from arcle_amd.engine import EnvBatch
        with pytest.raises(_lib.ArcleHipError):
            EnvBatch(2, H, W, 3, "o2arc")
        return
    errs = AL.run_size(hip(), H, W, full=True)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("H,W", ((5, 5), (7, 6)))
def test_device_equals_the_products_own_three_step_macros(H, W):
    """Every candidate (source, ox, oy) of every case as the three-step macro — the source's Copy on R, resize_grid on the canvas
    rectangle, Paste on P — through expand_macros with the dense pair, both sources and both Pastes: dense is (the mirror's count for
    that offset, ah * aw), and the device's (correct, total) of each source is the best of them under the tie rule."""
    from arcle_amd.engine import EnvBatch
    dev = torch.device("cuda:0")
    compared = 0
    for blank in (True, False):
        b = EnvBatch(1, H, W, 3, "o2arc")
        b.set_op_table(AL.ops_for("o2arc", blank))
        for c in AL.cases_of(H, W):
            rows_np = AL.case_rows(c)
            _, _, table, _ = S.align_numpy(c["grid"], c["dim"], c["inp"], c["idim"], c["answer"], c["adim"], None, 3, blank, full=True)
            cand, masks, op = AL.align_macro_set(c, "o2arc", table)
            K = len(cand)
            b.plane("answer").copy_(torch.as_tensor(c["answer"][None], device=dev))
            b.field("answer_dim").copy_(torch.as_tensor(c["adim"][None], device=dev))
            rows = torch.as_tensor(rows_np, device=dev)
            align, base = (t.cpu().numpy()[0] for t in b.align_rows(rows, None, None, 3, blank))
            ah, aw = int(c["adim"][0]), int(c["adim"][1])
            if not K:
                assert not align[:, :4].any(), c["name"]
                continue
            bits = S.pack_bits(torch.as_tensor(masks.reshape(K, 3, H, W), device=dev))
            ex = b.expand_macros(rows, "bits", bits, torch.as_tensor(op, device=dev), torch.full((K,), 3, dtype=torch.int32, device=dev), dense=True)
            dense, status = ex.dense.cpu().numpy()[0], ex.status.cpu().numpy()[0]
            assert not status.any(), c["name"]
            want = table[cand[:, 0], cand[:, 1] + H - 1, cand[:, 2] + W - 1]
            assert np.array_equal(dense[:, 0], want) and (dense[:, 1] == ah * aw).all(), (c["name"], blank, cand[dense[:, 0] != want][:3].tolist())
            compared += K
            for s in range(2):
                mine = cand[:, 0] == s
                if not mine.any():
                    assert align[s, :4].tolist() == [0, 0, 0, 0], (c["name"], s)
                else:
                    best = min((-int(v), abs(ox) + abs(oy), ox, oy) for (_, ox, oy), v in zip(cand[mine].tolist(), dense[mine, 0]))
                    assert align[s, :4].tolist() == [best[2], best[3], -best[0], ah * aw], (c["name"], s, blank)
        b.status(True)
    assert compared >= 2000, compared


def test_a_caller_chosen_plane_stride():
    """30 x 30 at plane stride 912 (57 live lanes, the last holding 4 cells and 12 padding bytes; rows never line-aligned): the plan's
    answers, zero padding and the slack behind every plane untouched."""
    inst, check = STR.family_with_stride(AL.HipAlign, 912)
    errs = AL.run_size(inst, 30, 30) + check()
    assert not errs, "\n".join(errs[:10])


def test_align_in_a_captured_graph_replays_with_new_rows():
    H, W = 20, 7
    cases = AL.cases_of(H, W)
    M = len(cases)
    rng = np.random.default_rng(1)
    b = hip().batch("o2arc", H, W, M)
    dev = b.device
    b.plane("answer").copy_(torch.as_tensor(np.stack([c["answer"] for c in cases]), device=dev))
    b.field("answer_dim").copy_(torch.as_tensor(np.stack([c["adim"] for c in cases]), device=dev))
    order = [np.arange(M), np.arange(M)[::-1].copy(), np.roll(np.arange(M), 3)]
    buf = torch.as_tensor(AL.make_rows("o2arc", cases, rng), device=dev)
    src = torch.arange(M, dtype=torch.int32, device=dev)
    b.align_rows(buf, src, 3)  # (warm: the module is loaded before the capture)
    out = (torch.full((M, 2, 8), AL.SENTINEL, dtype=torch.int32, device=dev), torch.full((M, 2), AL.SENTINEL, dtype=torch.int32, device=dev))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        b.align_rows(buf, src, 3, 2, False, out=out)
    for perm in order:
        cs = [cases[i] for i in perm]
        buf.copy_(torch.as_tensor(AL.make_rows("o2arc", cs, rng), device=dev))
        src.copy_(torch.as_tensor(perm.astype(np.int32), device=dev))
        for t in out:
            t.fill_(AL.SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        errs = AL.compare("graph", (out[0].cpu().numpy(), out[1].cpu().numpy(), []), cs, 3, True, 2, False)
        assert not errs, "\n".join(errs[:10])


def test_refusals_return_their_codes_and_write_nothing():
    from arcle_amd.engine import EnvBatch
    L = _lib.lib()
    dev = torch.device("cuda:0")
    b = hip().batch("o2arc", 12, 12, 4)
    rows = b.get_state_rows().clone()
    align = torch.full((8, 2, 8), 77, dtype=torch.int32, device=dev)
    base = torch.full((8, 2), 77, dtype=torch.int32, device=dev)
    src = torch.zeros(8, dtype=torch.int32, device=dev)
    ERR_ARG, ERR_CONFIG = -1, -2

    def call(h, n_rows, rows_t, stride, dist=8, sources=3, blank=1, align_t=align, src_t=None):
        return L.arcle_align_rows(h, n_rows, None if rows_t is None else rows_t.data_ptr(), stride, None if src_t is None else src_t.data_ptr(), dist, sources, blank,
                                  None if align_t is None else align_t.data_ptr(), base.data_ptr(), None)
    Lrow = b.state_row_size()
    assert call(b._h, 0, rows, rows.stride(0)) == ERR_ARG and call(b._h, -3, rows, rows.stride(0)) == ERR_ARG  # n_rows <= 0
    assert call(b._h, 4, rows, Lrow - 1) == ERR_ARG                                  # stride below the row length
    assert call(b._h, 4, rows, rows.stride(0), align_t=None) == ERR_ARG              # NULL align
    assert call(b._h, 4, rows, rows.stride(0), dist=-1) == ERR_ARG                   # max_dist < 0
    assert call(b._h, 4, rows, rows.stride(0), sources=0) == ERR_ARG                 # no source asked for
    assert call(b._h, 4, rows, rows.stride(0), sources=4) == ERR_ARG and call(b._h, 4, rows, rows.stride(0), sources=3 | 8) == ERR_ARG  # a bit above INPUT
    assert call(b._h, 4, rows, rows.stride(0), blank=2) == ERR_ARG and call(b._h, 4, rows, rows.stride(0), blank=-1) == ERR_ARG  # blank outside {0, 1}
    assert call(b._h, 5, None, 0) == ERR_ARG                                         # resident form with more rows than envs
    assert call(b._h, 5, None, 0, src_t=src) == ERR_ARG                              # (a src_env does not help: row m's grid is env m's)
    assert call(None, 4, rows, rows.stride(0)) == ERR_ARG
    big = EnvBatch(4, 40, 40, 3, "o2arc")
    big_rows = big.get_state_rows()
    assert call(big._h, 4, big_rows, big_rows.stride(0)) == ERR_CONFIG  # more than ARCLE_MAX_CELLS cells
    with pytest.raises(_lib.ArcleHipError, match="1024"):
        big.align_rows(big_rows)
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in (align, base))
    assert call(b._h, 4, rows, rows.stride(0), dist=1 << 30, sources=2, blank=0) == 0  # (and served when asked properly)
    torch.cuda.synchronize()
    assert bool((base[:4] != 77).all()) and bool((base[4:] == 77).all()) and bool((align[4:] == 77).all())
    assert bool((align[:4, 0] == 77).all()) and bool((align[:4, 1, 4:] != 77).all())  # the slot asked for, and only it
    assert call(b._h, 4, None, 0, sources=1) == 0
    torch.cuda.synchronize()
    assert bool((align[:4, 0, 4:] != 77).all()) and bool((align[4:] == 77).all())
    b.status(True)


def test_slots_of_unrequested_sources_keep_their_sentinel():
    """Every non-empty set of sources under both Pastes on one batch of rows: the slots asked for are the mirror's, the others keep the
    sentinel."""
    H, W = 7, 6
    cases = AL.cases_of(H, W)
    be = hip()
    for sources in (1, 2, 3):
        for blank in (True, False):
            got = be.run("o2arc", H, W, cases, "lib", AL.LARGE, False, True, sources, blank, np.random.default_rng(sources))
            errs = AL.compare(f"sources {sources}", got, cases, AL.LARGE, True, sources, blank)
            assert not errs and be.guards_intact(), "\n".join(errs[:10])
            for s in range(2):
                assert ((got[0][:, s] == AL.SENTINEL).all()) == (not (sources >> s) & 1)


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
    b.align_rows(None)
    b.align_rows(rows, torch.arange(b.N, dtype=torch.int32, device=b.device).flip(0).contiguous(), None, 2, False)
    b.align_rows(rows, None, 0, 1)
    after = snapshot()
    for x, y in zip(before[:5], after[:5]):
        assert np.array_equal(x, y)
    assert all(np.array_equal(before[5][k], after[5][k]) for k in before[5]) and np.array_equal(before[6], after[6])
    b.status(True)


# ---- planted tasks whose answer has another size than the grid, end to end -----------------------------------------------------------
def test_beam_search_solves_tasks_whose_answer_has_another_size():
    """The demonstration of tests/test_align_host.py through ARCVecEnv: each of the eight planted tasks has ONE perfect offset per
    source that can reach it (checked here on the CPU with the mirror, and the oracle replays the sequences); propose_alignments at
    width 1 and depth 1 solves 8 of 8; propose_objects, propose_placements, propose_stamps and propose_turns at the same width and depth
    solve 0 of 8; `align` equals the host mirror."""
    from arcle_amd.envs import ARCVecEnv, O2ARCv2Env
    from arcle_amd.envs.vec import Alignments
    from arcle_amd.loaders import SyntheticLoader
    inputs, idims, answers, adims, kinds, plans = AL.planted_align_tasks()
    rows_np = AL.planted_rows(inputs, idims, answers, adims, kinds)
    grids, gdims = SB._grids_of(rows_np, "o2arc", 12, 12)
    for i in range(8):
        perfect = AL.perfect_offsets(inputs[i], idims[i], grids[i], gdims[i], answers[i], adims[i])
        assert set(perfect) == {plans[i]} | ({(1,) + plans[i][1:]} if kinds[i] != "wiped" else set()), (i, perfect)
    venv = ARCVecEnv(O2ARCv2Env, 8, SyntheticLoader(n_tasks=2, max_size=(12, 12)), max_grid_size=(12, 12), max_trial=3)
    venv.batch.set_tasks_padded(inputs, idims, answers, adims)
    venv.batch.reset()
    fresh = venv.state_rows().cpu().numpy()
    wiped = np.array([k == "wiped" for k in kinds])
    assert np.array_equal(fresh[~wiped], rows_np[~wiped])
    rows = torch.as_tensor(rows_np, device=venv.device)
    for max_dist, sources, blank in ((None, 3, True), (4, 2, False)):
        got = venv.align(rows, None, max_dist, sources, blank)
        want = AL.align_numpy_rows(grids, gdims, inputs, idims, answers, adims, max_dist, sources, blank)
        assert isinstance(got, Alignments)
        for f in Alignments._fields:
            assert np.array_equal(getattr(got, f).cpu().numpy(), getattr(want, f).numpy()), f
    got = venv.align(rows)
    for i, (s, ox, oy) in enumerate(plans):
        assert (int(got.ox[i, s]), int(got.oy[i, s]), int(got.correct[i, s])) == (ox, oy, int(got.total[i, s])), i
    aligned, before = AL.searches(venv, rows, 8)
    assert sum(r.sequence is not None for r in aligned) == 8
    assert {k: sum(r.sequence is not None for r in v) for k, v in before.items()} == {"objects": 0, "placements": 0, "stamps": 0, "turns": 0}
    for i, r in enumerate(aligned):
        assert r.root == 0 and [op for _, op in r.sequence] == [(29, 28)[plans[i][0]], 33, 30], i
        assert AL.replay_on_oracle(rows_np[i], answers[i], adims[i], r.sequence) == 1, i
    venv.check_errors()
