"""arcle_stamp_rows on the MI355X: EnvBatch.stamp_rows against arcle_amd.search.stamp_numpy over the emulator test's plan (and every
case without a distance limit under both Pastes), on arcle_objects_rows' outputs as they stand, against the product's own CopyO + Paste
macros (arcle_expand_macros with the dense pair), under a caller-chosen plane stride, graph capture, the refusals, the untouched
handle, and beam search stamping copies into empty space."""
import numpy as np
import pytest
import torch

import components as CP
import objects as OB
import search as SR
import search_bits as SB
import stamp as ST
import strides as STR
from arcle_amd import _lib
from arcle_amd import search as S

pytestmark = pytest.mark.gpu

_HIP = []


def hip():
    if not _HIP:
        _HIP.append(ST.HipStamp())
    return _HIP[0]


def _creatable(H, W):
    """arcle_create serves the one-wavefront kernels where the reciprocal multiply divides every flat cell index by W exactly
    (tests/test_objects_hip.py)."""
    magic = 65536 // W + 1
    return all((n * magic) >> 16 == n // W for n in range(1024 + 16))


@pytest.mark.parametrize("H,W", ST.SIZES)
def test_device_equals_the_mirror(H, W):
    """The emulator test's plan through the product — plus every case at C = 16 without a distance limit under the Paste(s) the plan
    has not run that way (on the flat board: both): stamp and base exact, entries >= count and the words around both outputs
    untouched.  Then the outputs of arcle_objects_rows fed in unchanged: the same answers as the mirror gives for components_numpy's
    masks."""
    if not _creatable(H, W):
        from arcle_amd.engine import EnvBatch
        with pytest.raises(_lib.ArcleHipError):
            EnvBatch(2, H, W, 3, "o2arc")
        return
    errs = ST.run_size(hip(), H, W, full=True)
    assert not errs, "\n".join(errs[:10])
    cases = ST.cases_of(H, W)
    M = len(cases)
    b = hip().batch("o2arc", H, W, M)
    b.plane("answer").copy_(torch.as_tensor(np.stack([c["answer"] for c in cases]), device=b.device))
    b.field("answer_dim").copy_(torch.as_tensor(np.stack([c["adim"] for c in cases]), device=b.device))
    rows = torch.as_tensor(CP.make_rows("o2arc", cases, np.random.default_rng(4)), device=b.device)
    for any_color, diagonal, dist, blank in ((True, True, None, True), (False, False, 3, False)):
        count, comp, bits, _ = b.objects_rows(rows, 16, 0, any_color, diagonal, True)
        stamp, base = (t.cpu().numpy() for t in b.stamp_rows(rows, count, bits, None, dist, blank))
        for m, c in enumerate(cases):
            n, _, _, masks = S.components_numpy(c["grid"], c["dim"], 16, 0, any_color, diagonal)
            ws, wb = S.stamp_numpy(c["grid"], c["dim"], c["answer"], c["adim"], masks[:n], dist, blank)
            assert int(count[m, 0]) == n and np.array_equal(stamp[m, :n], ws) and not stamp[m, n:].any() and tuple(base[m]) == wb, (c["name"], dist)


@pytest.mark.parametrize("blank", [True, False])
@pytest.mark.parametrize("H,W", ST.ORACLE_SIZES)
def test_device_equals_the_products_own_copy_and_paste(H, W, blank):
    """Every cell of grid_dim for every object as a two-step macro — CopyO on the object's cells, Paste on the one cell — through
    expand_macros with the dense pair, on freshly reset rows (blank False: a table whose Paste has arg byte 0): dense[..., 0] is the
    mirror's table, stamp its arg-max under the tie rule, base the dense pair of a no-op child of the same parent."""
    from arcle_amd.engine import EnvBatch
    dev = torch.device("cuda:0")
    b = EnvBatch(1, H, W, 3, "o2arc")
    b.set_op_table(ST.ops_for("o2arc", blank))
    for c in ST.cases_of(H, W):
        rows_np, _ = CP.clean_rows("o2arc", c["grid"][None], c["dim"][None], c["answer"][None], c["adim"][None])
        grid = SB._grids_of(rows_np, "o2arc", H, W)[0][0]
        owner, cand, masks, op, length = ST.stamp_macro_set(c)
        _, _, table = S.stamp_numpy(grid, c["dim"], c["answer"], c["adim"], c["masks"], None, blank, full=True)
        b.plane("answer").copy_(torch.as_tensor(c["answer"][None], device=dev))
        b.field("answer_dim").copy_(torch.as_tensor(c["adim"][None], device=dev))
        rows = torch.as_tensor(rows_np, device=dev)
        K = len(cand)
        bits = ST.B.pack_bits(masks.reshape(K * 2, H, W)).reshape(K, 2, 128)
        noop_bits, noop_op = np.zeros((1, 2, 128), np.uint8), np.array([[ST.MOVE_OPS[0], -1]], np.int32)  # (a Move of the empty selection)
        ex = b.expand_macros(rows, "bits", torch.as_tensor(np.concatenate([bits, noop_bits]), device=dev), torch.as_tensor(np.concatenate([op, noop_op]), device=dev),
                             torch.as_tensor(np.concatenate([length, [1]]).astype(np.int32), device=dev), dense=True)
        dense, status = ex.dense.cpu().numpy()[0], ex.status.cpu().numpy()[0]
        assert not status.any(), c["name"]
        want = table[owner, cand[:, 0], cand[:, 1]]
        assert np.array_equal(dense[:K, 0], want), (c["name"], np.argwhere(dense[:K, 0] != want)[:3].tolist())
        gh, gw = int(c["dim"][0]), int(c["dim"][1])
        inside = np.zeros_like(c["masks"])
        inside[:, :gh, :gw] = c["masks"][:, :gh, :gw]
        stamp, base = (t.cpu().numpy()[0] for t in b.stamp_rows(rows, None, torch.as_tensor(ST.B.pack_bits(inside)[None], device=dev), None, None, blank))
        assert tuple(base) == tuple(dense[K]) and (dense[:K, 1] == base[1]).all(), c["name"]
        for k in range(len(c["masks"])):
            mine = owner == k
            xs, ys = np.nonzero(inside[k])
            if not mine.any():
                assert stamp[k].tolist() == [0, 0, int(base[0]), 0], (c["name"], k)
                continue
            x0, y0 = int(xs.min()), int(ys.min())
            best = min((-int(v), abs(px - x0) + abs(py - y0), px - x0, py - y0) for (px, py), v in zip(cand[mine].tolist(), dense[:K, 0][mine]))
            assert stamp[k].tolist() == [x0 + best[2], y0 + best[3], -best[0], len(xs)], (c["name"], k)
    b.status(True)


def test_a_caller_chosen_plane_stride():
    """30 x 30 at plane stride 912 (57 live lanes, the last holding 4 cells and 12 padding bytes; rows never line-aligned): the plan's
    answers, zero padding and the slack behind every plane untouched."""
    inst, check = STR.family_with_stride(ST.HipStamp, 912)
    errs = ST.run_size(inst, 30, 30) + check()
    assert not errs, "\n".join(errs[:10])


def test_stamp_in_a_captured_graph_replays_with_new_rows():
    H, W = 20, 7
    cases = ST.cases_of(H, W)
    M, C = len(cases), 16
    rng = np.random.default_rng(1)
    b = hip().batch("o2arc", H, W, M)
    dev = b.device
    b.plane("answer").copy_(torch.as_tensor(np.stack([c["answer"] for c in cases]), device=dev))
    b.field("answer_dim").copy_(torch.as_tensor(np.stack([c["adim"] for c in cases]), device=dev))
    order = [np.arange(M), np.arange(M)[::-1].copy(), np.roll(np.arange(M), 3)]
    buf = torch.as_tensor(CP.make_rows("o2arc", cases, rng), device=dev)
    count, bits = (torch.as_tensor(a, device=dev) for a in ST.PL.bit_rows(cases, C, True, rng))
    src = torch.arange(M, dtype=torch.int32, device=dev)
    b.stamp_rows(buf, count, bits, src, 3)  # (warm: the module is loaded before the capture)
    out = (torch.full((M, C, 4), ST.SENTINEL, dtype=torch.int32, device=dev), torch.full((M, 2), ST.SENTINEL, dtype=torch.int32, device=dev))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        b.stamp_rows(buf, count, bits, src, 3, True, out=out)
    for perm in order:
        cs = [cases[i] for i in perm]
        buf.copy_(torch.as_tensor(CP.make_rows("o2arc", cs, rng), device=dev))
        cn, bt = ST.PL.bit_rows(cs, C, True, rng)
        count.copy_(torch.as_tensor(cn, device=dev))
        bits.copy_(torch.as_tensor(bt, device=dev))
        src.copy_(torch.as_tensor(perm.astype(np.int32), device=dev))
        for t in out:
            t.fill_(ST.SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        errs = ST.compare("graph", (out[0].cpu().numpy(), out[1].cpu().numpy(), []), cs, C, 3, True, True, True)
        assert not errs, "\n".join(errs[:10])


def test_refusals_return_their_codes_and_write_nothing():
    from arcle_amd.engine import EnvBatch
    L = _lib.lib()
    dev = torch.device("cuda:0")
    b = hip().batch("o2arc", 12, 12, 4)
    rows = b.get_state_rows().clone()
    count = torch.full((8, 2), 2, dtype=torch.int32, device=dev)
    bits = torch.full((8 * 4 * 128 + 2,), 77, dtype=torch.uint8, device=dev)
    stamp = torch.full((8, 4, 4), 77, dtype=torch.int32, device=dev)
    base = torch.full((8, 2), 77, dtype=torch.int32, device=dev)
    ERR_ARG, ERR_CONFIG = -1, -2

    def call(h, n_rows, rows_t, stride, C, dist=8, blank=1, bits_ptr=bits.data_ptr(), stamp_t=stamp):
        return L.arcle_stamp_rows(h, n_rows, None if rows_t is None else rows_t.data_ptr(), stride, C, count.data_ptr(), bits_ptr, None, dist, blank,
                                  None if stamp_t is None else stamp_t.data_ptr(), base.data_ptr(), None)
    Lrow = b.state_row_size()
    assert call(b._h, 4, rows, rows.stride(0), 0) == ERR_ARG and call(b._h, 4, rows, rows.stride(0), 1025) == ERR_ARG  # max_comp outside [1, 1024]
    assert call(b._h, 0, rows, rows.stride(0), 4) == ERR_ARG and call(b._h, -3, rows, rows.stride(0), 4) == ERR_ARG  # n_rows <= 0
    assert call(b._h, 4, rows, Lrow - 1, 4) == ERR_ARG                                 # stride below the row length
    assert call(b._h, 4, rows, rows.stride(0), 4, bits_ptr=None) == ERR_ARG            # NULL bits
    assert call(b._h, 4, rows, rows.stride(0), 4, stamp_t=None) == ERR_ARG             # NULL stamp
    assert call(b._h, 4, rows, rows.stride(0), 4, bits_ptr=bits.data_ptr() + 1) == ERR_ARG  # odd bits address
    assert call(b._h, 4, rows, rows.stride(0), 4, dist=-1) == ERR_ARG                  # max_dist < 0
    assert call(b._h, 4, rows, rows.stride(0), 4, blank=2) == ERR_ARG and call(b._h, 4, rows, rows.stride(0), 4, blank=-1) == ERR_ARG  # blank outside {0, 1}
    assert call(b._h, 5, None, 0, 4) == ERR_ARG                                        # resident form with more rows than envs
    assert call(None, 4, rows, rows.stride(0), 4) == ERR_ARG
    big = EnvBatch(4, 40, 40, 3, "o2arc")
    big_rows = big.get_state_rows()
    assert call(big._h, 4, big_rows, big_rows.stride(0), 4) == ERR_CONFIG  # more than ARCLE_MAX_CELLS cells
    with pytest.raises(_lib.ArcleHipError, match="1024"):
        big.stamp_rows(big_rows, None, torch.zeros((4, 4, 128), dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in (bits, stamp, base))
    assert call(b._h, 4, rows, rows.stride(0), 4, dist=1 << 30) == 0 and call(b._h, 4, None, 0, 4, blank=0, bits_ptr=bits.data_ptr() + 2) == 0  # (and served when asked properly)
    torch.cuda.synchronize()
    assert bool((base[:4] != 77).all()) and bool((base[4:] == 77).all()) and bool((stamp[:4, :2] != 77).any()) and bool((stamp[:4, 2:] == 77).all()) and bool((stamp[4:] == 77).all())
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
    count, comp, bits, _ = b.objects_rows(rows, 16, 0, True, True, True)
    b.stamp_rows(None, count, bits, None, 8)
    b.stamp_rows(rows, count, bits, torch.arange(b.N, dtype=torch.int32, device=b.device).flip(0).contiguous(), None, False)
    b.stamp_rows(rows, None, bits, None, 0)
    after = snapshot()
    for x, y in zip(before[:5], after[:5]):
        assert np.array_equal(x, y)
    assert all(np.array_equal(before[5][k], after[5][k]) for k in before[5]) and np.array_equal(before[6], after[6])
    b.status(True)


# ---- planted stamp tasks, end to end ---------------------------------------------------------------------------------------------------
def test_beam_search_stamps_copies_into_empty_space():
    """The demonstration of tests/test_stamp_host.py through ARCVecEnv: propose_stamps at width 1, depth = the number of stamps solves
    8 of 8 and every sequence replays to the answer on the oracle; the macros the library had before solve ST.BEFORE_SOLVES at the
    same width and depth; `stamp` equals the host mirror."""
    from arcle_amd.envs import ARCVecEnv, O2ARCv2Env
    from arcle_amd.envs.vec import Stamps
    from arcle_amd.loaders import SyntheticLoader
    inputs, dims, answers, spots = ST.planted_stamp_tasks(8)
    venv = ARCVecEnv(O2ARCv2Env, 8, SyntheticLoader(n_tasks=2, max_size=(12, 12)), max_grid_size=(12, 12), max_trial=3)
    venv.batch.set_tasks_padded(inputs, dims, answers, dims)
    venv.batch.reset()
    rows = venv.state_rows().clone()
    objs = venv.objects(rows, skip_color=0, max_components=4, any_color=True, diagonal=True, bits=True)
    for max_dist, blank in ((None, True), (6, False)):
        got = venv.stamp(rows, objs, None, max_dist, blank)
        want = ST.stamp_numpy_rows(inputs, dims, answers, dims, OB.objects_numpy(inputs, dims, 4, 0, True, True, True, False), max_dist, blank)
        assert isinstance(got, Stamps) and objs.count.tolist() == [1] * 8
        for f in Stamps._fields:
            assert np.array_equal(getattr(got, f).cpu().numpy(), getattr(want, f).numpy()), f
    got = venv.stamp(rows, objs)
    assert all((int(got.px[i, 0]), int(got.py[i, 0])) in spots[i] for i in range(8))
    own = venv.stamp(None, venv.objects(skip_color=0, max_components=4, any_color=True, diagonal=True, bits=True))
    assert all(torch.equal(a, c) for a, c in zip(own, got))
    before, stamped = ST.stamp_searches(venv, rows, 8, [len(s) for s in spots])
    assert sum(r.sequence is not None for r in stamped) == 8
    assert sum(r.sequence is not None for r in before) == ST.BEFORE_SOLVES
    for i, (r, targets) in enumerate(zip(stamped, spots)):
        assert r.root == 0 and [op for _, op in r.sequence] == [ST.COPY_OP, ST.PASTE_OP] * len(targets), i
        assert SB.replay_masks_on_oracle(inputs[i], dims[i], answers[i], r.sequence) == 1, i
    venv.check_errors()
