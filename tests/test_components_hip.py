"""arcle_components_rows on the MI355X: the device against arcle_amd.search.components_numpy over the emulator test's case list,
self-consistency with the shipped FloodFill and with step_bits, the untouched handle, graph capture, the refusals, and beam search
with object proposals on planted two-object tasks."""
import numpy as np
import pytest
import torch

import backends as B
import components as CP
import search as SR
from arcle_amd import search as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu

_HIP = []


def hip():
    if not _HIP:
        _HIP.append(CP.HipComponents())
    return _HIP[0]


def _creatable(H, W):
    """arcle_create serves the one-wavefront kernels where the reciprocal multiply divides every flat cell index by W exactly
    (arcle_hip.hip); 8 x 127 is not such a shape (ARCLE_ERR_CONFIG from arcle_create, as on the parent commit): the emulator test
    covers it, no handle of the product can hold it."""
    magic = 65536 // W + 1
    return all((n * magic) >> 16 == n // W for n in range(1024 + 16))


@pytest.mark.parametrize("H,W", [hw for hw in CP.sizes() if _creatable(*hw)])
def test_device_equals_the_mirror(H, W):
    """The emulator test's plan through the product: both instantiations (FW_FAST at 16 <= W <= 32, FW_GENERIC with the row board and with the
    flat board elsewhere), rows at every layout and the resident form, bits, entries >= written untouched."""
    errs = CP.run_size(hip(), H, W)
    assert not errs, "\n".join(errs[:10])


def _grid_offset(kind, P):
    off = 0
    for f, ln in B.row_layout(kind, P):
        if f == "grid":
            return off
        off += ln


@pytest.mark.parametrize("H,W", [(30, 30), (12, 12)])
def test_every_component_is_what_floodfill_fills(H, W):
    """For every written component: `transition` with point = seed and FloodFill of a colour the grid does not hold changes exactly
    `cells` cells, exactly those of `bits`."""
    cases = [c for c in CP.cases_of(H, W) if len(np.unique(c["grid"])) < 10]
    free = [int(np.setdiff1d(np.arange(10), np.unique(c["grid"]))[0]) for c in cases]
    grids, dims = np.stack([c["grid"] for c in cases]), np.stack([c["dim"] for c in cases])
    rows_np, _ = CP.clean_rows("o2arc", grids, dims)
    dev = torch.device("cuda:0")
    b = hip().batch("o2arc", H, W, 2)
    rows = torch.as_tensor(rows_np, device=dev)
    C = 32
    count, comp, bits = b.components_rows(rows, C, -1, True)
    count, comp, bits = count.cpu().numpy(), comp.cpu().numpy(), bits.cpu().numpy()
    m_idx, k_idx = np.nonzero(np.arange(C)[None, :] < count[:, :1])
    assert len(m_idx) > 100
    T, P = len(m_idx), H * W
    point = torch.as_tensor(np.ascontiguousarray(comp[m_idx, k_idx, 4:6]), device=dev)
    op = torch.as_tensor((10 + np.array(free)[m_idx]).astype(np.int32), device=dev)
    out, _, _ = b.transition_rows(rows.index_select(0, torch.as_tensor(m_idx, device=dev)), "point", point, op,
                                  torch.zeros(T, dtype=torch.int32, device=dev))
    assert b.status(True) == 0
    off = _grid_offset("o2arc", P)
    changed = out.cpu().numpy()[:, off:off + P] != rows_np[m_idx, off:off + P]
    want = np.unpackbits(bits[m_idx, k_idx], axis=1, bitorder="little")[:, :P] != 0
    assert np.array_equal(changed, want)
    assert np.array_equal(changed.sum(1), comp[m_idx, k_idx, 7])


def test_bits_drive_step_bits_like_the_dfs_mask_drives_the_oracle():
    """bits[m, k] fed to step_bits with a Color op gives the oracle's step with the reference dfs mask (the fixture's) as selection."""
    H = W = 30
    cases = [c for c in CP.cases_of(H, W) if len(c["want"][0][0]) >= 3][:16]
    grids, dims = np.stack([c["grid"] for c in cases]), np.stack([c["dim"] for c in cases])
    M = len(cases)
    be = B.HipBackend(M, H, W, 3, "o2arc", O.o2arc_ops())
    orc = B.OracleBackend(M, H, W, 3, "o2arc", O.o2arc_ops())
    for x in (be, orc):
        x.set_tasks(grids, dims, grids, dims)
        x.reset()
    count, comp, bits = be.b.components_rows(None, 8, 0, True)
    assert int(count[:, 0].min()) >= 3
    for k in (0, 2):
        masks = np.stack([(c["want"][0][1] == k).astype(np.int8) for c in cases])
        op = np.full(M, 4 + k, np.int32)  # Color4 / Color6
        r1, t1 = be.step("bits", bits[:, k].cpu().numpy(), op)
        r0, t0 = orc.step("mask", masks, op)
        assert np.array_equal(r0, r1) and np.array_equal(t0, t1)
        for f in ("grid", "selected", "grid_dim"):
            assert np.array_equal(be.get(f), orc.get(f)), (k, f)
        # (the next round labels the recoloured grids on the device; the fixture's masks are of the ORIGINAL grids, so component 2 is
        # taken from the first call's bits as well)
    assert be.status() == 0 and orc.status() == 0


def test_handle_is_untouched():
    """State rows, status word, counters and the installed reward / term buffers are byte-identical before and after a call."""
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
    b.components_rows(None, 16, 0, True)
    b.components_rows(rows, 1024, -1, False)
    after = snapshot()
    for x, y in zip(before[:5], after[:5]):
        assert np.array_equal(x, y)
    assert all(np.array_equal(before[5][k], after[5][k]) for k in before[5]) and np.array_equal(before[6], after[6])
    b.status(True)


def test_components_in_a_captured_graph_replay_with_new_rows():
    H = W = 30
    cases = CP.cases_of(H, W)
    rng = np.random.default_rng(1)
    first, second = CP.make_rows("o2arc", cases, rng), CP.make_rows("o2arc", cases[::-1], rng)
    b = hip().batch("o2arc", H, W, 2)
    dev = b.device
    buf = torch.as_tensor(first, device=dev)
    C = 32
    b.components_rows(buf, C, 0, True)  # (warm: the module is loaded before the capture)
    out = hip()._out(b, len(cases), C, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        b.components_rows(buf, C, 0, True, out=out)
    for rows_np, cs in ((first, cases), (second, cases[::-1]), (first, cases)):
        buf.copy_(torch.as_tensor(rows_np, device=dev))
        for t in out:
            t.fill_(CP.SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        errs = CP.compare("graph", tuple(t.cpu().numpy() for t in out), cs, C, 0, True)
        assert not errs, "\n".join(errs[:10])


def test_refusals_return_their_codes_and_write_nothing():
    import ctypes
    from arcle_amd import _lib
    from arcle_amd.engine import EnvBatch
    L = _lib.lib()
    dev = torch.device("cuda:0")
    b = hip().batch("o2arc", 12, 12, 4)
    rows = b.get_state_rows().clone()
    count = torch.full((8, 2), 77, dtype=torch.int32, device=dev)
    comp = torch.full((8, 4, 8), 77, dtype=torch.int32, device=dev)
    bits = torch.full((8, 4, 128), 77, dtype=torch.uint8, device=dev)
    ERR_ARG, ERR_CONFIG = -1, -2

    def call(h, n_rows, rows_t, stride, C, cnt=count, cmp_=comp):
        return L.arcle_components_rows(h, n_rows, None if rows_t is None else rows_t.data_ptr(), stride, C, -1,
                                       None if cnt is None else cnt.data_ptr(), None if cmp_ is None else cmp_.data_ptr(), bits.data_ptr(), None)
    Lrow = b.state_row_size()
    assert call(b._h, 4, rows, rows.stride(0), 0) == ERR_ARG and call(b._h, 4, rows, rows.stride(0), 1025) == ERR_ARG  # max_comp outside [1, 1024]
    assert call(b._h, 4, rows, Lrow - 1, 4) == ERR_ARG              # stride below the row length
    assert call(b._h, 5, None, 0, 4) == ERR_ARG                     # resident form with more rows than envs
    assert call(b._h, 0, rows, rows.stride(0), 4) == ERR_ARG        # n_rows == 0: as arcle_hash_rows
    assert L.arcle_hash_rows(b._h, 0, rows.data_ptr(), rows.stride(0), count.data_ptr(), None) == ERR_ARG
    assert call(b._h, 4, rows, rows.stride(0), 4, cnt=None) == ERR_ARG and call(None, 4, rows, rows.stride(0), 4) == ERR_ARG
    big = EnvBatch(4, 40, 40, 3, "o2arc")
    big_rows = big.get_state_rows()
    assert call(big._h, 4, big_rows, big_rows.stride(0), 4) == ERR_CONFIG  # more than ARCLE_MAX_CELLS cells
    assert call(big._h, 4, big_rows, big_rows.stride(0), 0) == ERR_CONFIG  # ... is refused before the arguments are looked at
    with pytest.raises(_lib.ArcleHipError, match="1024"):
        big.components_rows(big_rows, 4)
    torch.cuda.synchronize()
    assert bool((count == 77).all()) and bool((comp == 77).all()) and bool((bits == 77).all())
    assert call(b._h, 4, rows, rows.stride(0), 4) == 0 and call(b._h, 4, None, 0, 4) == 0  # (and the same arrays are served when asked properly)
    torch.cuda.synchronize()
    assert bool((count[:4] != 77).all()) and bool((count[4:] == 77).all())


# ---- planted two-object tasks, end to end ----------------------------------------------------------------------------------------------
def test_beam_search_with_object_proposals_solves_every_planted_task():
    from arcle_amd.envs import ARCVecEnv, O2ARCv2Env
    from arcle_amd.loaders import SyntheticLoader
    inputs, dims, answers, seqs = CP.planted_object_tasks(16)
    venv = ARCVecEnv(O2ARCv2Env, 16, SyntheticLoader(n_tasks=2, max_size=(12, 12)), max_grid_size=(12, 12), max_trial=3)
    venv.batch.set_tasks_padded(inputs, dims, answers, dims)
    venv.batch.reset()
    rows = venv.state_rows().clone()
    comp = venv.components(skip_color=0, max_components=16)
    assert comp.count.tolist() == [2] * 16 and comp.left.tolist() == [0] * 16 and tuple(comp.box.shape) == (16, 16, 4)
    propose = S.propose_objects(CP.MOVE_OPS, CP.FLOODFILL_OPS, skip_color=0)
    K = 16 * (len(CP.MOVE_OPS) + len(CP.FLOODFILL_OPS))
    rng = np.random.default_rng(0)
    a, d = rng.integers(0, 12, (K, 2)), rng.integers(0, 3, (K, 2))
    fixed = {"bbox": torch.from_numpy(np.concatenate([a, np.minimum(11, a + d)], 1).astype(np.int32)).cuda(),
             "operation": torch.from_numpy(rng.choice(CP.MOVE_OPS + CP.FLOODFILL_OPS, K).astype(np.int32)).cuda()}
    P, off = 144, _grid_offset("o2arc", 144)
    solved_fixed = 0
    for n in range(16):
        src = torch.tensor([n])
        res = S.beam_search(venv, rows[n:n + 1], None, width=16, depth=2, src_env=src, propose=propose)
        assert res.sequence is not None and res.root == 0, f"task {n}: no sequence from the object proposals (planted: {seqs[n]})"
        state = rows[n:n + 1]
        for act in res.sequence:
            state, _, _ = venv.transition(state, {"bbox": torch.tensor([act[:4]], dtype=torch.int32), "operation": torch.tensor([act[4]], dtype=torch.int32)},
                                          src.to(torch.int32))
        assert np.array_equal(state.cpu().numpy()[0, off:off + P].reshape(12, 12), answers[n]), (n, res.sequence, seqs[n])
        solved_fixed += S.beam_search(venv, rows[n:n + 1], fixed, width=16, depth=2, src_env=src).sequence is not None
    venv.check_errors()
    print(f"object proposals: 16 of 16 planted tasks solved; a fixed random set of the same K = {K}: {solved_fixed} of 16")
