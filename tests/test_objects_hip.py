"""arcle_objects_rows on the MI355X: EnvBatch.objects_rows against the union-find labelling of tests/objects.py over the emulator test's
case list with every case included, mode 0 against components_rows on the same rows, graph capture, the refusals, the untouched handle,
and beam search moving whole multi-colour / diagonal objects on planted tasks."""
import numpy as np
import pytest
import torch

import components as CP
import objects as OB
import search as SR
import search_bits as SB
from arcle_amd import _lib
from arcle_amd import search as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu

_HIP = []


def hip():
    if not _HIP:
        _HIP.append(OB.HipObjects())
    return _HIP[0]


def _creatable(H, W):
    """arcle_create serves the one-wavefront kernels where the reciprocal multiply divides every flat cell index by W exactly
    (tests/test_components_hip.py): 8 x 127 is not such a shape."""
    magic = 65536 // W + 1
    return all((n * magic) >> 16 == n // W for n in range(1024 + 16))


@pytest.mark.parametrize("H,W", OB.SIZES)
def test_device_equals_the_mirror(H, W):
    """The emulator test's plan through the product, all four modes, with EVERY case of the size (the 900-object checkerboards too):
    (written, left), every descriptor, every bit row, every colours word exact, sentinels intact beyond `written`.  A shape no handle
    of the product can hold (8 x 127: the emulator test covers it) must be refused at creation as it always was."""
    if not _creatable(H, W):
        from arcle_amd.engine import EnvBatch
        with pytest.raises(_lib.ArcleHipError):
            EnvBatch(2, H, W, 3, "o2arc")
        return
    errs = OB.run_size(hip(), H, W)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("H,W", [(30, 30), (20, 7), (16, 33)])
def test_mode_0_is_components_rows(H, W):
    """Neither flag: count, comp and bits of components_rows on the same rows, byte for byte — without `colors` (the same kernel) and
    with it (the mode-0 instantiation of the new one)."""
    cases = OB.cases_of(H, W)
    b = hip().batch("o2arc", H, W, 2)
    rows = torch.as_tensor(CP.make_rows("o2arc", cases, np.random.default_rng(2)), device=b.device)
    for C, skip in ((5, -1), (1024, 0)):
        old = b.components_rows(rows, C, skip, True)  # (zero-filled outputs on both sides)
        for colors in (False, True):
            new = b.objects_rows(rows, C, skip, False, False, True, colors)
            assert all(torch.equal(a, c) for a, c in zip(old, new[:3])), (C, skip, colors)


def test_objects_in_a_captured_graph_replay_with_new_rows():
    H, W = 20, 7
    cases = OB.cases_of(H, W)
    rng = np.random.default_rng(1)
    first, second = CP.make_rows("o2arc", cases, rng), CP.make_rows("o2arc", cases[::-1], rng)
    b = hip().batch("o2arc", H, W, 2)
    buf = torch.as_tensor(first, device=b.device)
    C, mode = 8, OB.ANY | OB.DIAG
    b.objects_rows(buf, C, 0, True, True, True, True)  # (warm: the module is loaded before the capture)
    out = hip()._out(b, len(cases), C, True, True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        b.objects_rows(buf, C, 0, True, True, True, True, out=out)
    for rows_np, cs in ((first, cases), (second, cases[::-1]), (first, cases)):
        buf.copy_(torch.as_tensor(rows_np, device=b.device))
        for t in out:
            t.fill_(OB.SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        errs = OB.compare("graph", hip()._np(out), cs, C, 0, mode, True, True)
        assert not errs, "\n".join(errs[:10])


def test_refusals_return_their_codes_and_write_nothing():
    from arcle_amd.engine import EnvBatch
    L = _lib.lib()
    dev = torch.device("cuda:0")
    b = hip().batch("o2arc", 12, 12, 4)
    rows = b.get_state_rows().clone()
    count = torch.full((8, 2), 77, dtype=torch.int32, device=dev)
    comp = torch.full((8, 4, 8), 77, dtype=torch.int32, device=dev)
    bits = torch.full((8, 4, 128), 77, dtype=torch.uint8, device=dev)
    cols = torch.full((8, 4), 77, dtype=torch.int32, device=dev)
    ERR_ARG, ERR_CONFIG = -1, -2

    def call(h, n_rows, rows_t, stride, C, mode=3, cnt=count, cmp_=comp):
        return L.arcle_objects_rows(h, n_rows, None if rows_t is None else rows_t.data_ptr(), stride, C, -1, mode,
                                    None if cnt is None else cnt.data_ptr(), None if cmp_ is None else cmp_.data_ptr(), bits.data_ptr(), cols.data_ptr(), None)
    Lrow = b.state_row_size()
    for mode in (0, 1, 2, 3):
        assert call(b._h, 4, rows, rows.stride(0), 0, mode) == ERR_ARG and call(b._h, 4, rows, rows.stride(0), 1025, mode) == ERR_ARG  # max_comp outside [1, 1024]
        assert call(b._h, 4, rows, Lrow - 1, 4, mode) == ERR_ARG        # stride below the row length
        assert call(b._h, 5, None, 0, 4, mode) == ERR_ARG               # resident form with more rows than envs
        assert call(b._h, 0, rows, rows.stride(0), 4, mode) == ERR_ARG  # n_rows == 0
        assert call(b._h, 4, rows, rows.stride(0), 4, mode, cnt=None) == ERR_ARG and call(None, 4, rows, rows.stride(0), 4, mode) == ERR_ARG
    for mode in (4, 8, 7, 0x80000001):
        assert call(b._h, 4, rows, rows.stride(0), 4, mode) == ERR_ARG  # unknown mode bits
    big = EnvBatch(4, 40, 40, 3, "o2arc")
    big_rows = big.get_state_rows()
    assert call(big._h, 4, big_rows, big_rows.stride(0), 4) == ERR_CONFIG  # more than ARCLE_MAX_CELLS cells
    with pytest.raises(_lib.ArcleHipError, match="1024"):
        big.objects_rows(big_rows, 4, diagonal=True)
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in (count, comp, bits, cols))
    assert call(b._h, 4, rows, rows.stride(0), 4) == 0 and call(b._h, 4, None, 0, 4, 0) == 0  # (and the same arrays are served when asked properly)
    torch.cuda.synchronize()
    assert bool((count[:4] != 77).all()) and bool((count[4:] == 77).all())
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
    b.objects_rows(None, 16, 0, True, True, True, True)
    b.objects_rows(rows, 1024, -1, False, True, False, True)
    b.objects_rows(rows, 5, 3, True, False, True, False)
    after = snapshot()
    for x, y in zip(before[:5], after[:5]):
        assert np.array_equal(x, y)
    assert all(np.array_equal(before[5][k], after[5][k]) for k in before[5]) and np.array_equal(before[6], after[6])
    b.status(True)


# ---- planted whole-object tasks, end to end ---------------------------------------------------------------------------------------------
def test_beam_search_moves_whole_objects_only_with_the_wider_notion():
    """The demonstration of tests/test_objects_host.py through ARCVecEnv: 0 of 8 with the one-colour 4-connected components, 8 of 8
    with any_color + diagonal; the returned step replayed on the oracle gives the answer; `objects` equals the host mirror."""
    from arcle_amd.envs import ARCVecEnv, O2ARCv2Env
    from arcle_amd.envs.vec import Objects
    from arcle_amd.loaders import SyntheticLoader
    inputs, dims, answers, steps = OB.planted_whole_object_tasks(8)
    venv = ARCVecEnv(O2ARCv2Env, 8, SyntheticLoader(n_tasks=2, max_size=(12, 12)), max_grid_size=(12, 12), max_trial=3)
    venv.batch.set_tasks_padded(inputs, dims, answers, dims)
    venv.batch.reset()
    rows = venv.state_rows().clone()
    obj = venv.objects(skip_color=0, max_components=4, any_color=True, diagonal=True, bits=True, colors=True)
    want = OB.objects_numpy(inputs, dims, 4, 0, True, True, True, True)
    assert isinstance(obj, Objects) and obj.count.tolist() == [1] * 8 and obj.left.tolist() == [0] * 8
    for f in ("box", "seed", "color", "cells", "bits", "colors"):
        assert np.array_equal(getattr(obj, f).cpu().numpy()[:, :1], getattr(want, f).numpy()[:, :1]), f
    plain = venv.objects(rows, skip_color=0, max_components=4)
    comp = venv.components(rows, skip_color=0, max_components=4)
    assert plain.colors is None and all(torch.equal(a, b) for a, b in zip(plain[:6], comp[:6]))
    narrow, wide = OB.whole_object_searches(venv, rows, 8)
    assert sum(r.sequence is not None for r in narrow) == 0, [r.sequence for r in narrow]
    assert sum(r.sequence is not None for r in wide) == 8
    for i, r in enumerate(wide):
        assert len(r.sequence) == 1 and r.root == 0
        sel, op = r.sequence[0]
        assert np.array_equal(sel, steps[i][0]) and op == steps[i][1], i
        assert SB.replay_masks_on_oracle(inputs[i], dims[i], answers[i], r.sequence) == 1, i
    venv.check_errors()
