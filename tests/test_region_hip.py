"""arcle_region_rows on the MI355X: EnvBatch.region_rows against arcle_amd.search.region_numpy over the emulator test's plan, against
the product's own Color steps (arcle_expand_rows on best_bits), the resident form, src_env and count edge cases, a caller-chosen plane
stride, graph capture, the refusals, and beam search painting the planted regions."""
import numpy as np
import pytest
import torch

import align as AL
import components as CP
import objects as OB
import regions as RG
import strides as STR
from arcle_amd import _lib
from arcle_amd import search as S

pytestmark = pytest.mark.gpu

_HIP = []
DEVICE_SIZES = ((5, 5), (7, 6), (6, 9), (12, 12), (30, 30), (32, 32), (16, 33), (65, 15))
NK = len(RG.DEFAULT)


def hip():
    if not _HIP:
        _HIP.append(RG.HipRegion())
    return _HIP[0]


def _creatable(H, W):
    """arcle_create serves the one-wavefront kernels where the reciprocal multiply divides every flat cell index by W exactly
    (tests/test_objects_hip.py)."""
    magic = 65536 // W + 1
    return all((n * magic) >> 16 == n // W for n in range(1024 + 16))


@pytest.mark.parametrize("H,W", DEVICE_SIZES)
def test_device_equals_the_mirror(H, W):
    """The emulator test's plan through the product (both `through` values, the default kinds, 16 kinds with zeros, repeats and a code
    above 7, one kind; count, src_env, base and best_bits given and NULL) plus 64 rows at the small sizes / 8 at the large ones under
    both `through` values: region, best, best_bits and base exact, entries >= count and the words around every output untouched.  Then
    the outputs of arcle_objects_rows fed in unchanged: the same answers as the mirror gives for components_numpy's masks."""
    assert _creatable(H, W)
    M = 64 if H * W <= 144 else 8
    extra = [("o2arc", "lib", M, 16, "sixteen", 0, True, True, True, True, True), ("arc", "odd", M, 16, "default", 0, False, True, False, True, True)]
    errs = RG.run_size(hip(), H, W, runs=RG.plan(H, W, full=True) + extra)
    assert not errs, "\n".join(errs[:10])
    cases = RG.cases_of(H, W)
    M = len(cases)
    b = hip().batch("o2arc", H, W, M)
    b.plane("answer").copy_(torch.as_tensor(np.stack([c["answer"] for c in cases]), device=b.device))
    b.field("answer_dim").copy_(torch.as_tensor(np.stack([c["adim"] for c in cases]), device=b.device))
    rows = torch.as_tensor(CP.make_rows("o2arc", cases, np.random.default_rng(4)), device=b.device)
    kinds = torch.as_tensor(np.array(RG.DEFAULT, np.uint8), device=b.device)
    for any_color, diagonal, through in ((True, True, False), (False, False, True)):
        count, comp, bits, _ = b.objects_rows(rows, 16, 0, any_color, diagonal, True)
        reg, best, bbits, base = (t.cpu().numpy() for t in b.region_rows(rows, count, bits, kinds, 0, through))
        for m, c in enumerate(cases):
            n, _, _, masks = S.components_numpy(c["grid"], c["dim"], 16, 0, any_color, diagonal)
            wr, wb, wbase = S.region_numpy(c["grid"], c["dim"], c["answer"], c["adim"], masks[:n], RG.DEFAULT, 0, through)
            assert int(count[m, 0]) == n and np.array_equal(reg[m, :n], wr) and np.array_equal(best[m, :n], wb) and tuple(base[m]) == wbase, (c["name"], through)
            assert not reg[m, n:].any() and not best[m, n:].any() and not bbits[m, n:].any()


@pytest.mark.parametrize("through", [False, True])
@pytest.mark.parametrize("H,W", RG.ORACLE_SIZES + ((12, 12), (32, 32), (16, 33)))
def test_best_candidates_are_the_products_own_color_steps(H, W, through):
    """Every object's best candidate as the step it stands for — best_bits as a "bits" selection with color_ops[best_color] — through
    arcle_expand_rows with the dense pair, on freshly reset rows: status 0 and dense[..., 0] == best_correct; the slots without a
    candidate carry an all-zero bit row."""
    from arcle_amd.engine import EnvBatch
    dev = torch.device("cuda:0")
    cases = RG.cases_of(H, W)
    M, C = len(cases), 16
    b = EnvBatch(M, H, W, 3, "o2arc")
    b.set_op_table(CP.OPS["o2arc"]())
    rows_np, _ = CP.clean_rows("o2arc", np.stack([c["grid"] for c in cases]), np.stack([c["dim"] for c in cases]), np.stack([c["answer"] for c in cases]),
                               np.stack([c["adim"] for c in cases]))
    b.plane("answer").copy_(torch.as_tensor(np.stack([c["answer"] for c in cases]), device=dev))
    b.field("answer_dim").copy_(torch.as_tensor(np.stack([c["adim"] for c in cases]), device=dev))
    rows = torch.as_tensor(rows_np, device=dev)
    count, bits = (torch.as_tensor(a, device=dev) for a in RG.PL.bit_rows(cases, C, True, np.random.default_rng(2)))
    kinds = torch.as_tensor(np.array(RG.DEFAULT, np.uint8), device=dev)
    reg, best, bbits, base = b.region_rows(rows, count, bits, kinds, 0, through)
    there = (torch.arange(C, device=dev).reshape(1, C) < count[:, :1]) & (best[..., 0] >= 0)
    op = torch.where(there, torch.as_tensor(RG.COLOR_OPS, dtype=torch.int32, device=dev)[best[..., 1].clamp(0, 9).long()], torch.full((), -1, dtype=torch.int32, device=dev))
    pay = torch.where(there.unsqueeze(-1), bbits, torch.zeros((), dtype=torch.uint8, device=dev)).contiguous()
    ex = b.expand_rows(rows, "bits", pay, op.contiguous(), None, dense=True)
    status, dense = ex.status.cpu().numpy(), ex.dense.cpu().numpy()
    there, best, bbits = there.cpu().numpy(), best.cpu().numpy(), bbits.cpu().numpy()
    assert there.sum() > M and not status[there].any()
    assert np.array_equal(dense[..., 0][there], best[..., 2][there]) and (dense[..., 1][there] == base.cpu().numpy()[:, 1:].repeat(C, 1)[there]).all()
    for m in range(M):
        for k in range(int(count[m, 0])):
            assert bool(bbits[m, k].any()) == bool(best[m, k, 0] >= 0) and int(np.unpackbits(bbits[m, k]).sum()) == best[m, k, 3]
    b.status(True)


def test_resident_rows_src_env_and_count_edges():
    """rows == NULL with and without src_env; a src_env that names no env; count 0 and count above max_comp."""
    H, W, C = 12, 12, 4
    cases = RG.cases_of(H, W)[-6:]
    M = len(cases)
    b = hip().batch("o2arc", H, W, M)
    dev = b.device
    rng = np.random.default_rng(3)
    b.plane("answer").copy_(torch.as_tensor(np.stack([c["answer"] for c in cases]), device=dev))
    b.field("answer_dim").copy_(torch.as_tensor(np.stack([c["adim"] for c in cases]), device=dev))
    b.set_state_rows(torch.as_tensor(CP.make_rows("o2arc", cases, rng), device=dev))
    cnt, bits = RG.PL.bit_rows(cases, C, True, rng)
    kinds = torch.as_tensor(np.array(RG.DEFAULT, np.uint8), device=dev)
    bits_t = torch.as_tensor(bits, device=dev)
    own = b.region_rows(None, torch.as_tensor(cnt, device=dev), bits_t, kinds)
    for m, c in enumerate(cases):
        wr, wb, wbase, wbits = RG.mirror(c, RG.DEFAULT, 0, False)
        n = min(C, len(wr))
        assert np.array_equal(own[0][m, :n].cpu().numpy(), wr[:n]) and np.array_equal(own[1][m, :n].cpu().numpy(), wb[:n]), c["name"]
        assert np.array_equal(own[2][m, :n].cpu().numpy(), wbits[:n]) and tuple(own[3][m].tolist()) == tuple(wbase)
    # src_env: row m judged by env (m + 1) % M, the last row by an env that does not exist
    src = ((np.arange(M) + 1) % M).astype(np.int32)
    src[-1] = M + 5
    got = b.region_rows(None, torch.as_tensor(cnt, device=dev), bits_t, kinds, src_env=torch.as_tensor(src, device=dev))
    for m, c in enumerate(cases[:-1]):
        o = cases[src[m]]
        wr, wb, wbase = S.region_numpy(c["grid"], c["dim"], o["answer"], o["adim"], c["masks"][:C], RG.DEFAULT)
        n = len(wr)
        assert np.array_equal(got[0][m, :n].cpu().numpy(), wr) and np.array_equal(got[1][m, :n].cpu().numpy(), wb) and tuple(got[3][m].tolist()) == wbase
    n = min(C, len(cases[-1]["masks"]))
    assert not got[0][-1, :n].any() and not got[1][-1, :n].any() and not got[2][-1, :n].any() and got[3][-1].tolist() == [0, 0]
    # count 0: nothing but base; count above max_comp: C objects
    cnt2 = cnt.copy()
    cnt2[0, 0], cnt2[1, 0] = 0, C + 7
    full_bits = RG.PL.bit_rows(cases, C, False, rng)[1]
    out = (torch.full((M, C, NK, 4), 77, dtype=torch.int32, device=dev), torch.full((M, C, 4), 77, dtype=torch.int32, device=dev),
           torch.full((M, C, 128), 77, dtype=torch.uint8, device=dev), torch.full((M, 2), 77, dtype=torch.int32, device=dev))
    b.region_rows(None, torch.as_tensor(cnt2, device=dev), torch.as_tensor(full_bits, device=dev), kinds, out=out)
    assert bool((out[0][0] == 77).all()) and bool((out[1][0] == 77).all()) and bool((out[2][0] == 77).all()) and out[3][0].tolist() == list(RG.mirror(cases[0], RG.DEFAULT, 0, False)[2])
    assert bool((out[0][1] != 77).any(-1).all()) and bool((out[1][1, :, 2] != 77).all())
    b.status(True)


def test_a_caller_chosen_plane_stride():
    """30 x 30 at plane stride 912 (57 live lanes, the last holding 4 cells and 12 padding bytes; rows never line-aligned): the plan's
    answers, zero padding and the slack behind every plane untouched."""
    assert (30, 30, 912) in [c[:3] for c in STR.SMALL]
    inst, check = STR.family_with_stride(RG.HipRegion, 912)
    errs = RG.run_size(inst, 30, 30) + check()
    assert not errs, "\n".join(errs[:10])


def test_regions_in_a_captured_graph_replay_with_new_rows_and_new_kinds():
    H, W = 20, 7
    cases = RG.cases_of(H, W)
    M, C = len(cases), 16
    rng = np.random.default_rng(1)
    b = hip().batch("o2arc", H, W, M)
    dev = b.device
    b.plane("answer").copy_(torch.as_tensor(np.stack([c["answer"] for c in cases]), device=dev))
    b.field("answer_dim").copy_(torch.as_tensor(np.stack([c["adim"] for c in cases]), device=dev))
    order = [np.arange(M)[::-1].copy(), np.roll(np.arange(M), 3)]
    buf = torch.as_tensor(CP.make_rows("o2arc", cases, rng), device=dev)
    count, bits = (torch.as_tensor(a, device=dev) for a in RG.PL.bit_rows(cases, C, True, rng))
    src = torch.arange(M, dtype=torch.int32, device=dev)
    kinds = torch.as_tensor(np.array(RG.DEFAULT, np.uint8), device=dev)
    b.region_rows(buf, count, bits, kinds, 0, False, src)  # (warm: the module is loaded before the capture)
    _, out = hip().outputs(dev, M, C, NK)
    out = tuple(out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        b.region_rows(buf, count, bits, kinds, 0, False, src, out=out)
    # the second replay also changes `kinds` in place: the kernel reads the device array when the launch runs (include/arcle_hip.h), so a
    # replay sees the bytes the array holds then — seven other codes, a zero and a code above 7 among them
    other = tuple(RG.KINDS16[5:12])
    assert len(other) == NK and other != RG.DEFAULT and 0 in other and max(other) > 7
    for perm, now in zip(order, (RG.DEFAULT, other)):
        cs = [cases[i] for i in perm]
        buf.copy_(torch.as_tensor(CP.make_rows("o2arc", cs, rng), device=dev))
        cn, bt = RG.PL.bit_rows(cs, C, True, rng)
        count.copy_(torch.as_tensor(cn, device=dev))
        bits.copy_(torch.as_tensor(bt, device=dev))
        src.copy_(torch.as_tensor(perm.astype(np.int32), device=dev))
        kinds.copy_(torch.as_tensor(np.array(now, np.uint8), device=dev))
        for t in out:
            t.fill_(RG.SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        errs = RG.compare("graph", tuple(t.cpu().numpy() for t in out) + ([],), cs, C, now, 0, False, True, True, True)
        assert not errs, "\n".join(errs[:10])


def test_refusals_return_their_codes_and_write_nothing():
    from arcle_amd.engine import EnvBatch
    L = _lib.lib()
    dev = torch.device("cuda:0")
    b = hip().batch("o2arc", 12, 12, 4)
    rows = b.get_state_rows().clone()
    count = torch.full((8, 2), 2, dtype=torch.int32, device=dev)
    bits = torch.full((8 * 4 * 128 + 2,), 77, dtype=torch.uint8, device=dev)
    kinds = torch.as_tensor(np.array(RG.KINDS16, np.uint8), device=dev)
    reg = torch.full((8, 4, 16, 4), 77, dtype=torch.int32, device=dev)
    best = torch.full((8, 4, 4), 77, dtype=torch.int32, device=dev)
    bbits = torch.full((8 * 4 * 128 + 2,), 77, dtype=torch.uint8, device=dev)
    base = torch.full((8, 2), 77, dtype=torch.int32, device=dev)
    ERR_ARG, ERR_CONFIG = -1, -2

    def call(h, n_rows, rows_t, stride, C, n_kinds=16, fc=0, through=0, bits_ptr=bits.data_ptr(), kinds_ptr=kinds.data_ptr(), reg_ptr=reg.data_ptr(),
             best_ptr=best.data_ptr(), bb_ptr=bbits.data_ptr()):
        return L.arcle_region_rows(h, n_rows, None if rows_t is None else rows_t.data_ptr(), stride, C, count.data_ptr(), bits_ptr, None, kinds_ptr, n_kinds, fc,
                                   through, reg_ptr, best_ptr, bb_ptr, base.data_ptr(), None)
    Lrow, st = b.state_row_size(), rows.stride(0)
    assert call(b._h, 4, rows, st, 0) == ERR_ARG and call(b._h, 4, rows, st, 1025) == ERR_ARG  # max_comp outside [1, 1024]
    assert call(b._h, 0, rows, st, 4) == ERR_ARG and call(b._h, -3, rows, st, 4) == ERR_ARG    # n_rows <= 0
    assert call(b._h, 4, rows, Lrow - 1, 4) == ERR_ARG                                        # stride below the row length
    assert call(b._h, 4, rows, st, 4, bits_ptr=None) == ERR_ARG and call(b._h, 4, rows, st, 4, bits_ptr=bits.data_ptr() + 1) == ERR_ARG  # NULL / odd bits
    assert call(b._h, 4, rows, st, 4, kinds_ptr=None) == ERR_ARG and call(b._h, 4, rows, st, 4, reg_ptr=None) == ERR_ARG and call(b._h, 4, rows, st, 4, best_ptr=None) == ERR_ARG
    assert call(b._h, 4, rows, st, 4, n_kinds=0) == ERR_ARG and call(b._h, 4, rows, st, 4, n_kinds=17) == ERR_ARG  # n_kinds outside [1, 16]
    assert call(b._h, 4, rows, st, 4, bb_ptr=bbits.data_ptr() + 1) == ERR_ARG                 # odd best_bits address
    assert call(b._h, 4, rows, st, 4, through=2) == ERR_ARG and call(b._h, 4, rows, st, 4, through=-1) == ERR_ARG
    assert call(b._h, 4, rows, st, 4, fc=128) == ERR_ARG and call(b._h, 4, rows, st, 4, fc=-129) == ERR_ARG
    assert call(b._h, 5, None, 0, 4) == ERR_ARG                                               # resident form with more rows than envs
    assert call(None, 4, rows, st, 4) == ERR_ARG
    # (the refusal "an env kind without an answer plane" cannot be reached through arcle_create: every env kind it serves — o2arc, arc,
    # raw — has one, as the siblings' refusal tests found; the check guards handles of kinds yet to come)
    assert all(EnvBatch(1, 5, 5, 3, kind).plane("answer") is not None for kind in ("o2arc", "arc", "raw"))
    big = EnvBatch(4, 40, 40, 3, "o2arc")
    big_rows = big.get_state_rows()
    assert call(big._h, 4, big_rows, big_rows.stride(0), 4) == ERR_CONFIG  # more than ARCLE_MAX_CELLS cells
    with pytest.raises(_lib.ArcleHipError, match="1024"):
        big.region_rows(big_rows, None, torch.zeros((4, 4, 128), dtype=torch.uint8, device=dev), kinds)
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in (bits, reg, best, bbits, base))
    # (and served when asked properly: a zero entry and a code above 7 in `kinds` are no refusal — the array is read on the device —; fc
    # at both ends; best_bits NULL and at an even offset)
    assert 0 in RG.KINDS16 and max(RG.KINDS16) > 7
    assert call(b._h, 4, rows, st, 4, fc=-128) == 0 and call(b._h, 4, None, 0, 4, fc=127, through=1, bits_ptr=bits.data_ptr() + 2, bb_ptr=None) == 0
    assert call(b._h, 4, rows, st, 4, bb_ptr=bbits.data_ptr() + 2) == 0
    torch.cuda.synchronize()
    assert bool((base[:4] != 77).all()) and bool((base[4:] == 77).all()) and bool((best[:4, :2] != 77).any()) and bool((best[:4, 2:] == 77).all()) and bool((best[4:] == 77).all())
    assert bool((reg[:4, :2] != 77).any(-1).all()) and bool((reg[:4, 2:] == 77).all()) and bool((reg[4:] == 77).all())
    b.status(True)


# ---- planted region tasks, end to end ------------------------------------------------------------------------------------------------
def test_beam_search_paints_the_planted_regions():
    """The demonstration of tests/test_region_host.py through ARCVecEnv: propose_regions(range(10), through=True) at width 1, depth =
    the number of objects solves 8 of 8 with the same sequences as the oracle-backed stub, each replaying to the answer on the oracle;
    `regions` equals the host mirror.  (The seven earlier proposers solve RG.BEFORE_SOLVES = 0 of these tasks at the same width and
    depth: tests/test_region_host.py runs them on the stub.)"""
    from arcle_amd.envs import ARCVecEnv, O2ARCv2Env
    from arcle_amd.envs.vec import Regions
    from arcle_amd.loaders import SyntheticLoader
    inputs, dims, answers, depths, _ = RG.planted_region_tasks(8)
    venv = ARCVecEnv(O2ARCv2Env, 8, SyntheticLoader(n_tasks=2, max_size=(12, 12)), max_grid_size=(12, 12), max_trial=3)
    venv.batch.set_tasks_padded(inputs, dims, answers, dims)
    venv.batch.reset()
    rows = venv.state_rows().clone()
    objs = venv.components(rows, skip_color=0, max_components=16, bits=True)
    want_objs = OB.objects_numpy(inputs, dims, 16, 0, False, False, True, False)
    for kinds, through in ((None, False), (RG.KINDS16, True)):
        got = venv.regions(rows, objs, kinds, 0, through)
        want = RG.region_numpy_rows(inputs, dims, answers, dims, want_objs, kinds, 0, through)
        assert isinstance(got, Regions)
        for f in Regions._fields:
            assert np.array_equal(getattr(got, f).cpu().numpy(), getattr(want, f).numpy()), (f, through)
    assert venv.regions(rows, objs, bits=False).best_bits is None
    own = venv.regions(None, venv.components(skip_color=0, max_components=16, bits=True))
    assert all(torch.equal(a, c) for a, c in zip(own, venv.regions(rows, objs)))
    painted, _ = RG.searches(venv, rows, 8, depths, before=False)
    rows_np = CP.clean_rows("o2arc", inputs, dims, answers, dims)[0]
    stub, _ = RG.searches(RG.region_venv(answers, dims), torch.from_numpy(rows_np), 8, depths, before=False)
    assert sum(r.sequence is not None for r in painted) == 8
    for i, (r, s) in enumerate(zip(painted, stub)):
        assert r.root == 0 and len(r.sequence) == len(s.sequence) == depths[i], i
        assert all(np.array_equal(a[0], c[0]) and a[1] == c[1] for a, c in zip(r.sequence, s.sequence)), i
        assert AL.replay_on_oracle(rows_np[i], answers[i], dims[i], r.sequence) == 1, i
    venv.check_errors()
