"""Bit-packed selection masks in arcle_expand_rows / arcle_transition_rows on the MI355X: the checks of tests/search_bits.py through the
product, the components' bit rows fed into the expansion as they stand, graph capture, the refusals, and beam search over the objects'
exact masks on planted tasks a bounding box cannot solve."""
import numpy as np
import pytest
import torch

import components as CP
import search as SR
import search_bits as SB
from arcle_amd import search as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def test_bit_row_expansion_equals_oracle_hip():
    errs = SB.expansion(SB.HipBitsBackend)
    assert not errs, "\n".join(errs[:10])


def test_rectangle_bit_rows_equal_the_bbox_expansion_hip():
    errs = SB.rectangles(SB.HipBitsBackend)
    assert not errs, "\n".join(errs[:10])


def test_chunk_boundaries_do_not_matter_hip():
    errs = SB.chunks(SB.HipBitsBackend)
    assert not errs, "\n".join(errs[:10])


def test_bit_row_transitions_equal_oracle_and_expansion_hip():
    errs = SB.transitions(SB.HipBitsBackend)
    assert not errs, "\n".join(errs[:10])


def test_bit_row_transitions_under_every_flag_hip():
    errs = SB.flagged_transitions(SB.HipBitsBackend)
    assert not errs, "\n".join(errs[:10])


def test_bits_beyond_the_grid_are_ignored_hip():
    errs = SB.stray_bits(SB.HipBitsBackend)
    assert not errs, "\n".join(errs[:10])


def _case(kind="o2arc", H=30, W=30, mt=3):
    be, orc, rng, ops, base, answers, adims = SB.mix_case(SB.HipBitsBackend, kind, H, W, mt)
    return be, rng, ops, base, answers, adims


def test_components_bit_rows_feed_the_expansion_as_they_stand():
    """components_rows(bits=True, max_comp=K) IS a per-row `sel`: the tensor it wrote goes into expand_rows, no copy, no repacking."""
    kind, H, W, mt, K = "o2arc", 30, 30, 3, SB.K_MIX
    be, rng, ops, base, answers, adims = _case(kind, H, W, mt)
    dev, M = be.b.device, len(base)
    rows = torch.as_tensor(base, device=dev)
    count, comp, bits = be.b.components_rows(rows, K, 0, bits=True)
    n = count[:, 0].cpu().numpy()
    op = rng.integers(0, len(ops), (M, K)).astype(np.int32)
    pad = np.arange(K)[None, :] >= n[:, None]
    op[pad] = -1  # slots the components call never wrote (the bit rows there are the zeros the tensor was made with)
    ex = be.b.expand_rows(rows, "bits", bits, torch.as_tensor(op, device=dev), dense=True)
    masks = np.zeros((M, K, H, W), np.int8)
    grids, gdims = SB._grids_of(base, kind, H, W)
    for m in range(M):
        masks[m] = S.components_numpy(grids[m], gdims[m], K, 0)[3]
    want = SR.oracle_expand(base, answers, adims, kind, H, W, mt, ops, "mask", masks.reshape(M, K, -1), np.where(pad, 0, op).astype(np.int32))
    want["status"][pad] = SR.ST_BAD_OP
    want["rows"][pad] = np.broadcast_to(base[:, None, :], want["rows"].shape)[pad]
    want["reward"][pad], want["term"][pad], want["dense"][pad] = 0, 0, 0
    changed = float((want["rows"] != base[:, None, :]).any(2).mean())
    assert changed >= 0.40, f"only {changed:.2f} of the children differ from their parent"
    got = {"reward": ex.reward.cpu().numpy(), "term": ex.term.cpu().numpy(), "status": ex.status.cpu().numpy(), "dense": ex.dense.cpu().numpy(),
           "hash": ex.hash.cpu().numpy().view(np.uint64), "parent_hash": ex.parent_hash.cpu().numpy().view(np.uint64)}
    errs = []
    SB._compare(errs, "components bit rows", got, want, base, kind, H, W, op)
    assert not errs, "\n".join(errs[:10])


def test_bit_row_expansion_in_a_captured_graph():
    kind, H, W, mt, K = "o2arc", 30, 30, 3, SB.K_MIX
    be, rng, ops, base, _, _ = _case(kind, H, W, mt)
    dev, M = be.b.device, 11
    src = torch.as_tensor(rng.integers(0, 8, M).astype(np.int32), device=dev)
    rows = torch.as_tensor(base, device=dev).index_select(0, src.long()).contiguous()
    grids, gdims = SB._grids_of(rows.cpu().numpy(), kind, H, W)
    bits = S.pack_bits(torch.as_tensor(SB.mask_mix(rng, grids, gdims, K, H, W), device=dev))
    op = torch.as_tensor(rng.integers(0, len(ops), (M, K)).astype(np.int32), device=dev)
    ref = be.b.expand_rows(rows, "bits", bits, op, src, dense=True)
    torch.cuda.synchronize()
    out = type(ref)(*[torch.zeros_like(t) for t in ref])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        be.b.expand_rows(rows, "bits", bits, op, src, dense=True, out=out)
    for _ in range(3):
        for t in out:
            t.fill_(0x33)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, ref):
            assert torch.equal(a, b)


def test_refusals_return_their_codes_and_write_nothing():
    from arcle_amd import _lib
    from arcle_amd.engine import EnvBatch
    L = _lib.lib()
    ERR_ARG, ERR_CONFIG, MASK, BBOX5, BITS = -1, -2, 0, 3, 4
    be, rng, ops, base, _, _ = _case("o2arc", 12, 12, 1)
    dev, M, K = be.b.device, 8, 4
    rows = torch.as_tensor(base, device=dev)
    sel = torch.zeros(M * K * 144 + 2, dtype=torch.uint8, device=dev)  # (large enough for any form asked below)
    op = torch.zeros((M, K), dtype=torch.int32, device=dev)
    outs = [torch.full((M, K, 4), 0x77, dtype=torch.uint8, device=dev), torch.full((M, K), 0x77, dtype=torch.uint8, device=dev),
            torch.full((M, K), 0x77, dtype=torch.uint8, device=dev), torch.full((M, K, 16), 0x77, dtype=torch.uint8, device=dev),
            torch.full((M, K, 8), 0x77, dtype=torch.uint8, device=dev), torch.full((M, 16), 0x77, dtype=torch.uint8, device=dev)]

    def expand(h, r, ingress, sel_ptr):
        return L.arcle_expand_rows(h, M, r.data_ptr(), r.stride(0), K, ingress, sel_ptr, op.data_ptr(), K, None, outs[0].data_ptr(), outs[1].data_ptr(),
                                   outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr(), outs[5].data_ptr(), 0, None)
    assert sel.data_ptr() % 2 == 0
    assert expand(be.b._h, rows, MASK, sel.data_ptr()) == ERR_ARG         # int8 masks are not served by the expansion
    assert expand(be.b._h, rows, BBOX5, sel.data_ptr()) == ERR_ARG
    assert expand(be.b._h, rows, BITS, sel.data_ptr() + 1) == ERR_ARG     # a bit row is read as uint16 words: 2-byte aligned
    with pytest.raises(_lib.ArcleHipError, match="2-byte aligned"):
        be.b.expand_rows(rows, "bits", sel[1:1 + M * K * 128].reshape(M, K, 128), op)
    big = EnvBatch(M, 40, 40, 3, "o2arc")
    big.set_op_table(O.o2arc_ops())
    big_rows = big.get_state_rows()
    assert expand(big._h, big_rows, BITS, sel.data_ptr()) == ERR_CONFIG   # big grids: as for the tuple forms
    Lb = big.state_row_size()
    out_rows = torch.full((M, ((Lb + 15) & ~15) + 16), 0x77, dtype=torch.int8, device=dev)
    big_sel = torch.zeros((M, big.bits_stride), dtype=torch.uint8, device=dev)

    def transition(h, r, ingress, sel_ptr, out):
        return L.arcle_transition_rows(h, M, r.data_ptr(), r.stride(0), ingress, sel_ptr, op.data_ptr(), None, out.data_ptr(), out.stride(0), 1,
                                       outs[0].data_ptr(), outs[1].data_ptr(), 0, None)
    assert transition(big._h, big_rows, BITS, big_sel.data_ptr(), out_rows) == ERR_ARG  # bit rows beyond 30 x 30 are parked
    with pytest.raises(_lib.ArcleHipError, match=r"\(-1\)"):
        big.transition_rows(big_rows, "bits", big_sel, op[:, 0].contiguous())
    Ls = be.b.state_row_size()
    small_out = torch.full((M, ((Ls + 15) & ~15) + 16), 0x77, dtype=torch.int8, device=dev)
    assert transition(be.b._h, rows, BITS, sel.data_ptr() + 1, small_out) == ERR_ARG
    torch.cuda.synchronize()
    assert all(bool((t == 0x77).all()) for t in outs + [out_rows, small_out]), "a refused call wrote to its outputs"
    assert be.b.status(False) == 0 and big.status(False) == 0
    # ... and the same arrays are served when asked properly
    assert expand(be.b._h, rows, BITS, sel.data_ptr()) == 0 and transition(be.b._h, rows, BITS, sel.data_ptr(), small_out) == 0
    torch.cuda.synchronize()
    assert not bool((outs[3] == 0x77).all()) and not bool((small_out == 0x77).all())
    be.b.status(True)


def test_beam_search_on_masks_solves_the_planted_tasks_like_the_stub():
    """The planted tasks of tests/test_search_bits_host.py through ARCVecEnv: the sequences equal the oracle-backed stub's."""
    from arcle_amd.envs import ARCVecEnv, O2ARCv2Env
    from arcle_amd.loaders import SyntheticLoader
    n_tasks = 8
    inputs, dims, answers, depths = SB.planted_mask_tasks(n_tasks)
    venv = ARCVecEnv(O2ARCv2Env, n_tasks, SyntheticLoader(n_tasks=2, max_size=(10, 10)), max_grid_size=(10, 10), max_trial=3)
    venv.batch.set_tasks_padded(inputs, dims, answers, dims)
    venv.batch.reset()
    rows = venv.state_rows().clone()
    stub = SB.MaskVenv("o2arc", 10, 10, 3, O.o2arc_ops(), answers, dims)
    stub_rows, _ = CP.clean_rows("o2arc", inputs, dims, answers, dims)
    ops = SB.COLOR_OPS + SB.MOVE_OPS
    for n in range(n_tasks):
        src = torch.tensor([n])
        for masks in (True, False):
            propose = S.propose_objects(ops, [], max_components=4, masks=masks)
            res = S.beam_search(venv, rows[n:n + 1], None, width=64, depth=depths[n], src_env=src, propose=propose)
            want = S.beam_search(stub, torch.from_numpy(stub_rows[n:n + 1]), None, width=64, depth=depths[n], src_env=src, propose=propose)
            assert res.counts == want.counts and res.root == want.root, (n, masks, res.counts, want.counts)
            if not masks:
                assert res.sequence is None and want.sequence is None, (n, res.sequence)
                continue
            assert res.sequence is not None and len(res.sequence) == len(want.sequence) == depths[n], n
            for (sa, oa), (sb, ob) in zip(res.sequence, want.sequence):
                assert oa == ob and sa.dtype == bool and np.array_equal(sa, sb), (n, oa, ob)
            assert SB.replay_masks_on_oracle(inputs[n], dims[n], answers[n], res.sequence) == 1, n
    venv.check_errors()


def test_bit_rows_at_the_fast_widths_hip():
    """20 x 24 and 16 x 16 at the default stride: the FW_FAST kernels with 32 and 16 live lanes"""
    errs = SB.expansion(SB.HipBitsBackend, cases=SR.FAST_CASES) + SB.transitions(SB.HipBitsBackend, cases=SR.FAST_CASES)
    assert not errs, "\n".join(errs[:10])
