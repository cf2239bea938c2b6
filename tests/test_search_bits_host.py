"""The host side of the mask proposals: pack_bits / unpack_bits, object_actions(masks=True), and beam_search over bit-row candidates
on a stub vec env backed by the oracle (tests/search_bits.py::MaskVenv; torch CPU tensors, no GPU): planted tasks whose object is
not its filled bounding box are solved with the objects' exact masks and not with their boxes."""
import numpy as np
import pytest
import torch

import components as CP
import search_bits as SB
from arcle_amd import search as S
from oracle import oracle as O


@pytest.mark.parametrize("H,W", [(30, 30), (7, 12), (32, 32), (5, 5), (1, 1)])
def test_pack_bits_is_numpy_packbits_little(H, W):
    rng = np.random.default_rng(H * 100 + W)
    m = (rng.integers(-2, 3, (3, 5, H, W)) * (rng.random((3, 5, H, W)) < 0.4)).astype(np.int8)
    m[0, 0], m[0, 1] = 0, 1
    want = np.zeros((3, 5, 128), np.uint8)
    pk = np.packbits((m != 0).reshape(3, 5, -1), axis=-1, bitorder="little")
    want[..., :pk.shape[-1]] = pk
    for t in (torch.from_numpy(m), torch.from_numpy(m != 0)):
        got = S.pack_bits(t)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (3, 5, 128) and np.array_equal(got.numpy(), want)
    assert np.array_equal(S.pack_bits(torch.from_numpy(m[1, 2])).numpy(), want[1, 2])  # no leading axes
    back = S.unpack_bits(torch.from_numpy(want), H, W)
    assert back.dtype == torch.bool and np.array_equal(back.numpy(), m != 0)
    dirty = want.copy()
    dirty.reshape(-1, 1024 // 8)[:, (H * W + 7) // 8:] = 0xFF  # bits beyond H * W are dropped
    if H * W % 8:
        dirty[..., H * W // 8] |= (0xFF << (H * W % 8)) & 0xFF
    assert np.array_equal(S.unpack_bits(torch.from_numpy(dirty), H, W).numpy(), m != 0)


def test_object_actions_with_masks_against_numpy():
    cases = [c for c in CP.fixture() if c["grid"].shape == (12, 12)][:8]
    assert len(cases) >= 4
    venv = SB.MaskVenv("o2arc", 12, 12, 3, O.o2arc_ops(), None, None)
    rows, _ = CP.clean_rows("o2arc", np.stack([c["grid"] for c in cases]), np.stack([np.asarray(c["dim"], np.int8) for c in cases]))
    C, box_ops, seed_ops = 6, [20, 21, 3], [10, 15]
    comp = venv.components(torch.from_numpy(rows), C, 0, bits=True)
    a = S.object_actions(comp, box_ops, seed_ops, masks=True)
    M, per = len(cases), 5
    assert set(a) == {"bits", "operation"}
    assert tuple(a["bits"].shape) == (M, C * per, 128) and a["bits"].dtype == torch.uint8 and a["bits"].is_contiguous()
    assert tuple(a["operation"].shape) == (M, C * per) and a["operation"].dtype == torch.int32
    assert int(comp.count.min()) < C, "no padded row in the batch"
    bits, op = a["bits"].reshape(M, C, per, 128).numpy(), a["operation"].reshape(M, C, per).numpy()
    for m, c in enumerate(cases):
        n, _, desc, masks = S.components_numpy(c["grid"], c["dim"], C, 0)
        assert (op[m, n:] == -1).all() and not bits[m, n:].any() and (op[m, :n] == np.array(box_ops + seed_ops)).all()
        for k in range(n):
            cells = np.unpackbits(bits[m, k], axis=-1, bitorder="little")[:, :144].reshape(per, 12, 12)
            assert (cells[:3] == masks[k]).all()
            seed = np.zeros((12, 12), np.uint8)
            seed[desc[k, 4], desc[k, 5]] = 1
            assert (cells[3:] == seed).all()
    with pytest.raises(AssertionError):
        S.object_actions(venv.components(torch.from_numpy(rows), C, 0), box_ops, seed_ops, masks=True)
    # masks=False is the box form as before
    b = S.object_actions(comp, box_ops, seed_ops)
    assert set(b) == {"bbox", "operation"} and torch.equal(b["operation"], a["operation"])


N_TASKS = 8


def test_planted_objects_are_not_their_boxes():
    inputs, dims, answers, depths = SB.planted_mask_tasks(N_TASKS)
    assert len(inputs) >= 8 and sorted(set(depths)) == [1, 2]
    for g in inputs:
        n, left, comp, masks = S.components_numpy(g, (10, 10), 16, 0)
        assert n == 3 and left == 0
        big = int(np.argmax(comp[:n, 7]))
        x0, y0, x1, y1 = comp[big, :4]
        assert SB.not_filled_box(masks[big]) and (g[x0:x1 + 1, y0:y1 + 1][masks[big, x0:x1 + 1, y0:y1 + 1] == 0] != 0).any(), "no foreign cell in the box"


def test_beam_search_on_masks_solves_what_boxes_cannot():
    """The exact masks reach the planted answers, replayed on the oracle; the boxes of the same objects do not, at the same depth."""
    inputs, dims, answers, depths = SB.planted_mask_tasks(N_TASKS)
    rows, _ = CP.clean_rows("o2arc", inputs, dims, answers, dims)
    venv = SB.MaskVenv("o2arc", 10, 10, 3, O.o2arc_ops(), answers, dims)
    ops = SB.COLOR_OPS + SB.MOVE_OPS
    for n in range(N_TASKS):
        root, src = torch.from_numpy(rows[n:n + 1]), torch.tensor([n])
        res = S.beam_search(venv, root, None, width=64, depth=depths[n], src_env=src, propose=S.propose_objects(ops, [], max_components=4, masks=True))
        assert res.sequence is not None and len(res.sequence) == depths[n] and res.root == 0, n
        for sel, op in res.sequence:
            assert isinstance(sel, np.ndarray) and sel.dtype == bool and sel.shape == (10, 10) and isinstance(op, int)
        assert SB.replay_masks_on_oracle(inputs[n], dims[n], answers[n], res.sequence) == 1, (n, res.sequence)
        boxes = S.beam_search(venv, root, None, width=64, depth=depths[n], src_env=src, propose=S.propose_objects(ops, [], max_components=4))
        assert boxes.sequence is None, f"task {n}: the boxes reach the answer at depth {depths[n]}: {boxes.sequence}"


def test_beam_search_takes_one_shared_set_of_bit_rows():
    """Without `propose`: one candidate set for every state, the sequence is indices into it."""
    inputs, dims, answers, depths = SB.planted_mask_tasks(N_TASKS)
    rows, _ = CP.clean_rows("o2arc", inputs, dims, answers, dims)
    venv = SB.MaskVenv("o2arc", 10, 10, 3, O.o2arc_ops(), answers, dims)
    n = depths.index(1)
    comp = venv.components(torch.from_numpy(rows[n:n + 1]), 4, 0, bits=True)
    a = S.object_actions(comp, SB.COLOR_OPS, [], masks=True)
    acts = {"bits": a["bits"][0], "operation": a["operation"][0]}
    res = S.beam_search(venv, torch.from_numpy(rows[n:n + 1]), acts, width=64, depth=1, src_env=torch.tensor([n]))
    assert res.sequence is not None and len(res.sequence) == 1
    k = res.sequence[0]
    sel = S.unpack_bits(acts["bits"][k], 10, 10).numpy()
    assert SB.replay_masks_on_oracle(inputs[n], dims[n], answers[n], [(sel, int(acts["operation"][k]))]) == 1
