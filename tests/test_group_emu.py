"""The launch that orders itself, on the CPU (tests/grouping.py, tests/emu/group_emu.cpp: arcle_amd/csrc/arcle_group.h compiled with g++).

On the GPU a self-ordering launch is only ever compared with its plain twin under whatever wave schedule the hardware happens to produce.
Here the schedule is an argument: the slots of a launch run one after the other, each wave to completion, ascending, descending and
shuffled — so a permutation that depends on anything a wave of the launch writes (the step counters did, for the research step: an env
about to be re-initialised counted as a long wave) steps one env twice and another not at all, and the comparison fails."""
import numpy as np
import pytest

import grouping as G
from oracle import oracle as O

WPW = (1, 2, 4, 8, 16)


def test_smallest_size_and_reciprocal():
    """512 is the smallest batch grouped_applies admits (two groups per XCD); the reciprocal is launch_step's."""
    assert G.grouped_applies(512) and not any(G.grouped_applies(n) for n in range(1, 512))
    assert G.group_magic(512) == 0x80000001 and G.group_magic(8192) == (1 << 32) // 32 + 1


def test_geometry_every_size_and_workgroup_shape():
    """Every batch size a self-ordering launch can have up to the streaming regime, and 2^20: the slots' (group, position) cover each env
    exactly once and the reciprocal multiplication divides every s_local exactly."""
    errs = []
    for n in list(range(512, 66560 + 1, 256)) + [1 << 20]:
        assert G.grouped_applies(n)
        for wpw in WPW:
            errs += G.geometry_errors(n, wpw)
    assert not errs, "\n".join(errs[:10])


def _op_rows_from_masks(masks, rng, bad=True):
    """int32 [len(masks), 32] op indices whose object-op positions are the masks' bits: long = one of the eight Move / Rotate / Flip slots,
    other = any other slot of the table or (bad) an index beyond it — 35 .. 74, i.e. past bit 63 of the mask as well — or negative"""
    masks = np.asarray(masks, np.uint64)
    bits = ((masks[:, None] >> np.arange(32, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    other = np.array([k for k in range(35) if k not in range(20, 28)] + (list(range(35, 75)) + [-1, 1 << 30] if bad else []), np.int32)
    ops = other[rng.integers(0, len(other), bits.shape)]
    ops[bits] = rng.integers(20, 28, int(bits.sum()))
    return ops


def test_trade_is_a_permutation_for_every_kind_of_group():
    rng = np.random.default_rng(5)
    mask = G.long_mask(O.o2arc_ops())
    assert mask == 0xFF << 20
    full = (1 << 32) - 1
    special = [0, full] + [1 << k for k in range(32)] + [full ^ (1 << k) for k in range(32)]      # popcount 0, 32, 1, 31
    special += [(1 << k) - 1 for k in range(33)] + [full ^ ((1 << k) - 1) for k in range(33)]      # the first k / all but the first k
    errs = G.trade_errors(_op_rows_from_masks(special, rng), mask, "special masks")
    errs += G.trade_errors(_op_rows_from_masks(special, rng, bad=False), mask, "special masks, ops inside the table")
    errs += G.trade_errors(_op_rows_from_masks(rng.integers(0, 1 << 32, 100000, dtype=np.uint64), rng), mask, "random masks")
    assert not errs, "\n".join(errs[:10])


def test_trade_on_the_adversarial_streams_of_the_gpu_tests():
    """tests/test_round5_hip.py::_streams: the C3 mix, every env the same object op, none, one in the last position, the late half, alternating,
    all but position 0, a coin, half the batch, out-of-range op indices in every group"""
    from test_round5_hip import _streams
    _, op = _streams(10, 512, 77)
    assert (op[9] >= 35).any()
    errs = G.trade_errors(op.reshape(-1, 32), G.long_mask(O.o2arc_ops()), "adversarial streams")
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("ingress,row_name", [("bbox", "hot"), ("point", "hot"), ("bbox5", "hot"), ("bbox", "research_inc"), ("bbox5", "research_inc")])
def test_extraction_hands_the_slot_its_env_s_items(ingress, row_name):
    """readlane / quad_bcast_odd pick env my_env's record, counters, op index and tuple (bbox5 at its 20-byte, dword-aligned stride) out of
    the lanes — every item of the batch distinct.  (One counter layout: the per-lane one went with the classification by step counter.)"""
    errs = []
    for wpw in (4, 8):
        errs += G.extraction_errors(512, ingress, row_name, wpw, seed=3)
    errs += G.extraction_errors(768, ingress, row_name, 16, seed=4)  # (three groups per XCD: G is no power of two)
    assert not errs, "\n".join(errs[:10])


CELLS = [(row, form) for row, (_, _, forms) in G.LEAN_GROUPED.items() for form in forms]


@pytest.mark.parametrize("row_name,ingress", CELLS, ids=[f"{r}-{f}" for r, f in CELLS])
def test_whole_launches_under_every_slot_order(row_name, ingress):
    """n = 512 at 30 x 30 (two groups per XCD: the smallest launch), 6 steps, every cell of the LEAN table's grouped column.  The seed of the
    research case is one for which every group holds an env at limit - 2 or limit - 1 before every step (launch_errors checks it).  The
    plain launch is also compared with the oracle — the research row's with the episode model of tests/research_model.py."""
    errs = G.launch_errors(row_name, ingress, n=512, steps=6, seed=11, oracle=row_name in ("hot", "research_inc"))
    assert not errs, "\n".join(errs[:12])
