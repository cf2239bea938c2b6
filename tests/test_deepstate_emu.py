"""The state-aware streams of tests/deepstate.py through the CPU emulators (the kernel bodies of arcle_wave.h, arcle_big.h and
arcle_search.h run lock-step / on host threads) against the oracle: deep chains of continued Move / Rotate / Flip, objects off the
grid and back, the int8 wraps on big planes, grid-aware tuples, and the row / expansion kernels asked to continue the parent's active
object.  Every stream stepped here is one of deepstate.FLOOR_CASES, whole: tests/test_deepstate_host.py holds its census to the
floors.  The GPU side is tests/test_deepstate_hip.py."""
import pytest

import backends as B
import deepstate as D
import search as SR
import search_bits as SB

_id = lambda c: f"{c.stream}-{c.H}x{c.W}-{c.table}-f{c.flags}"  # noqa: E731


@pytest.mark.parametrize("case", D.EMU_STEP_CASES, ids=_id)
def test_wave_emulator_on_chain_streams(case):
    """int8 masks under autoreset | elide, bit rows under flags 0"""
    errs = D.compare(B.EmuBackend, case, "mask" if case.flags else "bits")
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("case", D.EMU_EXOTIC_CASES, ids=_id)
def test_wave_emulator_on_exotic_chain_streams(case):
    """ops without RESET_SEL sent while an object is active (the next continued op restores the background over their write), Rotate
    180, Flip D0 / D1 with the stale object_dim"""
    errs = D.compare(B.EmuBackend, case, "mask")
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("backend,form", [("BigEmuBackend", "mask"), ("BigEmuGenericBackend", "mask"), ("BigEmuTwoBackend", "mask"), ("BigEmuTwoBackend", "bits")])
@pytest.mark.parametrize("case", D.EMU_BIG_CASES, ids=_id)
def test_big_emulators_on_chain_streams(case, backend, form):
    errs = D.compare(getattr(B, backend), case, form)
    assert not errs, "\n".join(errs[:10])


def test_big_emulator_on_the_127x127_chain_stream():
    """one Move from the far edge wraps pos + dim, a continued Rotate there takes the wrapped sums (object.py:102-107 in int8)"""
    errs = D.compare(B.BigEmuBackend, D.EMU_127, "mask")
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("case", D.EMU_TUPLE_CASES, ids=_id)
def test_wave_emulator_on_grid_aware_tuples(case):
    errs = D.compare(B.EmuBackend, case, "bbox5" if case.stream == "bbox" else "point")
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("case", D.ROWS_CASES, ids=_id)
def test_transition_rows_continue_the_object(case):
    big = case.H * case.W > 1024
    errs = D.rows_check(B.BigEmuBackend if big else SB.EmuBitsBackend, case, forms=("mask",) if big else ("mask", "bits"))
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("kind,H,W,mt", [c for c in SR.CASES if c[0] == "o2arc"] + [("o2arc", 32, 32, 3)] + list(SR.FAST_CASES))
def test_expand_rows_continue_the_parents_object(kind, H, W, mt):
    errs = D.expansion_check(SB.EmuBitsBackend, kind, H, W, mt)
    assert not errs, "\n".join(errs[:10])
