"""Caller-chosen plane strides (tests/strides.py) through the CPU emulators: the kernel bodies of arcle_wave.h, arcle_big.h,
arcle_search.h, arcle_components.h, arcle_objects.h and arcle_place.h at strides that are no multiple of 128 — a last live lane
that is partly or wholly padding, PS == H * W, a small grid in a 1024-byte row, odd chunk counts and bit rows that are only 2-byte
aligned on the workgroup-per-env path.  Every comparison is a driver's of the suite, bit for bit against the oracle; after every
run the plane padding must be zero and the slack behind the planes untouched.  The GPU side is tests/test_strides_hip.py.

What the emulators cannot run, and why (tests/test_strides_hip.py runs all of it):
  arcle_create's argument checks, arcle_mask_bits_stride, arcle_launch_info, arcle_get_plane / arcle_set_plane, the allocation sizes
      and the scratch envs of a big handle's transition_rows: host code of arcle_hip.hip; the emulators take StepParams / BigParams
      filled in by tests/backends.py
  rollouts on handles of more than 1024 cells: the library runs them as n_steps step launches from the host (arcle_big.hip); the
      big emulator has no such entry point
  bit rows in transition_rows / expand_rows on handles of more than 1024 cells: the library refuses them (include/arcle_hip.h)
  the search family on handles of more than 1024 cells: the library refuses it there
  the padding invariant in tests/components.py, objects.py and place.py: their emulator classes fill whole plane rows, padding
      included, with 0x55 before they run (bytes the kernels must not read); the slack invariant holds and is checked
  search_bits.expansion at 1 x 1 / 16: the driver asserts on the ORACLE's side that at least 15 % of its masks are not their own
      filled bounding box, which no one-cell mask can be; bit rows reach expand_rows at 1 x 1 through search_bits.transitions and
      deepstate.expansion_check
tests/components.py holds fixture grids for 30 x 30, 5 x 5 and 1 x 1 only: at the other shapes arcle_components_rows runs on grids
it generates, against the same components_numpy."""
import pytest

import backends as B
import components as CP
import macros as MC
import objects as OB
import place as PL
import search_bits as SB
import strides as ST

SMALL = pytest.mark.parametrize("H,W,ps", [c[:3] for c in ST.SMALL], ids=[ST.case_id(c) for c in ST.SMALL])
ALL = pytest.mark.parametrize("H,W,ps", [c[:3] for c in ST.CASES], ids=[ST.case_id(c) for c in ST.CASES])
BIG = pytest.mark.parametrize("H,W,ps", [c[:3] for c in ST.BIG], ids=[ST.case_id(c) for c in ST.BIG])


def _emu(H, W):
    """The wave emulator, or the big emulator with the product's default instantiation (two chunks per thread)."""
    return B.BigEmuTwoBackend if ST.is_big(H, W) else B.EmuBackend


@pytest.mark.parametrize("form", ST.STEP_FORMS)
@pytest.mark.parametrize("flags", ST.FLAG_SETS)
@ALL
def test_step(H, W, ps, flags, form):
    """every ingress form under both flag sets at every case"""
    errs = ST.step(_emu(H, W), H, W, ps, flags, form)
    assert not errs, "\n".join(errs[:10])


OTHER_BIG = [c[:3] + v for c in ST.BIG for v in (("BigEmuBackend", "bits", 3), ("BigEmuGenericBackend", "mask", 0), ("BigEmuOneBackend", "bits", 3),
                                                ("BigEmuFourBackend", "mask", 0))
             if not (v[0] == "BigEmuOneBackend" and c[:2] == (127, 127))]  # (one host thread per chunk: a thousand threads behind a barrier)


@pytest.mark.parametrize("H,W,ps,backend,form,flags", OTHER_BIG, ids=[f"{ST.case_id(c)}-{c[3]}" for c in OTHER_BIG])
def test_step_other_big_instantiations(H, W, ps, backend, form, flags):
    """the run-time chunk loop on 16 threads, the generic body, one and four chunks per thread"""
    errs = ST.step(getattr(B, backend), H, W, ps, flags, form)
    assert not errs, "\n".join(errs[:10])


@ALL
def test_resets(H, W, ps):
    errs = ST.resets(_emu(H, W), H, W, ps)
    assert not errs, "\n".join(errs[:10])


@ALL
def test_state_rows_and_bit_packer(H, W, ps):
    errs = ST.state_rows(B.BigEmuBackend if ST.is_big(H, W) else B.EmuBackend, H, W, ps)
    assert not errs, "\n".join(errs[:10])


@ALL
def test_transition_rows(H, W, ps):
    errs = ST.transitions(B.BigEmuBackend if ST.is_big(H, W) else SB.EmuBitsBackend, H, W, ps)
    assert not errs, "\n".join(errs[:10])


@SMALL
def test_rollouts(H, W, ps):
    errs = ST.rollout(B.EmuBackend, H, W, ps)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("stream,form", ST.RESEARCH_FORMS)
@ALL
def test_research_flags(H, W, ps, stream, form):
    errs = ST.research(B.BigEmuBackend if ST.is_big(H, W) else B.EmuBackend, H, W, ps, stream, form)
    assert not errs, "\n".join(errs[:10])


@ALL
def test_byte_accounting(H, W, ps):
    errs = ST.accounting(B.BigEmuBackend if ST.is_big(H, W) else B.EmuBackend, H, W, ps)
    assert not errs, "\n".join(errs[:10])


@SMALL
def test_expand_and_hash(H, W, ps):
    errs = ST.expand_and_hash(SB.EmuBitsBackend, H, W, ps)
    assert not errs, "\n".join(errs[:10])


@SMALL
def test_expand_macros(H, W, ps):
    errs = ST.macros(MC.EmuMacroBackend, H, W, ps)
    assert not errs, "\n".join(errs[:10])


@SMALL
def test_components_objects_place(H, W, ps):
    errs = ST.objects_family(CP.EmuComponents, OB.EmuObjects, PL.EmuPlace, H, W, ps)
    assert not errs, "\n".join(errs[:10])
