"""Caller-chosen plane strides (tests/strides.py) on the MI355X: arcle_config.plane_stride / EnvBatch(plane_stride=) through every
kernel family and the host layer, at strides no other test uses — what the CPU emulators of tests/test_strides_emu.py cannot stand
in for: the lane predication and non-temporal stores as compiled, the wave-op mask ingest and launch geometry of the
workgroup-per-env kernels with odd chunk counts and 2-byte aligned bit rows, the allocation sizes, hipMemcpy2D pitches and scratch
carve-up of arcle_hip.hip.  Every comparison is a driver's of the suite, bit for bit against the oracle; after every run the plane
padding must be zero and the PLANE_SLACK bytes behind every plane, filled with 0x55 beforehand, untouched.

Not run: search_bits.expansion at 1 x 1 / 16 — the driver asserts on the ORACLE's side that at least 15 % of its masks are not their
own filled bounding box, which no one-cell mask can be; bit rows reach expand_rows at 1 x 1 through search_bits.transitions and
deepstate.expansion_check.  tests/components.py holds fixture grids for 30 x 30, 5 x 5 and 1 x 1 only: at the other shapes
arcle_components_rows runs on grids it generates, against the same components_numpy."""
import ctypes

import numpy as np
import pytest

import backends as B
import components as CP
import deepstate as D
import features as F
import macros as MC
import objects as OB
import place as PL
import search_bits as SB
import strides as ST
from oracle import oracle as O

pytestmark = pytest.mark.gpu

SMALL = pytest.mark.parametrize("H,W,ps", [c[:3] for c in ST.SMALL], ids=[ST.case_id(c) for c in ST.SMALL])
ALL = pytest.mark.parametrize("H,W,ps", [c[:3] for c in ST.CASES], ids=[ST.case_id(c) for c in ST.CASES])


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from arcle_amd import _lib
    _lib.build()  # no-op when csrc/libarcle_hip.so is up to date
    _lib.lib()    # the product library must be present and loadable: no silent fallback


@pytest.fixture(autouse=True)
def _oracle_threads(request):
    """the oracle of the big planes on 16 threads (tests/test_big_hip.py)"""
    O.set_threads(16)
    yield
    O.set_threads(1)


# ---- every kernel family ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ST.STEP_FORMS)
@pytest.mark.parametrize("flags", ST.FLAG_SETS)
@ALL
def test_step(H, W, ps, flags, form):
    errs = ST.step(B.HipBackend, H, W, ps, flags, form)
    assert not errs, "\n".join(errs[:10])


@ALL
def test_resets(H, W, ps):
    errs = ST.resets(B.HipBackend, H, W, ps)
    assert not errs, "\n".join(errs[:10])


@ALL
def test_state_rows_and_bit_packer(H, W, ps):
    errs = ST.state_rows(B.HipBackend, H, W, ps)
    assert not errs, "\n".join(errs[:10])


@ALL
def test_plane_copies(H, W, ps):
    errs = ST.run(ST.plane_copies, B.HipBackend, ps, H, W)
    assert not errs, "\n".join(errs[:10])


@ALL
def test_transition_rows(H, W, ps):
    errs = ST.transitions(SB.HipBitsBackend, H, W, ps)
    assert not errs, "\n".join(errs[:10])


@ALL
def test_rollouts(H, W, ps):
    errs = ST.rollout(B.HipBackend, H, W, ps)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("stream,form", ST.RESEARCH_FORMS)
@ALL
def test_research_flags(H, W, ps, stream, form):
    errs = ST.research(B.HipBackend, H, W, ps, stream, form)
    assert not errs, "\n".join(errs[:10])


@ALL
def test_byte_accounting(H, W, ps):
    errs = ST.accounting(B.HipBackend, H, W, ps)
    assert not errs, "\n".join(errs[:10])


@SMALL
def test_expand_and_hash(H, W, ps):
    errs = ST.expand_and_hash(SB.HipBitsBackend, H, W, ps)
    assert not errs, "\n".join(errs[:10])


@SMALL
def test_expand_macros(H, W, ps):
    errs = ST.macros(MC.HipMacroBackend, H, W, ps)
    assert not errs, "\n".join(errs[:10])


@SMALL
def test_components_objects_place(H, W, ps):
    errs = ST.objects_family(CP.HipComponents, OB.HipObjects, PL.HipPlace, H, W, ps)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("H,W,ps", [(30, 30, 912), (12, 20, 240), (40, 40, 1616), (100, 20, 2000)])
def test_library_owned_planes(H, W, ps):
    """arcle_create with NULL planes: the library's own allocations (n_envs * PS + ARCLE_PLANE_SLACK per plane) through the raw C ABI —
    bbox steps against the oracle, then every plane, its padding and the slack behind it"""
    F.raw_c_abi(33, H, W, ps)


# ---- argument checks ------------------------------------------------------------------------------------------------------------------
MAX_PS = (127 * 127 + 127) & ~127  # arcle_big::MAX_PS
ERR_CONFIG = -2                    # ARCLE_ERR_CONFIG


@pytest.mark.parametrize("H,W,ps", [(30, 30, 904), (30, 30, 920), (30, 30, 896), (12, 20, 224), (12, 20, 1040), (1, 1, 8), (40, 40, 1592), (40, 40, 1608),
                                    (40, 40, 1024), (127, 127, MAX_PS + 16), (40, 40, MAX_PS + 128)])
def test_create_refuses_the_stride(H, W, ps):
    """not a multiple of 16, below H * W, above 1024 on a one-wavefront handle, above MAX_PS on a workgroup-per-env one: ARCLE_ERR_CONFIG
    from arcle_create (library-owned planes) with no handle left behind, ArcleHipError from EnvBatch"""
    from arcle_amd import _lib
    from arcle_amd.engine import ArcleHipError, EnvBatch
    h = ctypes.c_void_p()
    cfg = _lib.Config(4, H, W, 3, -1, ps)
    assert _lib.lib().arcle_create(ctypes.byref(cfg), None, ctypes.byref(h)) == ERR_CONFIG
    assert not h.value
    with pytest.raises(ArcleHipError):
        EnvBatch(4, H, W, 3, "o2arc", plane_stride=ps)


@pytest.mark.parametrize("H,W,ps", [(30, 30, 1024), (40, 40, MAX_PS), (127, 127, MAX_PS), (1, 1, 1024)])
def test_create_accepts_the_largest_stride(H, W, ps):
    from arcle_amd.engine import EnvBatch
    assert EnvBatch(4, H, W, 3, "o2arc", plane_stride=ps).PS == ps


@ALL
def test_mask_bits_stride(H, W, ps):
    """128 on one-wavefront handles at any stride, PS / 8 on the others"""
    from arcle_amd.engine import EnvBatch
    assert EnvBatch(4, H, W, 3, "o2arc", plane_stride=ps).bits_stride == (ps // 8 if ST.is_big(H, W) else 128)


def test_environment_variable_sets_the_stride():
    from arcle_amd.engine import EnvBatch
    with D.env_vars(ARCLE_PLANE_STRIDE=912):
        assert EnvBatch(4, 30, 30, 3, "o2arc").PS == 912
    assert EnvBatch(4, 30, 30, 3, "o2arc").PS == 1024


def test_self_ordering_and_lean_plans_need_the_1024_byte_row():
    """the 30 x 30 launch plans written for PS == 1024 — the launch that orders itself, the lean streaming instantiations — are taken
    at the default stride and not at 912"""
    case = D.GROUPED_CASE
    ops = D.table_of(case.table)
    for ps, want in ((None, True), (912, False)):
        cls = ST.with_stride(B.HipBackend, ps) if ps else B.HipBackend
        with D.env_vars(ARCLE_GROUPED=1, ARCLE_GROUP_MIN=0, ARCLE_GROUP_MAX=10000000):
            assert cls(case.N, 30, 30, 2, "o2arc", ops).b.launch_info("bbox", case.flags)["orders_itself"] == want
        with D.env_vars(ARCLE_GROUPED=0, ARCLE_STREAM_POLICY="B"):
            info = cls(case.N, 30, 30, 2, "o2arc", ops).b.launch_info("bbox", case.flags)
            assert not info["orders_itself"] and info["policy"] == ("B" if want else "")


def test_grid_aware_tuples_at_912_with_the_self_ordering_launch_asked_for():
    """the 2304-env batch of tests/test_deepstate_hip.py with ARCLE_GROUPED = 1 at PS = 912: the plain launch, every env against the oracle"""
    with D.env_vars(ARCLE_GROUPED=1, ARCLE_GROUP_MIN=0, ARCLE_GROUP_MAX=10000000):
        errs = ST.run(D.compare, B.HipBackend, 912, D.GROUPED_CASE, "bbox")
    assert not errs, "\n".join(errs[:10])
