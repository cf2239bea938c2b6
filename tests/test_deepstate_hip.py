"""The state-aware streams of tests/deepstate.py on the MI355X: what the CPU emulators cannot stand in for — the wave-op reductions, the
LDS staging, the compile-time LEAN instantiations, the rollout and expansion kernels as compiled — asked to continue active objects
eight and more ops deep, off the grid and back, through the int8 wraps of pos + dim and of the Rotate sums, through ROTATE_DOMAIN
refusals of continued ops, and fed tuples drawn relative to each env's grid_dim.  Every stream's census is held to its floors by
tests/test_deepstate_host.py; every comparison is bit for bit against the oracle."""
import pytest

import backends as B
import deepstate as D
import search as SR
import search_bits as SB

pytestmark = pytest.mark.gpu

_id = lambda c: f"{c.stream}-{c.H}x{c.W}-{c.table}-f{c.flags}"  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from arcle_amd import _lib
    _lib.build()  # no-op when csrc/libarcle_hip.so is up to date
    _lib.lib()    # the product library must be present and loadable: no silent fallback


@pytest.mark.parametrize("form", ["mask", "bits"])
@pytest.mark.parametrize("case", D.STEP_CASES, ids=_id)
def test_step_launches_on_chain_streams(case, form):
    """one shape per width class: FW_FULL 30 x 30 and 32 x 32, FW_FAST 12 x 20, FW_GENERIC 7 x 12 and 2 x 100"""
    errs = D.compare(B.HipBackend, case, form)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("form", ["mask", "bits"])
@pytest.mark.parametrize("case", D.EXOTIC_CASES, ids=_id)
def test_step_launches_on_exotic_chain_streams(case, form):
    """the exotic table: ops without RESET_SEL while an object is active, Rotate 180, Flip D0 / D1 with the stale object_dim"""
    errs = D.compare(B.HipBackend, case, form)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("form", ["mask", "bits"])
@pytest.mark.parametrize("case", D.BIG_CASES, ids=_id)
def test_big_grid_kernels_on_chain_streams(case, form):
    """40 x 40: LEAN, one wavefront; 64 x 64; 127 x 127: one Move from the far edge wraps pos + dim; 33 x 100; 100 x 12: W < 16, the
    generic kernel"""
    errs = D.compare(B.HipBackend, case, form)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("case", D.ROLLOUT_CASES, ids=_id)
def test_rollout_of_a_chain_stream(case):
    """the 48 recorded steps as one launch, the state resident in registers between the continued ops"""
    errs = D.rollout_check(B.HipBackend, case)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("case", D.ROWS_CASES, ids=_id)
def test_transition_rows_continue_the_object(case):
    big = case.H * case.W > 1024  # (big handles refuse bit rows)
    errs = D.rows_check(SB.HipBitsBackend, case, forms=("mask",) if big else ("mask", "bits"))
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("kind,H,W,mt", [c for c in SR.CASES if c[0] == "o2arc"] + [("o2arc", 32, 32, 3)] + list(SR.FAST_CASES))
def test_expand_rows_continue_the_parents_object(kind, H, W, mt):
    errs = D.expansion_check(SB.HipBitsBackend, kind, H, W, mt)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("case", D.TUPLE_CASES, ids=_id)
def test_grid_aware_tuples(case):
    for form in (("bbox", "bbox5") if case.stream == "bbox" else ("point",)):
        errs = D.compare(B.HipBackend, case, form)
        assert not errs, "\n".join(errs[:10])


def test_grid_aware_tuples_through_the_self_ordering_launch():
    """2304 envs x 16 steps of grid-aware bbox tuples through the launch that orders itself (tests/test_round5_hip.py), every env of the
    batch against the oracle"""
    case = D.GROUPED_CASE
    with D.env_vars(ARCLE_GROUPED=1, ARCLE_GROUP_MIN=0, ARCLE_GROUP_MAX=10000000):
        probe = B.HipBackend(case.N, case.H, case.W, D.max_trial_of(case), "o2arc", D.table_of(case.table))
        assert probe.b.launch_info("bbox", case.flags)["orders_itself"]
        del probe
        errs = D.compare(B.HipBackend, case, "bbox")
    assert not errs, "\n".join(errs[:10])
