"""Elided plane stores (arcle_wave.h Wave::store_if) on the lock-step wavefront emulator: every env starts from garbage planes
(tests/adversarial.py) and the C3 op mix, the exotic op table and int8-mask streams are compared with the oracle field by field,
with and without ARCLE_STEP_ELIDE_SELECTED.  CPU only."""
import pytest

import adversarial as A
import backends as B
from oracle import oracle as O

FLAGS = (0, B.STEP_ELIDE_SELECTED, O.STEP_AUTORESET | B.STEP_ELIDE_SELECTED)


def exotic_table():
    from oracle import refdriver as RD
    return RD.variant_table("o2arc_exotic")[1]


@pytest.mark.parametrize("H,W", [(30, 30), (16, 16), (20, 17), (12, 12)])
@pytest.mark.parametrize("flags", FLAGS)
def test_adversarial_c3_mix(H, W, flags):
    errs = A.adversarial_compare(B.EmuBackend, O.o2arc_ops(), H, W, N=8, S=40, seed=H * 31 + W + flags, flags=flags)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("H,W", [(30, 30), (17, 20), (9, 32)])
def test_adversarial_object_heavy_restated(H, W):
    """Object operations only (the ops whose stores are narrowed the most), the garbage state re-installed every 5 steps."""
    w = [0] * 20 + [1] * 8 + [0] * 7
    for flags in FLAGS:
        errs = A.adversarial_compare(B.EmuBackend, O.o2arc_ops(), H, W, N=8, S=30, seed=7 * H + W + flags, flags=flags, op_weights=w,
                                     restate_every=5)
        assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("H,W", [(30, 30), (16, 16), (20, 17)])
def test_adversarial_exotic_ops(H, W):
    # (the exotic table holds keep_sel: ARCLE_STEP_ELIDE_SELECTED is not valid for it — arcle_can_elide_selected)
    errs = A.adversarial_compare(B.EmuBackend, exotic_table(), H, W, N=8, S=40, seed=5 * H + W, op_weights=[1] * 20 + [4] * 8 + [2] * 7)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("H,W", [(30, 30), (12, 12)])
@pytest.mark.parametrize("flags", FLAGS)
def test_adversarial_int8_masks(H, W, flags):
    errs = A.adversarial_compare(B.EmuBackend, O.o2arc_ops(), H, W, N=8, S=30, seed=3 * H + W + flags, flags=flags, int8_masks=True)
    assert not errs, "\n".join(errs[:10])
