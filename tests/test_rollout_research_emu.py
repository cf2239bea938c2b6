"""The FEAT 1 rollout body (wave_rollout of arcle_wave.h: TimeLimit, device-side resampling, dense pairs, flat rows and packed rows with
every step's outputs) on the wave emulator, against T emulated steps with the same flags (tests/research_rollouts.py)."""
import pytest

import research_rollouts as RR

SIZES = [(30, 30), (10, 10), (12, 20), (5, 5)]


@pytest.mark.parametrize("H,W", SIZES)
@pytest.mark.parametrize("ingress", ["bbox", "point", "mask"])
@pytest.mark.parametrize("name,flags,rows", RR.CASES, ids=[c[0] for c in RR.CASES])
def test_rollout_matches_steps(H, W, ingress, name, flags, rows):
    limit = 3 + (H + W + len(name)) % 3  # step limits of 3-5: envs end two or more episodes inside the rollout
    errs = RR.case_compare(RR.EmuResearchBackend, RR.EmuResearchBackend, H, W, N=6, T=14, seed=H * 31 + W + len(name), flags=flags,
                           rows=rows, ingress=ingress, step_limit=limit)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("H,W", [(30, 30), (12, 20)])
def test_mask_rollout_continue_rule_reset_on_submit_dense(H, W):
    errs = RR.mask_rules_compare(RR.EmuResearchBackend, RR.EmuResearchBackend, H, W, N=8, T=16, seed=H + W)
    assert not errs, "\n".join(errs[:10])


def test_golden_dense_vectors_as_one_mask_rollout():
    errs = RR.golden_dense_rollout(RR.EmuResearchBackend)
    assert not errs, "\n".join(errs[:10])
