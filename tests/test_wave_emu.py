"""The kernel body (arcle_amd/csrc/arcle_wave.h — the same header hipcc compiles for gfx950) executed by the
lock-step wavefront emulator of tests/emu, checked against the golden vectors and against the oracle.
This validates the kernel LOGIC on the CPU (plus: cross-lane ops only in wave-uniform control flow, values
declared uniform really are, stale LDS never matters).  The GPU parity tests proper are in test_hip_parity.py."""
import pytest

import backends as B
from oracle import oracle as O

OBJ_HEAVY = [1] * 10 + [2] * 10 + [4] * 8 + [2] * 3 + [1] * 4


@pytest.mark.parametrize("name", B.fixture_names())
def test_emulated_kernel_matches_golden(name):
    errs = B.replay_fixture(B.EmuBackend, name, max_steps=96)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("name", ["o2arc_30", "o2arc_10", "quirks_30", "o2arc_crop_10"])
def test_emulated_kernel_matches_golden_with_selected_elision(name):
    """ARCLE_STEP_ELIDE_SELECTED (skip the redundant zero-fill of `selected` for inactive envs) changes no state."""
    errs = B.replay_fixture(B.EmuBackend, name, max_steps=96, flags=B.STEP_ELIDE_SELECTED)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("H,W", [(30, 30), (10, 10), (5, 5), (3, 3), (7, 12), (12, 7), (32, 32), (1, 17), (20, 1), (16, 16)])
def test_emulated_kernel_vs_oracle_o2arc(H, W):
    for flags in (0, O.STEP_AUTORESET, B.STEP_ELIDE_SELECTED, O.STEP_AUTORESET | B.STEP_ELIDE_SELECTED):
        errs = B.random_trace_compare(B.EmuBackend, "o2arc", O.o2arc_ops(), H, W, N=6, S=40, seed=H * 100 + W + flags,
                                      max_trial=3 if flags else -1, flags=flags, op_weights=OBJ_HEAVY, bad_ops=True)
        assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("kind,ops", [("arc", O.arc_ops()), ("raw", O.raw_ops())])
def test_emulated_kernel_vs_oracle_other_kinds(kind, ops):
    errs = B.random_trace_compare(B.EmuBackend, kind, ops, 30, 30, N=6, S=40, seed=7, max_trial=3)
    assert not errs, "\n".join(errs[:10])


def exotic_table():
    """Rot180, Flip D0/D1, keep_sel, un-wrapped Color, wrapped Move, paste_blank=False, Crop — generators no shipped
    env installs (oracle/refdriver.py::variant_table, validated against the reference by diff_vs_reference.py)."""
    from oracle import refdriver as RD
    return RD.variant_table("o2arc_exotic")[1]


@pytest.mark.parametrize("H,W", [(30, 30), (16, 16), (20, 17), (17, 20), (12, 12), (9, 32)])
def test_emulated_kernel_vs_oracle_exotic_ops(H, W):
    w = [1] * 20 + [4] * 8 + [2] * 7
    errs = B.random_trace_compare(B.EmuBackend, "o2arc", exotic_table(), H, W, N=6, S=48, seed=3 * H + W, op_weights=w)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("H,W", [(30, 30), (10, 10), (5, 7)])
def test_emulated_reset_from_task_table(H, W):
    errs = B.task_table_compare(B.EmuBackend, H, W, N=12, T=9, seed=H)
    assert not errs, "\n".join(errs)


@pytest.mark.parametrize("H,W,ingress", [(30, 30, "bbox"), (10, 10, "bbox"), (30, 30, "point"), (5, 7, "bbox")])
def test_emulated_rollout_equals_sequential_steps(H, W, ingress):
    for flags in (0, O.STEP_AUTORESET, B.STEP_ELIDE_SELECTED):
        errs = B.rollout_compare(B.EmuBackend, "o2arc", O.o2arc_ops(), H, W, N=6, T=40, seed=H + W + flags,
                                 ingress=ingress, flags=flags)
        assert not errs, "\n".join(errs[:10])


def test_emulated_rollout_other_kinds():
    for kind, ops in (("arc", O.arc_ops()), ("raw", O.raw_ops())):
        errs = B.rollout_compare(B.EmuBackend, kind, ops, 30, 30, N=4, T=30, seed=9)
        assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("H,W", [(30, 30), (16, 24), (5, 7), (32, 32), (31, 33)])
def test_emulated_mask_rollout_vs_oracle(H, W):
    """wave_rollout with mask ingress (arcle_rollout_mask) at a 30 x 30, a FW_FAST and a FW_GENERIC shape: flags 0-3, 0/1 or arbitrary
    int8 masks, out-of-range ops; per-step reward / terminated, every step's packed row (odd flags) and the final state vs the oracle.
    32 x 32 and 31 x 33 (P + 7 > 1024): the packed row's metadata lies past the 64 lanes' windows."""
    for flags in (0, O.STEP_AUTORESET, B.STEP_ELIDE_SELECTED, O.STEP_AUTORESET | B.STEP_ELIDE_SELECTED):
        errs = B.rollout_compare(B.EmuBackend, "o2arc", O.o2arc_ops(), H, W, N=6, T=40, seed=H * 7 + W + flags, ingress="mask", flags=flags,
                                 int8_masks=bool(flags & 1), op_weights=OBJ_HEAVY, bad_ops=True, packed=bool(flags & 1))
        assert not errs, f"flags {flags}:\n" + "\n".join(errs[:10])


@pytest.mark.parametrize("ingress", ["bbox", "point"])
def test_emulated_lean_rollout_twins(ingress):
    """At 30 x 30 with AUTORESET | ELIDE_SELECTED (+ PACK_OBS) the emulator runs the rollout twin whose flag set is a compile-time
    constant, as launch_rollout_tbl does; out-of-range tuples and ops compare ARCLE_ST_BAD_SELECTION / _BAD_OP too."""
    for flags in (3, 3 | B.STEP_PACK_OBS):
        errs = B.rollout_compare(B.EmuBackend, "o2arc", O.o2arc_ops(), 30, 30, N=6, T=40, seed=flags, ingress=ingress, flags=flags & 3,
                                 op_weights=OBJ_HEAVY, bad_ops=True, bad_tuples=True, packed=bool(flags & B.STEP_PACK_OBS))
        assert not errs, f"flags {flags}:\n" + "\n".join(errs[:10])


@pytest.mark.parametrize("H,W", [(10, 10), (16, 24)])
@pytest.mark.parametrize("flags", [B.STEP_CONTINUE_RULE, B.STEP_RESET_ON_SUBMIT, B.STEP_CONTINUE_RULE | B.STEP_RESET_ON_SUBMIT])
def test_emulated_mask_rollout_trace_flags(H, W, flags):
    """The rollout takes CONTINUE_RULE / RESET_ON_SUBMIT (mask ingress only): equal to the same steps taken singly, on a stream whose
    logged selections equal the current `selected` plane before a Move / Rotate / Flip (the continuation branch)."""
    errs, hits = B.rollout_vs_steps(B.EmuBackend, H, W, N=6, T=40, seed=flags + H, flags=flags, int8_masks=(H == 10),
                                    continue_stream=True, packed=True)
    assert not errs, "\n".join(errs[:10])
    assert hits >= 10, hits


@pytest.mark.parametrize("H,W", [(30, 30), (32, 32), (17, 21), (12, 12), (6, 40)])
def test_emulated_floodfill_worst_case(H, W):
    errs = B.floodfill_worst_case_compare(B.EmuBackend, H, W)
    assert not errs, "\n".join(errs)
