"""The episode model of tests/research_model.py on the CPU with the oracle alone: the guard against vacuity of
tests/test_research_model_emu.py and tests/test_research_model_hip.py (every stream they send reaches every situation it is meant to
reach at least FLOOR times; the printed counts are the ones DESIGN.md §4 records), and the model's own parts against what is already
pinned: its dense pair and its augmentation on the golden vectors of research.npz, its plain-AUTORESET form on the oracle."""
import numpy as np
import pytest

import backends as B
import features as F
import research_model as M
from oracle import oracle as O

_id = lambda c: f"{c.stream}-{c.H}x{c.W}-{c.mode}-n{c.N}-s{c.S}"  # noqa: E731


@pytest.mark.parametrize("case", M.FLOOR_CASES, ids=_id)
def test_stream_reaches_every_situation(case):
    st = M.stream_of(case)
    print(M.table_line(case))
    assert st.payload.shape[:2] == (case.S, case.N) and st.op.shape == (case.S, case.N)
    missed = M.check_floors(case)
    assert not missed, "\n".join(missed)


def test_every_case_of_the_emulator_and_gpu_tests_is_held_to_the_floors():
    """The lists the other two files parametrise over (they draw their cases from research_model's lists only) are parts of FLOOR_CASES."""
    used = (M.GPU_LEAN + M.GPU_WIDTHS + [M.GPU_GROUPED] + M.GPU_ROLLOUT + M.GPU_BIG + M.GPU_SHARDS + [M.GPU_VEC] + M.EMU + M.EMU_AUTORESET + M.EMU_ROLLOUT
            + M.EMU_BIG + [M.EMU_GROUPED])
    assert set(used) <= set(M.FLOOR_CASES) and len(set(M.FLOOR_CASES)) == len(M.FLOOR_CASES)


def test_model_dense_pair_on_the_golden_dense_trace():
    """features.dense with the model in the product's place: sparse * 100 - 1 + correct / total of every step, float64-exact"""
    g = F.golden()
    S, N, H, W = g["dense_mask"].shape
    m = M.ResearchModel(N, H, W, -1, M.crop_table(), None, None, None, None, 0, 0, 0, 0, M.DENSE,
                        tasks=(g["aug_out_in"], g["aug_out_in_dim"], g["aug_out_ans"], g["aug_out_ans_dim"]))
    for s in range(S):
        out = m.step("mask", g["dense_mask"][s], g["dense_op"][s])
        d = out["dense"].astype(np.float64)
        assert out["what"] == ["executed"] * N, f"step {s}: the golden trace skips nothing"
        assert np.array_equal(out["reward"].astype(np.float64) * 100 - 1 + d[:, 0] / d[:, 1], g["dense_reward"][s]), f"step {s}"
        assert np.array_equal(out["terminated"], g["dense_term"][s])
    assert np.array_equal(m.get("grid"), g["dense_final_grid"]) and np.array_equal(m.get("grid_dim"), g["dense_final_grid_dim"])


def test_model_augmentation_on_the_golden_planes():
    g = F.golden()
    N, H, W = g["aug_in"].shape
    for n in range(N):
        a = g["aug_in"][n][:g["aug_in_dim"][n, 0], :g["aug_in_dim"][n, 1]]
        b = g["aug_ans"][n][:g["aug_ans_dim"][n, 0], :g["aug_ans_dim"][n, 1]]
        inp, idim, ans, adim, k = M.augmented(a, b, int(g["aug_k"][n]), g["aug_perm"][n], H, W)
        assert k == int(g["aug_k"][n])
        assert np.array_equal(inp, g["aug_out_in"][n]) and np.array_equal(ans, g["aug_out_ans"][n]), n
        assert tuple(idim) == tuple(g["aug_out_in_dim"][n]) and tuple(adim) == tuple(g["aug_out_ans_dim"][n]), n


@pytest.mark.parametrize("stream,H,W", [("bbox", 30, 30), ("mask", 7, 12), ("point", 12, 12)])
def test_model_with_plain_autoreset_is_the_oracle(stream, H, W):
    """no time limit reached (step_limit beyond the stream's length): the model's rule 2 is the oracle's ARCLE_STEP_AUTORESET"""
    case = M.Case(stream, H, W, "autoreset", 32, 40)
    st = M.stream_of(case)
    m = M.model_of(case, flags=M.AUTORESET | M.DENSE)
    m.step_limit = 1 << 30
    orc = B.OracleBackend(case.N, H, W, M.MAX_TRIAL, "o2arc", M.crop_table())
    orc.set_tasks(m.get("input"), m.get("input_dim"), m.get("answer"), m.get("answer_dim"))
    orc.reset()
    resets = 0
    for s in range(case.S):
        out = m.step(stream, st.payload[s], st.op[s])
        r, t = orc.step(stream, st.payload[s], st.op[s], O.STEP_AUTORESET)
        assert np.array_equal(out["reward"], r) and np.array_equal(out["terminated"], t) and out["status"] == orc.status(), s
        assert not out["truncated"].any()
        for f in M.FIELDS:
            assert np.array_equal(m.get(f), orc.get(f)), (s, f)
        assert np.array_equal(m.counters(), orc.counters())
        resets += sum(w.startswith("ended") for w in out["what"])
    assert resets >= M.FLOOR and (m.episode == 1).all()
