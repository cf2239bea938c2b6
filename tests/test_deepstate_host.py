"""The guard against vacuity of tests/test_deepstate_emu.py and tests/test_deepstate_hip.py, on the CPU with the oracle alone: every
stream those tests send reaches every situation it is meant to reach (tests/deepstate.py: census, applicable) at least FLOOR times,
chains of eight continued object ops at least FLOOR_CHAIN8 times.  The second test records what the random streams of
tests/test_hip_parity.py::test_hip_vs_oracle_o2arc reach — the reason this file exists."""
from collections import Counter

import pytest

import backends as B
import deepstate as D
from oracle import oracle as O


@pytest.mark.parametrize("case", D.FLOOR_CASES, ids=lambda c: f"{c.stream}-{c.H}x{c.W}-{c.table}-f{c.flags}-n{c.N}-s{c.S}")
def test_stream_reaches_every_situation(case):
    st = D.stream_of(case)
    print(D.table_line(case, st.counts))
    assert st.payload.shape[:2] == (case.S, case.N) and st.op.shape == (case.S, case.N)
    missed = D.check_floors(case)
    assert not missed, "\n".join(missed)


def test_every_case_of_the_emulator_and_gpu_tests_is_held_to_the_floors():
    """The lists the other two files parametrise over are parts of FLOOR_CASES — the rows and the emulators' streams included."""
    used = D.STEP_CASES + D.EXOTIC_CASES + D.BIG_CASES + D.ROLLOUT_CASES + D.ROWS_CASES + D.TUPLE_CASES + [D.GROUPED_CASE] + D.EMU_CASES
    assert set(used) <= set(D.FLOOR_CASES) and len(set(D.FLOOR_CASES)) == len(D.FLOOR_CASES)


def test_rows_cases_continue_objects():
    """rows_check's own condition on top of the floors: at least a third of the rows of steps 8, 24 and 40 continue an active object."""
    for case in D.ROWS_CASES:
        st = D.stream_of(case)
        for s in D.ROW_STEPS:
            cont = sum(any(nm.startswith("cont:") for nm in st.names[s][n]) for n in range(case.N))
            print(f"rows {case.H}x{case.W} step {s}: {cont} of {case.N} rows continue")
            assert 3 * cont >= case.N, (case, s, cont)


class _Census:
    """backends.random_trace_compare's observer: the census of the stream it draws."""

    def __init__(self, ops, H, W):
        self.ops, self.H, self.W, self.total, self.steps, self.track = ops, H, W, Counter(), 0, {}

    def before(self, orc):
        self.pre = D.snapshot(orc)

    def after(self, orc, ing, pay, op, flags, reward):
        post = D.snapshot(orc)
        post["reward"] = reward
        self.total += D.census(self.pre, {"form": ing, "payload": pay, "op": op, "flags": flags, "ops": self.ops, "H": self.H, "W": self.W}, post, self.track)
        self.steps += len(op)


@pytest.mark.parametrize("H,W", [(30, 30), (7, 12)])
def test_census_of_the_random_streams(H, W):
    """Prints (no floor) what the streams of tests/test_hip_parity.py::test_hip_vs_oracle_o2arc reach: that test's call of
    backends.random_trace_compare (its seeds, OBJ_HEAVY weights, bad_ops, N = S = 96, four flag sets) with the oracle in the place of
    the backend under test and the census as the observer — the generator itself draws the stream, nothing is copied here."""
    from test_hip_parity import OBJ_HEAVY
    ops = O.o2arc_ops()
    obs = _Census(ops, H, W)
    for flags in (0, O.STEP_AUTORESET, B.STEP_ELIDE_SELECTED, O.STEP_AUTORESET | B.STEP_ELIDE_SELECTED):
        obs.track = {}
        errs = B.random_trace_compare(B.OracleBackend, "o2arc", ops, H, W, N=96, S=96, seed=H * 100 + W + flags, max_trial=3 if flags else -1,
                                      flags=flags, op_weights=OBJ_HEAVY, bad_ops=True, observer=obs)
        assert not errs
    print(f"random streams {H}x{W}, {obs.steps} env-steps: " + ", ".join(f"{k} {obs.total[k]}" for k in sorted(obs.total)))
    assert obs.steps == 4 * 96 * 96
