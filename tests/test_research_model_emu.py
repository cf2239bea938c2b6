"""The CPU emulators of the step kernels against the independent episode model of tests/research_model.py, after every step of streams
that end 7-12 episodes per env by reward, by trials and by the time limit: the one-wavefront body (every width class, every ingress form,
filtered / full / incremental rows, four flag sets), its rollout (T steps in one launch), the big-grid bodies in all their
instantiations, and the self-ordering launch of the research row in its three slot orders.  Every stream is held to its floors by
tests/test_research_model_host.py."""
import numpy as np
import pytest

import backends as B
import grouping as GR
import research_model as M
import research_rollouts as RR

PACK, INC = M.PACK_OBS, M.ROWS_INC
PLAIN = M.RESAMPLE | M.TRUNCATE
BY_KEY = {(c.stream, c.H, c.W): c for c in M.EMU}

# (stream, H, W, form, flags, rows): every shape meets every stream, every form, every row kind and the incremental writer; 30 x 30 (the
# LEAN rows' flag sets) meets all five forms
STEP_RUNS = [
    ("bbox", 30, 30, "bbox", M.RESEARCH_INC, "filtered"), ("bbox", 30, 30, "bbox5", M.RESEARCH, "full"),
    ("mask", 30, 30, "mask", M.RESEARCH, "filtered"), ("mask", 30, 30, "bits", M.RESEARCH | PACK, "filtered"),
    ("point", 30, 30, "point", M.RESEARCH_INC, "filtered"), ("bbox", 30, 30, "bbox", PLAIN, None),
    ("bbox", 32, 32, "bbox5", M.RESEARCH_INC, "full"), ("mask", 32, 32, "mask", M.RESEARCH | PACK, "filtered"), ("point", 32, 32, "point", M.RESEARCH, "filtered"),
    ("bbox", 20, 24, "bbox5", M.RESEARCH, "filtered"), ("mask", 20, 24, "bits", M.RESEARCH_INC, "filtered"), ("point", 20, 24, "point", PLAIN, None),
    ("bbox", 12, 12, "bbox", M.RESEARCH | PACK, "full"), ("mask", 12, 12, "mask", M.RESEARCH_INC, "full"), ("point", 12, 12, "point", M.RESEARCH, "filtered"),
    ("bbox", 7, 12, "bbox", M.RESEARCH_INC, "filtered"), ("mask", 7, 12, "bits", M.RESEARCH, "full"), ("mask", 7, 12, "mask", PLAIN, None),
    ("point", 7, 12, "point", M.RESEARCH | PACK, "filtered"),
]


def _run_id(r):
    return f"{r[0]}-{r[1]}x{r[2]}-{r[3]}-f{r[4]}-{r[5]}"


@pytest.mark.parametrize("run", STEP_RUNS, ids=_run_id)
def test_step_against_the_model(run):
    stream, H, W, form, flags, rows = run
    case = BY_KEY[(stream, H, W)]
    be = M.setup(B.EmuBackend, case, flags, rows)
    errs = M.compare(be, M.model_of(case, flags=flags), M.stream_of(case), flags, rows, form)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("case", M.EMU_AUTORESET, ids=lambda c: f"{c.stream}-{c.H}x{c.W}")
def test_autoreset_truncate_dense_against_the_model(case):
    """AUTORESET | TRUNCATE | DENSE: the env keeps its task through every reset, the time limit still ends episodes"""
    flags = M.MODE_FLAGS["autoreset"]
    be = M.setup(B.EmuBackend, case, flags)
    errs = M.compare(be, M.model_of(case), M.stream_of(case), flags)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("case,rows", list(zip(M.EMU_ROLLOUT, ("filtered", "filtered", "full", "filtered", "full"))), ids=lambda v: v if isinstance(v, str) else f"{v.stream}-{v.H}x{v.W}")
def test_rollout_against_the_model(case, rows):
    """EmuResearchBackend.rollout_ex: the stream's 40 steps in one launch, every step's outputs against the model step by step"""
    flags = M.RESEARCH | (PACK if rows == "full" else 0)
    be = M.setup(RR.EmuResearchBackend, case, flags & ~(M.FLAT_OBS | PACK), None)
    errs = M.compare_rollout(be, M.model_of(case), M.stream_of(case), flags, rows)
    assert not errs, "\n".join(errs[:10])


BIG = {"40x40": B.BigEmuBackend, "36x41": B.BigEmuTwoBackend, "64x64": B.BigEmuGenericBackend, "100x12": B.BigEmuFourBackend}


@pytest.mark.parametrize("case", M.EMU_BIG, ids=lambda c: f"{c.stream}-{c.H}x{c.W}")
def test_big_grid_bodies_against_the_model(case):
    """arcle_big.h: the research set through the generic body (full rows for bbox, filtered rows for masks), then RESAMPLE | TRUNCATE
    through the LEAN body of the shape's class (run-time loop, two chunks per thread, generic, four chunks per thread; 100 x 12 has
    W < 16 and stays generic) — and the one-chunk instantiation at 40 x 40"""
    st = M.stream_of(case)
    rows = "full" if case.stream == "bbox" else "filtered"
    form = {"bbox": "bbox5", "mask": "mask"}[case.stream] if case.H == 36 else case.stream
    runs = [(B.BigEmuBackend, M.RESEARCH, rows), (BIG[f"{case.H}x{case.W}"], PLAIN, None)]
    if (case.H, case.stream) == (40, "bbox"):
        runs.append((B.BigEmuOneBackend, PLAIN, None))
    for cls, flags, rw in runs:
        be = M.setup(cls, case, flags, rw)
        errs = M.compare(be, M.model_of(case, flags=flags), st, flags, rw, form)
        assert not errs, cls.__name__ + "\n" + "\n".join(errs[:10])
        if flags == PLAIN and cls.LEAN and case.W >= 16:
            assert be.lean_steps == case.S, "the LEAN body did not run"


class _Grouped(GR.GroupEmuBackend):
    row_name = "research_inc"

    def step(self, ingress, payload, op, flags=0):
        if not flags & INC:  # the one full row write before the incremental ones: the wave emulator's plain step
            return B.EmuBackend.step(self, ingress, payload, op, flags)
        return GR.GroupEmuBackend.step(self, ingress, payload, op, flags)


@pytest.mark.parametrize("form,order,steps", [("bbox", "shuffled", 12), ("bbox", "ascending", 6), ("bbox5", "descending", 6)])
def test_self_ordering_research_row_against_the_model(form, order, steps):
    """GroupEmuBackend, row research_inc: the launch that orders itself with its slots run in each of the three orders, every launch
    against the model on the state-aware stream (test_group_emu.py runs all three orders of both forms on its random stream, the plain
    twin of which it compares with the model too)"""
    case = M.EMU_GROUPED
    be = M.setup(_Grouped, case, M.RESEARCH_INC, "filtered")
    be.order = GR.orders(case.N, 5)[order]
    errs = M.compare(be, M.model_of(case), M.stream_of(case), M.RESEARCH_INC, "filtered", form, steps=steps)
    assert not errs, "\n".join(errs[:10])
    assert not np.array_equal(be.env_of_slot, np.arange(case.N)), "no slot traded"
