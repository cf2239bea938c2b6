"""The research env's step on the MI355X against the independent episode model of tests/research_model.py, after every step: what the
CPU emulators do not stand in for — the compile-time-flag instantiations (the LEAN rows RESEARCH_FL / RESEARCH_INC_FL, their self-ordering
twin, the lean rollout kernels, the generic FEAT 1 kernels of every width class), the compiled big-grid kernels, sharded handles and the
ARCVecEnv layer (single steps, step_many, capture + replay, the float32 dense reward).  Every stream is held to its floors by
tests/test_research_model_host.py."""
import numpy as np
import pytest

import backends as B
import deepstate as D
import research_model as M
import research_rollouts as RR

pytestmark = pytest.mark.gpu

PACK = M.PACK_OBS
PLAIN = M.RESAMPLE | M.TRUNCATE
_id = lambda c: f"{c.stream}-{c.H}x{c.W}-n{c.N}"  # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from arcle_amd import _lib
    _lib.build()  # no-op when csrc/libarcle_hip.so is up to date
    _lib.lib()    # the product library must be present and loadable: no silent fallback


def _check(case, form, flags, rows, cls=B.HipBackend):
    be = M.setup(cls, case, flags, rows)
    errs = M.compare(be, M.model_of(case, flags=flags), M.stream_of(case), flags, rows, form)
    assert not errs, "\n".join(errs[:10])


LEAN = [(c, f) for c in M.GPU_LEAN for f in M.FORMS[c.stream]]


@pytest.mark.parametrize("flags", [M.RESEARCH, M.RESEARCH_INC], ids=["RESEARCH_FL", "RESEARCH_INC_FL"])
@pytest.mark.parametrize("case,form", LEAN, ids=[f"{c.stream}-{f}" for c, f in LEAN])
def test_lean_rows(case, form, flags):
    """30 x 30, FilterO2ARC rows: the two LEAN rows with FEAT 1, all five ingress forms, 64 envs x 48 steps"""
    _check(case, form, flags, "filtered")


@pytest.mark.parametrize("case,form,flags", [(M.GPU_LEAN[0], "bbox", M.RESEARCH), (M.GPU_LEAN[1], "mask", M.RESEARCH_INC), (M.GPU_LEAN[2], "point", M.RESEARCH | PACK),
                                             (M.GPU_LEAN[0], "bbox5", PLAIN)], ids=["bbox", "mask-inc", "point-pack", "bbox5-plain"])
def test_generic_feature_kernel_at_30x30(case, form, flags):
    """full rows (and the flag sets beside the LEAN rows): the generic <ING, FW_FULL, 1, 1> step kernel"""
    _check(case, form, flags, "full" if flags & M.FLAT_OBS else None)


@pytest.mark.parametrize("flags", [M.RESEARCH, M.RESEARCH_INC], ids=["full-write", "incremental"])
@pytest.mark.parametrize("case", M.GPU_WIDTHS, ids=_id)
def test_other_width_classes(case, flags):
    """32 x 32 (FW_FULL), 20 x 24 (FW_FAST, non-square: dropped quarter turns, refused Rotates), 12 x 12 and 7 x 12 (FW_GENERIC)"""
    _check(case, case.stream, flags, "filtered")


@pytest.mark.parametrize("form", ["bbox", "bbox5"])
def test_self_ordering_launch_of_the_incremental_research_row(form):
    """512 envs x 12 steps through the launch that orders itself (the first step, the full row write, is a plain launch)"""
    case = M.GPU_GROUPED
    with D.env_vars(ARCLE_GROUPED=1, ARCLE_GROUP_MIN=0, ARCLE_GROUP_MAX=10000000):
        be = M.setup(B.HipBackend, case, M.RESEARCH_INC, "filtered")
        assert be.b.launch_info(form, M.RESEARCH_INC)["orders_itself"]
        errs = M.compare(be, M.model_of(case), M.stream_of(case), M.RESEARCH_INC, "filtered", form)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("case,rows,extra", [(M.GPU_ROLLOUT[0], "filtered", 0), (M.GPU_ROLLOUT[2], "filtered", 0), (M.GPU_ROLLOUT[1], "full", PACK),
                                             (M.GPU_ROLLOUT[3], "filtered", 0)], ids=["lean-bbox", "lean-point", "mask-full-packed", "bbox-10x10"])
def test_rollout_ex(case, rows, extra):
    """arcle_rollout_ex: the stream's 48 steps in ONE launch, every step's reward / terminated / truncated / dense pair / row against the
    model step by step, then the final state"""
    flags = M.RESEARCH | extra
    be = M.setup(RR.HipResearchBackend, case, M.RESEARCH & ~M.FLAT_OBS)
    errs = M.compare_rollout(be, M.model_of(case), M.stream_of(case), flags, rows)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("case", M.GPU_BIG, ids=_id)
def test_big_grid_kernels(case):
    """40 x 40, 36 x 41, 64 x 64, 100 x 12 (W < 16), 127 x 127: the research set through the generic workgroup-per-env kernel (bbox: full
    rows, masks: FilterO2ARC rows), then RESAMPLE | TRUNCATE through the LEAN one"""
    rows = "full" if case.stream == "bbox" else "filtered"
    _check(case, case.stream, M.RESEARCH, rows)
    _check(case, "bbox5" if case.stream == "bbox" else "mask", PLAIN, None)


def test_big_grid_kernels_other_rows():
    _check(M.GPU_BIG[0], "bbox", M.RESEARCH | PACK, "filtered")
    _check(M.GPU_BIG[1], "mask", M.RESEARCH, "full")


@pytest.mark.parametrize("case", M.GPU_SHARDS, ids=_id)
def test_two_shards_against_one_model(case):
    """two handles of N / 2 envs with env_base 0 and N / 2 against ONE model of N envs: the draw is keyed by the global env id"""
    h = case.N // 2
    parts = [(M.setup(B.HipBackend, case, M.RESEARCH, "filtered", N=h, env_base=base), slice(base, base + h)) for base in (0, h)]
    errs = M.compare(parts, M.model_of(case), M.stream_of(case), M.RESEARCH, "filtered")
    assert not errs, "\n".join(errs[:10])


# ---- ARCVecEnv in the research configuration, on the task table it builds from its own loader -----------------------------------------
def _vec_env(case):
    from arcle_amd import actions
    from arcle_amd.envs import ARCVecEnv, O2ARCv2Env

    class Crop(O2ARCv2Env):  # agents/env.py:23-28
        def create_operations(self):
            ops = super().create_operations()
            ops[33] = actions.reset_sel(actions.crop_grid)
            return ops
    v = ARCVecEnv(Crop, case.N, M.vec_env_table()[0], seed=M.VEC_SEED, autoreset="resample", augment=("permute", "rot90"), dense_reward=True,
                  max_episode_steps=M.STEP_LIMIT, max_trial=M.MAX_TRIAL)
    v.reset()
    v.enable_flat_rows(filtered=True)
    return v


def _dense_reward(want):
    """the float32 ARCVecEnv._dense forms: sparse * 100 - 1 + correct / total, 0 where the pair is (0, 0)"""
    r, c, t = want["reward"].astype(np.float32), want["dense"][:, 0].astype(np.float32), want["dense"][:, 1].astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(want["dense"][:, 1] > 0, r * np.float32(100) - np.float32(1) + c / t, np.float32(0)).astype(np.float32)


def test_vec_env_research_configuration():
    """16 single steps, a step_many of 16 and a capture + replay of 16: reward (float32, exact), terminated, truncated, info["steps"]
    and the incremental FilterO2ARC rows against the model"""
    import torch
    case = M.GPU_VEC
    st, model, v = M.stream_of(case), M.model_of(case), _vec_env(case)
    dev = v.device
    errs = []

    def state(tag, want, op):
        torch.cuda.synchronize()
        M._diff(errs, tag, "info steps", v._info()["steps"].cpu().numpy(), model.counters()[:, 0], want["what"], op)
        M._diff(errs, tag, "rows", v.rows.cpu().numpy(), model.rows(True), want["what"], op)
        M._diff(errs, tag, "grid", v._obs["grid"].cpu().numpy(), model.get("grid"), want["what"], op)
        M._diff(errs, tag, "table_index", v._info()["table_index"].cpu().numpy(), model.cur_task, want["what"], op)

    def outputs(tag, want, op, r, tm, tr):
        assert r.dtype == torch.float32
        M._diff(errs, tag, "reward", r.cpu().numpy(), _dense_reward(want), want["what"], op)
        M._diff(errs, tag, "terminated", tm.cpu().numpy().astype(np.uint8), want["terminated"], want["what"], op)
        M._diff(errs, tag, "truncated", tr.cpu().numpy().astype(np.uint8), want["truncated"], want["what"], op)

    M._diff(errs, "after reset", "rows", v.rows.cpu().numpy(), model.rows(True), ["reset"] * case.N, st.op[0])
    bbox, op = torch.as_tensor(st.payload, device=dev).contiguous(), torch.as_tensor(st.op, device=dev).contiguous()
    for s in range(16):
        _, r, tm, tr, _ = v.step_bbox(bbox[s], op[s])
        want = model.step("bbox", st.payload[s], st.op[s])
        outputs(f"step_bbox {s}", want, st.op[s], r, tm, tr)
        state(f"step_bbox {s}", want, st.op[s])
    assert not errs, "\n".join(errs[:10])
    _, r, tm, tr, _ = v.step_many(bbox[16:32].contiguous(), op[16:32].contiguous(), form="bbox")
    for s in range(16, 32):
        want = model.step("bbox", st.payload[s], st.op[s])
        outputs(f"step_many {s}", want, st.op[s], r[s - 16], tm[s - 16], tr[s - 16])
    state("after step_many", want, st.op[31])
    assert not errs, "\n".join(errs[:10])
    cs = v.capture(bbox[32:48].contiguous(), op[32:48].contiguous(), form="bbox")
    _, r, tm, tr = cs.replay()
    torch.cuda.synchronize()
    for s in range(32, 48):
        want = model.step("bbox", st.payload[s], st.op[s])
        outputs(f"replay {s}", want, st.op[s], r[s - 32], tm[s - 32], tr[s - 32])
    state("after replay", want, st.op[47])
    assert not errs, "\n".join(errs[:10])
    assert v.batch.status() == B.O.ST_BAD_OP, "the stream's op indices beyond the table raise ARCLE_ST_BAD_OP, and nothing else is raised"
