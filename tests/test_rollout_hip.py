"""Every rollout kernel of the full build (arcle_rollout_kernel<ING, FW, WC, FL>; ING 0 mask, 1 bbox, 2 point; FW 1 FW_FAST, 0 FW_GENERIC;
WC 30 + FL >= 0: the lean 30 x 30 twins of arcle_hip.hip's LEAN table) launched through arcle_rollout_mask / _bbox / _point and compared
with the oracle step by step (reward, terminated, every step's packed row where the launch writes one) and on the final state; the
trace-replay flags against the golden vectors; state that outlives a rollout; ARCVecEnv's rollouts; the launcher's refusals."""
import numpy as np
import pytest

import backends as B
import features as F
from oracle import oracle as O
from oracle import refdriver as RD

pytestmark = pytest.mark.gpu

O2, ARC, RAW = O.o2arc_ops(), O.arc_ops(), O.raw_ops()
EXOTIC = RD.variant_table("o2arc_exotic")[1]  # keep_sel, Rot180, Flip D0/D1, un-wrapped Color, wrapped Move, Crop (no ELIDE_SELECTED)
TABLES = {"o2arc": ("o2arc", O2), "arc": ("arc", ARC), "raw": ("raw", RAW), "exotic": ("o2arc", EXOTIC)}
OBJ_HEAVY = [1] * 10 + [2] * 10 + [4] * 8 + [2] * 3 + [1] * 4  # (35-op tables: Move / Rotate / Flip weighted up)
PACK = B.STEP_PACK_OBS

# (H, W, ingress, flags, table, T, N, packed): `flags` is the caller's; packed=True adds ARCLE_STEP_PACK_OBS (flags | 256 at launch)
MATRIX = [
    # arcle_rollout_kernel<1,1,30,3>: bbox, AUTORESET | ELIDE_SELECTED as a constant (ARCVecEnv.rollout_bbox, bench.py's rollout leg)
    (30, 30, "bbox", 3, "o2arc", 64, 65, False),
    (30, 30, "bbox", 3, "o2arc", 1, 7, False),
    # <2,1,30,3>
    (30, 30, "point", 3, "o2arc", 64, 65, False),
    (30, 30, "point", 3, "o2arc", 2, 257, False),
    # <1,1,30,259>: ... plus every step's packed row
    (30, 30, "bbox", 3, "o2arc", 64, 65, True),
    (30, 30, "bbox", 3, "arc", 2, 1, True),
    # <2,1,30,259>
    (30, 30, "point", 3, "o2arc", 64, 7, True),
    # <0,1,30,-1>: every mask rollout at 30 x 30, whatever its flags
    (30, 30, "mask", 0, "o2arc", 64, 65, False),
    (30, 30, "mask", 1, "exotic", 64, 7, False),
    (30, 30, "mask", 2, "o2arc", 2, 65, False),
    (30, 30, "mask", 3, "o2arc", 64, 65, True),
    (30, 30, "mask", 1, "arc", 64, 7, True),
    (30, 30, "mask", 0, "raw", 1, 1, False),
    # <1,1,30,-1>: bbox rollouts at 30 x 30 with another flag set
    (30, 30, "bbox", 0, "arc", 64, 65, False),
    (30, 30, "bbox", 1, "exotic", 64, 65, True),
    (30, 30, "bbox", 2, "o2arc", 256, 65, False),
    # <2,1,30,-1>
    (30, 30, "point", 1, "raw", 64, 7, True),
    (30, 30, "point", 0, "exotic", 2, 65, False),
    # <0|1|2,1,0,-1>: FW_FAST (16 <= W <= 32; FW_FULL shapes such as 32 x 32 share the code)
    (16, 24, "mask", 3, "o2arc", 64, 65, True),
    (32, 32, "mask", 1, "exotic", 64, 7, False),
    (15, 17, "mask", 0, "raw", 1, 65, False),
    (17, 21, "bbox", 2, "o2arc", 64, 65, False),
    (32, 32, "bbox", 3, "o2arc", 2, 257, True),
    (16, 16, "point", 0, "arc", 64, 65, False),
    (1, 17, "point", 3, "o2arc", 64, 7, False),  # (P % 4 != 0)
    # <0|1|2,0,0,-1>: FW_GENERIC (W < 16 or W > 32)
    (10, 10, "mask", 0, "o2arc", 64, 65, False),
    (5, 7, "mask", 3, "o2arc", 64, 7, True),  # (P % 4 != 0: byte-wise mask loads)
    (3, 3, "mask", 1, "exotic", 64, 65, False),
    (17, 15, "bbox", 1, "o2arc", 64, 65, True),
    (2, 100, "bbox", 0, "arc", 2, 65, False),
    (20, 1, "point", 2, "o2arc", 64, 7, False),
    (10, 10, "point", 1, "exotic", 64, 257, True),
]


def _case_id(c):
    H, W, ing, fl, tab, T, N, packed = c
    return f"{H}x{W}-{ing}-{tab}-fl{fl | (PACK if packed else 0)}-T{T}-N{N}"


@pytest.mark.parametrize("case", MATRIX, ids=[_case_id(c) for c in MATRIX])
def test_rollout_instantiation_vs_oracle(case):
    H, W, ing, flags, tab, T, N, packed = case
    kind, ops = TABLES[tab]
    errs = B.rollout_compare(B.HipBackend, kind, ops, H, W, N=N, T=T, seed=H * 31 + W + flags + T, ingress=ing, flags=flags,
                             int8_masks=bool(T & 64), op_weights=OBJ_HEAVY if len(ops) == 35 else None, bad_ops=True,
                             bad_tuples=ing != "mask", packed=packed)
    assert not errs, "\n".join(errs[:10])


class _OffsetHip(B.HipBackend):
    """Mask payloads placed OFF bytes past a 256-byte aligned base inside a larger device tensor."""
    OFF = 0

    def rollout(self, ingress, payload, op, flags=0, packed=False):
        t, dev = self.torch, self.b.device
        assert ingress == "mask" and not packed
        pay = np.ascontiguousarray(np.asarray(payload).astype(np.int8))
        big = t.zeros(pay.size + 64, dtype=t.int8, device=dev)
        view = big[self.OFF:self.OFF + pay.size].view(pay.shape)
        view.copy_(t.from_numpy(pay))
        assert view.is_contiguous() and view.data_ptr() % 256 == self.OFF
        r, tm = self.b.rollout(view, t.as_tensor(np.ascontiguousarray(op, np.int32), device=dev), flags, mask=True)
        return r.cpu().numpy(), tm.cpu().numpy()


@pytest.mark.parametrize("H,W", [(30, 30), (16, 24), (10, 10), (5, 7)])
@pytest.mark.parametrize("off", [1, 4])
def test_mask_rollout_payload_at_an_offset(H, W, off):
    """A mask payload whose base is 1 byte (byte loads) or 4 bytes (dword-aligned 16-byte loads where P % 4 == 0) past an aligned base."""
    cls = type(f"OffsetHip{off}", (_OffsetHip,), {"OFF": off})
    errs = B.rollout_compare(cls, "o2arc", O2, H, W, N=65, T=24, seed=off * 100 + H + W, ingress="mask", flags=1, int8_masks=True,
                             op_weights=OBJ_HEAVY, bad_ops=True)
    assert not errs, "\n".join(errs[:10])


def test_full_size_c3_stream_every_env():
    """8192 envs x 30 x 30 on bench.py's C3 stream with AUTORESET | ELIDE_SELECTED (<1,1,30,3>): every env vs the oracle."""
    import bench
    T, N = 16, 8192
    bb, op = bench.make_actions(T, N, 7)
    O.set_threads(16)
    try:
        errs = B.rollout_compare(B.HipBackend, "o2arc", O2, 30, 30, N=N, T=T, seed=5, ingress="bbox", flags=3, actions=(bb, op))
    finally:
        O.set_threads(1)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("H,W", [(32, 32), (31, 33), (30, 34)])
def test_packed_rows_of_a_1024_cell_grid(H, W):
    """Regression: where P + 7 > 1024 (P = 1018 ... 1024) the packed row's metadata (grid_dim, reward, terminated) runs past the 64
    lanes' 16-byte windows; it was never written (pack_row).  Rollout rows, the step kernel's fused rows and arcle_pack_obs vs the oracle."""
    errs = B.rollout_compare(B.HipBackend, "o2arc", O2, H, W, N=65, T=8, seed=H + W, ingress="mask", flags=1, packed=True)
    assert not errs, "\n".join(errs[:10])
    rng = np.random.default_rng(H * W)
    N = 65
    be, orc = B.HipBackend(N, H, W, 3, "o2arc", O2), B.OracleBackend(N, H, W, 3, "o2arc", O2)
    inp, idim = B.rollout_tasks(rng, N, H, W)
    for b in (be, orc):
        b.set_tasks(inp, idim, inp.copy(), idim.copy())
        b.reset()
    be.set_packed_output()
    for s in range(6):
        pay, op = B.rollout_actions(rng, O2, "bbox", N, H, W, 1, op_weights=OBJ_HEAVY)
        r1, t1 = be.step("bbox", pay[0], op[0], 1 | PACK)
        r2, t2 = orc.step("bbox", pay[0], op[0], 1)
        assert np.array_equal(r1, r2) and np.array_equal(t1, t2), s
        for name, rows in (("fused", be.fused_packed()), ("arcle_pack_obs", be.packed_obs())):
            g, d, pr, pt = B.unpack_rows(rows, H, W)
            assert np.array_equal(g, orc.get("grid")) and np.array_equal(d, orc.get("grid_dim")), f"{name} step {s}: grid"
            assert np.array_equal(pr, r2) and np.array_equal(pt, t2), f"{name} step {s}: reward / terminated"
            assert not rows[:, H * W + 7:].any(), f"{name} step {s}: padding"


# ---- trace-replay flags (mask ingress only) against the golden vectors ------------------------------------------------------------
def test_rollout_continue_rule_replays_the_golden_traces():
    """arcle_rollout_mask with CONTINUE_RULE | PACK_OBS over the synthetic O2ARC traces: every live step's grid and grid_dim, read from
    the packed rows, equal the reference harness's (tests/features.py::continue_rule replays the same traces by single steps)."""
    g = F.golden()
    n, T = g["replay_op"].shape
    be = B.HipBackend(n, 30, 30, -1, "o2arc", O2)
    be.set_tasks(g["replay_in"], g["replay_in_dim"], g["replay_ans"], g["replay_ans_dim"])
    be.reset()
    live = g["replay_op"] >= 0
    op = np.where(live, g["replay_op"], 32).astype(np.int32).T
    _, _, rows = be.rollout("mask", np.ascontiguousarray(g["replay_sel"].transpose(1, 0, 2, 3)), op, F.STEP_CONTINUE, packed=True)
    for t in range(T):
        grid, dim, _, _ = B.unpack_rows(rows[t], 30, 30)
        bad = [i for i in np.nonzero(live[:, t])[0]
               if not (np.array_equal(grid[i], g["replay_grid"][i, t]) and np.array_equal(dim[i], g["replay_grid_dim"][i, t]))]
        assert not bad, f"trace replay step {t}: grid differs for traces {bad}"


def test_rollout_reset_on_submit_golden():
    """RESET_ON_SUBMIT in a mask rollout, one handle per max_trial as in tests/features.py::reset_on_submit: per-step reward / terminated
    and grid (packed rows) of one rollout, then the full state after every step from prefix rollouts of a fresh reset."""
    g = F.golden()
    S, N, H, W = g["ros_mask"].shape
    for mt in sorted(set(g["ros_max_trial"].tolist())):
        sel = np.nonzero(g["ros_max_trial"] == mt)[0]
        n = len(sel)
        be = B.HipBackend(n, H, W, int(mt), "o2arc", O2)
        be.set_tasks(g["ros_in"][sel], g["ros_in_dim"][sel], g["ros_ans"][sel], g["ros_ans_dim"][sel])
        be.reset()
        masks, ops = np.ascontiguousarray(g["ros_mask"][:, sel]), np.ascontiguousarray(g["ros_op"][:, sel])
        r, tm, rows = be.rollout("mask", masks, ops, F.STEP_ROS, packed=True)
        for s in range(S):
            grid, dim, pr, pt = B.unpack_rows(rows[s], H, W)
            for name, got, want in (("reward", r[s], g["ros_reward"][s][sel]), ("term", tm[s], g["ros_term"][s][sel]),
                                    ("packed reward", pr, g["ros_reward"][s][sel]), ("packed term", pt, g["ros_term"][s][sel]),
                                    ("packed grid", grid, g["ros_grid"][s][sel]), ("packed grid_dim", dim, g["ros_grid_dim"][s][sel])):
                assert np.array_equal(np.asarray(got).reshape(n, -1), np.asarray(want).reshape(n, -1)), f"max_trial {mt} step {s}: {name}"
        for t in range(1, S + 1):
            be.reset()
            be.rollout("mask", masks[:t], ops[:t], F.STEP_ROS)
            cnt = be.counters()
            checks = [("steps", cnt[:, 0], g["ros_steps"][t - 1][sel]), ("submit_count", cnt[:, 1], g["ros_submit"][t - 1][sel])]
            checks += [(f, be.get(f), g["ros_" + f][t - 1][sel]) for f in ("grid", "grid_dim", "selected", "clip", "trials_remain", "terminated")]
            for name, got, want in checks:
                assert np.array_equal(np.asarray(got).reshape(n, -1), np.asarray(want).reshape(n, -1)), f"max_trial {mt} prefix {t}: {name}"


@pytest.mark.parametrize("H,W", [(30, 30), (16, 24), (10, 10)])
@pytest.mark.parametrize("flags", [F.STEP_CONTINUE, F.STEP_ROS, F.STEP_CONTINUE | F.STEP_ROS])
def test_rollout_trace_flags_equal_single_steps(H, W, flags):
    """CONTINUE_RULE / RESET_ON_SUBMIT (alone and together) in <0,1,30,-1>, <0,1,0,-1> and <0,0,0,-1> == the same handle kind's single steps
    (the path the golden vectors pin), on a stream that takes the continuation branch."""
    errs, hits = B.rollout_vs_steps(B.HipBackend, H, W, N=65, T=48, seed=flags + H * W, flags=flags, int8_masks=(H == 10),
                                    continue_stream=True, packed=True)
    assert not errs, "\n".join(errs[:10])
    assert hits >= 100, hits


# ---- state that outlives a rollout -------------------------------------------------------------------------------------------------
def _same_state(be, orc, tag):
    for f in B.PLANES + list(B.REC):
        assert np.array_equal(be.get(f), orc.get(f)), f"{tag}: field {f}"
    assert np.array_equal(be.counters(), orc.counters()), f"{tag}: counters"


def test_steps_rollouts_and_step_many_interleaved():
    """Single steps, a bbox rollout (lean <1,1,30,3>), a mask rollout, then step_many, all with AUTORESET | ELIDE_SELECTED on one handle:
    the rollouts write back only the planes they dirtied, and the zero-`selected` invariant the elision relies on holds across them."""
    import torch
    H = W = 30
    N, FL = 65, 3
    rng = np.random.default_rng(12)
    be, orc = B.HipBackend(N, H, W, 3, "o2arc", O2), B.OracleBackend(N, H, W, 3, "o2arc", O2)
    inp, idim = B.rollout_tasks(rng, N, H, W)
    for b in (be, orc):
        b.set_tasks(inp, idim, inp.copy(), idim.copy())
        b.reset()

    def steps(ing, k):
        for s in range(k):
            pay, op = B.rollout_actions(rng, O2, ing, N, H, W, 1, op_weights=OBJ_HEAVY)
            r1, t1 = be.step(ing, pay[0], op[0], FL)
            r2, t2 = orc.step(ing, pay[0], op[0], FL)
            assert np.array_equal(r1, r2) and np.array_equal(t1, t2), f"{ing} step {s}"

    def rollout(ing, T):
        pay, op = B.rollout_actions(rng, O2, ing, N, H, W, T, op_weights=OBJ_HEAVY)
        r1, t1 = be.rollout(ing, pay, op, FL)
        for s in range(T):
            r2, t2 = orc.step(ing, pay[s], op[s], FL)
            assert np.array_equal(r1[s], r2) and np.array_equal(t1[s], t2), f"{ing} rollout step {s}"

    steps("bbox", 6)
    _same_state(be, orc, "after the first steps")
    rollout("bbox", 16)
    _same_state(be, orc, "after the bbox rollout")
    steps("mask", 3)
    rollout("mask", 12)
    _same_state(be, orc, "after the mask rollout")
    bb, op = B.rollout_actions(rng, O2, "bbox", N, H, W, 8, op_weights=OBJ_HEAVY)
    dev = be.b.device
    r1, t1 = be.b.step_many("bbox", torch.as_tensor(bb, device=dev), torch.as_tensor(op, device=dev), FL)
    r1, t1 = r1.cpu().numpy(), t1.cpu().numpy()
    for s in range(8):
        r2, t2 = orc.step("bbox", bb[s], op[s], FL)
        assert np.array_equal(r1[s], r2) and np.array_equal(t1[s], t2), f"step_many step {s}"
    _same_state(be, orc, "after step_many")
    assert be.status() == orc.status()


def test_dense_pair_after_a_rollout():
    """DENSE step, rollout, DENSE step == the same actions as single steps on a twin handle (DESIGN.md note (10): a rollout drops the
    per-env pair cache, as a step without ARCLE_STEP_DENSE does)."""
    H = W = 30
    N, T = 65, 10
    rng = np.random.default_rng(4)
    a, b = B.HipBackend(N, H, W, -1, "o2arc", O2), B.HipBackend(N, H, W, -1, "o2arc", O2)
    inp, idim = B.rollout_tasks(rng, N, H, W)
    ans, adim = B.rollout_tasks(rng, N, H, W)
    for x in (a, b):
        x.set_tasks(inp, idim, ans, adim)
        x.reset()
        x.set_dense_output()
    m0, op0 = B.rollout_actions(rng, O2, "mask", N, H, W, 1)
    bb, op = B.rollout_actions(rng, O2, "bbox", N, H, W, T, op_weights=OBJ_HEAVY)
    m1, op1 = B.rollout_actions(rng, O2, "mask", N, H, W, 1)
    ra, _ = a.step("mask", m0[0], op0[0], F.STEP_DENSE)
    rb, _ = b.step("mask", m0[0], op0[0], F.STEP_DENSE)
    assert np.array_equal(ra, rb) and np.array_equal(a.dense, b.dense)
    a.rollout("bbox", bb, op)
    for s in range(T):
        b.step("bbox", bb[s], op[s])
    ra, ta = a.step("mask", m1[0], op1[0], F.STEP_DENSE)
    rb, tb = b.step("mask", m1[0], op1[0], F.STEP_DENSE)
    assert np.array_equal(ra, rb) and np.array_equal(ta, tb)
    assert np.array_equal(a.dense, b.dense), "dense pair after the rollout"
    for f in B.PLANES + list(B.REC):
        assert np.array_equal(a.get(f), b.get(f)), f


@pytest.mark.parametrize("flags", [0, 3, F.STEP_CONTINUE, F.STEP_CONTINUE | F.STEP_ROS])
def test_big_grid_mask_rollout_equals_single_steps(flags):
    """40 x 40 (the workgroup-per-env kernels): a rollout is n step launches; equal to the same steps taken singly, packed rows included."""
    errs, hits = B.rollout_vs_steps(B.HipBackend, 40, 40, N=16, T=24, seed=40 + flags, flags=flags, continue_stream=True, packed=True)
    assert not errs, "\n".join(errs[:10])
    assert hits >= 10, hits


# ---- the Python API ----------------------------------------------------------------------------------------------------------------
def _vec(n, **kw):
    import torch
    from arcle_amd.envs import ARCVecEnv, O2ARCv2Env
    from arcle_amd.loaders import SyntheticLoader
    return ARCVecEnv(O2ARCv2Env, n, SyntheticLoader(n_tasks=12, seed=3, max_size=(30, 30)), device=torch.device("cuda:0"), seed=9, **kw)


def _same_obs(a, b, tag):
    import torch
    assert a.keys() == b.keys(), tag
    for k in b:
        if isinstance(b[k], dict):
            _same_obs(a[k], b[k], f"{tag}: obs[{k}]")
        else:
            assert torch.equal(a[k], b[k]), f"{tag}: obs[{k}]"


def _same_vec(va, vb, oa, ob, ia, ib, tag):
    import torch
    _same_obs(oa, ob, tag)
    for k in ("input", "input_dim", "answer", "answer_dim", "steps", "submit_count"):
        assert torch.equal(ia[k], ib[k]), f"{tag}: info[{k}]"
    for k in va.batch.planes:
        assert torch.equal(va.batch.planes[k], vb.batch.planes[k]), f"{tag}: plane {k}"
    assert torch.equal(va.batch.rec, vb.batch.rec) and torch.equal(va.batch.cnt, vb.batch.cnt), tag


@pytest.mark.parametrize("autoreset", [True, False])
def test_vec_env_rollouts_equal_single_steps(autoreset):
    """ARCVecEnv.rollout_bbox (with packed= rows) and rollout_point == a twin env's step_bbox / step_point: reward, terminated, every obs
    key, the info fields, and every step's packed row against the twin's state after that step."""
    import torch
    from arcle_amd.engine import EnvBatch
    n, T, dev = 65, 24, torch.device("cuda:0")
    rng = np.random.default_rng(autoreset)
    va, vb = _vec(n, autoreset=autoreset), _vec(n, autoreset=autoreset)
    va.reset()
    vb.reset()
    bb, op = B.rollout_actions(rng, O2, "bbox", n, 30, 30, T, op_weights=OBJ_HEAVY)
    op[rng.random((T, n)) < 0.1] = 34
    bb_t, op_t = torch.as_tensor(bb, device=dev), torch.as_tensor(op, device=dev)
    rows = torch.full((T, n, va.batch.packed_obs_size()), 0x55, dtype=torch.uint8, device=dev)
    oa, ra, ta, ia = va.rollout_bbox(bb_t, op_t, packed=rows)
    for s in range(T):
        ob, rb, tb, _, ib = vb.step_bbox(bb_t[s], op_t[s])
        assert torch.equal(ra[s], rb) and torch.equal(ta[s], tb), f"rollout_bbox step {s}"
        grid, gdim, pr, pt = EnvBatch.unpack_obs(rows[s], 30, 30)
        assert torch.equal(grid, ob["grid"]) and torch.equal(gdim, ob["grid_dim"]), f"packed row step {s}"
        assert torch.equal(pr, rb) and torch.equal(pt, tb), f"packed reward / terminated step {s}"
    _same_vec(va, vb, oa, ob, ia, ib, "after rollout_bbox")
    xy, op = B.rollout_actions(rng, O2, "point", n, 30, 30, T, op_weights=OBJ_HEAVY)
    op[rng.random((T, n)) < 0.1] = 34
    xy_t, op_t = torch.as_tensor(xy, device=dev), torch.as_tensor(op, device=dev)
    oa, ra, ta, ia = va.rollout_point(xy_t, op_t)
    for s in range(T):
        ob, rb, tb, _, ib = vb.step_point(xy_t[s], op_t[s])
        assert torch.equal(ra[s], rb) and torch.equal(ta[s], tb), f"rollout_point step {s}"
    _same_vec(va, vb, oa, ob, ia, ib, "after rollout_point")
    assert va.batch.status() == vb.batch.status() == 0


def test_vec_env_rollout_refusals_leave_the_env_untouched():
    """Resample, truncation, dense reward and host-callable op tables refuse rollouts (NotImplementedError) without touching the env."""
    import torch
    from arcle_amd.envs import ARCVecEnv, O2ARCv2Env
    from arcle_amd.loaders import SyntheticLoader

    class Custom(O2ARCv2Env):
        def create_operations(self):
            ops = super().create_operations()
            ops[5] = lambda state, action: None
            return ops
    n, T, dev = 8, 4, torch.device("cuda:0")
    envs = [_vec(n, autoreset="resample"), _vec(n, max_episode_steps=5), _vec(n, dense_reward=True),
            ARCVecEnv(Custom, n, SyntheticLoader(n_tasks=4, seed=3, max_size=(30, 30)), device=dev, seed=9)]
    bb = torch.zeros((T, n, 4), dtype=torch.int32, device=dev)
    op = torch.full((T, n), 20, dtype=torch.int32, device=dev)
    for v in envs:
        v.reset()
        v.step_bbox(bb[0], op[0])
        before = {k: t.clone() for k, t in v.batch.planes.items()}
        rec, cnt = v.batch.rec.clone(), v.batch.cnt.clone()
        with pytest.raises(NotImplementedError):
            v.rollout_bbox(bb, op)
        with pytest.raises(NotImplementedError):
            v.rollout_point(bb[:, :, :2].contiguous(), op)
        for k, t in before.items():
            assert torch.equal(v.batch.planes[k], t), k
        assert torch.equal(v.batch.rec, rec) and torch.equal(v.batch.cnt, cnt)
        assert v.batch.status() == 0


# ---- the launcher's refusals -------------------------------------------------------------------------------------------------------
def test_rollout_refusals_return_the_documented_code_and_change_nothing():
    import torch
    from arcle_amd.engine import _ptr
    ERR_ARG, ERR_CONFIG = -1, -2
    N, T, H, W = 7, 3, 10, 10
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2)
    bufs = {"bbox": torch.zeros((T, N, 4), dtype=torch.int32, device=dev), "point": torch.zeros((T, N, 2), dtype=torch.int32, device=dev),
            "mask": torch.ones((T, N, H, W), dtype=torch.int8, device=dev)}
    op = torch.full((T, N), 20, dtype=torch.int32, device=dev)
    reward = torch.zeros((T, N), dtype=torch.int32, device=dev)
    term = torch.zeros((T, N), dtype=torch.uint8, device=dev)
    for kind, ops in (("o2arc", O2), ("arc", ARC), ("raw", RAW)):
        be = B.HipBackend(N, H, W, 3, kind, ops)
        inp, idim = B.rollout_tasks(rng, N, H, W)
        be.set_tasks(inp, idim, inp, idim)
        be.reset()
        be.step("bbox", np.tile([[0, 0, 3, 3]], (N, 1)), np.full(N, len(ops) + 2))  # (an out-of-range op: status ARCLE_ST_BAD_OP)
        b = be.b
        L, h, st = b.L, b._h, b._stream()
        fns = {"bbox": L.arcle_rollout_bbox, "point": L.arcle_rollout_point, "mask": L.arcle_rollout_mask}
        before = {f: be.get(f) for f in O.KIND_PLANES[kind]}
        rec, cnt = be.get("grid_dim"), be.counters()
        rec_all = b.rec.clone()
        cases = [(ing, T, fl, ERR_ARG) for ing in fns for fl in (F.STEP_TRUNCATE, F.STEP_DENSE, F.STEP_FLAT_OBS, F.STEP_RESAMPLE, 1 << 10)]
        cases += [(ing, T, fl, ERR_CONFIG) for ing in ("bbox", "point") for fl in (F.STEP_CONTINUE, F.STEP_ROS, F.STEP_CONTINUE | F.STEP_ROS)]
        cases += [(ing, T, F.STEP_PACK_OBS, ERR_CONFIG) for ing in fns]  # (no packed output installed)
        cases += [(ing, n, 0, ERR_ARG) for ing in fns for n in (0, -1)]
        if kind != "o2arc":  # no `selected` plane: the continuation rule has nothing to compare with (as arcle_step_* refuses it)
            cases += [("mask", T, fl, ERR_CONFIG) for fl in (F.STEP_CONTINUE, F.STEP_CONTINUE | F.STEP_ROS)]
        for ing, n, fl, want in cases:
            reward.fill_(77)
            rc = fns[ing](h, n, _ptr(bufs[ing]), _ptr(op), _ptr(reward), _ptr(term), fl, st)
            assert rc == want, f"{kind} {ing} n_steps {n} flags {fl}: {rc} (want {want})"
            assert L.arcle_last_error(h), f"{kind} {ing} flags {fl}: no error message"
        torch.cuda.synchronize()
        assert bool((reward == 77).all()), "a refused rollout wrote its outputs"
        for f, v in before.items():
            assert np.array_equal(be.get(f), v), f"{kind}: plane {f} changed"
        assert np.array_equal(be.get("grid_dim"), rec) and np.array_equal(be.counters(), cnt) and torch.equal(b.rec, rec_all)
        assert be.status() == O.ST_BAD_OP, kind
