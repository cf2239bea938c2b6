"""arcle_rollout_ex on the MI355X: every arcle_rollout_feat_kernel instantiation (the lean 30 x 30 research twins for bbox / point, the
generic FW_FAST / FW_GENERIC bodies for bbox / point / mask) and the step loop of a 40 x 40 handle against T step launches of a twin
handle (tests/research_rollouts.py); ARCVecEnv.rollout in the research configuration against a twin stepping with step_bbox; the bbox5
form; sharded batches; the library's refusals and the Python checks, which must leave the env untouched."""
import ctypes

import numpy as np
import pytest
import torch

import research_rollouts as RR
from arcle_amd import _lib
from arcle_amd.engine import ArcleHipError

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CONFIG = -1, -2

# (H, W, ingress, flags, rows, N, T): the instantiation each row reaches is in its id
KERNELS = [
    ("feat<1,1,30,RESEARCH_FL>", 30, 30, "bbox", RR.RESEARCH, "filtered", 257, 24),
    ("feat<2,1,30,RESEARCH_FL>", 30, 30, "point", RR.RESEARCH, "filtered", 257, 24),
    ("feat<1,1,0,-1> full rows", 30, 30, "bbox", RR.RESEARCH, "full", 129, 20),
    ("feat<1,1,0,-1> 20x24", 20, 24, "bbox", RR.RESAMPLE | RR.TRUNCATE | RR.DENSE, None, 129, 20),
    ("feat<2,1,0,-1>", 20, 24, "point", RR.RESAMPLE | RR.TRUNCATE | RR.PACK_OBS, None, 129, 20),
    ("feat<1,0,0,-1>", 10, 10, "bbox", RR.RESEARCH, "filtered", 129, 20),
    ("feat<2,0,0,-1>", 12, 12, "point", RR.DENSE | RR.TRUNCATE | RR.AUTORESET, None, 129, 20),
    ("feat<0,1,0,-1>", 30, 30, "mask", RR.RESEARCH, "filtered", 65, 16),
    ("feat<0,0,0,-1>", 5, 5, "mask", RR.PACK_OBS | RR.RESAMPLE | RR.DENSE, None, 65, 16),
]


@pytest.mark.parametrize("name,H,W,ingress,flags,rows,N,T", KERNELS, ids=[k[0] for k in KERNELS])
def test_rollout_ex_matches_step_launches(name, H, W, ingress, flags, rows, N, T):
    errs = RR.case_compare(RR.HipResearchBackend, RR.HipResearchBackend, H, W, N, T, seed=H * 7 + W + len(name), flags=flags, rows=rows,
                           ingress=ingress, step_limit=4)
    assert not errs, "\n".join(errs[:10])


def test_rollout_ex_big_grid_loops_step_launches():
    """40 x 40: the workgroup-per-env kernels; every step's outputs land in their own slices."""
    roll, twin, ops = RR.make_pair(RR.HipResearchBackend, RR.HipResearchBackend, 40, 40, 24, 5, 0, step_limit=3, aug=0)
    rng = np.random.default_rng(6)
    pay, op = RR._actions(rng, ops, "bbox", 24, 40, 40, 10)
    errs = RR.compare(roll, twin, "bbox", pay, op, RR.RESAMPLE | RR.TRUNCATE | RR.DENSE | RR.FLAT_OBS, "full", tag="40x40")
    assert not errs, "\n".join(errs[:10])
    assert np.asarray(roll.episode).max() >= 3


def test_step_after_big_grid_rollout_ex_writes_the_installed_outputs():
    """A rollout's step launches carry their own destinations and leave the handle's alone: arcle_rollout_ex on a 40 x 40 handle with all
    four outputs writes nothing into the buffers the setters installed, and the plain step after it (FLAT_OBS | PACK_OBS | TRUNCATE |
    DENSE) fills them — rows, tail and sequence number included — exactly as on a twin that only ever stepped."""
    N, SEQ = 24, 7
    roll, twin, ops = RR.make_pair(RR.HipResearchBackend, RR.HipResearchBackend, 40, 40, N, 8, 0, step_limit=3, aug=0)
    roll.set_flat_output(filtered=False, tail=True)
    roll.set_packed_output()
    assert roll.b.L.arcle_set_flat_seq(roll.b._h, SEQ) == 0
    rng = np.random.default_rng(12)
    pay, op = RR._actions(rng, ops, "bbox", N, 40, 40, 7)
    errs = RR.compare(roll, twin, "bbox", pay[:6], op[:6], RR.RESAMPLE | RR.TRUNCATE | RR.DENSE | RR.FLAT_OBS | RR.PACK_OBS, "full", tag="40x40")
    assert not errs, "\n".join(errs[:10])
    torch.cuda.synchronize()
    assert bool((roll.b._flat_buf == 0x55).all()) and bool((roll.b.packed == 0x55).all()), "the rollout wrote into the installed buffers"
    twin.set_flat_output(filtered=False, tail=True)
    twin.set_packed_output()
    assert twin.b.L.arcle_set_flat_seq(twin.b._h, SEQ) == 0
    flags = RR.FLAT_OBS | RR.PACK_OBS | RR.TRUNCATE | RR.DENSE
    got, want = roll.step("bbox", pay[6], op[6], flags), twin.step("bbox", pay[6], op[6], flags)
    for k, a, b in (("reward", got[0], want[0]), ("terminated", got[1], want[1]), ("trunc", roll.trunc, twin.trunc), ("dense", roll.dense, twin.dense),
                    ("rows", roll.fused_flat(), twin.fused_flat()), ("tail", roll.fused_tail(), twin.fused_tail()),
                    ("packed", roll.fused_packed(), twin.fused_packed())):
        assert np.array_equal(np.asarray(a), np.asarray(b)), f"{k} of the step after the rollout differs from the twin's"
    assert not (roll.fused_flat() == 0x55).all(1).any() and not (roll.fused_packed() == 0x55).all(1).any()
    assert (((roll.fused_tail()[:, 3] >> 24) & 0xFF) == SEQ).all(), "the tail's sequence number"


def test_mask_rollout_continue_rule_reset_on_submit_dense():
    errs = RR.mask_rules_compare(RR.HipResearchBackend, RR.HipResearchBackend, 30, 30, N=65, T=16, seed=9)
    assert not errs, "\n".join(errs[:10])


def test_golden_dense_vectors_as_one_mask_rollout():
    errs = RR.golden_dense_rollout(RR.HipResearchBackend)
    assert not errs, "\n".join(errs[:10])


# ---- ARCVecEnv.rollout in the research configuration ----------------------------------------------------------------------------------
def research_env(n, env_base=0, limit=100):
    from arcle_amd import actions
    from arcle_amd.envs import ARCVecEnv, O2ARCv2Env
    from arcle_amd.loaders import SyntheticLoader

    class Crop(O2ARCv2Env):  # agents/env.py:23-28 (bench.py research_env_leg)
        def create_operations(self):
            ops = super().create_operations()
            ops[33] = actions.reset_sel(actions.crop_grid)
            return ops
    v = ARCVecEnv(Crop, n, SyntheticLoader(n_tasks=400, seed=1, max_size=(30, 30)), seed=7, autoreset="resample",
                  augment=("permute", "rot90"), dense_reward=True, max_episode_steps=limit, env_base=env_base)
    v.reset()
    return v


def desync(envs, n_total, seed=3, limit=100):
    """The same desynchronised step counters (bench.py research_env_leg) in every env / shard of the list."""
    g = torch.Generator().manual_seed(seed)
    steps = torch.randint(0, limit, (n_total,), generator=g, dtype=torch.int32)
    off = 0
    for v in envs:
        v.batch.cnt[:, 0] = steps[off:off + v.N].to(v.device)
        off += v.N


def actions_bbox(n, T, seed=4):
    g = torch.Generator().manual_seed(seed)
    bbox = torch.randint(0, 30, (T, n, 4), generator=g, dtype=torch.int32)
    op = torch.randint(0, 35, (T, n), generator=g, dtype=torch.int32)
    op[torch.rand((T, n), generator=g) < 0.05] = 34
    return bbox.cuda(), op.cuda()


def obs_equal(a, b):
    for k, v in a.items():
        if isinstance(v, dict):
            if not obs_equal(v, b[k]):
                return False
        elif not torch.equal(v, b[k]):
            return False
    return True


def info_equal(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("steps", "submit_count", "table_index", "input_dim", "answer_dim"))


def test_vec_env_research_rollout_matches_step_bbox_8192():
    N, T = 8192, 32
    v, tw = research_env(N), research_env(N)
    tw.enable_flat_rows(filtered=True)
    v.enable_flat_rows(filtered=True)
    desync([v], N)
    desync([tw], N)
    tw._refresh_rows()
    v._refresh_rows()
    bbox, op = actions_bbox(N, T)
    want = []
    for t in range(T):
        _, r, tm, tr, _ = tw.step_bbox(bbox[t], op[t])
        want.append((r.clone(), tm.clone(), tr.clone(), tw.rows.clone()))
    L = v.batch.flat_obs_size(True)
    rows = torch.full((T, N, (L + 15) & ~15), 0x55, dtype=torch.int8, device=v.device)
    obs, r, tm, tr, info = v.rollout(bbox, op, form="bbox", rows=rows, rows_kind="filtered")
    torch.cuda.synchronize()
    assert r.dtype == torch.float32 and r.shape == (T, N)
    for t, (wr, wtm, wtr, wrows) in enumerate(want):
        assert torch.equal(r[t], wr), f"step {t}: reward"
        assert torch.equal(tm[t], wtm), f"step {t}: terminated"
        assert torch.equal(tr[t], wtr), f"step {t}: truncated"
        assert torch.equal(rows[t, :, :L], wrows), f"step {t}: rows"
        assert not rows[t, :, L:].any()
    assert bool(tr.any()) and bool(tm.any()), "the stretch should truncate and terminate episodes"
    assert obs_equal(obs, tw._obs) and info_equal(info, tw._info())
    assert torch.equal(v.batch.episode, tw.batch.episode) and torch.equal(v.rows, tw.rows)
    assert v.batch.status() == 0 and tw.batch.status() == 0


def test_vec_env_rollout_bbox5_and_packed_rows():
    N, T = 1024, 12
    v, tw = research_env(N, limit=6), research_env(N, limit=6)
    bbox, op = actions_bbox(N, T, seed=8)
    rec = torch.cat([bbox, op[..., None]], dim=2).contiguous()
    want = [tuple(x.clone() for x in tw.step_bbox(bbox[t], op[t])[1:4]) + (tw._obs["grid"].clone(),) for t in range(T)]
    R = v.batch.packed_obs_size()
    packed = torch.full((T, N, R), 0x55, dtype=torch.uint8, device=v.device)
    obs, r, tm, tr, info = v.rollout(rec, form="bbox5", rows=packed, rows_kind="packed")
    for t, (wr, wtm, wtr, wg) in enumerate(want):
        assert torch.equal(r[t], wr) and torch.equal(tm[t], wtm) and torch.equal(tr[t], wtr), f"step {t}"
        g, _, _, term = v.batch.unpack_obs(packed[t], 30, 30)
        assert torch.equal(g, wg) and torch.equal(term, wtm), f"step {t}: packed row"
    assert obs_equal(obs, tw._obs) and info_equal(info, tw._info())


def test_vec_env_rollout_half_shards_reproduce_the_whole_batch():
    N, T = 2048, 16
    whole, lo, hi = research_env(N, limit=8), research_env(N // 2, 0, limit=8), research_env(N // 2, N // 2, limit=8)
    desync([whole], N, limit=8)
    desync([lo, hi], N, limit=8)
    bbox, op = actions_bbox(N, T, seed=12)
    _, r, tm, tr, _ = whole.rollout(bbox, op)
    parts = [s.rollout(bbox[:, sl].contiguous(), op[:, sl].contiguous()) for s, sl in ((lo, slice(0, N // 2)), (hi, slice(N // 2, N)))]
    for i, x in ((1, r), (2, tm), (3, tr)):
        assert torch.equal(x, torch.cat([parts[0][i], parts[1][i]], dim=1))
    for k in ("grid", "input"):
        assert torch.equal(whole._obs[k], torch.cat([lo._obs[k], hi._obs[k]]))
    assert torch.equal(whole.batch.episode, torch.cat([lo.batch.episode, hi.batch.episode]))
    assert int(whole.batch.episode.max()) >= 3


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def snapshot(b):
    return [t.clone() for t in list(b.planes.values()) + [b.rec, b.cnt] + ([b.episode, b.cur_task] if hasattr(b, "episode") else [])]


def unchanged(b, snap):
    torch.cuda.synchronize()
    return all(torch.equal(a, c) for a, c in zip(snapshot(b), snap))


def test_rollout_ex_refusals_return_their_code_and_change_nothing():
    v = research_env(256)
    b = v.batch
    T, N = 3, b.N
    L = b.flat_obs_size(True)
    dev = b.device
    bbox, op = actions_bbox(N, T)
    reward = torch.full((T, N), 0x55, dtype=torch.int32, device=dev)
    term = torch.full((T, N), 0x55, dtype=torch.uint8, device=dev)
    trunc = torch.full((T, N), 0x55, dtype=torch.uint8, device=dev)
    dense = torch.full((T, N, 2), 0x55, dtype=torch.int32, device=dev)
    rows = torch.full((T, N, ((L + 15) & ~15) + 16), 0x55, dtype=torch.int8, device=dev)
    packed = torch.full((T, N, b.packed_obs_size()), 0x55, dtype=torch.uint8, device=dev)
    bufs = [reward, term, trunc, dense, rows, packed]
    keep = [x.clone() for x in bufs]
    snap = snapshot(b)
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731

    def call(flags, ingress=1, n_steps=T, out=None):
        o = None if out is None else ctypes.byref(out)
        return b.L.arcle_rollout_ex(b._h, ingress, n_steps, p(bbox), p(op), p(reward), p(term), o, flags, b._stream())

    full = lambda **kw: _lib.RolloutOut(*[kw.get(k, d) for k, d in (("trunc", p(trunc)), ("dense", p(dense)), ("rows", p(rows)),  # noqa: E731
                                                                    ("rows_stride", (L + 15) & ~15), ("rows_filtered", 1), ("packed", p(packed)))])
    R = RR.RESEARCH
    cases = [
        ("incremental rows", dict(flags=R | 512, out=full()), ERR_ARG),
        ("no out struct", dict(flags=RR.TRUNCATE), ERR_ARG),
        ("truncate without trunc", dict(flags=RR.TRUNCATE, out=full(trunc=None)), ERR_ARG),
        ("dense without dense", dict(flags=RR.DENSE, out=full(dense=None)), ERR_ARG),
        ("rows without rows", dict(flags=R, out=full(rows=None)), ERR_ARG),
        ("wrong row stride", dict(flags=R, out=full(rows_stride=((L + 15) & ~15) + 16)), ERR_ARG),
        ("misaligned rows", dict(flags=R, out=full(rows=p(rows) + 8)), ERR_ARG),
        ("packed without packed", dict(flags=RR.PACK_OBS, out=full(packed=None)), ERR_ARG),
        ("unknown flag", dict(flags=1024, out=full()), ERR_ARG),
        ("bbox5 ingress", dict(flags=R, ingress=3, out=full()), ERR_ARG),
        ("no steps", dict(flags=R, n_steps=0, out=full()), ERR_ARG),
        ("continue rule with tuples", dict(flags=RR.CONTINUE, out=full()), ERR_CONFIG),
        ("reset_on_submit with tuples", dict(flags=RR.ROS, out=full()), ERR_CONFIG),
    ]
    for name, kw, code in cases:
        assert call(**kw) == code, name
        assert unchanged(b, snap) and all(torch.equal(x, y) for x, y in zip(bufs, keep)), f"{name}: something was written"
    # TRUNCATE without a positive step limit (arcle_set_truncation stores the limit unchecked when its output is NULL)
    assert b.L.arcle_set_truncation(b._h, None, 0) == 0
    assert call(RR.TRUNCATE, out=full()) == ERR_CONFIG
    assert b.L.arcle_set_truncation(b._h, b.trunc.data_ptr(), 100) == 0
    # RESAMPLE without a sampler
    from arcle_amd.engine import EnvBatch
    plain = EnvBatch(N, 30, 30, 3, "o2arc")
    plain.set_op_table(RR.O.o2arc_ops())
    plain.reset()
    psnap = snapshot(plain)
    rc = plain.L.arcle_rollout_ex(plain._h, 1, T, p(bbox), p(op), p(reward), p(term), ctypes.byref(full()), RR.RESAMPLE, plain._stream())
    assert rc == ERR_CONFIG and unchanged(plain, psnap)
    assert unchanged(b, snap) and all(torch.equal(x, y) for x, y in zip(bufs, keep))
    # the existing entry points keep refusing the research flags
    assert b.L.arcle_rollout_bbox(b._h, T, p(bbox), p(op), p(reward), p(term), RR.TRUNCATE, b._stream()) == ERR_ARG
    assert b.status() == 0


def test_python_checks_raise_before_any_launch():
    v = research_env(256)
    b = v.batch
    T, N = 2, b.N
    bbox, op = actions_bbox(N, T)
    L = (b.flat_obs_size(True) + 15) & ~15
    snap = snapshot(b)
    dev = b.device
    ok = dict(trunc=torch.zeros((T, N), dtype=torch.uint8, device=dev), dense=torch.zeros((T, N, 2), dtype=torch.int32, device=dev),
              rows=torch.zeros((T, N, L), dtype=torch.int8, device=dev), rows_filtered=True)
    bad = [
        dict(trunc=torch.zeros((T, N + 1), dtype=torch.uint8, device=dev)),
        dict(trunc=torch.zeros((T, N), dtype=torch.int32, device=dev)),
        dict(trunc=torch.zeros((T, N), dtype=torch.uint8)),
        dict(dense=torch.zeros((T, N, 3), dtype=torch.int32, device=dev)),
        dict(dense=torch.zeros((T, 2, N), dtype=torch.int32, device=dev).transpose(1, 2)),
        dict(rows=torch.zeros((T, N, L + 16), dtype=torch.int8, device=dev)),
        dict(rows=torch.zeros((T, N, L), dtype=torch.int8, device=dev), rows_filtered=False),
        dict(rows=torch.zeros((T + 1, N, L), dtype=torch.int8, device=dev)),
    ]
    for i, kw in enumerate(bad):
        with pytest.raises(ValueError):
            b.rollout_ex(bbox, op, RR.RESEARCH, "bbox", **{**ok, **kw})
        assert unchanged(b, snap), f"case {i}"
    with pytest.raises(ValueError):
        b.rollout_ex(bbox[:, :, :2], op, RR.RESEARCH, "bbox", **ok)
    with pytest.raises(ValueError):
        b.rollout_ex(bbox, op.to(torch.int64), RR.RESEARCH, "bbox", **ok)
    with pytest.raises(ValueError):
        b.rollout_ex(bbox, op, RR.RESEARCH & ~RR.DENSE, "bbox", **ok)  # a tensor without its flag
    with pytest.raises(ValueError):
        b.rollout_ex(bbox, op, RR.RESEARCH, "bbox5", **ok)
    with pytest.raises(ValueError):
        v.rollout(bbox, op, rows=ok["rows"], rows_kind="nope")
    with pytest.raises(ValueError):
        v.rollout(bbox.cpu(), op)
    with pytest.raises(ValueError):
        v.rollout(torch.zeros((T, N, 4), dtype=torch.int32, device=dev), form="bbox5")
    with pytest.raises(ArcleHipError):  # the library refuses a flag whose output is missing (ARCLE_ERR_ARG)
        b.rollout_ex(bbox, op, RR.RESEARCH, "bbox", trunc=ok["trunc"], dense=ok["dense"])
    assert unchanged(b, snap)
