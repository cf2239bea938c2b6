"""Round-4 GPU tests: the oracle meets exactly what bench.py times, at the sizes BASELINE.json names.

  * the headline kernel `arcle_step_kernel<bbox, FULL, 0, 0, autoreset|elide|grouped, 30>` (K single-step calls whose launches order
    themselves; since round 5 also what one arcle_step_many call enqueues) and the plain `<..., autoreset|elide, 30>` (dispatch order
    off), 8192 envs x 64 steps of bench.py's own task / action streams, against the oracle stepping the WHOLE batch (round 5);
  * c4's per-node batch on ONE GPU: 65 536 envs stepped with the fused packed-row epilogue, the packed rows unpacked and compared;
  * c5 at 32 768 envs (ARCEnv, 70 % flood fills);
  * a 300-step slice of tools/soak.py;
  * `bench.py --gpus 2` on one GPU (the N > 1 path: spawn, rendezvous, sharding, max-over-ranks, the compact last line).
Bit-exact everywhere."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import backends as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS_O2 = ["grid", "selected", "clip", "object", "object_sel", "background", "input", "answer", "input_dim", "grid_dim", "clip_dim", "object_dim",
             "object_pos", "trials_remain", "terminated", "active", "rotation_parity", "answer_dim"]
FIELDS_ARC = ["grid", "clip", "input", "answer", "input_dim", "grid_dim", "clip_dim", "trials_remain", "terminated", "answer_dim"]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from arcle_amd import _lib
    _lib.build()
    _lib.lib()
    yield
    O.set_threads(1)


def _sample(n, k, seed):
    """Round 5: the WHOLE batch (the oracle steps 8192 envs x 64 steps in 0.03 s on 16 threads, 196 608 x 10 in 0.2 s): a slot-dependent
    defect of a launch that permutes env <-> dispatch slot cannot hide in an env that was not sampled.  ARCLE_TEST_SAMPLED=1 restores the
    round-4 samples (edges + k random envs) for quick local runs."""
    if not os.environ.get("ARCLE_TEST_SAMPLED"):
        return np.arange(n)
    edge = np.r_[0:32, n // 2 - 16:n // 2 + 16, n - 32:n]
    return np.unique(np.r_[edge, np.random.default_rng(seed).choice(n, k, replace=False)])


def _oracle_for(sample, tasks, H, W, max_trial, kind, ops):
    O.set_threads(16)  # (the C restatement steps envs in an OpenMP loop; the module fixture puts it back to one thread)
    orc = B.OracleBackend(len(sample), H, W, max_trial, kind, ops)
    orc.set_tasks(*(t[sample] for t in tasks))
    orc.reset()
    return orc


def _compare_sample(batch, orc, sample, fields, what):
    import torch
    full = len(sample) == batch.N
    idx = None if full else torch.as_tensor(sample, device=batch.device)
    for f in fields:
        t = batch.plane(f) if f in batch.planes else batch.field(f)
        got = (t if full else t[idx]).cpu().numpy()
        assert np.array_equal(got, orc.get(f)), f"{what}: field {f} differs from the oracle"
    assert np.array_equal((batch.cnt if full else batch.cnt[idx]).cpu().numpy(), orc.counters()), f"{what}: counters differ"


@pytest.mark.parametrize("form", ["per_step_calls", "unordered_calls", "step_many", "step_many_bbox5", "hinted_calls"])
@pytest.mark.parametrize("max_trial", [-1, 3])
def test_bench_headline_kernels_vs_oracle_8192(form, max_trial):
    """What bench.py times, checked DIRECTLY against the oracle: 8192 envs x 64 steps of bench.make_tasks / make_actions with
    ARCLE_STEP_AUTORESET | ARCLE_STEP_ELIDE_SELECTED — as K arcle_step_bbox calls (`value`: self-ordering launches), the same with the
    dispatch order off (the plain instantiation), as one arcle_step_many call (bbox + op arrays and 5-tuple records) and as hinted single
    steps.  Every env of the batch, every field, reward and terminated of every step; the sticky status must stay 0."""
    import torch
    import bench
    from arcle_amd import actions
    from arcle_amd.engine import EnvBatch
    from arcle_amd.envs import O2ARCv2Env
    n, K, dev = 8192, 64, torch.device("cuda:0")
    tasks = bench.make_tasks(n, 1000)
    bb_np, op_np = bench.make_actions(K, n, 2000)
    batch = EnvBatch(n, 30, 30, max_trial, "o2arc", dev)
    batch.set_op_table(actions.table_descs(O2ARCv2Env.default_operations()))
    batch.set_tasks_padded(*tasks)
    batch.reset()
    FL = batch.elide_flag | 1
    assert FL == 3, "the O2ARC table permits the zero-fill elision: this is the instantiation bench.py launches"
    bb, op = torch.from_numpy(bb_np).to(dev), torch.from_numpy(op_np).to(dev)
    if form in ("per_step_calls", "unordered_calls"):
        batch.set_dispatch_order(form == "per_step_calls")  # (off: the plain instantiation, every wave steps the env of its own slot)
        rew, trm = torch.empty((K, n), dtype=torch.int32, device=dev), torch.empty((K, n), dtype=torch.uint8, device=dev)
        for s in range(K):
            r, t = batch.step_bbox(bb[s], op[s], FL)
            rew[s], trm[s] = r, t
    elif form == "hinted_calls":  # single-step calls, each told the NEXT step's operations (arcle_hint_next_ops)
        rew, trm = torch.empty((K, n), dtype=torch.int32, device=dev), torch.empty((K, n), dtype=torch.uint8, device=dev)
        for s in range(K):
            if s + 1 < K:
                batch.hint_next_ops(op[s + 1])
            r, t = batch.step_bbox(bb[s], op[s], FL)
            rew[s], trm[s] = r, t
    elif form == "step_many":
        rew, trm = batch.step_many("bbox", bb, op, FL)
    else:
        rew, trm = batch.step_many("bbox5", torch.cat([bb, op[:, :, None]], 2).contiguous(), None, FL)
    torch.cuda.synchronize()
    assert batch.status() == 0
    sample = _sample(n, 352, 5)
    orc = _oracle_for(sample, tasks, 30, 30, max_trial, "o2arc", O.o2arc_ops())
    rew, trm = rew.cpu().numpy(), trm.cpu().numpy()
    ended = 0
    for s in range(K):
        r2, t2 = orc.step("bbox", bb_np[s][sample], op_np[s][sample], O.STEP_AUTORESET)
        assert np.array_equal(rew[s][sample], r2) and np.array_equal(trm[s][sample], t2), f"{form}: reward / terminated differ at step {s}"
        ended += int(t2.sum())
    assert ended > 0, "the trace must exercise the auto-reset path"
    _compare_sample(batch, orc, sample, FIELDS_O2, form)


@pytest.mark.parametrize("variant", ["bbox", "point", "bbox5", "bbox_pack"])
def test_hinted_single_steps_are_scheduling_only(variant):
    """arcle_hint_next_ops (ABI 4's hint of the next step's operations; launches order themselves since ABI 5 and ignore it) + single-step
    calls with the flag sets ARCVecEnv / ShardedVecEnv step with: rewards, terminated flags, packed rows and every byte of state equal
    the run that never hints and has the dispatch order switched off — wrong hints (the ops of some other step) and dropped hints included."""
    import torch
    import bench
    from arcle_amd.engine import STEP_PACK_OBS
    n, K, dev = 4096, 20, torch.device("cuda:0")
    bb_np, op_np = bench.make_actions(K, n, 321)
    bb, op = torch.from_numpy(bb_np).to(dev), torch.from_numpy(op_np).to(dev)
    xy = bb[:, :, :2].contiguous()
    act5 = torch.cat([bb, op[:, :, None]], 2).contiguous()
    a, b = bench.make_batch(dev, n, seed=11), bench.make_batch(dev, n, seed=11)
    a.set_dispatch_order(False)
    FL = a.elide_flag | 1
    if variant == "bbox_pack":
        FL |= STEP_PACK_OBS
        pa, pb = a.set_packed_output(), b.set_packed_output()

    def one(batch, s):
        if variant == "point":
            return batch.step_point(xy[s], op[s], FL)
        if variant == "bbox5":
            return batch.step_bbox5(act5[s], FL)
        return batch.step_bbox(bb[s], op[s], FL)
    for s in range(K):
        ra, ta = one(a, s)
        ra, ta = ra.clone(), ta.clone()
        if s + 1 < K and s % 7 != 5:  # (every 7th step: no hint — the next launch must fall back to the identity order)
            wrong = s % 5 == 3        # (every 5th: the ops of ANOTHER step — costs nothing but the ordering)
            nxt = (s + 4) % K if wrong else s + 1
            b.hint_next_ops(act5[nxt] if variant == "bbox5" else op[nxt])
        rb, tb = one(b, s)
        assert torch.equal(ra, rb) and torch.equal(ta, tb), (variant, s)
        if variant == "bbox_pack":
            assert torch.equal(pa, pb), (variant, s)
    torch.cuda.synchronize()
    for k in a.planes:
        assert torch.equal(a.planes[k], b.planes[k]), (variant, k)
    assert torch.equal(a.rec, b.rec) and torch.equal(a.cnt, b.cnt) and a.status() == b.status() == 0


def test_vec_env_next_operation_argument_and_research_flags_ordered():
    """ARCVecEnv.step_bbox(bbox, op, next_operation=...) and the research env's flag set (dense reward, TimeLimit, device-drawn tasks,
    incremental FilterO2ARC rows) with ordered dispatch: identical to a twin that never hints / has ordered dispatch switched off."""
    import torch
    import bench
    from arcle_amd.envs import ARCVecEnv, O2ARCv2Env
    from arcle_amd.loaders import SyntheticLoader
    n, K, dev = 4096, 24, torch.device("cuda:0")  # (batches of at most 2048 envs run 256-thread workgroups, unordered)
    bb_np, op_np = bench.make_actions(K, n, 99)
    bb, op = torch.from_numpy(bb_np).to(dev), torch.from_numpy(op_np).to(dev)
    kw = dict(device=dev, seed=5, autoreset="resample", augment=("permute", "rot90"), dense_reward=True, max_episode_steps=9)
    va = ARCVecEnv(O2ARCv2Env, n, SyntheticLoader(n_tasks=60, seed=2, max_size=(30, 30)), **kw)
    vb = ARCVecEnv(O2ARCv2Env, n, SyntheticLoader(n_tasks=60, seed=2, max_size=(30, 30)), **kw)
    va.batch.set_dispatch_order(False)
    for v in (va, vb):
        v.reset()
        v.enable_flat_rows(filtered=True)
    for s in range(K):
        _, ra, ta, tra, _ = va.step_bbox(bb[s], op[s])
        _, rb, tb, trb, _ = vb.step_bbox(bb[s], op[s], next_operation=op[s + 1] if s + 1 < K else None)
        assert torch.equal(ra, rb) and torch.equal(ta, tb) and torch.equal(tra, trb), s
        assert torch.equal(va.rows, vb.rows), s
    # K steps per call: step_many on the ordered twin (the library hints every step itself) vs single steps on the other
    _, rm, tm, trm, _ = vb.step_many(bb, op)
    for s in range(K):
        _, ra, ta, tra, _ = va.step_bbox(bb[s], op[s])
        assert torch.equal(ra, rm[s]) and torch.equal(ta, tm[s]) and torch.equal(tra, trm[s]), s
    assert torch.equal(va.rows, vb.rows)
    for k in va.batch.planes:
        assert torch.equal(va.batch.planes[k], vb.batch.planes[k]), k
    va.check_errors(), vb.check_errors()


class _Env:
    """Tuning overrides the library reads at arcle_create (ARCLE_STREAM_POLICY, ARCLE_SPEC_SMALL_MAX, ARCLE_WPW)."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.mark.parametrize("policy", ["0", "A", "B", "H", "J"])
@pytest.mark.parametrize("form", ["bbox", "bbox5"])
def test_speculative_grid_instantiations_vs_oracle(policy, form):
    """The instantiations that request the grid plane beside the per-env scalars (ARCLE_STEPX_STREAM with write-through / non-temporal
    stores and a plain / non-temporal speculative load: policies A, B, H, J — what small and very large batches run), forced onto an
    8192-env batch through ARCLE_STREAM_POLICY, against the oracle: rewards and terminated flags of every step, every state field of a
    448-env sample, max_trial = 3 so that auto-resets (which discard the speculative plane) are frequent."""
    import torch
    import bench
    n, K, dev = 8192, 48, torch.device("cuda:0")
    tasks = bench.make_tasks(n, 1000)
    bb_np, op_np = bench.make_actions(K, n, 2000)
    with _Env(ARCLE_STREAM_POLICY=policy):
        from arcle_amd import actions
        from arcle_amd.engine import EnvBatch
        from arcle_amd.envs import O2ARCv2Env
        batch = EnvBatch(n, 30, 30, 3, "o2arc", dev)
    batch.set_op_table(actions.table_descs(O2ARCv2Env.default_operations()))
    batch.set_tasks_padded(*tasks)
    batch.reset()
    bb, op = torch.from_numpy(bb_np).to(dev), torch.from_numpy(op_np).to(dev)
    act5 = torch.cat([bb, op[:, :, None]], 2).contiguous()
    rew, trm = torch.empty((K, n), dtype=torch.int32, device=dev), torch.empty((K, n), dtype=torch.uint8, device=dev)
    for s in range(K):
        r, t = batch.step_bbox(bb[s], op[s], 3) if form == "bbox" else batch.step_bbox5(act5[s], 3)
        rew[s], trm[s] = r, t
    torch.cuda.synchronize()
    assert batch.status() == 0
    sample = _sample(n, 352, 15)
    orc = _oracle_for(sample, tasks, 30, 30, 3, "o2arc", O.o2arc_ops())
    rew, trm = rew.cpu().numpy(), trm.cpu().numpy()
    for s in range(K):
        r2, t2 = orc.step("bbox", bb_np[s][sample], op_np[s][sample], O.STEP_AUTORESET)
        assert np.array_equal(rew[s][sample], r2) and np.array_equal(trm[s][sample], t2), f"policy {policy} {form}: reward / terminated differ at step {s}"
    _compare_sample(batch, orc, sample, FIELDS_O2, f"policy {policy} {form}")


@pytest.mark.parametrize("n", [40960, 131072, 196608])
def test_streaming_regime_at_its_own_sizes_vs_oracle(n):
    """The batch sizes at which the launcher itself switches policy (B from 34 816, H from 110 592, J from 155 648 envs): 131 072 envs is
    bench.py's out-of-cache leg.  10 steps of bench's streams, a 600-env sample against the oracle, every field."""
    import torch
    import bench
    K, dev = 10, torch.device("cuda:0")
    tasks = bench.make_tasks(n, 1000)
    bb_np, op_np = bench.make_actions(K, n, 2000)
    batch = bench.make_batch(dev, n, seed=1000)
    bb, op = torch.from_numpy(bb_np).to(dev), torch.from_numpy(op_np).to(dev)
    rew, trm = batch.step_many("bbox", bb, op, 3)
    torch.cuda.synchronize()
    assert batch.status() == 0
    sample = _sample(n, 504, 21)
    orc = _oracle_for(sample, tasks, 30, 30, -1, "o2arc", O.o2arc_ops())
    rew, trm = rew.cpu().numpy(), trm.cpu().numpy()
    for s in range(K):
        r2, t2 = orc.step("bbox", bb_np[s][sample], op_np[s][sample], O.STEP_AUTORESET)
        assert np.array_equal(rew[s][sample], r2) and np.array_equal(trm[s][sample], t2), s
    _compare_sample(batch, orc, sample, FIELDS_O2, f"streaming @ {n}")
    del batch
    torch.cuda.empty_cache()


@pytest.mark.parametrize("small_max,wpw", [(0, None), (4096, None), (4096, 8), (0, 4)])
def test_small_batch_speculation_and_workgroup_size_are_invisible(small_max, wpw):
    """Batches of at most 2048 envs request the grid speculatively and run 256-thread workgroups by default; every test of this suite
    with a small batch therefore exercises those paths.  Here the same differential traces run with the speculation off / on and both
    workgroup sizes (ARCLE_SPEC_SMALL_MAX, ARCLE_WPW): 30x30 with ARCVecEnv's flags (the lean instantiations), a FAST-width and a
    generic-width shape, ARCEnv / RawARCEnv tables, record and point ingress."""
    with _Env(ARCLE_SPEC_SMALL_MAX=small_max, ARCLE_WPW=wpw):
        for H, W, flags in ((30, 30, 3), (30, 30, 0), (24, 32, 1), (10, 10, 3), (7, 12, 1)):
            errs = B.random_trace_compare(B.HipBackend, "o2arc", O.o2arc_ops(), H, W, N=160, S=64, seed=H * 17 + W + flags, max_trial=3, flags=flags,
                                          bad_ops=True)
            assert not errs, f"{H}x{W} flags {flags}: " + "\n".join(errs[:6])
        errs = B.random_trace_compare(B.HipBackend, "o2arc", O.o2arc_ops(), 30, 30, N=96, S=48, seed=4, max_trial=3, flags=3, new_forms=True)
        assert not errs, "\n".join(errs[:6])
        for kind, ops in (("arc", O.arc_ops()), ("raw", O.raw_ops())):
            errs = B.random_trace_compare(B.HipBackend, kind, ops, 10, 10, N=64, S=64, seed=9, max_trial=3, flags=1)
            assert not errs, kind + ": " + "\n".join(errs[:6])


def test_c4_65536_envs_packed_rows_vs_oracle():
    """BASELINE configs[3]'s per-node batch on one GPU: 65 536 envs (state 0.5 GB, the streaming regime: 4-wave workgroups) stepped
    with the fused packed-row epilogue ShardedVecEnv uses; after every step the packed rows of the sampled envs — grid | grid_dim |
    reward | terminated — and at the end every state field equal the oracle's."""
    import torch
    import bench
    from arcle_amd import actions
    from arcle_amd.engine import EnvBatch, STEP_PACK_OBS
    from arcle_amd.envs import O2ARCv2Env
    n, K, dev = 65536, 20, torch.device("cuda:0")
    tasks = bench.make_tasks(n, 1000)
    bb_np, op_np = bench.make_actions(K, n, 2000)
    batch = EnvBatch(n, 30, 30, -1, "o2arc", dev)
    batch.set_op_table(actions.table_descs(O2ARCv2Env.default_operations()))
    batch.set_tasks_padded(*tasks)
    batch.reset()
    packed = batch.set_packed_output()
    packed.fill_(0x55)
    FL = batch.elide_flag | 1 | STEP_PACK_OBS
    sample = _sample(n, 416, 6)
    idx = torch.as_tensor(sample, device=dev)
    orc = _oracle_for(sample, tasks, 30, 30, -1, "o2arc", O.o2arc_ops())
    bb, op = torch.from_numpy(bb_np).to(dev), torch.from_numpy(op_np).to(dev)
    for s in range(K):
        r, t = batch.step_bbox(bb[s], op[s], FL)
        r2, t2 = orc.step("bbox", bb_np[s][sample], op_np[s][sample], O.STEP_AUTORESET)
        grid, gdim, rew, term = EnvBatch.unpack_obs(packed[idx], 30, 30)
        assert np.array_equal(rew.cpu().numpy(), r2) and np.array_equal(term.cpu().numpy(), t2.astype(bool)), s
        assert np.array_equal(r[idx].cpu().numpy(), r2) and np.array_equal(t[idx].cpu().numpy(), t2), s
        assert np.array_equal(grid.cpu().numpy(), orc.get("grid")) and np.array_equal(gdim.cpu().numpy(), orc.get("grid_dim")), s
        assert not packed[idx][:, 907:].any(), "row padding must be zero"
    assert batch.status() == 0
    _compare_sample(batch, orc, sample, FIELDS_O2, "c4 @ 65536")
    # every row of the batch, not only the sample: the packed grid IS the grid plane, reward / terminated ARE the step outputs
    grid, gdim, rew, term = EnvBatch.unpack_obs(packed, 30, 30)
    assert torch.equal(grid, batch.plane("grid")) and torch.equal(gdim, batch.field("grid_dim"))
    assert torch.equal(rew, batch.reward) and torch.equal(term, batch.term != 0)


def test_c5_32768_envs_floodfill_vs_oracle():
    """BASELINE configs[4] at its full size on one GPU: ARCEnv 27-op table, 32 768 envs, 70 % FloodFill point seeds on stripes / blobs /
    spiral corridors (bench.make_tasks_c5 / make_actions_c5), 12 steps; a 1056-env sample against the oracle, every field."""
    import torch
    import bench
    from arcle_amd import actions
    from arcle_amd.engine import EnvBatch
    from arcle_amd.envs import ARCEnv
    n, K, dev = 32768, 12, torch.device("cuda:0")
    tasks = bench.make_tasks_c5(n, 1000)
    bb_np, op_np = bench.make_actions_c5(K, n, 2000)
    batch = EnvBatch(n, 30, 30, -1, "arc", dev)
    batch.set_op_table(actions.table_descs(ARCEnv.default_operations()))
    batch.set_tasks_padded(*tasks)
    batch.reset()
    FL = batch.elide_flag | 1
    bb, op = torch.from_numpy(bb_np).to(dev), torch.from_numpy(op_np).to(dev)
    rew, trm = batch.step_many("bbox", bb, op, FL)
    torch.cuda.synchronize()
    assert batch.status() == 0
    sample = _sample(n, 960, 7)
    O.set_threads(8)
    try:
        orc = _oracle_for(sample, tasks, 30, 30, -1, "arc", O.arc_ops())
        rew, trm = rew.cpu().numpy(), trm.cpu().numpy()
        for s in range(K):
            r2, t2 = orc.step("bbox", bb_np[s][sample], op_np[s][sample], O.STEP_AUTORESET)
            assert np.array_equal(rew[s][sample], r2) and np.array_equal(trm[s][sample], t2), s
    finally:
        O.set_threads(1)
    _compare_sample(batch, orc, sample, FIELDS_ARC, "c5 @ 32768")
    filled = (batch.plane("grid") != batch.plane("input")).flatten(1).any(1).float().mean().item()
    assert filled > 0.5, "most envs must have seen an effective flood fill"


def test_soak_slice():
    """1000 steps of tools/soak.py (every state field after every step vs the oracle: the lean 30x30 instantiations with runtime and
    compile-time flags, FAST / GENERIC width classes, ARCEnv flood fills, 5-tuple / bit-packed ingress, the research flag set with
    the dense cache and incremental rows)."""
    env = dict(os.environ, SOAK_STEPS="1000")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "soak.py")], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if " S=1000" in ln or " S=166" in ln]
    assert len(lines) >= 11 and sum(" policy " in ln for ln in p.stdout.splitlines()) == 5, p.stdout
    bad = [ln for ln in lines if ": OK" not in ln]
    assert not bad, "\n".join(bad)


def _bench(args, launcher=None, timeout=900):
    cmd = (launcher or [sys.executable]) + [os.path.join(ROOT, "bench.py")] + args
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-1500:] + p.stderr[-3000:]
    last = p.stdout.strip().splitlines()[-1]
    assert len(last) < 4000, f"the last stdout line must stay compact ({len(last)} bytes)"
    return json.loads(last), p


@pytest.mark.parametrize("cfg", ["c3", "c4"])
def test_bench_two_ranks_on_one_gpu(cfg):
    """The N > 1 path without a multi-GPU node: `python bench.py --gpus 2` spawns two ranks that share cuda:0 (gloo control plane),
    shards the global batch, takes the max over ranks per region and prints ONE compact, parseable last line."""
    import torch
    if torch.cuda.device_count() != 1:
        pytest.skip("the shared-GPU leg is for one-GPU boxes")
    out, p = _bench(["--gpus", "2", "--steps", "6", "--warmup", "2", "--config", cfg, "--regions", "3", "--full", "--no-cpu-baseline", "--no-extras"])
    assert out["n_gpus"] == 2 and out["steps"] == 6 and out["warmup"] == 2 and out["scaling"] == "weak"
    assert out["config"]["global_envs"] == 2 * out["config"]["envs_per_gpu"] == 16384
    c = out["collective"]
    assert c["world"] == 2 and c["ranks_seen"] == 2 and c["backend"] == "gloo" and c["shared_gpu"] is True
    assert out["value"] > 0 and abs(out["value"] - 6 * 16384 / (out["ms_per_step"] * 6e-3)) / out["value"] < 1e-3
    assert out["roofline"]["frac"] > 0 and out["roofline"]["algorithmic_bytes_per_launch"] > 8192 * 1000
    ranks = [ln for ln in p.stderr.splitlines() if ln.startswith("bench: rank ")]
    assert len(ranks) == 2 and any("rank 0/2" in ln for ln in ranks) and any("rank 1/2" in ln for ln in ranks), p.stderr[-1500:]
    if cfg == "c3":  # the driver's own command (no --config) also measures BASELINE configs[3] / [4] on the same process group
        m = out["multi"]
        assert "error" not in m, m
        assert m["c4_global_envs"] == 16384 and m["c5_global_envs"] == 8192
        for k in ("c4_us_per_step", "c4_serial_us_per_step", "c4_gather_only_us", "gather_GBps", "gather_GBps_per_link_dir", "c5_us_per_step",
                  "c4_value", "c5_value"):
            assert m[k] > 0, k
        assert abs(m["c5_value"] - 8192 / (m["c5_us_per_step"] * 1e-6)) / m["c5_value"] < 1e-2
    else:
        assert "multi" not in out


def test_bench_one_rank_is_the_same_line_with_and_without_a_launcher():
    """SCALE(N = 1) is BENCH: `python bench.py --gpus 1` and the driver's torchrun form run the same code path and print the same keys
    (no process group, no `collective` block), and the stdout of either ends in the compact line."""
    args = ["--gpus", "1", "--steps", "8", "--warmup", "2", "--regions", "3", "--full", "--no-cpu-baseline", "--no-extras"]
    plain, _ = _bench(args)
    launched, _ = _bench(args, launcher=[sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                                         "--master-port", "29533"])
    assert sorted(plain) == sorted(launched) and "collective" not in plain
    for k in ("metric", "unit", "n_gpus", "steps", "warmup", "config", "headline_form", "dtype", "scaling"):
        assert plain[k] == launched[k], k
    assert plain["roofline"]["algorithmic_bytes_per_launch"] == launched["roofline"]["algorithmic_bytes_per_launch"]
    assert plain["forms"]["step_many"]["value"] > 0 and plain["forms"]["dispatch_order_off"]["value"] > 0
    assert plain["roofline"]["kernel"].startswith("arcle_step_kernel<bbox, FULL, 0, 0, autoreset|elide|grouped, 30>")
    assert plain["roofline"]["plan"]["orders_itself"] is True


def test_bench_plain_run_times_k_steps_and_dumps_the_last_one_vs_oracle(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` times exactly K steps (one region) and measures nothing else; --dump-outputs writes
    what the last timed step left, float32 / float64 under 64 MB, the same files from run to run — and equal to the oracle stepping all
    8192 envs through the W warm-up and K timed action batches of bench's own streams."""
    import bench
    K, Wm, n = 8, 3, 8192
    runs = []
    for r in range(2):
        d = tmp_path / f"run{r}"
        out, _ = _bench(["--gpus", "1", "--steps", str(K), "--warmup", str(Wm), "--dump-outputs", str(d)])
        assert out["steps"] == K and out["warmup"] == Wm and out["timing"]["regions"] == 1
        assert out["unit"] == "env-steps/s" and out["higher_is_better"] is True and out["dtype"] == "int8" and out["metric"].startswith("env-steps/sec")
        assert out["value"] > 0 and abs(out["value"] - K * n / (out["ms_per_step"] * K * 1e-3)) / out["value"] < 1e-3
        for k in ("roofline", "forms", "cpu_baseline", "sustained", "legs_us_per_step", "multi"):
            assert k not in out, f"a plain run must not measure `{k}`"
        files = sorted(os.listdir(d))
        arrays = {f[:-4]: np.load(d / f) for f in files}
        assert all(f.endswith(".npy") for f in files) and all(v.dtype in (np.float32, np.float64) for v in arrays.values())
        assert sum(v.nbytes for v in arrays.values()) <= 64 << 20
        runs.append(arrays)
    assert runs[0].keys() == runs[1].keys() and all(np.array_equal(runs[0][k], runs[1][k]) for k in runs[0]), "same arguments, different outputs"
    got = runs[0]
    assert np.array_equal(got["env_index"], np.arange(n))
    S = bench.staged_batches(K, Wm)
    tasks = bench.make_tasks(n, 1000)
    bb_np, op_np = bench.make_actions(S, n, 2000)
    orc = _oracle_for(np.arange(n), tasks, 30, 30, -1, "o2arc", O.o2arc_ops())
    for i in range(Wm + K):
        rew, trm = orc.step("bbox", bb_np[i % S], op_np[i % S], O.STEP_AUTORESET)
    assert np.array_equal(got["reward"], rew) and np.array_equal(got["terminated"], trm), "reward / terminated of the last step"
    assert np.array_equal(got["grid"], orc.get("grid")) and np.array_equal(got["counters"], orc.counters())
    pidx = got["plane_env_index"].astype(np.int64)
    for f in ("selected", "clip", "object", "object_sel", "background"):
        assert np.array_equal(got[f], orc.get(f)[pidx]), f
    for f in ("grid_dim", "clip_dim", "object_dim", "object_pos", "trials_remain", "terminated", "active", "rotation_parity"):
        want = orc.get(f)
        assert np.array_equal(got["rec_" + f], want.reshape(got["rec_" + f].shape)), f
