"""hipGraph captures of the package (ARCVecEnv.capture) against Python garbage: an EnvBatch that is only reachable from dead reference
cycles frees its device buffers (hipFree) when the collector finds it.  If that happened while a capture is under way it would invalidate
the capture, so the package keeps the collector off during captures (engine.capture_guard)."""
import gc
import weakref

import pytest

pytestmark = pytest.mark.gpu

N, K, H = 96, 12, 12


def _env():
    from arcle_amd.envs import ARCVecEnv, O2ARCv2Env
    from arcle_amd.loaders import SyntheticLoader
    v = ARCVecEnv(O2ARCv2Env, N, SyntheticLoader(n_tasks=12, seed=4, max_size=(H, H)), max_grid_size=(H, H), seed=11,
                  autoreset="resample", max_episode_steps=7, dense_reward=True, augment=True)
    v.reset()
    return v


def _actions(seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    bb = torch.randint(0, H, (K, N, 4), generator=g, dtype=torch.int32).cuda().contiguous()
    op = torch.randint(0, 35, (K, N), generator=g, dtype=torch.int32).cuda().contiguous()
    return bb, op


def test_capture_is_not_invalidated_by_an_env_that_dies_during_it(monkeypatch):
    import torch
    from arcle_amd.engine import EnvBatch
    from arcle_amd.envs import ARCVecEnv
    c, twin = _env(), _env()
    holder = [EnvBatch(N, H, H, 3, "o2arc")]  # an env handle whose last reference goes away inside the capture
    dead = weakref.ref(holder[0])
    alive_in_capture = []
    orig = ARCVecEnv._enqueue_steps

    def enqueue(self, *args):
        orig(self, *args)
        if holder:
            cyc = {"b": holder.pop()}
            cyc["self"] = cyc  # the handle is now reachable only from this dead cycle ...
            del cyc
            junk = [[i] for i in range(2000)]  # ... and the allocations here are what normally starts a collection
            del junk
            alive_in_capture.append(dead() is not None)
    monkeypatch.setattr(ARCVecEnv, "_enqueue_steps", enqueue)
    old = gc.get_threshold()
    gc.set_threshold(50, 1, 1)
    try:
        bb, op = _actions(3)
        cs = c.capture(bb, op)
    finally:
        gc.set_threshold(*old)
    assert alive_in_capture == [True], "the handle must not be destroyed while the capture is under way"
    gc.collect()
    assert dead() is None, "the handle was only reachable from garbage"
    monkeypatch.setattr(ARCVecEnv, "_enqueue_steps", orig)
    _, r3, t3, tr3 = cs.replay()
    _, r2, t2, tr2, _ = twin.step_many(bb, op)
    torch.cuda.synchronize()
    assert torch.equal(r2, r3) and torch.equal(t2, t3) and torch.equal(tr2, tr3)
    for k in c.batch.planes:
        assert torch.equal(c.batch.planes[k], twin.batch.planes[k]), k
    assert torch.equal(c.batch.rec, twin.batch.rec) and torch.equal(c.batch.cnt, twin.batch.cnt)
    assert gc.isenabled()
