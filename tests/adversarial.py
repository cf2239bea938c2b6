"""Adversarial state streams for the step kernel's elided plane stores.

The step kernel stores a plane chunk only where it can prove the bytes in memory already hold the new value (arcle_wave.h
Wave::store_if).  These streams start every env from a state whose planes hold non-zero garbage everywhere — also outside the
rectangles the record describes (object tile, placed selection, grid_dim) — installed through arcle_set_state_rows, then step
the kernel and the oracle side by side and compare every field after every step.  A chunk skipped on a wrong assumption leaves
stale bytes behind and shows up as a field mismatch."""
import numpy as np

import backends as B
from oracle import oracle as O

# the garbage planes: every plane of the state row except input (the task) and answer (not part of a row)
GARBAGE = ("grid", "selected", "clip", "object", "object_sel", "background")


def adversarial_state(orc, rng, elide):
    """Fills the oracle's state with in-domain records and garbage planes.  With `elide` the state keeps the invariant
    ARCLE_STEP_ELIDE_SELECTED documents (active == 0 implies an all-zero `selected`) and nothing else."""
    env = orc.env
    N, H, W = env.N, env.H, env.W
    for f in GARBAGE:
        g = rng.integers(1, 12, (N, H, W)).astype(np.int8)
        g[rng.random((N, H, W)) < 0.1] = 0
        env.planes[f][:] = g
    env.field("grid_dim")[:] = np.stack([rng.integers(1, H + 1, N), rng.integers(1, W + 1, N)], 1)
    env.field("clip_dim")[:] = np.stack([rng.integers(0, H + 1, N), rng.integers(0, W + 1, N)], 1)
    env.field("object_dim")[:] = np.stack([rng.integers(1, H + 1, N), rng.integers(1, W + 1, N)], 1)
    env.field("object_pos")[:] = np.stack([rng.integers(-2, H, N), rng.integers(-2, W, N)], 1)
    active = (rng.random(N) < 0.5).astype(np.int8)
    env.field("active")[:, 0] = active
    env.field("rotation_parity")[:, 0] = rng.integers(0, 2, N)
    if elide:
        env.planes["selected"][active == 0] = 0


def payloads(rng, N, H, W, int8_masks):
    if int8_masks:
        pay = np.zeros((N, H, W), np.int8)
        for n in range(N):
            t = rng.integers(0, 4)
            x, y = rng.integers(0, H), rng.integers(0, W)
            if t == 0:
                pay[n] = rng.integers(-3, 4, (H, W)) * (rng.random((H, W)) < rng.random() * 0.2)
            elif t == 1:
                pay[n, x, y] = [1, 2, -1, 127][rng.integers(0, 4)]
            elif t == 2:
                pay[n, x:x + rng.integers(1, 8), y:y + rng.integers(1, 8)] = 1
            else:
                pay[n] = rng.random((H, W)) < rng.random() * 0.3
        return "mask", pay
    pay = np.stack([rng.integers(0, H, N), rng.integers(0, W, N), rng.integers(0, H, N), rng.integers(0, W, N)], 1)
    small = rng.random(N) < 0.3
    pay[small, 2] = np.minimum(H - 1, pay[small, 0] + rng.integers(0, 3, small.sum()))
    pay[small, 3] = np.minimum(W - 1, pay[small, 1] + rng.integers(0, 3, small.sum()))
    return "bbox", pay.astype(np.int32)


def adversarial_compare(backend_cls, ops, H, W, N, S, seed, flags=0, int8_masks=False, op_weights=None, restate_every=0):
    """Steps `backend_cls` and the oracle from the same garbage state (set through set_state_rows); returns mismatches.
    restate_every > 0: every that many steps all envs get a fresh garbage state (between steps, as a user write would)."""
    rng = np.random.default_rng(seed)
    be = backend_cls(N, H, W, 3, "o2arc", ops)
    orc = B.OracleBackend(N, H, W, 3, "o2arc", ops)
    inp = rng.integers(0, 10, (N, H, W)).astype(np.int8)
    ans = rng.integers(0, 10, (N, H, W)).astype(np.int8)
    idim = np.stack([rng.integers(1, H + 1, N), rng.integers(1, W + 1, N)], 1).astype(np.int8)
    adim = np.stack([rng.integers(1, H + 1, N), rng.integers(1, W + 1, N)], 1).astype(np.int8)
    for b in (be, orc):
        b.set_tasks(inp, idim, ans, adim)
        b.reset()
    elide = bool(flags & B.STEP_ELIDE_SELECTED)
    n_ops = len(ops)
    w = np.ones(n_ops) if op_weights is None else np.asarray(op_weights, float)
    w = w / w.sum()
    fields = [f for f in O.PLANES if f != "answer"] + [f for f in O.REC if f != "answer_dim"]
    errs = []
    for s in range(S):
        if s == 0 or (restate_every and s % restate_every == 0):
            adversarial_state(orc, rng, elide)
            be.set_state_rows(B.state_rows(orc))
        op = rng.choice(n_ops, size=N, p=w).astype(np.int32)
        ing, pay = payloads(rng, N, H, W, int8_masks)
        r1, t1 = be.step(ing, pay, op, flags)
        r2, t2 = orc.step(ing, pay, op, flags)
        tag = f"{H}x{W} N={N} seed {seed} flags {flags} step {s} ingress {ing}"
        if not np.array_equal(r1, r2):
            errs.append(f"{tag}: reward mismatch envs {np.nonzero(r1 != r2)[0][:16].tolist()}")
        if not np.array_equal(t1, t2):
            errs.append(f"{tag}: terminated mismatch envs {np.nonzero(t1 != t2)[0][:16].tolist()}")
        if not np.array_equal(be.counters(), orc.counters()):
            errs.append(f"{tag}: counters mismatch")
        s1, s2 = be.status(), orc.status()
        if s1 != s2:
            errs.append(f"{tag}: status {s1} vs oracle {s2}")
        for f in fields:
            a, b = be.get(f), orc.get(f)
            if not np.array_equal(a, b):
                bad = np.nonzero((a != b).reshape(N, -1).any(1))[0]
                errs.append(f"{tag} field {f}: envs {bad[:16].tolist()} ops {op[bad][:16].tolist()}")
        if errs:
            break
    return errs
