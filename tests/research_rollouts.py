"""Rollouts with the research env's step flags (arcle_rollout_ex / the FEAT 1 rollout body of arcle_wave.h) against T single steps of a
twin with the same flags.  Shared by tests/test_rollout_research_emu.py (wave emulator) and tests/test_rollout_research_hip.py (MI355X).
Each compare function returns a list of mismatch strings."""
import ctypes

import numpy as np

import backends as B
import features as F
from oracle import oracle as O

TRUNCATE, RESAMPLE, DENSE, FLAT_OBS, PACK_OBS = F.STEP_TRUNCATE, F.STEP_RESAMPLE, F.STEP_DENSE, F.STEP_FLAT_OBS, F.STEP_PACK_OBS
AUTORESET, ELIDE, CONTINUE, ROS = F.STEP_AUTORESET, F.STEP_ELIDE, F.STEP_CONTINUE, F.STEP_ROS
RESEARCH = ELIDE | TRUNCATE | RESAMPLE | DENSE | FLAT_OBS  # ARCVecEnv's research env without incremental rows


class EmuResearchBackend(B.EmuBackend):
    """The wave emulator's rollout (emu_run kind 3) with every per-step output: trunc / dense / flat rows / packed rows point at
    [T][N]... arrays (0x55-filled, so that a byte the kernel should write and did not shows)."""

    def rollout_ex(self, ingress, payload, op, flags, rows=None):
        p = self._params()
        self._extras(p)
        T = len(op)
        pay = (np.ascontiguousarray(np.asarray(payload).astype(np.int8)).reshape(T, self.N, self.P) if ingress == "mask"
               else np.ascontiguousarray(payload, np.int32))
        opa = np.ascontiguousarray(op, np.int32)
        reward, term = np.zeros((T, self.N), np.int32), np.zeros((T, self.N), np.uint8)
        out = {}
        p.dense_cache = None  # (the launcher passes none: a rollout keeps no pairs)
        if flags & TRUNCATE:
            out["trunc"] = np.full((T, self.N), 0x55, np.uint8)
            p.trunc = out["trunc"].ctypes.data
        if flags & DENSE:
            out["dense"] = np.full((T, self.N, 2), 0x55, np.int32)
            p.dense = out["dense"].ctypes.data
        if flags & FLAT_OBS:
            L = self._flat_len(rows == "filtered")
            out["rows"] = np.full((T, self.N, (L + 15) & ~15), 0x55, np.int8)
            p.flat_out, p.flat_stride, p.flat_filter, p.flat_tail = out["rows"].ctypes.data, out["rows"].shape[2], int(rows == "filtered"), 0
        if flags & PACK_OBS:
            out["packed"] = np.full((T, self.N, (self.P + 7 + 15) & ~15), 0x55, np.uint8)
            p.pack_out = out["packed"].ctypes.data
        p.sel, p.op, p.ingress, p.flags, p.n_steps = pay.ctypes.data, opa.ctypes.data, self.INGRESS[ingress], flags, T
        p.reward, p.term = reward.ctypes.data, term.ctypes.data
        rc = B.emu_lib().emu_run(3, ctypes.byref(p))
        assert rc == 0, f"wave emulator reported error {rc}"
        return reward, term, out


class HipResearchBackend(B.HipBackend):
    """EnvBatch.rollout_ex with 0x55-filled output tensors."""

    def rollout_ex(self, ingress, payload, op, flags, rows=None):
        t, dev, b = self.torch, self.b.device, self.b
        T = len(op)
        if ingress == "mask":
            pay = t.as_tensor(np.ascontiguousarray(np.asarray(payload).astype(np.int8)), device=dev).reshape(T, self.N, self.H, self.W)
        else:
            pay = t.as_tensor(np.ascontiguousarray(payload, np.int32), device=dev)
        opt = t.as_tensor(np.ascontiguousarray(op, np.int32), device=dev)
        kw = {}
        if flags & TRUNCATE:
            kw["trunc"] = t.full((T, self.N), 0x55, dtype=t.uint8, device=dev)
        if flags & DENSE:
            kw["dense"] = t.full((T, self.N, 2), 0x55, dtype=t.int32, device=dev)
        if flags & FLAT_OBS:
            L = b.flat_obs_size(rows == "filtered")
            kw["rows"] = t.full((T, self.N, (L + 15) & ~15), 0x55, dtype=t.int8, device=dev)
            kw["rows_filtered"] = rows == "filtered"
        if flags & PACK_OBS:
            kw["packed"] = t.full((T, self.N, b.packed_obs_size()), 0x55, dtype=t.uint8, device=dev)
        r, tm = b.rollout_ex(pay, opt, flags, ingress, **kw)
        out = {k: v.cpu().numpy() for k, v in kw.items() if k != "rows_filtered"}
        return r.cpu().numpy(), tm.cpu().numpy(), out


def _table(rng, H, W, n):
    ins = [rng.integers(0, 10, (rng.integers(1, H + 1), rng.integers(1, W + 1))).astype(np.int8) for _ in range(n)]
    outs = [rng.integers(0, 10, (rng.integers(1, H + 1), rng.integers(1, W + 1))).astype(np.int8) for _ in range(n)]
    return ins, outs


def _actions(rng, ops, ingress, N, H, W, T, submit=0.2):
    """Random actions with many Submits (small trial budgets then end episodes often)."""
    pay, op = B.rollout_actions(rng, ops, ingress, N, H, W, T)
    op[rng.random((T, N)) < submit] = len(ops) - 1
    return pay, op


def make_pair(roll_cls, step_cls, H, W, N, seed, flags, step_limit=4, max_trial=2, aug=F.AUG_PERMUTE | F.AUG_ROT90, ops=None, env_base=0):
    """Two backends in the same state: tasks from a random table (sampled resets), sampler / truncation / outputs installed."""
    ops = O.o2arc_ops() if ops is None else ops
    rng = np.random.default_rng(seed)
    ins, outs = _table(rng, H, W, 9)
    pair_off, pair_cnt = np.array([0, 2, 3, 7], np.int32), np.array([2, 1, 4, 2], np.int32)
    pair = []
    for cls in (roll_cls, step_cls):
        be = cls(N, H, W, max_trial, "o2arc", ops)
        be.set_task_table(ins, outs)
        be.set_sampler(pair_off, pair_cnt, 0xABC0 + seed, env_base, aug)
        be.set_truncation(step_limit)
        be.set_dense_output()
        be.reset_sampled()
        pair.append(be)
    return pair[0], pair[1], ops


def compare(roll, twin, ingress, pay, op, flags, rows=None, tag=""):
    """roll.rollout_ex(T steps) vs T twin.step calls: per step reward / terminated / truncated / dense pair / rows / packed rows, then the
    final planes, record, counters, episode, cur_task and status."""
    T, N = len(op), roll.N
    if flags & FLAT_OBS:
        twin.set_flat_output(filtered=rows == "filtered")
    if flags & PACK_OBS:
        twin.set_packed_output()
    want = []
    for t in range(T):
        r, tm = twin.step(ingress, pay[t], op[t], flags)
        w = {"reward": r, "terminated": tm}
        if flags & TRUNCATE:
            w["trunc"] = np.asarray(twin.trunc).copy()
        if flags & DENSE:
            w["dense"] = np.asarray(twin.dense).copy()
        if flags & FLAT_OBS:
            w["rows"] = twin.fused_flat()
        if flags & PACK_OBS:
            w["packed"] = twin.fused_packed()
        want.append(w)
    reward, term, out = roll.rollout_ex(ingress, pay, op, flags, rows)
    errs = []
    for t, w in enumerate(want):
        got = {"reward": reward[t], "terminated": term[t]}
        if flags & TRUNCATE:
            got["trunc"] = out["trunc"][t]
        if flags & DENSE:
            got["dense"] = out["dense"][t]
        if flags & FLAT_OBS:
            L = w["rows"].shape[1]
            got["rows"] = out["rows"][t][:, :L]
            if out["rows"][t][:, L:].any():
                errs.append(f"{tag} step {t}: row padding not zero")
        if flags & PACK_OBS:
            got["packed"] = out["packed"][t]
        for k, v in w.items():
            a, b = np.asarray(got[k]).reshape(N, -1), np.asarray(v).reshape(N, -1)
            bad = np.nonzero((a != b).any(1))[0]
            if len(bad):
                errs.append(f"{tag} step {t}: {k} differs for envs {bad.tolist()[:8]}")
        if len(errs) > 10:
            return errs
    for f in [k for k in O.PLANES if k in O.KIND_PLANES["o2arc"]] + list(O.REC):
        if not np.array_equal(roll.get(f), twin.get(f)):
            errs.append(f"{tag} final state: field {f} differs")
    if not np.array_equal(roll.counters(), twin.counters()):
        errs.append(f"{tag} final counters differ")
    if not np.array_equal(np.asarray(roll.episode), np.asarray(twin.episode)):
        errs.append(f"{tag} episode counters differ: {np.asarray(roll.episode).tolist()} vs {np.asarray(twin.episode).tolist()}")
    if not np.array_equal(np.asarray(roll.cur_task), np.asarray(twin.cur_task)):
        errs.append(f"{tag} cur_task differs")
    s1, s2 = roll.status(), twin.status()
    if s1 != s2:
        errs.append(f"{tag} status {s1} vs single steps {s2}")
    return errs


# the flag sets of the issue: (flags, rows, ingress forms)
CASES = [
    ("trunc_autoreset", TRUNCATE | AUTORESET, None),
    ("resample_trunc", RESAMPLE | TRUNCATE, None),
    ("dense", DENSE, None),
    ("research_filtered", RESEARCH, "filtered"),
    ("research_full", RESEARCH, "full"),
    ("packed_resample", PACK_OBS | RESAMPLE, None),
]


def case_compare(roll_cls, step_cls, H, W, N, T, seed, flags, rows, ingress, step_limit=4, max_trial=2):
    roll, twin, ops = make_pair(roll_cls, step_cls, H, W, N, seed, flags, step_limit, max_trial)
    rng = np.random.default_rng(seed + 1)
    pay, op = _actions(rng, ops, ingress, N, H, W, T)
    errs = compare(roll, twin, ingress, pay, op, flags, rows, tag=f"{H}x{W} {ingress} flags {flags}")
    ep = np.asarray(roll.episode)
    if flags & RESAMPLE and not errs and ep.max() < 3:
        errs.append(f"{H}x{W} {ingress}: no env started two episodes inside the rollout (episodes {ep.tolist()})")
    return errs


def mask_rules_compare(roll_cls, step_cls, H, W, N, T, seed):
    """Mask ingress with CONTINUE_RULE | RESET_ON_SUBMIT | DENSE: about 40 % of the envs resend the twin's current `selected` plane with
    an object op (the continuation branch); the actions are chosen step by step from the twin's state, then replayed as one rollout."""
    roll, twin, ops = make_pair(roll_cls, step_cls, H, W, N, seed, 0)
    flags = CONTINUE | ROS | DENSE
    rng = np.random.default_rng(seed + 2)
    pays, opl, want = [], [], []
    twin.set_dense_output()
    for t in range(T):
        pay, op = _actions(rng, ops, "mask", N, H, W, 1, submit=0.15)
        pay, op = pay[0], op[0]
        sel = twin.get("selected")
        live = sel.reshape(N, -1).any(1)
        hit = (rng.random(N) < 0.4) & live
        pay[hit] = sel[hit]
        lift = ((rng.random(N) < 0.4) & ~live) | hit
        op[lift] = rng.integers(B.MOVE_ROTATE_FLIP.start, B.MOVE_ROTATE_FLIP.stop, int(lift.sum()))
        r, tm = twin.step("mask", pay, op, flags)
        pays.append(pay)
        opl.append(op)
        want.append((r, tm, np.asarray(twin.dense).copy()))
    reward, term, out = roll.rollout_ex("mask", np.stack(pays), np.stack(opl), flags)
    errs = []
    for t, (r, tm, d) in enumerate(want):
        for k, a, b in (("reward", reward[t], r), ("terminated", term[t], tm), ("dense", out["dense"][t], d)):
            if not np.array_equal(a, b):
                errs.append(f"mask rules step {t}: {k} differs")
    for f in [k for k in O.PLANES if k in O.KIND_PLANES["o2arc"]] + list(O.REC):
        if not np.array_equal(roll.get(f), twin.get(f)):
            errs.append(f"mask rules final state: field {f} differs")
    if not np.array_equal(roll.counters(), twin.counters()):
        errs.append("mask rules: final counters differ")
    return errs


def golden_dense_rollout(roll_cls):
    """research.npz's dense vectors (captured from the reference, tests/features.py dense) replayed as ONE mask rollout: the host-formed
    reward sparse*100 - 1 + correct/total of every step equals the fixture's dense_reward."""
    g, errs = F.golden(), []
    S, N, H, W = g["dense_mask"].shape
    be = roll_cls(N, H, W, -1, "o2arc", F.crop_table())
    be.set_tasks(g["aug_out_in"], g["aug_out_in_dim"], g["aug_out_ans"], g["aug_out_ans_dim"])
    be.reset()
    be.set_dense_output()
    reward, term, out = be.rollout_ex("mask", g["dense_mask"], g["dense_op"], DENSE)
    d = out["dense"].astype(np.float64)
    got = reward.astype(np.float64) * 100 - 1 + d[..., 0] / d[..., 1]
    for s in range(S):
        if not np.array_equal(got[s], g["dense_reward"][s]):
            bad = np.nonzero(got[s] != g["dense_reward"][s])[0]
            errs.append(f"dense rollout step {s}: envs {bad.tolist()} got {got[s][bad].tolist()} want {g['dense_reward'][s][bad].tolist()}")
        if not np.array_equal(term[s], g["dense_term"][s]):
            errs.append(f"dense rollout step {s}: terminated differs")
    if not np.array_equal(be.get("grid"), g["dense_final_grid"]) or not np.array_equal(be.get("grid_dim"), g["dense_final_grid_dim"]):
        errs.append("dense rollout: final grid differs")
    return errs
