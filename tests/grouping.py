"""The launch that orders itself (ARCLE_STEPX_GROUPED; arcle_amd/csrc/arcle_group.h) on the CPU: tests/emu/group_emu.cpp runs the deal —
slot geometry, the trade inside a group of 32 envs, the extraction of the slot's inputs — and whole step launches whose slots run in an
order the TEST chooses, each wave to completion before the next starts, on the launch's shared in-place buffers.  Used by
tests/test_group_emu.py and the sanitized build of tests/test_emu_sanitized.py.  Compare functions return lists of mismatch strings."""
import ctypes
import os
import subprocess

import numpy as np

import backends as B
import features as F
from oracle import oracle as O

GROUP = 32  # ARCLE_GROUP_SIZE
INC = 512   # ARCLE_STEP_ROWS_INCREMENTAL
# the rows of the LEAN table (arcle_hip.hip) that have a self-ordering twin: name -> (row of group_emu.cpp, step flags, ingress forms)
HOT = F.STEP_AUTORESET | F.STEP_ELIDE
RESEARCH_INC = F.STEP_ELIDE | F.STEP_TRUNCATE | F.STEP_RESAMPLE | F.STEP_DENSE | F.STEP_FLAT_OBS | INC
LEAN_GROUPED = {
    "hot": (0, HOT, ("mask", "bbox", "point", "bbox5", "bits")),
    "noreset": (1, F.STEP_ELIDE, ("bbox", "bbox5", "point")),
    "hot_pack": (2, HOT | F.STEP_PACK_OBS, ("bbox", "bbox5")),
    "research_inc": (3, RESEARCH_INC, ("bbox", "bbox5")),
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        d = os.path.join(B.ROOT, "tests", "emu")
        so, src = os.path.join(d, "libgroup_emu.so"), os.path.join(d, "group_emu.cpp")
        hdrs = [os.path.join(B.ROOT, "arcle_amd", "csrc", h) for h in ("arcle_wave.h", "arcle_group.h")]
        if os.environ.get("ARCLE_GROUP_EMU_LIB"):  # (tests/test_emu_sanitized.py: the ASan + UBSan build)
            so = os.environ["ARCLE_GROUP_EMU_LIB"]
        elif not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, src])
        L = ctypes.CDLL(so)
        vp, i32, u32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint32
        L.group_emu_slots.argtypes = [i32, i32, u32, vp, vp]
        L.group_emu_trade.argtypes = [i32, vp, ctypes.c_uint64, vp]
        L.group_emu_launch.argtypes = [ctypes.POINTER(B._StepParams), i32, i32, vp, i32, vp, vp]
        assert L.group_emu_params_size() == ctypes.sizeof(B._StepParams), "StepParams layout drifted"
        _lib = L
    return _lib


# ---- what the launcher computes (arcle_hip.hip: launch_step, grouped_applies, arcle_set_op_table) -------------------------------------
def group_magic(n_envs):
    """p.group_magic of launch_step: floor(2^32 / G) + 1, G = n_envs / (8 * 32) groups per XCD."""
    return (0x100000000 // (n_envs // (8 * GROUP)) + 1) & 0xFFFFFFFF


def grouped_applies(n_envs):
    """the batch-size part of grouped_applies: whole groups on every XCD, at least two of them"""
    return n_envs % (8 * GROUP) == 0 and n_envs >= 16 * GROUP


def long_mask(ops):
    """bit i: op table slot i is Move / Rotate / Flip (arcle_set_op_table)"""
    return sum(1 << i for i, d in enumerate(list(ops)[:63]) if (int(d) & 0xFF) in (O.OP_MOVE, O.OP_ROTATE, O.OP_FLIP))


# ---- deal only ------------------------------------------------------------------------------------------------------------------------
def slots(n_envs, wpw, magic=None):
    """(j, gfirst) uint32 [n_envs] of every slot s = block * wpw + wave of the launch (arcle::group_slot)"""
    j, g = np.zeros(n_envs, np.uint32), np.zeros(n_envs, np.uint32)
    rc = lib().group_emu_slots(n_envs, wpw, group_magic(n_envs) if magic is None else magic, j.ctypes.data, g.ctypes.data)
    assert rc == 0, rc
    return j, g


def geometry_errors(n_envs, wpw):
    """Over all (block, wave): gfirst + position covers each env exactly once, groups are 32-aligned inside their XCD's range, and the
    reciprocal divides every s_local exactly."""
    j, g = slots(n_envs, wpw)
    j, g = j.astype(np.int64), g.astype(np.int64)
    s = np.arange(n_envs)
    block, wave = s // wpw, s % wpw
    s_local = (block >> 3) * wpw + wave
    G, rs = n_envs // (8 * GROUP), n_envs // 8
    errs = []
    if not np.array_equal(j, s_local // G):
        errs.append(f"n {n_envs} wpw {wpw}: umulhi(s_local, magic) != s_local // G for {int((j != s_local // G).sum())} slots")
    if not np.array_equal(g, (block & 7) * rs + GROUP * (s_local % G)):
        errs.append(f"n {n_envs} wpw {wpw}: first env of the group")
    if j.max(initial=0) >= GROUP or g.min(initial=0) < 0 or (g + j).max(initial=0) >= n_envs:
        errs.append(f"n {n_envs} wpw {wpw}: slot outside the batch")
    elif not (np.bincount(g + j, minlength=n_envs) == 1).all():
        errs.append(f"n {n_envs} wpw {wpw}: gfirst + position does not cover each env exactly once")
    return errs


def trade(ops32, mask):
    """ops int32 [n_groups, 32] -> pos int32 [n_groups, 32]: pos[g, j] = the position whose env position j steps (arcle::group_position)"""
    ops32 = np.ascontiguousarray(ops32, np.int32)
    pos = np.full(ops32.shape, -1, np.int32)
    rc = lib().group_emu_trade(len(ops32), ops32.ctypes.data, mask, pos.ctypes.data)
    assert rc == 0, f"group emulator reported error {rc}"
    return pos


def trade_errors(ops32, mask, tag=""):
    """The rule of arcle_group.h: the 32 positions pick a permutation; the long envs (all of them, they are L) occupy exactly the
    positions < L; a position that is neither a late long one nor an early other one keeps its own env; the k-th late long position trades
    with the k-th early other position."""
    ops32 = np.asarray(ops32, np.int64)
    pos = trade(ops32, mask).astype(np.int64)
    n = len(ops32)
    idx = np.minimum(np.where(ops32 < 0, 63, ops32), 63).astype(np.uint64)  # (unsigned min, as the kernel: a negative index reads bit 63)
    is_long = ((np.uint64(mask) >> idx) & np.uint64(1)).astype(bool)
    L = is_long.sum(1)
    errs = []
    if not (np.sort(pos, 1) == np.arange(GROUP)).all():
        bad = np.nonzero((np.sort(pos, 1) != np.arange(GROUP)).any(1))[0]
        return [f"{tag}: not a permutation in groups {bad.tolist()[:5]} (ops {ops32[bad[0]].tolist()} -> {pos[bad[0]].tolist()})"]
    early = np.arange(GROUP)[None, :] < L[:, None]
    stepped_long = np.take_along_axis(is_long, pos, 1)
    if not (stepped_long == early).all():
        errs.append(f"{tag}: the long envs are not exactly in the positions < L in {int((stepped_long != early).any(1).sum())} groups")
    stays = is_long == early  # an early long one or a late other one
    if not (pos[stays] == np.broadcast_to(np.arange(GROUP), (n, GROUP))[stays]).all():
        errs.append(f"{tag}: a position that trades nothing lost its env")
    for g in np.nonzero(~stays.all(1))[0][:64]:  # (k-th with k-th: checked on a sample of the groups that trade)
        a, b = np.nonzero(is_long[g] & ~early[g])[0], np.nonzero(~is_long[g] & early[g])[0]
        if not (np.array_equal(pos[g, a], b) and np.array_equal(pos[g, b], a)):
            errs.append(f"{tag}: group {g}: late long {a.tolist()} / early other {b.tolist()} trade as {pos[g, a].tolist()} / {pos[g, b].tolist()}")
    return errs


# ---- whole launches -------------------------------------------------------------------------------------------------------------------
class GroupEmuBackend(B.EmuBackend):
    """EmuBackend whose step() is one emulated LAUNCH of a lean 30 x 30 instantiation: `order` None = the plain twin (slot i steps env i),
    otherwise the self-ordering launch with its slots run in that order.  Resets and the row writer stay the wave emulator's."""
    name = "group_emu"
    PLANE_STRIDE = 1024
    row_name, order, wpw = "hot", None, 4

    def launch_params(self, ingress, payload, op):
        p = self._params()
        self._extras(p)
        if ingress == "mask":
            pay = np.ascontiguousarray(np.asarray(payload).astype(np.int8)).reshape(self.N, self.P)
        elif ingress == "bits":
            pay = np.ascontiguousarray(payload, np.uint8).reshape(self.N, B.BITS_STRIDE)
        else:
            pay = np.ascontiguousarray(payload, np.int32)
        opa = np.ascontiguousarray(op if op is not None else np.zeros(self.N), np.int32)
        p.sel, p.op, p.ingress = pay.ctypes.data, opa.ctypes.data, self.INGRESS[ingress]
        if ingress == "bbox5":
            p.op = None
        p.wpw, p.long_mask, p.group_magic = self.wpw, long_mask(self.ops), group_magic(self.N)
        return p, (pay, opa)

    def step(self, ingress, payload, op, flags=0):
        row, row_flags, forms = LEAN_GROUPED[self.row_name]
        assert flags == row_flags and ingress in forms, (self.row_name, flags, ingress)
        p, keep = self.launch_params(ingress, payload, op)
        if getattr(self, "dense_cache", None) is not None and not flags & F.STEP_DENSE:
            self.dense_cache[:] = 0  # (the launcher's rule, as EmuBackend.step)
        order = np.arange(self.N, dtype=np.int32) if self.order is None else np.ascontiguousarray(self.order, np.int32)
        self.env_of_slot = np.full(self.N, -1, np.int32)
        rc = lib().group_emu_launch(ctypes.byref(p), row, 2 if self.order is None else 1, order.ctypes.data, len(order), self.env_of_slot.ctypes.data, None)
        assert rc == 0, f"group emulator reported error {rc} (divergent cross-lane op / non-uniform value)"
        del keep
        return self.reward.copy(), self.term.copy()

    def deal(self, ingress, payload, op):
        """(env of every slot int32 [N], extracted inputs int32 [N, 11] = rec[4], cnt[2], op, payload[4]) — nothing is stepped"""
        p, keep = self.launch_params(ingress, payload, op)
        order = np.arange(self.N, dtype=np.int32)
        env, inputs = np.full(self.N, -1, np.int32), np.zeros((self.N, 11), np.int32)
        rc = lib().group_emu_launch(ctypes.byref(p), LEAN_GROUPED[self.row_name][0], 0, order.ctypes.data, self.N, env.ctypes.data, inputs.ctypes.data)
        assert rc == 0, f"group emulator reported error {rc}"
        del keep
        return env, inputs


def extraction_errors(n, ingress, row_name, wpw, seed):
    """in.rec, in.cnt, in.op and in.payload of every slot equal the items of the env it picked; every item of the batch is distinct."""
    rng = np.random.default_rng(seed)
    be = GroupEmuBackend(n, 30, 30, 3, "o2arc", O.o2arc_ops())
    be.row_name, be.wpw = row_name, wpw
    words = rng.permutation(1 << 20).astype(np.int32)  # distinct dwords for every array
    be.rec[:] = words[:4 * n].reshape(n, 4).view(np.int8)
    be.cnt[:] = words[4 * n:6 * n].reshape(n, 2)
    op = rng.permutation(n).astype(np.int32) - 3  # distinct op indices: object ops, others, beyond the table, beyond 63, negative
    width = {"bbox": 4, "point": 2, "bbox5": 5}[ingress]
    pay = words[6 * n:(6 + width) * n].reshape(n, width).copy()
    if ingress == "bbox5":
        pay[:, 4] = op
    env, got = be.deal(ingress, pay, None if ingress == "bbox5" else op)
    errs = []
    if not np.array_equal(np.sort(env), np.arange(n)):
        return [f"{ingress} {row_name} wpw {wpw}: the slots do not pick each env once"]
    if np.array_equal(env, np.arange(n)):
        errs.append(f"{ingress} {row_name}: no slot traded (the case does not exercise the extraction)")
    want_pay = np.zeros((n, 4), np.int32)
    want_pay[:, :min(width, 4)] = pay[:, :min(width, 4)]
    for name, a, b in (("rec", got[:, 0:4], be.rec.view(np.int32)[env]), ("cnt", got[:, 4:6], be.cnt[env]), ("op", got[:, 6], op[env]),
                       ("payload", got[:, 7:11], want_pay[env])):
        if not np.array_equal(a, b):
            bad = np.nonzero((a != b).reshape(n, -1).any(1))[0]
            errs.append(f"{ingress} {row_name} wpw {wpw}: in.{name} is not env my_env's for slots {bad.tolist()[:8]}")
    return errs


def orders(n, seed):
    """the extremes of what the hardware may do with a group's slots, and one in between"""
    return {"ascending": np.arange(n, dtype=np.int32), "descending": np.arange(n, dtype=np.int32)[::-1].copy(),
            "shuffled": np.random.default_rng(seed).permutation(n).astype(np.int32)}


def _tasks(rng, N, H, W):
    inp, ans = np.zeros((N, H, W), np.int8), np.zeros((N, H, W), np.int8)
    idim, adim = np.zeros((N, 2), np.int8), np.zeros((N, 2), np.int8)
    for n in range(N):
        ih, iw = rng.integers(1, H + 1), rng.integers(1, W + 1)
        inp[n, :ih, :iw] = rng.integers(0, 10, (ih, iw)) * (rng.random((ih, iw)) < 0.7)
        idim[n] = (ih, iw)
        same = rng.random() < 0.5
        ah, aw = (ih, iw) if same else (rng.integers(1, H + 1), rng.integers(1, W + 1))
        ans[n, :ah, :aw] = inp[n, :ah, :aw] if same else rng.integers(0, 10, (ah, aw))
        adim[n] = (ah, aw)
    return inp, idim, ans, adim


def _actions(rng, ops, ingress, N, research):
    """One step's actions: a third object operations (every group trades), Submits, and — research=False; launch_errors passes that for
    the research step too when it compares with the episode model — op indices beyond the table: the 35-74 range of the adversarial GPU
    streams, 64 and more included."""
    n_ops = len(ops)
    op = rng.integers(0, n_ops, N).astype(np.int32)
    lng = rng.random(N) < 0.33
    op[lng] = rng.integers(B.MOVE_ROTATE_FLIP.start, B.MOVE_ROTATE_FLIP.stop, int(lng.sum()))
    op[rng.random(N) < 0.1] = n_ops - 1
    if not research:
        bad = rng.random(N) < 0.04
        op[bad] = rng.integers(n_ops, 75, int(bad.sum()))
    form = "mask" if ingress in ("mask", "bits") else "bbox" if ingress == "bbox5" else ingress
    pay = B.random_payload(rng, form, N, 30, 30)
    if ingress == "bbox5":
        return np.concatenate([pay, op[:, None]], 1).astype(np.int32), None, pay, op
    if ingress == "bits":
        return B.pack_bits(pay), op, pay, op
    return pay, op, pay, op


def _snapshot(be):
    """every byte a launch may write"""
    s = {"reward": be.reward, "terminated": be.term, "rec": be.rec, "cnt": be.cnt, "status": be.stat}
    s.update({"plane " + k: v for k, v in be.buf.items()})
    for k in ("trunc", "dense", "dense_cache", "episode", "cur_task", "_pack"):
        if getattr(be, k, None) is not None:
            s[k] = getattr(be, k)
    if getattr(be, "_flat", None) is not None:
        s["rows"] = be._flat[0]
    return {k: np.array(v, copy=True) for k, v in s.items()}


def launch_errors(row_name, ingress, n=512, steps=6, seed=0, wpw=4, step_limit=4, oracle=False):
    """`steps` launches of the row's flag set: the plain twin (the same emulator stepping env i in slot i) against the self-ordering launch
    with its slots run ascending, descending and shuffled.  Compared bit-exact after every launch: reward, terminated, truncated, dense
    pairs, the rows, every byte of planes, records and counters, the sampler's side state, the status word.  oracle: the plain twin also
    against OracleBackend — the research step against the episode model of tests/research_model.py (every output, field and the row),
    and then with op indices beyond the table in its stream.  The research step: step_limit 4 and counters drawn from 0..3; every group must hold an env at limit - 2 or
    limit - 1 before every step (a condition on the inputs, read from the reference run — returned as an error if the draw misses it)."""
    row, flags, forms = LEAN_GROUPED[row_name]
    assert ingress in forms and grouped_applies(n)
    research = row_name == "research_inc"
    ops = O.o2arc_ops()
    rng = np.random.default_rng(seed)
    runs = {"plain": None}
    runs.update(orders(n, seed + 1))
    bes = {}
    tasks = _tasks(rng, n, 30, 30)
    ins = [rng.integers(0, 10, (rng.integers(1, 31), rng.integers(1, 31))).astype(np.int8) for _ in range(9)]
    outs = [rng.integers(0, 10, (rng.integers(1, 31), rng.integers(1, 31))).astype(np.int8) for _ in range(9)]
    cnt0 = rng.integers(0, step_limit, n).astype(np.int32)
    for name, order in runs.items():
        be = GroupEmuBackend(n, 30, 30, 2, "o2arc", ops)
        be.row_name, be.order, be.wpw = row_name, order, wpw
        if research:
            be.set_task_table(ins, outs)
            be.set_sampler(np.array([0, 2, 3, 7], np.int32), np.array([2, 1, 4, 2], np.int32), 0xABC0 + seed, 0, F.AUG_PERMUTE | F.AUG_ROT90)
            be.set_truncation(step_limit)
            be.set_dense_output()
            be.reset_sampled()
            be.cnt[:, 0] = cnt0  # desynchronised episodes
            be.set_flat_output(filtered=True)
            be._flat[0][:, :be._flat[1]] = be.flat_obs(True)  # (incremental rows: the buffer holds every env's row of the previous step)
            be._flat[0][:, be._flat[1]:] = 0
        else:
            be.set_tasks(*tasks)
            be.reset()
            if flags & F.STEP_PACK_OBS:
                be.set_packed_output()
        bes[name] = be
    orc = model = None
    if oracle and research:
        import research_model as M
        model = M.ResearchModel(n, 30, 30, 2, ops, ins, outs, np.array([0, 2, 3, 7], np.int32), np.array([2, 1, 4, 2], np.int32), 0xABC0 + seed, 0,
                                F.AUG_PERMUTE | F.AUG_ROT90, step_limit, flags)
        model.orc.env.cnt[:, 0] = cnt0
    elif oracle:
        orc = B.OracleBackend(n, 30, 30, 2, "o2arc", ops)
        orc.set_tasks(*tasks)
        orc.reset()
    errs = []
    for s in range(steps):
        if research:
            c = bes["plain"].cnt[:, 0].reshape(-1, GROUP)
            near = ((c == step_limit - 2) | (c == step_limit - 1)).any(1)
            if not near.all():
                errs.append(f"step {s}: groups {np.nonzero(~near)[0].tolist()} hold no env at limit - 2 or limit - 1: pick another seed")
        pay, op, opay, oop = _actions(rng, ops, ingress, n, research and model is None)
        snaps = {}
        for name, be in bes.items():
            be.step(ingress, pay, op, flags)
            snaps[name] = _snapshot(be)
            if name != "plain" and not np.array_equal(np.sort(be.env_of_slot), np.arange(n)):
                cnt = np.bincount(be.env_of_slot, minlength=n)
                errs.append(f"{row_name} {ingress} step {s} {name}: envs {np.nonzero(cnt == 0)[0].tolist()[:6]} not stepped, {np.nonzero(cnt > 1)[0].tolist()[:6]} stepped twice")
        for name in runs:
            if name == "plain":
                continue
            for k, v in snaps["plain"].items():
                if not np.array_equal(v, snaps[name][k]):
                    bad = np.nonzero((v != snaps[name][k]).reshape(len(v), -1).any(1))[0].tolist() if len(v) == n else []
                    errs.append(f"{row_name} {ingress} step {s} {name}: {k} differs from the plain launch (envs {bad[:8]})")
        if model is not None:
            want, be, tag = model.step("bbox", opay, oop), bes["plain"], f"{row_name} {ingress} step {s} against the model"
            for name, got, exp in (("reward", be.reward, want["reward"]), ("terminated", be.term, want["terminated"]), ("truncated", be.trunc, want["truncated"]),
                                   ("dense pair", be.dense, want["dense"]), ("filtered row", be.fused_flat(), model.rows(True))):
                M._diff(errs, tag, name, got, exp, want["what"], oop)
            M._state_diff(errs, tag, [(be, None)], model, want["what"], oop)
            if want["status"] != int(snaps["plain"]["status"][0]):
                errs.append(f"{tag}: status {int(snaps['plain']['status'][0])}, the oracle's {want['status']}")
        if orc is not None:
            r, t = orc.step("mask" if ingress in ("mask", "bits") else "bbox" if ingress == "bbox5" else ingress, opay, oop, flags)
            be = bes["plain"]
            if not (np.array_equal(r, be.reward) and np.array_equal(t, be.term) and np.array_equal(orc.counters(), be.counters())):
                errs.append(f"{row_name} {ingress} step {s}: reward / terminated / counters differ from the oracle")
            for f in [f for f in B.PLANES[:-1] if f in O.KIND_PLANES["o2arc"]] + [f for f in B.REC if f != "answer_dim"]:
                if not np.array_equal(be.get(f), orc.get(f)):
                    errs.append(f"{row_name} {ingress} step {s}: field {f} differs from the oracle")
            if orc.status() != int(snaps["plain"]["status"][0]):
                errs.append(f"{row_name} {ingress} step {s}: status differs from the oracle")
        for be in bes.values():
            be.status()
        if len(errs) > 12:
            break
    if research and not errs and np.asarray(bes["plain"].episode).max() < 2:
        errs.append("no env was re-initialised inside the run")
    return errs
