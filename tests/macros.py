"""Backend-independent checks of macro expansion (arcle_expand_macros: K candidate step SEQUENCES per state row, one set of verdicts
per sequence) and of the macro side of arcle_amd.search (run_macros, object_macros, beam_search with a "length" key).  The pattern
of tests/search.py and tests/search_bits.py, which this module builds on: every check takes a backend class — EmuMacroBackend
(tests/emu/macro_emu.cpp: wave_expand_macros_row lock-step on the CPU) or HipMacroBackend (the product) — and returns a list of
mismatch strings.  The reference is the existing oracle CHAINED: SR.oracle_from_rows of the replicated parents, then one oracle step
over the children that still have a step at position t, for t = 0 .. T-1 (oracle_macros), and hash_rows_numpy of the final rows."""
import ctypes
import os
import subprocess

import numpy as np

import backends as B
import rows as R
import search as SR
import search_bits as SB
from arcle_amd import search as S
from oracle import oracle as O

EMU_SRC = os.path.join(SR.EMU_DIR, "macro_emu.cpp")
STRIDE = B.BITS_STRIDE
K_MACROS, T_MACROS = 24, 3
STEP_ROS = R.STEP_ROS


class _MacroParams(ctypes.Structure):  # mirror of arcle::MacroParams (arcle_amd/csrc/arcle_search.h)
    _fields_ = [("x", SR._ExpandParams), ("max_len", ctypes.c_int32), ("len", ctypes.c_void_p)]


_emu = None


def macro_emu_lib():
    global _emu
    if _emu is None:
        so = os.path.join(SR.EMU_DIR, "libmacro_emu.so")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [EMU_SRC, SR.EMU_SRC] + SR.EMU_HDRS):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, EMU_SRC])
        _emu = ctypes.CDLL(so)
        _emu.macro_emu_run.argtypes = [ctypes.POINTER(_MacroParams)]
        assert _emu.macro_emu_params_size() == ctypes.sizeof(_MacroParams), "MacroParams layout drifted"
    return _emu


def _outputs(M, K, dense):
    return {"reward": np.full((M, K), -7, np.int32), "term": np.full((M, K), 7, np.uint8), "status": np.full((M, K), 0x55, np.uint8),
            "hash": np.zeros((M, K, 2), np.uint64), "dense": np.full((M, K, 2), -7, np.int32) if dense else None,
            "parent_hash": np.zeros((M, 2), np.uint64)}


class EmuMacroBackend(SB.EmuBitsBackend):
    """EmuBitsBackend (expand_rows / transition_rows in every form, the hash) + the emulated macro expansion."""

    def expand_macros(self, rows, ingress, payload, op, length=None, src_env=None, dense=True, flags=0, chunk=None):
        rows = np.ascontiguousarray(rows, np.int8)
        opa = np.ascontiguousarray(op, np.int32)
        pay = np.ascontiguousarray(payload, np.uint8 if ingress == "bits" else np.int32)
        M, K, T = rows.shape[0], opa.shape[-2], opa.shape[-1]
        assert pay.shape == opa.shape + ({"bbox": 4, "point": 2, "bits": STRIDE}[ingress],)
        y = _MacroParams()
        y.x = self._xparams(rows)
        x = y.x
        out = _outputs(M, K, dense)
        src = None if src_env is None else np.ascontiguousarray(src_env, np.int32)
        ln = None if length is None else np.ascontiguousarray(length, np.int32)
        assert ln is None or ln.shape == opa.shape[:-1]
        x.p.sel, x.p.op, x.p.ingress = pay.ctypes.data, opa.ctypes.data, self.INGRESS[ingress]
        x.p.flags = flags | (SR.STEP_DENSE if dense else 0)
        x.p.reward, x.p.term = out["reward"].ctypes.data, out["term"].ctypes.data
        x.p.dense = out["dense"].ctypes.data if dense else None
        x.p.task_idx = None if src is None else src.ctypes.data
        x.n_actions, x.action_row_stride = K, (K if opa.ndim == 3 else 0)
        x.chunk = chunk or self.CHUNK
        x.n_chunks = (K + x.chunk - 1) // x.chunk
        x.status_out, x.hash, x.parent_hash = out["status"].ctypes.data, out["hash"].ctypes.data, out["parent_hash"].ctypes.data
        y.max_len, y.len = T, (None if ln is None else ln.ctypes.data)
        rc = macro_emu_lib().macro_emu_run(ctypes.byref(y))
        assert rc == 0, f"macro emulator reported error {rc} (divergent cross-lane op / non-uniform value)"
        return out


class HipMacroBackend(SB.HipBitsBackend):
    """HipBitsBackend + EnvBatch.expand_macros.  chunk: the library's tuning variable ARCLE_EXPAND_CHUNK, read at every call."""

    def expand_macros(self, rows, ingress, payload, op, length=None, src_env=None, dense=True, flags=0, chunk=None):
        t, dev = self.torch, self.b.device
        pay = np.ascontiguousarray(payload, np.uint8 if ingress == "bits" else np.int32)
        dv = lambda a: None if a is None else t.as_tensor(np.ascontiguousarray(a, np.int32), device=dev)  # noqa: E731
        old = os.environ.get("ARCLE_EXPAND_CHUNK")
        if chunk is not None:
            os.environ["ARCLE_EXPAND_CHUNK"] = str(chunk)
        try:
            ex = self.b.expand_macros(t.as_tensor(np.ascontiguousarray(rows, np.int8), device=dev), ingress, t.as_tensor(pay, device=dev),
                                      dv(op), dv(length), dv(src_env), dense=dense, flags=flags)
        finally:
            if chunk is not None:
                os.environ.pop("ARCLE_EXPAND_CHUNK")
                if old is not None:
                    os.environ["ARCLE_EXPAND_CHUNK"] = old
        return {"reward": ex.reward.cpu().numpy(), "term": ex.term.cpu().numpy(), "status": ex.status.cpu().numpy(),
                "hash": ex.hash.cpu().numpy().view(np.uint64), "dense": None if ex.dense is None else ex.dense.cpu().numpy(),
                "parent_hash": ex.parent_hash.cpu().numpy().view(np.uint64)}


# ---- the oracle's side: the existing oracle, chained ---------------------------------------------------------------------------------
def oracle_step_rows(rows, answers, adims, kind, H, W, mt, ops, form, pay, op):
    """ONE oracle step of n (row, action) pairs -> (rows after, reward, terminated, status uint8 [n], dense pairs [n, 2]).  The
    oracle's status word is per batch: a batch that raised something is stepped again pair by pair (as SR.oracle_expand does)."""
    n = len(rows)
    orc = SR.oracle_from_rows(rows, answers, adims, kind, H, W, mt, ops)
    r, t = orc.step(form, pay, op)
    status = np.zeros(n, np.uint8)
    if orc.status():
        for c in range(n):
            one = SR.oracle_from_rows(rows[c:c + 1], answers[c:c + 1], adims[c:c + 1], kind, H, W, mt, ops)
            one.step(form, pay[c:c + 1], op[c:c + 1])
            status[c] = one.status()
    dense = SR.dense_pairs(orc.get("grid"), orc.get("grid_dim"), answers, adims)
    dense[(status & (SR.ST_BAD_OP | SR.ST_ROTATE_DOMAIN)) != 0] = 0
    return B.state_rows(orc), r, t, status, dense


def oracle_macros(rows, answers, adims, kind, H, W, mt, ops, form, pay, op, length):
    """Every (row m, macro (m, k)) on the chained oracle.  rows [M, L]; answers / adims of the env each row is judged against; pay
    [M, K, T, ..], op [M, K, T], length [M, K].  -> dict of [M, K] reward (summed) / term (the last step's) / status (OR), [M, K, L]
    final rows, [M, K, L] rows after step 0, [M, K, 2] dense pairs of the last step.  A length outside [1, T]: ST_BAD_OP, no step.
    A step with operation < 0 (the padding of arcle_amd.search's candidate sets) is answered as the device answers it — ST_BAD_OP,
    the step did not happen — without asking the oracle, whose table lookup a negative index would wrap."""
    M, K, T = op.shape
    C = M * K
    rep = np.repeat(np.arange(M), K)
    cur = rows[rep].copy()
    pay, op, length = pay.reshape(C, T, -1), op.reshape(C, T), length.reshape(C)
    reward, term, status, dense = np.zeros(C, np.int32), np.zeros(C, np.uint8), np.zeros(C, np.uint8), np.zeros((C, 2), np.int32)
    valid = (length >= 1) & (length <= T)
    status[~valid] = SR.ST_BAD_OP
    first = cur.copy()
    for t in range(T):
        live = valid & (length > t)
        pad = live & (op[:, t] < 0)
        status[pad] |= SR.ST_BAD_OP
        dense[pad] = 0
        idx = np.nonzero(live & ~pad)[0]
        if len(idx):
            out, r, tm, st, d = oracle_step_rows(cur[idx], answers[rep[idx]], adims[rep[idx]], kind, H, W, mt, ops, form,
                                                 np.ascontiguousarray(pay[idx, t]), np.ascontiguousarray(op[idx, t]))
            cur[idx], term[idx], dense[idx] = out, tm, d
            reward[idx] += r
            status[idx] |= st
        if t == 0:
            first = cur.copy()
    return {"reward": reward.reshape(M, K), "term": term.reshape(M, K), "status": status.reshape(M, K), "rows": cur.reshape(M, K, -1),
            "first": first.reshape(M, K, -1), "dense": dense.reshape(M, K, 2)}


# ---- check 1: parity -----------------------------------------------------------------------------------------------------------------
def draw_macros(rng, form, rows, lead, kind, H, W, n_ops, T=T_MACROS):
    """Macros of T steps for the leading shape `lead` ((M, K) or (K,)) -> (the oracle's payload [lead, T, ..] and form, the backend's
    payload, op [lead, T], length [lead] uniform in 1 .. T).  bbox / point: SR.draw_actions' op mix; bits: SB.mask_mix' masks (the
    components of the PARENT's grid, single cells, random masks) — the oracle steps the int8 masks, the backend gets the bit rows."""
    n = int(np.prod(lead))
    length = rng.integers(1, T + 1, lead).astype(np.int32)
    if form != "bits":
        pay, op = SR.draw_actions(rng, form, n * T, H, W, n_ops)
        pay = pay.reshape(tuple(lead) + (T, -1))
        return form, pay, pay, op.reshape(tuple(lead) + (T,)).astype(np.int32), length
    grids, gdims = SB._grids_of(rows, kind, H, W)
    if len(lead) == 2:
        masks = SB.mask_mix(rng, grids, gdims, lead[1] * T, H, W)
    else:
        masks = SB.mask_mix(rng, grids[:1], gdims[:1], n * T, H, W)[0]
    op = rng.integers(0, n_ops, tuple(lead) + (T,)).astype(np.int32)
    bits = B.pack_bits(masks.reshape(-1, H, W)).reshape(tuple(lead) + (T, STRIDE))
    return "mask", masks.reshape(tuple(lead) + (T, H * W)), bits, op, length


def compare(errs, tag, got, want, rows, kind, H, W, op_full, bad_len):
    M, K = want["reward"].shape
    hw = S.hash_rows_numpy(want["rows"].reshape(M * K, -1), kind, H, W).reshape(M, K, 2)
    for name, a, b in (("reward", got["reward"], want["reward"]), ("terminated", got["term"], want["term"]),
                       ("status", got["status"], want["status"]), ("dense", got["dense"], want["dense"]), ("hash", got["hash"], hw),
                       ("parent_hash", got["parent_hash"], S.hash_rows_numpy(rows, kind, H, W))):
        if not np.array_equal(a, b):
            bad = np.argwhere(np.asarray(a != b).reshape(a.shape[0], a.shape[1] if name != "parent_hash" else 1, -1).any(2))[:4]
            errs.append(f"{tag}: {name} differs at (m, k) {bad.tolist()} (ops {[op_full[m, k].tolist() for m, k in bad] if name != 'parent_hash' else ''})")
    if not np.array_equal(got["hash"][bad_len], np.broadcast_to(got["parent_hash"][:, None, :], got["hash"].shape)[bad_len]):
        errs.append(f"{tag}: a macro with a length outside 1 .. T does not hash as its parent")
    if not ((got["status"][bad_len] == SR.ST_BAD_OP).all() and not got["reward"][bad_len].any() and not got["term"][bad_len].any() and not got["dense"][bad_len].any()):
        errs.append(f"{tag}: a macro with a length outside 1 .. T: status / reward / terminated / dense are not BAD_OP / 0 / 0 / (0, 0)")


def parity(cls, cases=SR.CASES, forms=("bbox", "point", "bits"), T=T_MACROS):
    """Check 1: every (m, k) of expand_macros equals the chained oracle — reward, terminated, status, dense pair, hash ==
    hash_rows_numpy(the oracle's final row), parent_hash — for the three forms, shared and per-row sets, default and permuted src_env
    with M = N + 3; an out-of-range op in the middle step, a Submit first, an all-Submit macro, lengths 0 and T + 1 in every set; a
    src_env out of range; nothing of the handle moves.  (ARCLE_STEP_RESET_ON_SUBMIT: reset_on_submit below — the oracle has no such flag.)  The vacuity conditions are asserted on the
    oracle's results first."""
    errs = []
    for kind, H, W, mt in cases:
        be, orc, rng, ops = SR.case_pair(cls, kind, H, W, mt)
        N, K, n_ops = 8, K_MACROS, len(ops)
        base = B.state_rows(orc)
        answers, adims = orc.get("answer"), orc.get("answer_dim")
        before = {f: be.get(f) for f in R._state_fields(kind) + ["answer", "answer_dim"]}
        cnt_before, st_before = be.counters(), be.sticky_status()
        for form, per_row, permuted in [(form, per_row, permuted) for form in forms for per_row in (True, False) for permuted in (False, True)]:
            tag = f"{kind} {H}x{W} {form} {'per-row' if per_row else 'shared'} {'src' if permuted else 'default'}"
            M = N + 3 if permuted else N
            src = rng.integers(0, N, M).astype(np.int32) if permuted else np.arange(N, dtype=np.int32)
            rows = base[src]
            oform, opay, pay, op, length = draw_macros(rng, form, rows, (M, K) if per_row else (K,), kind, H, W, n_ops, T)
            sl = (lambda m, k: (m, k)) if per_row else (lambda m, k: (k,))  # noqa: E731  (the planted macros: slot k of row m / of the set)
            op[sl(0, 3) + (1,)], length[sl(0, 3)] = n_ops + 2, T    # an out-of-range op in the middle step: the last step still runs
            op[sl(1, 5) + (0,)], length[sl(1, 5)] = n_ops - 1, T    # a Submit first, then more steps
            op[sl(2, 7)], length[sl(2, 7)] = n_ops - 1, T           # an all-Submit macro
            length[sl(3, 9)], length[sl(3, 11)] = 0, T + 1          # lengths outside 1 .. T
            if per_row:
                opay_full, op_full, len_full = opay, op, length
            else:
                opay_full, op_full, len_full = (np.broadcast_to(a, (M,) + a.shape).copy() for a in (opay, op, length))
            want = oracle_macros(rows, answers[src], adims[src], kind, H, W, mt, ops, oform, opay_full, op_full, len_full)
            if form == "bbox" and per_row and not permuted:  # the vacuity conditions, on the oracle's results alone
                changed = float((want["rows"] != rows[:, None, :]).any(2).mean())
                two = (len_full >= 2) & (len_full <= T)
                moved = float((want["rows"] != want["first"]).any(2)[two].mean())
                print(f"corpus {tag}: {changed:.2f} of the children differ from their parent; {moved:.2f} of the macros of 2+ steps end in another row than their first step's")
                assert changed >= 0.60, f"{tag}: only {changed:.2f} of the children differ from their parent"
                assert moved >= 0.60, f"{tag}: only {moved:.2f} of the macros of 2+ steps go on after their first step"
            got = be.expand_macros(rows, form, pay, op, length, src_env=src if permuted else None, dense=True)
            compare(errs, tag, got, want, rows, kind, H, W, op_full, (len_full < 1) | (len_full > T))
            if len(errs) > 10:
                return errs
        for f, v in before.items():
            if not np.array_equal(be.get(f), v):
                errs.append(f"{kind} {H}x{W}: resident field {f} was touched by expand_macros")
        if not np.array_equal(be.counters(), cnt_before) or be.sticky_status() != st_before:
            errs.append(f"{kind} {H}x{W}: counters / sticky status were touched by expand_macros")
        # a row whose src_env names no env: every child is the parent with ARCLE_ST_BAD_TASK
        _, _, pay, op, length = draw_macros(rng, "bbox", base[:2], (4,), kind, H, W, n_ops, T)
        got = be.expand_macros(base[:2], "bbox", pay, op, length, src_env=np.array([1, N + 5], np.int32))
        if not (got["status"][1] == SR.ST_BAD_TASK).all() or not (got["hash"][1] == got["parent_hash"][1]).all() or (got["status"][0] & SR.ST_BAD_TASK).any() \
                or got["reward"][1].any() or got["term"][1].any() or got["dense"][1].any():
            errs.append(f"{kind} {H}x{W}: src_env out of range: status {got['status'].tolist()}")
        if be.sticky_status() != st_before:
            errs.append(f"{kind} {H}x{W}: sticky status moved")
    return errs


def reset_on_submit(cls, T=T_MACROS):
    """Check 1, ARCLE_STEP_RESET_ON_SUBMIT.  The oracle does not know the flag; its reference is the reference's own traces
    (tests/golden/research.npz, as tests/features.py and SB.flagged_transitions replay them).  The traces are walked forward through
    transition_rows (whose rows those checks pin on the golden fields); from the rows before step s every env gets two macros of
    the trace's own steps — s .. s+2 and s .. s+1, as bit rows — and their summed reward and last terminated must equal the
    GOLDEN per-step values, their hash hash_rows_numpy of the walked rows after those steps."""
    import features as F
    g, errs = F.golden(), []
    S_, N, H, W = g["ros_mask"].shape
    submits = 0
    for mt in sorted(set(g["ros_max_trial"].tolist())):
        sel = np.nonzero(g["ros_max_trial"] == mt)[0]
        pad = np.concatenate([sel, np.repeat(sel[:1], 8)])  # (8 envs behind the ones used: see SB.flagged_transitions)
        be = cls(len(pad), H, W, int(mt), "o2arc", O.o2arc_ops())
        be.set_tasks(g["ros_in"][pad], g["ros_in_dim"][pad], g["ros_ans"][pad], g["ros_ans_dim"][pad])
        be.reset()
        n = len(sel)
        walk = [B.state_rows(be)[:n]]
        L = walk[0].shape[1]
        bits = np.stack([B.pack_bits(g["ros_mask"][s][sel]) for s in range(S_)], 1)  # [n, S, 128]
        ops = np.ascontiguousarray(g["ros_op"][:, sel].T.astype(np.int32))           # [n, S]
        for s in range(S_):
            out, _, _ = be.transition_rows(walk[-1], "bits", np.ascontiguousarray(bits[:, s]), np.ascontiguousarray(ops[:, s]), flags=STEP_ROS)
            be.status()
            walk.append(np.ascontiguousarray(out[:, :L]))
        for s in range(0, S_ - T + 1, 2):
            pay = np.ascontiguousarray(np.broadcast_to(bits[:, None, s:s + T], (n, 2, T, STRIDE)))
            op = np.ascontiguousarray(np.broadcast_to(ops[:, None, s:s + T], (n, 2, T)))
            length = np.tile(np.array([[T, T - 1]], np.int32), (n, 1))
            submits += int((ops[:, s:s + T - 1] == len(O.o2arc_ops()) - 1).sum())
            got = be.expand_macros(walk[s], "bits", pay, op, length, dense=False, flags=STEP_ROS)
            for k, ln in enumerate((T, T - 1)):
                want_r = g["ros_reward"][s:s + ln][:, sel].sum(0)
                want_t = g["ros_term"][s + ln - 1][sel]
                want_h = S.hash_rows_numpy(walk[s + ln], "o2arc", H, W)
                if not (np.array_equal(got["reward"][:, k], want_r) and np.array_equal(got["term"][:, k] != 0, want_t != 0)):
                    errs.append(f"reset_on_submit max_trial {mt} steps {s}..{s + ln - 1}: reward / terminated differ from the reference's trace (ops {ops[:, s:s + ln].tolist()})")
                if not np.array_equal(got["hash"][:, k], want_h):
                    errs.append(f"reset_on_submit max_trial {mt} steps {s}..{s + ln - 1}: hash differs from the walked rows' (ops {ops[:, s:s + ln].tolist()})")
            if got["status"].any():
                errs.append(f"reset_on_submit max_trial {mt} step {s}: status {got['status'].tolist()}")
            if len(errs) > 8:
                return errs
    assert submits >= 5, f"only {submits} Submits before a macro's last step: a step after the re-initialisation is not exercised"
    return errs


# ---- check 2: T = 1 is arcle_expand_rows -----------------------------------------------------------------------------------------------
def single_steps(cls, cases=(SR.CASES[0], SR.CASES[2]), forms=("bbox", "point", "bits")):
    """Check 2: with T = 1 and no lengths, expand_macros' outputs are bit-equal to expand_rows' on the same backend — one case per
    width class (30 x 30: fast; 12 x 12: generic), the three forms, a set per row."""
    errs = []
    for kind, H, W, mt in cases:
        be, orc, rng, ops = SR.case_pair(cls, kind, H, W, mt)
        base = B.state_rows(orc)
        M, K = len(base), K_MACROS
        for form in forms:
            _, _, pay, op, _ = draw_macros(rng, form, base, (M, K), kind, H, W, len(ops), 1)
            op[0, 3, 0] = len(ops) + 2
            a = be.expand_rows(base, form, pay[:, :, 0], op[:, :, 0], dense=True)
            b = be.expand_macros(base, form, pay, op, None, dense=True)
            errs += [f"{kind} {H}x{W} {form}: {name} of expand_macros(T = 1) differs from expand_rows" for name in a if not np.array_equal(a[name], b[name])]
    return errs


# ---- check 3: chunk boundaries -------------------------------------------------------------------------------------------------------
def chunks(cls, kind="o2arc", H=12, W=12, mt=1):
    """Check 3: ONE parent row, K = 24 macros: the launcher's split into one chunk (chunk 24), into several with a short last one
    (chunk 7: 7 + 7 + 7 + 3; chunk 5: four and a short fifth) and into one macro per wave give the outputs of the per-row launch —
    row 0 of the launch over all eight rows."""
    be, orc, rng, ops = SR.case_pair(cls, kind, H, W, mt)
    base = B.state_rows(orc)
    M, K = len(base), K_MACROS
    _, _, pay, op, length = draw_macros(rng, "bbox", base, (M, K), kind, H, W, len(ops))
    length[0, 6], length[0, 7] = 0, T_MACROS + 1  # (a macro that runs nothing at the end of one chunk and at the start of the next)
    ref = be.expand_macros(base, "bbox", pay, op, length, chunk=K)
    errs = []
    for c in (K, 7, 5, 1):
        got = be.expand_macros(base[:1], "bbox", pay[:1], op[:1], length[:1], chunk=c)
        errs += [f"chunk {c}: {k} of the one-row launch differs from the per-row launch" for k, v in got.items() if not np.array_equal(v, ref[k][:1])]
    return errs


# ---- an oracle-backed vec env with macros --------------------------------------------------------------------------------------------
class MacroVenv(SB.MaskVenv):
    """SR.OracleVenv (through SB.MaskVenv: `expand` / `transition` in the bbox and bits forms, `components`) + what beam_search needs
    for macro candidates: `expand_macros` from oracle_macros, and `transition_macros` = the PRODUCT's host logic
    (arcle_amd.search.run_macros, what ARCVecEnv.transition_macros runs) over this stub's oracle-backed `transition`."""

    def expand_macros(self, rows, action, src_env=None):
        import torch
        from arcle_amd.engine import Expansion
        rows_n, op = rows.numpy(), action["operation"].numpy()
        form, pay = self._form(action)
        M, K, T = len(rows_n), op.shape[-2], op.shape[-1]
        length = action["length"].numpy() if action.get("length") is not None else np.full(op.shape[:-1], T, np.int32)
        if op.ndim == 2:
            pay, op, length = (np.broadcast_to(a, (M,) + a.shape) for a in (pay, op, length))
        src = np.arange(M) if src_env is None else src_env.numpy()
        w = oracle_macros(rows_n, self.answers[src], self.adims[src], self.kind, self.H, self.W, self.mt, self.ops, form,
                          np.ascontiguousarray(pay).reshape(M, K, T, -1), np.ascontiguousarray(op), np.ascontiguousarray(length))
        h = S.hash_rows_numpy(w["rows"].reshape(M * K, -1), self.kind, self.H, self.W).view(np.int64).reshape(M, K, 2)
        return Expansion(torch.from_numpy(w["reward"]), torch.from_numpy(w["term"]), torch.from_numpy(w["status"]), torch.from_numpy(h),
                         torch.from_numpy(w["dense"]), self.hash_rows(rows))

    def transition_macros(self, rows, action, src_env=None):
        return S.run_macros(self.transition, rows, action, src_env)


# ---- check 4 (host half): run_macros with mixed lengths equals the chained oracle --------------------------------------------------------
def materialisation_host(cases=SR.CASES[1:3]):
    """One macro per row through MacroVenv.transition_macros (arcle_amd.search.run_macros: launch t over the rows that still have a
    step at t) equals oracle_macros for the same (row, macro) pairs: rows, summed reward, last terminated — lengths 1 .. T mixed, one
    of 0 and one of T + 1 (nothing runs), and without lengths."""
    import torch
    errs = []
    for kind, H, W, mt in cases:
        _, orc, rng, ops = SR.case_pair(B.OracleBackend, kind, H, W, mt)
        base = B.state_rows(orc)
        answers, adims = orc.get("answer"), orc.get("answer_dim")
        venv = MacroVenv(kind, H, W, mt, ops, answers, adims)
        M, T = len(base), T_MACROS
        src = rng.permutation(M).astype(np.int32)
        rows = base[src]
        _, _, pay, op, length = draw_macros(rng, "bbox", rows, (M, 1), kind, H, W, len(ops))
        length[:, 0] = [1, 2, 3, 0, T + 1, 2, 3, 1]
        for with_len in (True, False):
            ln = length if with_len else np.full_like(length, T)
            want = oracle_macros(rows, answers[src], adims[src], kind, H, W, mt, ops, "bbox", pay, op, ln)
            act = {"bbox": torch.from_numpy(pay[:, 0]), "operation": torch.from_numpy(op[:, 0])}
            if with_len:
                act["length"] = torch.from_numpy(ln[:, 0])
            out, r, t = venv.transition_macros(torch.from_numpy(rows), act, torch.from_numpy(src))
            if not np.array_equal(out.numpy(), want["rows"][:, 0]):
                errs.append(f"{kind} {H}x{W} lengths {with_len}: rows differ for rows {np.nonzero((out.numpy() != want['rows'][:, 0]).any(1))[0].tolist()}")
            if not (np.array_equal(r.numpy(), want["reward"][:, 0]) and np.array_equal(t.numpy(), want["term"][:, 0] != 0)):
                errs.append(f"{kind} {H}x{W} lengths {with_len}: reward / terminated differ")
    return errs


# ---- check 5: the stamp tasks ----------------------------------------------------------------------------------------------------------
COPY_O, PASTE = 29, 30  # O2ARCv2Env's table
PLUS = ((0, 1), (1, 0), (1, 1), (1, 2), (2, 1))


def stamp_tasks(n=8, H=10, W=10):
    """n 10 x 10 O2ARC tasks, seeds 0 .. n-1: a marker cell at (1, y) of colour c1, a 5-cell plus of colour c2 != c1 with its box at
    rows 5-7, a second c1 marker at (3, y'); the answer is the ORACLE's grid after CopyO on the plus's box, then Paste on the first
    marker's cell.  -> (inputs [n, H, W], dims [n, 2], answers, the two planted steps per task as (x1, y1, x2, y2, op))."""
    ops = O.o2arc_ops()
    inputs, answers, steps = [], [], []
    dims = np.tile(np.array([[H, W]], np.int8), (n, 1))
    for seed in range(n):
        rng = np.random.default_rng(seed)
        c1, c2 = (int(c) for c in rng.permutation(np.arange(1, 10))[:2])
        y, px, y2 = int(rng.integers(0, W - 2)), int(rng.integers(0, W - 2)), int(rng.integers(0, W))
        g = np.zeros((H, W), np.int8)
        g[1, y] = c1
        g[3, y2] = c1
        for a, b in PLUS:
            g[5 + a, px + b] = c2
        seq = [(5, px, 7, px + 2, COPY_O), (1, y, 1, y, PASTE)]
        orc = B.OracleBackend(1, H, W, 3, "o2arc", ops)
        orc.set_tasks(g[None], dims[:1], g[None], dims[:1])
        orc.reset()
        for s in seq:
            orc.step("bbox", np.array([s[:4]], np.int32), np.array([s[4]], np.int32))
        ans = orc.get("grid")[0]
        assert not orc.status() and int((ans == c2).sum()) == 10, f"stamp task {seed}: the planted steps do not stamp the plus"
        inputs.append(g)
        answers.append(ans)
        steps.append(seq)
    return np.stack(inputs), dims, np.stack(answers), steps


def stamp_rows(inputs, dims, answers):
    """The initial state rows of the stamp tasks, from the oracle."""
    orc = B.OracleBackend(len(inputs), inputs.shape[1], inputs.shape[2], 3, "o2arc", O.o2arc_ops())
    orc.set_tasks(inputs, dims, answers, dims)
    orc.reset()
    return B.state_rows(orc)


def replay_steps_on_oracle(inp, dim, ans, seq):
    """The (x1, y1, x2, y2, op) steps + a Submit on the oracle from the task's initial state -> the Submit's reward."""
    ops = O.o2arc_ops()
    H, W = inp.shape
    orc = B.OracleBackend(1, H, W, 3, "o2arc", ops)
    orc.set_tasks(inp[None], dim[None], ans[None], dim[None])
    orc.reset()
    for s in seq:
        orc.step("bbox", np.array([s[:4]], np.int32), np.array([s[4]], np.int32))
    r, _ = orc.step("bbox", np.zeros((1, 4), np.int32), np.array([len(ops) - 1], np.int32))
    return int(r[0])


def stamp_searches(venv, rows, n):
    """The two searches of check 5 on every task -> (results of the single-step beam, results of the macro beam)."""
    import torch
    singles = [S.beam_search(venv, rows[i:i + 1], None, width=1, depth=2, src_env=torch.tensor([i]), propose=S.propose_objects([COPY_O, PASTE], []))
               for i in range(n)]
    macros = [S.beam_search(venv, rows[i:i + 1], None, width=1, depth=1, src_env=torch.tensor([i]),
                            propose=S.propose_object_macros([], [], [(COPY_O, PASTE)])) for i in range(n)]
    return singles, macros


# ---- one dumped case for the standalone sanitized emulator ---------------------------------------------------------------------------
def dump_case(path, be, rows, ingress, pay, op, length, src, flags, chunk):
    """Writes the inputs of one emulated macro expansion in the format macro_emu.cpp's main() reads: the selections as exactly
    A * T * w bytes, the lengths as exactly A int32."""
    rows = np.ascontiguousarray(rows, np.int8)
    M, K, T = rows.shape[0], op.shape[-2], op.shape[-1]
    mask = sum(1 << i for i, k in enumerate(B.PLANES[:-1]) if k in be.buf)
    hdr = np.array([0x4D414352, be.H, be.W, mask, len(be.ops), be.max_trial, be.N, M, K, be.INGRESS[ingress], K if op.ndim == 3 else 0,
                    flags, rows.shape[1], int(src is not None), 1, chunk, T, int(length is not None), 0, 0], np.int32)
    ops = np.zeros(65, np.uint32)
    ops[:len(be.ops)] = be.ops
    with open(path, "wb") as f:
        for a in (hdr, ops, be.buf["answer"], be.rec, rows, np.ascontiguousarray(pay, np.uint8 if ingress == "bits" else np.int32),
                  np.ascontiguousarray(op, np.int32)):
            f.write(np.ascontiguousarray(a).tobytes())
        for a in (length, src):
            if a is not None:
                f.write(np.ascontiguousarray(a, np.int32).tobytes())
