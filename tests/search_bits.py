"""Backend-independent checks of the bit-packed selection masks (ARCLE_INGRESS_BITS) in arcle_expand_rows and arcle_transition_rows,
and the oracle-backed stub vec env of the mask proposals (arcle_amd.search: pack_bits, object_actions(masks=True), beam_search).
The pattern of tests/search.py, which this module builds on: every check takes a backend class — EmuBitsBackend
(tests/emu/search_bits_emu.cpp: wave_expand_row<4, FW> and wave_transition_row<4, FW> lock-step on the CPU) or HipBitsBackend (the
product) — and returns a list of mismatch strings.  The reference is always the oracle stepped with the UNPACKED int8 0/1 masks
(SR.oracle_expand(..., "mask", ...)) and arcle_amd.search.hash_rows_numpy of the oracle's child rows."""
import ctypes
import os
import subprocess

import numpy as np

import backends as B
import rows as R
import search as SR
from arcle_amd import search as S
from oracle import oracle as O

EMU_SRC = os.path.join(SR.EMU_DIR, "search_bits_emu.cpp")
STRIDE = B.BITS_STRIDE
K_MIX = 24

_emu = None


def bits_emu_lib():
    global _emu
    if _emu is None:
        so = os.path.join(SR.EMU_DIR, "libsearch_bits_emu.so")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [EMU_SRC, SR.EMU_SRC] + SR.EMU_HDRS):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, EMU_SRC])
        _emu = ctypes.CDLL(so)
        _emu.search_bits_emu_run.argtypes = [ctypes.c_int, ctypes.POINTER(SR._ExpandParams)]
        assert _emu.search_bits_emu_params_size() == ctypes.sizeof(SR._ExpandParams), "ExpandParams layout drifted"
    return _emu


def _bit_rows(payload, lead):
    pay = np.ascontiguousarray(payload, np.uint8)
    assert pay.shape == tuple(lead) + (STRIDE,), f"bit rows: {pay.shape}, expected {tuple(lead) + (STRIDE,)}"
    return pay


class EmuBitsBackend(SR.EmuSearchBackend):
    """EmuSearchBackend (the tuple forms, the hash) + the emulated bit-row kernels."""

    def expand_rows(self, rows, ingress, payload, op, src_env=None, dense=True, flags=0, chunk=None):
        if ingress != "bits":
            return super().expand_rows(rows, ingress, payload, op, src_env, dense, flags, chunk)
        rows = np.ascontiguousarray(rows, np.int8)
        opa = np.ascontiguousarray(op, np.int32)
        M, K = rows.shape[0], opa.shape[-1]
        pay = _bit_rows(payload, opa.shape)
        x = self._xparams(rows)
        out = {"reward": np.full((M, K), -7, np.int32), "term": np.full((M, K), 7, np.uint8), "status": np.full((M, K), 0x55, np.uint8),
               "hash": np.zeros((M, K, 2), np.uint64), "dense": np.full((M, K, 2), -7, np.int32) if dense else None,
               "parent_hash": np.zeros((M, 2), np.uint64)}
        src = None if src_env is None else np.ascontiguousarray(src_env, np.int32)
        x.p.sel, x.p.op, x.p.ingress = pay.ctypes.data, opa.ctypes.data, self.INGRESS["bits"]
        x.p.flags = flags | (SR.STEP_DENSE if dense else 0)
        x.p.reward, x.p.term = out["reward"].ctypes.data, out["term"].ctypes.data
        x.p.dense = out["dense"].ctypes.data if dense else None
        x.p.task_idx = None if src is None else src.ctypes.data
        x.n_actions, x.action_row_stride = K, (K if opa.ndim == 2 else 0)
        x.chunk = chunk or self.CHUNK
        x.n_chunks = (K + x.chunk - 1) // x.chunk
        x.status_out, x.hash, x.parent_hash = out["status"].ctypes.data, out["hash"].ctypes.data, out["parent_hash"].ctypes.data
        rc = bits_emu_lib().search_bits_emu_run(0, ctypes.byref(x))
        assert rc == 0, f"bit-row search emulator reported error {rc} (divergent cross-lane op / non-uniform value)"
        return out

    def transition_rows(self, rows, ingress, payload, op, src_env=None, tail=False, flags=0, in_place=False):
        if ingress != "bits":
            return super().transition_rows(rows, ingress, payload, op, src_env, tail, flags, in_place)
        x = SR._ExpandParams()
        p = self._params()
        self._extras(p)
        rows = np.ascontiguousarray(rows, np.int8)
        M, L = rows.shape[0], self._flat_len(False)
        out = np.full((M, ((L + 15) & ~15) + (16 if tail else 0)), 0x55, np.int8)
        if in_place:  # rows_out IS rows_in: untouched planes stay where they are (the library sets the writer's incremental mode)
            out[:, :L] = rows[:, :L]
            out[:, L:(L + 15) & ~15] = 0
            rows = out
            flags |= R.STEP_ROWS_INC
        pay, opa = _bit_rows(payload, (M,)), np.ascontiguousarray(op, np.int32)
        reward, term = np.zeros(M, np.int32), np.zeros(M, np.uint8)
        src = None if src_env is None else np.ascontiguousarray(src_env, np.int32)
        p.n_resident, p.n_envs = self.N, M
        p.rows_in, p.rows_in_stride = rows.ctypes.data, rows.shape[1]
        p.flat_out, p.flat_stride, p.flat_filter, p.flat_tail = out.ctypes.data, out.shape[1], 0, int(tail)
        p.sel, p.op, p.ingress, p.flags = pay.ctypes.data, opa.ctypes.data, self.INGRESS["bits"], flags
        p.reward, p.term = reward.ctypes.data, term.ctypes.data
        p.task_idx = None if src is None else src.ctypes.data
        x.p = p
        rc = bits_emu_lib().search_bits_emu_run(2, ctypes.byref(x))
        assert rc == 0, f"bit-row search emulator reported error {rc}"
        return out, reward, term


class HipBitsBackend(SR.HipSearchBackend):
    """HipSearchBackend + uint8 bit rows through EnvBatch.expand_rows / transition_rows.  chunk: the library's tuning variable
    ARCLE_EXPAND_CHUNK, which it reads at every call."""

    def expand_rows(self, rows, ingress, payload, op, src_env=None, dense=True, flags=0, chunk=None):
        if ingress != "bits" and chunk is None:
            return super().expand_rows(rows, ingress, payload, op, src_env, dense, flags)
        t, dev = self.torch, self.b.device
        pay = np.ascontiguousarray(payload, np.uint8 if ingress == "bits" else np.int32)
        old = os.environ.get("ARCLE_EXPAND_CHUNK")
        if chunk is not None:
            os.environ["ARCLE_EXPAND_CHUNK"] = str(chunk)
        try:
            ex = self.b.expand_rows(t.as_tensor(np.ascontiguousarray(rows, np.int8), device=dev), ingress, t.as_tensor(pay, device=dev),
                                    t.as_tensor(np.ascontiguousarray(op, np.int32), device=dev),
                                    None if src_env is None else t.as_tensor(np.ascontiguousarray(src_env, np.int32), device=dev),
                                    dense=dense, flags=flags)
        finally:
            if chunk is not None:
                os.environ.pop("ARCLE_EXPAND_CHUNK")
                if old is not None:
                    os.environ["ARCLE_EXPAND_CHUNK"] = old
        return {"reward": ex.reward.cpu().numpy(), "term": ex.term.cpu().numpy(), "status": ex.status.cpu().numpy(),
                "hash": ex.hash.cpu().numpy().view(np.uint64), "dense": None if ex.dense is None else ex.dense.cpu().numpy(),
                "parent_hash": ex.parent_hash.cpu().numpy().view(np.uint64)}

    def transition_rows(self, rows, ingress, payload, op, src_env=None, tail=False, flags=0, in_place=False):
        if ingress != "bits":
            return super().transition_rows(rows, ingress, payload, op, src_env, tail, flags, in_place)
        t, dev = self.torch, self.b.device
        M, L = len(rows), self.b.state_row_size()
        buf = None
        rows_t = t.as_tensor(np.ascontiguousarray(rows, np.int8), device=dev)
        if in_place:
            buf = t.zeros((M, ((L + 15) & ~15) + (16 if tail else 0)), dtype=t.int8, device=dev)
            buf[:, :L] = rows_t[:, :L]
            rows_t = buf
        out, r, tm = self.b.transition_rows(rows_t, "bits", t.as_tensor(_bit_rows(payload, (M,)), device=dev),
                                            t.as_tensor(np.ascontiguousarray(op, np.int32), device=dev),
                                            None if src_env is None else t.as_tensor(np.ascontiguousarray(src_env, np.int32), device=dev),
                                            out=buf, tail=tail, flags=flags)
        return out.cpu().numpy(), r.cpu().numpy(), tm.cpu().numpy()


# ---- the mask mix --------------------------------------------------------------------------------------------------------------
def mask_mix(rng, grids, gdims, K, H, W):
    """K int8 0/1 masks for each of the grids [M, H, W]: slot k by k mod 4 — 0 and 1: a component of that grid (components_numpy,
    skip_color 0; a random 15 % mask where the grid has none), 2: one cell inside grid_dim, 3: a random 15 % mask."""
    M = len(grids)
    out = np.zeros((M, K, H, W), np.int8)
    for m in range(M):
        n, _, _, comps = S.components_numpy(grids[m], gdims[m], 48, 0)
        gh, gw = min(int(gdims[m][0]), H), min(int(gdims[m][1]), W)
        for k in range(K):
            if k % 4 < 2 and n:
                out[m, k] = comps[rng.integers(0, n)]
            elif k % 4 == 2:
                out[m, k, rng.integers(0, gh), rng.integers(0, gw)] = 1
            else:
                out[m, k] = rng.random((H, W)) < 0.15
    return out


def not_filled_box(masks):
    """[..., H, W] -> bool [...]: the mask is not its bounding box filled (an empty mask counts as a box)."""
    m = np.asarray(masks) != 0
    r, c = m.any(-1), m.any(-2)
    span = lambda a: (a.cumsum(-1) > 0) & (a[..., ::-1].cumsum(-1)[..., ::-1] > 0)  # noqa: E731  (first .. last truthy index)
    return (m != (span(r)[..., :, None] & span(c)[..., None, :])).any((-1, -2))


def mix_case(cls, kind, H, W, mt):
    be, orc, rng, ops = SR.case_pair(cls, kind, H, W, mt)
    return be, orc, rng, ops, B.state_rows(orc), orc.get("answer"), orc.get("answer_dim")


def _grids_of(rows, kind, H, W):
    P, off = H * W, 0
    for f, ln in B.row_layout(kind, P):
        if f == "grid":
            return rows[:, off:off + P].reshape(-1, H, W), rows[:, off + P:off + P + 2]
        off += ln


def _compare(errs, tag, got, want, rows, kind, H, W, op_full):
    M, K = op_full.shape
    hw = S.hash_rows_numpy(want["rows"].reshape(M * K, -1), kind, H, W).reshape(M, K, 2)
    for name, a, b in (("reward", got["reward"], want["reward"]), ("terminated", got["term"], want["term"]),
                       ("status", got["status"], want["status"]), ("dense", got["dense"], want["dense"]), ("hash", got["hash"], hw),
                       ("parent_hash", got["parent_hash"], S.hash_rows_numpy(rows, kind, H, W))):
        if not np.array_equal(a, b):
            bad = np.argwhere(np.asarray(a != b).reshape(a.shape[0], a.shape[1] if a.ndim > 1 and name != "parent_hash" else 1, -1).any(2))[:4]
            errs.append(f"{tag}: {name} differs at (m, k) {bad.tolist()} (ops {[int(op_full[m, k]) for m, k in bad] if name != 'parent_hash' else ''})")
    st = want["status"] != 0
    if not np.array_equal(got["hash"][st], np.broadcast_to(got["parent_hash"][:, None, :], got["hash"].shape)[st]):
        errs.append(f"{tag}: a child with a status bit does not hash as its parent")


def expansion(cls, cases=SR.CASES):
    """Check 1: every (m, k) of expand_rows with bit rows equals the oracle stepped with the unpacked masks — shared and per-row
    sets, default and permuted src_env with M = 11 > N = 8, the out-of-range op and the Submit-heavy rows of SR.expansion; a src_env
    out of range; nothing of the handle moves.  The vacuity conditions are asserted on the oracle's results first."""
    errs = []
    for kind, H, W, mt in cases:
        be, orc, rng, ops, base, answers, adims = mix_case(cls, kind, H, W, mt)
        N, K, n_ops = 8, K_MIX, len(ops)
        before = {f: be.get(f) for f in R._state_fields(kind) + ["answer", "answer_dim"]}
        cnt_before, st_before = be.counters(), be.sticky_status()
        for per_row in (True, False):
            for permuted in (False, True):
                tag = f"{kind} {H}x{W} bits {'per-row' if per_row else 'shared'} {'src' if permuted else 'default'}"
                M = N + 3 if permuted else N
                src = rng.integers(0, N, M).astype(np.int32) if permuted else np.arange(N, dtype=np.int32)
                rows = base[src]
                grids, gdims = _grids_of(rows, kind, H, W)
                if per_row:
                    masks, op = mask_mix(rng, grids, gdims, K, H, W), rng.integers(0, n_ops, (M, K)).astype(np.int32)
                    op[0, 3] = n_ops + 2        # an out-of-range op
                    op[1, :] = n_ops - 1        # a Submit-heavy set
                    op[2, ::2] = n_ops - 1
                    masks_full, op_full = masks, op
                else:
                    masks, op = mask_mix(rng, grids[:1], gdims[:1], K, H, W)[0], rng.integers(0, n_ops, K).astype(np.int32)
                    op[5] = n_ops + 2
                    op[6:12] = n_ops - 1
                    masks_full, op_full = np.broadcast_to(masks, (M,) + masks.shape).copy(), np.broadcast_to(op, (M, K)).copy()
                want = SR.oracle_expand(rows, answers[src], adims[src], kind, H, W, mt, ops, "mask", masks_full.reshape(M, K, H * W), op_full)
                SR._keep(kind, H, W, want["rows"])
                if per_row and not permuted:  # the vacuity conditions, on the oracle's results before any comparison
                    ch = (want["rows"] != rows[:, None, :]).any(2)
                    nr = not_filled_box(masks_full)
                    changed, share, changed_nr = float(ch.mean()), float(nr.mean()), float(ch[nr].mean())
                    print(f"mix {tag}: changed {changed:.2f}, not a filled box {share:.2f}, changed among those {changed_nr:.2f}")
                    assert changed >= 0.40, f"{tag}: only {changed:.2f} of the children differ from their parent"
                    assert share >= 0.15, f"{tag}: only {share:.2f} of the masks are not their filled bounding box"
                    assert changed_nr >= 0.35, f"{tag}: only {changed_nr:.2f} of the children of such masks differ from their parent"
                got = be.expand_rows(rows, "bits", B.pack_bits(masks.reshape(-1, H, W)).reshape(masks.shape[:-2] + (STRIDE,)), op,
                                     src_env=src if permuted else None, dense=True)
                _compare(errs, tag, got, want, rows, kind, H, W, op_full)
                if len(errs) > 10:
                    return errs
        for f, v in before.items():
            if not np.array_equal(be.get(f), v):
                errs.append(f"{kind} {H}x{W}: resident field {f} was touched by expand_rows")
        if not np.array_equal(be.counters(), cnt_before) or be.sticky_status() != st_before:
            errs.append(f"{kind} {H}x{W}: counters / sticky status were touched by expand_rows")
        # a row whose src_env names no env: every child is the parent with ARCLE_ST_BAD_TASK
        grids, gdims = _grids_of(base[:1], kind, H, W)
        bits = B.pack_bits(mask_mix(rng, grids, gdims, 4, H, W)[0])
        got = be.expand_rows(base[:2], "bits", bits, rng.integers(0, n_ops, 4).astype(np.int32), src_env=np.array([1, N + 5], np.int32))
        if not (got["status"][1] == SR.ST_BAD_TASK).all() or not (got["hash"][1] == got["parent_hash"][1]).all() or (got["status"][0] & SR.ST_BAD_TASK).any():
            errs.append(f"{kind} {H}x{W}: src_env out of range: status {got['status'].tolist()}")
        if be.sticky_status() != st_before:
            errs.append(f"{kind} {H}x{W}: sticky status moved")
    return errs


def rectangles(cls, cases=SR.CASES[:3]):
    """Check 2: the bit rows of filled rectangles give bit for bit the outputs of the bbox expansion of those rectangles, on the same
    backend."""
    errs = []
    for kind, H, W, mt in cases:
        be, orc, rng, ops, base, _, _ = mix_case(cls, kind, H, W, mt)
        M, K = len(base), K_MIX
        bbox, op = SR.draw_actions(rng, "bbox", M * K, H, W, len(ops))
        bbox, op = bbox.reshape(M, K, 4), op.reshape(M, K)
        x0, x1 = np.minimum(bbox[..., 0], bbox[..., 2]), np.maximum(bbox[..., 0], bbox[..., 2])
        y0, y1 = np.minimum(bbox[..., 1], bbox[..., 3]), np.maximum(bbox[..., 1], bbox[..., 3])
        xs, ys = np.arange(H)[None, None, :, None], np.arange(W)[None, None, None, :]
        masks = (xs >= x0[..., None, None]) & (xs <= x1[..., None, None]) & (ys >= y0[..., None, None]) & (ys <= y1[..., None, None])
        a = be.expand_rows(base, "bbox", bbox, op)
        b = be.expand_rows(base, "bits", B.pack_bits(masks.reshape(-1, H, W)).reshape(M, K, STRIDE), op)
        for name in a:
            if not np.array_equal(a[name], b[name]):
                bad = np.argwhere((a[name] != b[name]).reshape(M, K if name != "parent_hash" else 1, -1).any(2))[:4]
                errs.append(f"{kind} {H}x{W}: {name} of the rectangles' bit rows differs from the bbox expansion at {bad.tolist()} (ops {[int(op[m, k]) for m, k in bad]})")
    return errs


def chunks(cls, kind="o2arc", H=12, W=12, mt=1):
    """Check 3: one wave per action, one wave per row and chunks in between give identical outputs."""
    be, orc, rng, ops, base, _, _ = mix_case(cls, kind, H, W, mt)
    grids, gdims = _grids_of(base, kind, H, W)
    bits = B.pack_bits(mask_mix(rng, grids, gdims, K_MIX, H, W).reshape(-1, H, W)).reshape(len(base), K_MIX, STRIDE)
    op = rng.integers(0, len(ops), (len(base), K_MIX)).astype(np.int32)
    ref = be.expand_rows(base, "bits", bits, op, chunk=24)
    return [f"chunk {c}: {k} differs from one wave per row" for c in (1, 7, 23) for k, v in be.expand_rows(base, "bits", bits, op, chunk=c).items()
            if not np.array_equal(v, ref[k])]


def transitions(cls, cases=SR.CASES):
    """Check 4: transition_rows with bit rows equals the oracle step with the unpacked masks, out of place and in place, with the tail;
    hash_rows of the rows it writes equals expand_rows' hash for the same (row, action) pairs, and so do the verdicts."""
    errs = []
    for kind, H, W, mt in cases:
        be, orc, rng, ops, base, answers, adims = mix_case(cls, kind, H, W, mt)
        N, K, n_ops = 8, K_MIX, len(ops)
        L = base.shape[1]
        grids, gdims = _grids_of(base, kind, H, W)
        masks, op = mask_mix(rng, grids, gdims, K, H, W), rng.integers(0, n_ops, (N, K)).astype(np.int32)
        op[0, 3] = n_ops + 2
        op[2, ::2] = n_ops - 1
        bits = B.pack_bits(masks.reshape(-1, H, W)).reshape(N, K, STRIDE)
        want = SR.oracle_expand(base, answers, adims, kind, H, W, mt, ops, "mask", masks.reshape(N, K, H * W), op)
        ex = be.expand_rows(base, "bits", bits, op, dense=True)
        be.status()
        for k in range(0, K, 5):  # N pairs per launch: slot k of every row (the dense output is per env)
            for in_place in (False, True):
                tag = f"{kind} {H}x{W} slot {k} {'in place' if in_place else 'out of place'}"
                out, r, t = be.transition_rows(base, "bits", bits[:, k], op[:, k], tail=True, in_place=in_place)
                st = be.status()
                tail = np.ascontiguousarray(out[:, -16:]).view(np.int32)
                if not np.array_equal(out[:, :L], want["rows"][:, k]):
                    errs.append(f"{tag}: output rows differ for rows {np.nonzero((out[:, :L] != want['rows'][:, k]).any(1))[0].tolist()} (ops {op[:, k].tolist()})")
                if out[:, L:(L + 15) & ~15].any():
                    errs.append(f"{tag}: row padding not zero")
                if not (np.array_equal(r, want["reward"][:, k]) and np.array_equal(t, want["term"][:, k])):
                    errs.append(f"{tag}: reward / terminated differ from the oracle")
                if not (np.array_equal(tail[:, 0], r) and np.array_equal(tail[:, 3] & 0xff, t) and np.array_equal((tail[:, 3] >> 16) & 0xff, want["status"][:, k])):
                    errs.append(f"{tag}: the tail differs (reward, terminated, status {((tail[:, 3] >> 16) & 0xff).tolist()})")
                if st != int(np.bitwise_or.reduce(want["status"][:, k])):
                    errs.append(f"{tag}: sticky status {st}")
                if not np.array_equal(be.hash_rows(np.ascontiguousarray(out[:, :L])), ex["hash"][:, k]):
                    errs.append(f"{tag}: hash_rows of the written rows differs from expand_rows' hash")
                if not (np.array_equal(ex["reward"][:, k], r) and np.array_equal(ex["term"][:, k], t) and np.array_equal(ex["status"][:, k], (tail[:, 3] >> 16) & 0xff)):
                    errs.append(f"{tag}: expand_rows' verdicts differ from transition_rows'")
        if len(errs) > 10:
            return errs
    return errs


def _fields_of(rows, kind, H, W):
    out, off = {}, 0
    for f, ln in B.row_layout(kind, H * W):
        out[f] = rows[:, off:off + ln]
        off += ln
    return out


def flagged_transitions(cls):
    """transition_rows with bit rows under every flag the entry point takes.  RESET_ON_SUBMIT and CONTINUE_RULE: the reference's own
    traces (tests/golden/research.npz, as tests/features.py replays them through step()) walked forward through transition_rows, the
    rows of one call the input of the next, alternately out of place and in place — reward, terminated and the state fields of the
    rows after every step equal the reference's.  DENSE: the pair of every row equals SR.dense_pairs of the oracle's child grid."""
    import features as F
    g, errs = F.golden(), []
    assert set(np.unique(g["ros_mask"])) <= {0, 1} and set(np.unique(g["replay_sel"])) <= {0, 1}  # boolean masks: a bit row says the same
    S_, N, H, W = g["ros_mask"].shape  # 10 x 10: the generic-width kernel
    for mt in sorted(set(g["ros_max_trial"].tolist())):
        sel = np.nonzero(g["ros_max_trial"] == mt)[0]
        # (the handle holds 8 envs more than the trace uses: the row kernel requests the answer plane from all 64 lanes, 1024 bytes
        # from the env's plane on, whatever the plane stride — DESIGN.md §3, "Search on state rows" — and behind the LAST env of a
        # 128-byte-stride handle that is 896 bytes past the allocation; the envs used here are followed by 8 planes of the same array)
        pad = np.concatenate([sel, np.repeat(sel[:1], 8)])
        be = cls(len(pad), H, W, int(mt), "o2arc", O.o2arc_ops())
        be.set_tasks(g["ros_in"][pad], g["ros_in_dim"][pad], g["ros_ans"][pad], g["ros_ans_dim"][pad])
        be.reset()
        rows = B.state_rows(be)[:len(sel)]
        L = rows.shape[1]
        for s in range(S_):
            out, r, t = be.transition_rows(rows, "bits", B.pack_bits(g["ros_mask"][s][sel]), g["ros_op"][s][sel], tail=True, flags=F.STEP_ROS, in_place=s % 2 == 1)
            be.status()
            rows = np.ascontiguousarray(out[:, :L])
            got = _fields_of(rows, "o2arc", H, W)
            checks = [("reward", r, g["ros_reward"][s][sel]), ("term", t, g["ros_term"][s][sel])]
            checks += [(f, got[f], g["ros_" + f][s][sel]) for f in ("grid", "grid_dim", "selected", "clip", "trials_remain", "terminated")]
            for name, a, b in checks:
                if not np.array_equal(np.asarray(a).reshape(len(sel), -1), np.asarray(b).reshape(len(sel), -1)):
                    errs.append(f"reset_on_submit max_trial {mt} step {s}: {name} differs (ops {g['ros_op'][s][sel].tolist()})")
            if len(errs) > 8:
                return errs
    n, T = g["replay_op"].shape  # 30 x 30: the fast-width kernel
    be = cls(n, 30, 30, -1, "o2arc", O.o2arc_ops())
    be.set_tasks(g["replay_in"], g["replay_in_dim"], g["replay_ans"], g["replay_ans_dim"])
    be.reset()
    rows = B.state_rows(be)
    L = rows.shape[1]
    continued = 0
    for t in range(T):
        live = g["replay_op"][:, t] >= 0
        op = np.where(live, g["replay_op"][:, t], 32).astype(np.int32)  # finished traces: any op, no longer compared
        same = (g["replay_sel"][:, t].reshape(n, -1) == _fields_of(rows, "o2arc", 30, 30)["selected"]).all(1) & g["replay_sel"][:, t].reshape(n, -1).any(1)
        continued += int((same & live).sum())
        out, _, _ = be.transition_rows(rows, "bits", B.pack_bits(g["replay_sel"][:, t]), op, flags=F.STEP_CONTINUE, in_place=t % 2 == 1)
        be.status()
        rows = np.ascontiguousarray(out[:, :L])
        got = _fields_of(rows, "o2arc", 30, 30)
        bad = [i for i in np.nonzero(live)[0] if not (np.array_equal(got["grid"][i].reshape(30, 30), g["replay_grid"][i, t]) and np.array_equal(got["grid_dim"][i], g["replay_grid_dim"][i, t]))]
        if bad:
            errs.append(f"continue rule, trace replay step {t}: grid differs for traces {bad} (ops {op[bad].tolist()})")
            break
    assert continued >= 5, f"only {continued} steps of the traces resend the current selection: the rule is not exercised"
    kind, H, W, mt = SR.CASES[2]
    be, orc, rng, ops, base, answers, adims = mix_case(cls, kind, H, W, mt)
    be.set_dense_output()
    grids, gdims = _grids_of(base, kind, H, W)
    masks, op = mask_mix(rng, grids, gdims, 4, H, W), rng.integers(0, len(ops) - 1, (len(base), 4)).astype(np.int32)
    want = SR.oracle_expand(base, answers, adims, kind, H, W, mt, ops, "mask", masks.reshape(len(base), 4, H * W), op)
    for k in range(4):
        out, r, t = be.transition_rows(base, "bits", B.pack_bits(masks[:, k]), op[:, k], flags=SR.STEP_DENSE)
        be.status()
        if not (np.array_equal(np.asarray(be.dense), want["dense"][:, k]) and np.array_equal(out[:, :base.shape[1]], want["rows"][:, k]) and np.array_equal(r, want["reward"][:, k])):
            errs.append(f"dense: slot {k}: pair {np.asarray(be.dense).tolist()} vs {want['dense'][:, k].tolist()}, or rows / reward differ")
    return errs


def stray_bits(cls, kind="o2arc", H=7, W=12, mt=-1):
    """Check 5: every bit at a cell index >= H * W set to 1 changes nothing (7 x 12: bits 84 .. 1023 are free)."""
    be, orc, rng, ops, base, _, _ = mix_case(cls, kind, H, W, mt)
    grids, gdims = _grids_of(base, kind, H, W)
    M = len(base)
    masks, op = mask_mix(rng, grids, gdims, K_MIX, H, W), rng.integers(0, len(ops), (M, K_MIX)).astype(np.int32)
    bits = B.pack_bits(masks.reshape(-1, H, W)).reshape(M, K_MIX, STRIDE)
    free = np.unpackbits(np.zeros(STRIDE, np.uint8), bitorder="little")
    free[H * W:] = 1
    dirty = bits | np.packbits(free, bitorder="little")
    assert np.array_equal(np.unpackbits(dirty, axis=-1, bitorder="little")[..., :H * W], masks.reshape(M, K_MIX, -1)) and dirty[..., -1].min() == 255
    a, b = be.expand_rows(base, "bits", bits, op), be.expand_rows(base, "bits", dirty, op)
    errs = [f"expand_rows: {k} moved with the bits beyond H * W" for k in a if not np.array_equal(a[k], b[k])]
    ta, tb = be.transition_rows(base, "bits", bits[:, 1], op[:, 1], tail=True), be.transition_rows(base, "bits", dirty[:, 1], op[:, 1], tail=True)
    be.status()
    return errs + [f"transition_rows: output {i} moved with the bits beyond H * W" for i in range(3) if not np.array_equal(ta[i], tb[i])]


def dump_case(path, be, rows, bits, op, src, flags, chunk):
    """Writes the inputs of one emulated bit-row expansion in the format search_bits_emu.cpp's main() reads: SR.dump_case's with the
    selection as exactly A * 128 bytes."""
    rows = np.ascontiguousarray(rows, np.int8)
    M, K = rows.shape[0], op.shape[-1]
    mask = sum(1 << i for i, k in enumerate(B.PLANES[:-1]) if k in be.buf)
    hdr = np.array([0x53454152, be.H, be.W, mask, len(be.ops), be.max_trial, be.N, M, K, be.INGRESS["bits"], K if op.ndim == 2 else 0,
                    flags, rows.shape[1], int(src is not None), 1, chunk], np.int32)
    ops = np.zeros(65, np.uint32)
    ops[:len(be.ops)] = be.ops
    with open(path, "wb") as f:
        for a in (hdr, ops, be.buf["answer"], be.rec, rows, _bit_rows(bits, op.shape), np.ascontiguousarray(op, np.int32)):
            f.write(np.ascontiguousarray(a).tobytes())
        if src is not None:
            f.write(np.ascontiguousarray(src, np.int32).tobytes())


# ---- the mask proposals: a stub vec env over the oracle, and planted tasks a box cannot solve -----------------------------------
class MaskVenv(SR.OracleVenv):
    """What beam_search(propose=propose_objects(...)) needs of a vec env, backed by the oracle on torch CPU tensors: `expand` /
    `transition` take "bits" (unpacked and stepped as int8 masks) or "bbox", one set per row or one for all; `components` comes
    from components_numpy, with the bit rows.  Slots with operation -1 are answered as the device answers them — ARCLE_ST_BAD_OP,
    the child is its parent — without asking the oracle."""

    def _form(self, action):
        if "bits" in action:
            m = np.unpackbits(action["bits"].numpy(), axis=-1, bitorder="little")[..., :self.H * self.W]
            return "mask", np.ascontiguousarray(m.astype(np.int8))
        return "bbox", action["bbox"].numpy()

    def expand(self, rows, action, src_env=None):
        import torch
        from arcle_amd.engine import Expansion
        rows_n, op = rows.numpy(), action["operation"].numpy()
        form, pay = self._form(action)
        M, K = len(rows_n), op.shape[-1]
        if op.ndim == 1:
            pay, op = np.broadcast_to(pay, (M,) + pay.shape), np.broadcast_to(op, (M, K))
        src = np.arange(M) if src_env is None else src_env.numpy()
        pad = op < 0
        w = SR.oracle_expand(rows_n, self.answers[src], self.adims[src], self.kind, self.H, self.W, self.mt, self.ops, form,
                             np.where(pad[..., None], 0, pay).astype(pay.dtype), np.where(pad, 0, op).astype(np.int32))
        w["status"][pad] = SR.ST_BAD_OP
        w["rows"][pad] = np.broadcast_to(rows_n[:, None, :], w["rows"].shape)[pad]
        h = S.hash_rows_numpy(w["rows"].reshape(M * K, -1), self.kind, self.H, self.W).view(np.int64).reshape(M, K, 2)
        return Expansion(torch.from_numpy(w["reward"].astype(np.int32)), torch.from_numpy(w["term"].astype(np.uint8)),
                         torch.from_numpy(w["status"]), torch.from_numpy(h), torch.from_numpy(w["dense"]), self.hash_rows(rows))

    def transition(self, rows, action, src_env=None):
        import torch
        rows_n = rows.numpy()
        form, pay = self._form(action)
        src = np.arange(len(rows_n)) if src_env is None else src_env.numpy()
        orc = SR.oracle_from_rows(rows_n, self.answers[src], self.adims[src], self.kind, self.H, self.W, self.mt, self.ops)
        r, t = orc.step(form, pay, action["operation"].numpy())
        orc.status()
        return torch.from_numpy(B.state_rows(orc)), torch.from_numpy(r), torch.from_numpy(t.astype(bool))

    def components(self, rows, max_components=32, skip_color=-1, bits=False):
        import torch
        from arcle_amd.envs.vec import Components
        grids, gdims = _grids_of(rows.numpy(), self.kind, self.H, self.W)
        M, C = len(grids), int(max_components)
        count, left, comp = np.zeros(M, np.int32), np.zeros(M, np.int32), np.zeros((M, C, 8), np.int32)
        mbits = np.zeros((M, C, STRIDE), np.uint8)
        for m in range(M):
            count[m], left[m], comp[m], masks = S.components_numpy(grids[m], gdims[m], C, skip_color)
            mbits[m] = B.pack_bits(masks)
        t = torch.from_numpy(comp)
        return Components(torch.from_numpy(count), torch.from_numpy(left), t[:, :, 0:4], t[:, :, 4:6], t[:, :, 6], t[:, :, 7],
                          torch.from_numpy(mbits) if bits else None)


COLOR_OPS, MOVE_OPS = list(range(1, 10)), list(range(20, 24))  # O2ARCv2Env's table: Color1-9, MoveU / D / R / L
SHAPES = (((0, 0), (1, 0), (2, 0), (2, 1), (2, 2)),            # an L; (0, 2) of its box is free
          ((0, 0), (0, 1), (0, 2), (1, 0), (2, 0), (2, 1), (2, 2)),  # a C; (1, 1) and (1, 2) are free
          ((0, 1), (1, 0), (1, 1), (1, 2), (2, 1)),            # a plus; the corners are free
          ((0, 0), (0, 1), (1, 1), (1, 2)))                    # an S; (0, 2) and (1, 0) are free


def planted_mask_tasks(n=8, H=10, W=10, seed=5):
    """n 10 x 10 O2ARC tasks on background 0: one object that is not its filled bounding box (SHAPES) with a cell of another colour
    inside its box, and a filled 2 x 2 object apart from it.  Even tasks: the answer is the first object recoloured (depth 1); odd
    tasks: the object moved by one cell, then recoloured (depth 2) — both made by the ORACLE with the object's exact mask, both out
    of reach of its box, which paints or drags the foreign cell along.  -> (inputs [n, H, W], dims [n, 2], answers, depths)"""
    rng = np.random.default_rng(seed)
    ops = O.o2arc_ops()
    inputs, answers, depths = [], [], []
    while len(inputs) < n:
        i = len(inputs)
        shape = np.array(SHAPES[i % len(SHAPES)])
        bh, bw = shape.max(0) + 1
        x, y = rng.integers(2, H - 2 - bh), rng.integers(2, W - 2 - bw)
        c_obj, c_in, c_other, c_new = rng.permutation(np.arange(1, 10))[:4]
        g = np.zeros((H, W), np.int8)
        g[x + shape[:, 0], y + shape[:, 1]] = c_obj
        free = [(a, b) for a in range(bh) for b in range(bw) if g[x + a, y + b] == 0]
        fa, fb = free[rng.integers(0, len(free))]
        g[x + fa, y + fb] = c_in
        ox, oy = rng.integers(0, H - 1), rng.integers(0, W - 1)
        if g[max(0, ox - 1):ox + 3, max(0, oy - 1):oy + 3].any() or (x - 2 <= ox <= x + bh + 1 and y - 2 <= oy <= y + bw + 1):
            continue
        g[ox:ox + 2, oy:oy + 2] = c_other
        mask = (g == c_obj).astype(np.int8)
        dims = np.array([[H, W]], np.int8)
        orc = B.OracleBackend(1, H, W, 3, "o2arc", ops)
        orc.set_tasks(g[None], dims, g[None], dims)
        orc.reset()
        depth = 1 + i % 2
        if depth == 2:
            move = int(rng.integers(20, 24))
            orc.step("mask", mask[None], np.array([move], np.int32))
            mask = (orc.get("grid")[0] == c_obj).astype(np.int8)
        orc.step("mask", mask[None], np.array([int(c_new)], np.int32))
        ans = orc.get("grid")[0]
        if orc.status() or int((ans == c_new).sum()) != len(shape) or int((ans == c_in).sum()) != 1:
            continue
        inputs.append(g)
        answers.append(ans)
        depths.append(depth)
    return np.stack(inputs), np.tile(np.array([[H, W]], np.int8), (n, 1)), np.stack(answers), depths


def replay_masks_on_oracle(inp, dim, ans, seq):
    """The (selection, op) sequence + a Submit on the oracle from the task's initial state -> the Submit's reward."""
    ops = O.o2arc_ops()
    H, W = inp.shape
    orc = B.OracleBackend(1, H, W, 3, "o2arc", ops)
    orc.set_tasks(inp[None], dim[None], ans[None], dim[None])
    orc.reset()
    for sel, op in seq:
        assert sel.dtype == bool and sel.shape == (H, W)
        orc.step("mask", sel[None].astype(np.int8), np.array([op], np.int32))
    r, _ = orc.step("mask", np.zeros((1, H, W), np.int8), np.array([len(ops) - 1], np.int32))
    return int(r[0])
