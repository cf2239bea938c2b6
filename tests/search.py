"""Backend-independent checks of the search additions: arcle_expand_rows (K candidate actions per state row, verdicts and child
hashes only), arcle_hash_rows and arcle_amd.search (the NumPy mirror of the hash, beam_search).  The pattern of tests/rows.py: every
check takes a backend class — EmuSearchBackend (tests/emu/search_emu.cpp: the kernel bodies of arcle_search.h lock-step on the CPU)
or HipSearchBackend (the product) — and returns a list of mismatch strings; the reference point is always the oracle stepped from
the replicated parent, and arcle_amd.search.hash_rows_numpy of the oracle's child rows."""
import ctypes
import os
import subprocess

import numpy as np

import backends as B
import rows as R
from arcle_amd import search as S
from oracle import oracle as O

CASES = (("o2arc", 30, 30, 3), ("o2arc", 7, 12, -1), ("o2arc", 12, 12, 1), ("arc", 30, 30, 3), ("raw", 5, 5, 2))  # = rows.transition_rows
FAST_CASES = (("o2arc", 20, 24, 3), ("o2arc", 16, 16, 3))  # the FW_FAST kernels below 1024 bytes: rows of 512 and 256 bytes, 32 and 16 live lanes
ST_BAD_OP, ST_ROTATE_DOMAIN, ST_BAD_TASK = 1, 2, 4
STEP_DENSE = 16
EMU_DIR = os.path.join(B.ROOT, "tests", "emu")
EMU_SRC = os.path.join(EMU_DIR, "search_emu.cpp")
EMU_HDRS = [os.path.join(B.ROOT, "arcle_amd", "csrc", h) for h in ("arcle_wave.h", "arcle_search.h")]


class _ExpandParams(ctypes.Structure):  # mirror of arcle::ExpandParams (arcle_amd/csrc/arcle_search.h)
    _fields_ = [("p", B._StepParams), ("n_actions", ctypes.c_int32), ("action_row_stride", ctypes.c_int32), ("chunk", ctypes.c_int32),
                ("n_chunks", ctypes.c_int32), ("status_out", ctypes.c_void_p), ("hash", ctypes.c_void_p), ("parent_hash", ctypes.c_void_p)]


_emu = None


def search_emu_lib():
    global _emu
    if _emu is None:
        so = os.path.join(EMU_DIR, "libsearch_emu.so")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [EMU_SRC] + EMU_HDRS):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, EMU_SRC])
        _emu = ctypes.CDLL(so)
        _emu.search_emu_run.argtypes = [ctypes.c_int, ctypes.POINTER(_ExpandParams)]
        assert _emu.search_emu_params_size() == ctypes.sizeof(_ExpandParams), "ExpandParams layout drifted"
    return _emu


class EmuSearchBackend(B.EmuBackend):
    """EmuBackend + the emulated search kernels.  `chunk` (actions per emulated wave) defaults to 5, so that K = 24 exercises whole
    chunks, a short last chunk and the per-wave parent set-up several times per row."""
    name = "emu"
    CHUNK = 5

    def _xparams(self, rows):
        x = _ExpandParams()
        p = self._params()
        self._scratch = np.zeros(1, np.uint32)  # (the library points p.status at a word of its own: the sticky word stays)
        p.status = self._scratch.ctypes.data
        p.acct = None
        assert rows.dtype == np.int8 and rows.strides[1] == 1
        p.n_resident, p.n_envs = self.N, rows.shape[0]
        p.rows_in, p.rows_in_stride = rows.ctypes.data, rows.strides[0]
        x.p = p
        return x

    def hash_rows(self, rows):
        """rows: int8 [M, >= L], any row stride / base alignment (a view is passed as it is)."""
        x = self._xparams(rows)
        out = np.zeros((rows.shape[0], 2), np.uint64)
        x.hash = out.ctypes.data
        rc = search_emu_lib().search_emu_run(1, ctypes.byref(x))
        assert rc == 0, f"search emulator reported error {rc}"
        return out

    def expand_rows(self, rows, ingress, payload, op, src_env=None, dense=True, flags=0, chunk=None):
        rows = np.ascontiguousarray(rows, np.int8)
        pay, opa = np.ascontiguousarray(payload, np.int32), np.ascontiguousarray(op, np.int32)
        M, K = rows.shape[0], opa.shape[-1]
        x = self._xparams(rows)
        out = {"reward": np.full((M, K), -7, np.int32), "term": np.full((M, K), 7, np.uint8), "status": np.full((M, K), 0x55, np.uint8),
               "hash": np.zeros((M, K, 2), np.uint64), "dense": np.full((M, K, 2), -7, np.int32) if dense else None,
               "parent_hash": np.zeros((M, 2), np.uint64)}
        src = None if src_env is None else np.ascontiguousarray(src_env, np.int32)
        x.p.sel, x.p.op, x.p.ingress = pay.ctypes.data, opa.ctypes.data, self.INGRESS[ingress]
        x.p.flags = flags | (STEP_DENSE if dense else 0)
        x.p.reward, x.p.term = out["reward"].ctypes.data, out["term"].ctypes.data
        x.p.dense = out["dense"].ctypes.data if dense else None
        x.p.task_idx = None if src is None else src.ctypes.data
        x.n_actions, x.action_row_stride = K, (K if opa.ndim == 2 else 0)
        x.chunk = chunk or self.CHUNK
        x.n_chunks = (K + x.chunk - 1) // x.chunk
        x.status_out, x.hash, x.parent_hash = out["status"].ctypes.data, out["hash"].ctypes.data, out["parent_hash"].ctypes.data
        rc = search_emu_lib().search_emu_run(0, ctypes.byref(x))
        assert rc == 0, f"search emulator reported error {rc} (divergent cross-lane op / non-uniform value)"
        return out

    def sticky_status(self):
        return int(self.stat[0])


class HipSearchBackend(B.HipBackend):
    """HipBackend + EnvBatch.expand_rows / hash_rows."""
    name = "hip"

    def hash_rows(self, rows):
        t = self.torch
        buf = t.as_tensor(np.ascontiguousarray(rows), device=self.b.device)  # (strided views: see hash_rows_strided)
        return self.b.hash_rows(buf).cpu().numpy().view(np.uint64)

    def hash_rows_strided(self, rows, stride, offset):
        """The same rows laid out `stride` bytes apart from byte `offset` of a 16-byte aligned device buffer."""
        t = self.torch
        M, L = rows.shape
        buf = t.zeros(offset + M * stride + 16, dtype=t.int8, device=self.b.device)
        view = t.as_strided(buf, (M, L), (stride, 1), offset)
        view.copy_(t.as_tensor(np.ascontiguousarray(rows, np.int8), device=self.b.device))
        return self.b.hash_rows(view).cpu().numpy().view(np.uint64)

    def expand_rows(self, rows, ingress, payload, op, src_env=None, dense=True, flags=0, chunk=None):
        t, dev = self.torch, self.b.device
        ex = self.b.expand_rows(t.as_tensor(np.ascontiguousarray(rows, np.int8), device=dev), ingress,
                                t.as_tensor(np.ascontiguousarray(payload, np.int32), device=dev),
                                t.as_tensor(np.ascontiguousarray(op, np.int32), device=dev),
                                None if src_env is None else t.as_tensor(np.ascontiguousarray(src_env, np.int32), device=dev),
                                dense=dense, flags=flags)
        return {"reward": ex.reward.cpu().numpy(), "term": ex.term.cpu().numpy(), "status": ex.status.cpu().numpy(),
                "hash": ex.hash.cpu().numpy().view(np.uint64), "dense": None if ex.dense is None else ex.dense.cpu().numpy(),
                "parent_hash": ex.parent_hash.cpu().numpy().view(np.uint64)}

    def sticky_status(self):
        return self.b.status(False)


# ---- the oracle's side ---------------------------------------------------------------------------------------------------------
def draw_actions(rng, form, n, H, W, n_ops):
    """n actions of one tuple form from rows._random_actions (its op mix, its 10 % forced Submits): draws of the other forms are
    discarded."""
    while True:
        ing, pay, op = R._random_actions(rng, n, H, W, n_ops)
        if ing == form:
            return pay, op


def dense_pair(grid, gdim, ans, adim):
    """(correct cells, total cells) of one grid against one answer — DESIGN.md §3 / step_core: matches inside the common rectangle;
    total = the common rectangle + the cells only one of the two has."""
    gh, gw, ah, aw = int(gdim[0]), int(gdim[1]), int(adim[0]), int(adim[1])
    mh, mw = min(gh, ah), min(gw, aw)
    correct = int((grid[:mh, :mw] == ans[:mh, :mw]).sum())
    if (gh <= ah) == (gw <= aw):
        total = mh * mw + abs(ah * aw - gh * gw)
    else:
        total = mh * mw + abs(gh - ah) * mw + abs(gw - aw) * mh
    return correct, total


def dense_pairs(grid, gdim, ans, adim):
    """dense_pair for n (grid, answer) pairs at once -> int32 [n, 2]."""
    n, H, W = grid.shape
    gh, gw, ah, aw = (gdim[:, 0].astype(np.int64), gdim[:, 1].astype(np.int64), adim[:, 0].astype(np.int64), adim[:, 1].astype(np.int64))
    mh, mw = np.minimum(gh, ah), np.minimum(gw, aw)
    inside = (np.arange(H)[None, :, None] < mh[:, None, None]) & (np.arange(W)[None, None, :] < mw[:, None, None])
    correct = ((grid == ans) & inside).sum((1, 2))
    total = np.where((gh <= ah) == (gw <= aw), mh * mw + np.abs(ah * aw - gh * gw), mh * mw + np.abs(gh - ah) * mw + np.abs(gw - aw) * mh)
    return np.stack([correct, total], 1).astype(np.int32)


def oracle_from_rows(rows, answers, adims, kind, H, W, mt, ops):
    """An OracleBackend of len(rows) envs holding the states in `rows` with the given answers."""
    n = len(rows)
    orc = B.OracleBackend(n, H, W, mt, kind, ops)
    off = 0
    vals = {}
    for f, ln in B.row_layout(kind, H * W):
        vals[f] = np.ascontiguousarray(rows[:, off:off + ln]).view(np.int8)
        off += ln
    orc.set_tasks(vals["input"].reshape(n, H, W), vals["input_dim"], answers, adims)
    orc.reset()
    for f, v in vals.items():
        dst = orc.env.planes[f] if f in orc.env.planes else orc.env.field(f)
        dst[:] = v.reshape(dst.shape)
    return orc


def oracle_expand(rows, answers, adims, kind, H, W, mt, ops, form, pay, op):
    """Every (row m, action (m, k)) stepped on the oracle from the replicated parent.  rows [M, L]; answers [M, H, W] / adims [M, 2] of
    the env each row is judged against; pay [M, K, ..], op [M, K].  -> dict of [M, K] reward / term / status, [M, K, L] child rows,
    [M, K, 2] dense pairs ((0, 0) where the step did not happen: bad op, Rotate domain)."""
    M, K = op.shape
    rep = np.repeat(np.arange(M), K)
    big = oracle_from_rows(rows[rep], answers[rep], adims[rep], kind, H, W, mt, ops)
    r, t = big.step(form, pay.reshape(M * K, -1), op.reshape(-1))
    status = np.zeros(M * K, np.uint8)
    if big.status():  # the oracle's status word is per batch: children of a batch that raised something are re-stepped one by one
        for c in range(M * K):
            one = oracle_from_rows(rows[rep[c]:rep[c] + 1], answers[rep[c]:rep[c] + 1], adims[rep[c]:rep[c] + 1], kind, H, W, mt, ops)
            one.step(form, pay.reshape(M * K, -1)[c:c + 1], op.reshape(-1)[c:c + 1])
            status[c] = one.status()
    child = B.state_rows(big)
    dense = dense_pairs(big.get("grid"), big.get("grid_dim"), answers[rep], adims[rep])
    dense[(status & (ST_BAD_OP | ST_ROTATE_DOMAIN)) != 0] = 0
    return {"reward": r.reshape(M, K), "term": t.reshape(M, K), "status": status.reshape(M, K), "rows": child.reshape(M, K, -1),
            "dense": dense.reshape(M, K, 2)}


CORPUS = {}  # (kind, H, W) -> list of [n, L] int8 arrays: every state row the checks produced (hash identity runs over all of them)


def _keep(kind, H, W, rows):
    CORPUS.setdefault((kind, H, W), []).append(np.ascontiguousarray(rows.reshape(-1, rows.shape[-1])))


def case_pair(cls, kind, H, W, mt):
    return R._pair(cls, 8, H, W, seed=H * W + mt, max_trial=mt, kind=kind, warm=12)


def vacuity(tag, want, parents):
    """The corpus is worth comparing against — asserted on the ORACLE's results alone.  -> (changed share, rewards, distinct rows)."""
    M, K, L = want["rows"].shape
    changed = float((want["rows"] != parents[:, None, :]).any(2).mean())
    rewards = int((want["reward"] == 1).sum())
    distinct = len(np.unique(want["rows"].reshape(M * K, L), axis=0))
    return changed, rewards, distinct


def expansion(cls, cases=CASES, forms=("bbox", "point")):
    """Checks 1, 2 and 5: every (m, k) of expand_rows equals the oracle stepped from the replicated parent — reward, terminated, status,
    dense pair, hash == hash_rows_numpy(oracle child row), parent_hash — for shared and per-row action sets, default and permuted
    src_env with more rows than envs, an out-of-range op and a Submit-heavy set per case; nothing of the handle moves."""
    errs = []
    for kind, H, W, mt in cases:
        be, orc, rng, ops = case_pair(cls, kind, H, W, mt)
        N, K, n_ops = 8, 24, len(ops)
        base = B.state_rows(orc)
        answers, adims = orc.get("answer"), orc.get("answer_dim")
        before = {f: be.get(f) for f in R._state_fields(kind) + ["answer", "answer_dim"]}
        cnt_before, st_before = be.counters(), be.sticky_status()
        for form in forms:
            for per_row in (True, False):
                for permuted in (False, True):
                    tag = f"{kind} {H}x{W} {form} {'per-row' if per_row else 'shared'} {'src' if permuted else 'default'}"
                    M = N + 3 if permuted else N
                    src = rng.integers(0, N, M).astype(np.int32) if permuted else np.arange(N, dtype=np.int32)
                    rows = base[src]
                    pay, op = draw_actions(rng, form, M * K if per_row else K, H, W, n_ops)
                    if per_row:
                        pay, op = pay.reshape(M, K, -1), op.reshape(M, K)
                        op[0, 3] = n_ops + 2        # an out-of-range op
                        op[1, :] = n_ops - 1        # a Submit-heavy set
                        op[2, ::2] = n_ops - 1
                        pay_full, op_full = pay, op
                    else:
                        op[5] = n_ops + 2
                        op[6:12] = n_ops - 1
                        pay_full, op_full = np.broadcast_to(pay, (M,) + pay.shape).copy(), np.broadcast_to(op, (M, K)).copy()
                    want = oracle_expand(rows, answers[src], adims[src], kind, H, W, mt, ops, form, pay_full, op_full)
                    _keep(kind, H, W, want["rows"])
                    if per_row and not permuted:  # check 2, on the oracle's results before any comparison
                        changed, rewards, distinct = vacuity(tag, want, rows)
                        print(f"corpus {tag}: changed {changed:.2f}, rewards {rewards}, distinct {distinct} of {M * K}")
                        assert changed >= 0.40, f"{tag}: only {changed:.2f} of the children differ from their parent"
                        assert distinct <= 0.90 * M * K, f"{tag}: {distinct} distinct child rows of {M * K}: fewer than 10 % duplicates"
                        if (H, W) == (30, 30) or kind == "raw":
                            assert rewards >= 1, f"{tag}: no child with reward 1"
                    got = be.expand_rows(rows, form, pay, op, src_env=src if permuted else None, dense=True)
                    hw = S.hash_rows_numpy(want["rows"].reshape(M * K, -1), kind, H, W).reshape(M, K, 2)
                    for name, a, b in (("reward", got["reward"], want["reward"]), ("terminated", got["term"], want["term"]),
                                       ("status", got["status"], want["status"]), ("dense", got["dense"], want["dense"]),
                                       ("hash", got["hash"], hw),
                                       ("parent_hash", got["parent_hash"], S.hash_rows_numpy(rows, kind, H, W))):
                        if not np.array_equal(a, b):
                            bad = np.argwhere(np.asarray(a != b).reshape(a.shape[0], a.shape[1] if a.ndim > 1 else 1, -1).any(2))[:4]
                            errs.append(f"{tag}: {name} differs at (m, k) {bad.tolist()} (ops {[int(op_full[m, k]) for m, k in bad] if name != 'parent_hash' else ''})")
                    st = want["status"] != 0
                    if not np.array_equal(got["hash"][st], np.broadcast_to(got["parent_hash"][:, None, :], got["hash"].shape)[st]):
                        errs.append(f"{tag}: a child with a status bit does not hash as its parent")
                    if len(errs) > 10:
                        return errs
        # check 5: expansion is speculation
        for f, v in before.items():
            if not np.array_equal(be.get(f), v):
                errs.append(f"{kind} {H}x{W}: resident field {f} was touched by expand_rows")
        if not np.array_equal(be.counters(), cnt_before) or be.sticky_status() != st_before:
            errs.append(f"{kind} {H}x{W}: counters / sticky status were touched by expand_rows")
        # a row whose src_env names no env: every child is the parent with ARCLE_ST_BAD_TASK
        pay, op = draw_actions(rng, "bbox", 4, H, W, n_ops)
        got = be.expand_rows(base[:2], "bbox", pay, op, src_env=np.array([1, N + 5], np.int32))
        if not (got["status"][1] == ST_BAD_TASK).all() or not (got["hash"][1] == got["parent_hash"][1]).all() or (got["status"][0] & ST_BAD_TASK).any():
            errs.append(f"{kind} {H}x{W}: src_env out of range: status {got['status'].tolist()}")
        if be.sticky_status() != st_before:
            errs.append(f"{kind} {H}x{W}: sticky status moved")
    return errs


def hash_strides(cls, cases=CASES):
    """Check 3, first half: the same rows at strides L, L + 5, a 16-multiple, from aligned and odd base offsets hash alike, and equal
    the mirror."""
    errs = []
    for kind, H, W, mt in cases:
        be, orc, rng, ops = case_pair(cls, kind, H, W, mt)
        rows = B.state_rows(orc)
        M, L = rows.shape
        want = S.hash_rows_numpy(rows, kind, H, W)
        for stride, offset in ((L, 0), (L + 5, 0), ((L + 15) & ~15, 16), (L + 5, 3), ((L + 31) & ~15, 7)):
            if hasattr(be, "hash_rows_strided"):
                got = be.hash_rows_strided(rows, stride, offset)
            else:
                buf = np.zeros(offset + M * stride + 64, np.int8)
                a0 = (-buf.ctypes.data) % 16  # (a 16-byte aligned origin, then the offset)
                view = np.lib.stride_tricks.as_strided(buf[a0 + offset:], (M, L), (stride, 1))
                view[:] = rows
                got = be.hash_rows(view)
            if not np.array_equal(got, want):
                errs.append(f"{kind} {H}x{W}: hash_rows at stride {stride} offset {offset} differs from the mirror")
    return errs


# ---- hash structure (check 4) ----------------------------------------------------------------------------------------------------
def structure_rows(delta_pairs=(1, 8, -128)):
    """Yields (tag, rows) batches of single-change and pair-change variants of one warmed 12 x 12 o2arc row."""
    kind, H, W = "o2arc", 12, 12
    _, orc, _, _ = R._pair(B.OracleBackend, 8, H, W, seed=H * W + 1, max_trial=1, kind=kind, warm=12)
    base = B.state_rows(orc)[3].copy()
    P = H * W
    yield "base", base[None]
    off = 0
    for f, ln in B.row_layout(kind, P):
        if ln == P:
            for d in (1, 8, -128):  # every single cell
                v = np.repeat(base[None], P, 0)
                v[np.arange(P), off + np.arange(P)] = (v[np.arange(P), off + np.arange(P)].astype(np.int16) + d).astype(np.int8)
                yield f"{f} single {d}", v
            ia, ib = np.triu_indices(P, 1)
            for d in delta_pairs:  # every pair of cells of the plane, same delta
                v = np.repeat(base[None], len(ia), 0)
                r = np.arange(len(ia))
                v[r, off + ia] = (v[r, off + ia].astype(np.int16) + d).astype(np.int8)
                v[r, off + ib] = (v[r, off + ib].astype(np.int16) + d).astype(np.int8)
                yield f"{f} pairs {d}", v
        else:
            for j in range(ln):  # every scalar byte
                for d in (1, 8, -128):
                    v = base[None].copy()
                    v[0, off + j] = np.int8((int(v[0, off + j]) + d + 128) % 256 - 128)
                    yield f"{f}[{j}] {d}", v
        off += ln


def hash_structure(spot_backend=None, spot=40):
    """Every single-cell change, every single scalar change and every pair of cells of one plane changed by the same delta (1, 8,
    -128) gives a state_hash different from the base row's and from every other variant's — on the mirror; `spot` rows of every batch
    are also hashed by `spot_backend` and compared."""
    errs, hashes, n = [], [], 0
    be = spot_backend(8, 12, 12, 1, "o2arc", O.o2arc_ops()) if spot_backend else None
    rng = np.random.default_rng(4)
    for tag, rows in structure_rows():
        h = S.hash_rows_numpy(rows, "o2arc", 12, 12)
        hashes.append(h[:, 0])
        n += len(rows)
        if len(rows) > 1:
            _keep("o2arc", 12, 12, rows[rng.integers(0, len(rows), 64)])
        if be is not None:
            pick = rng.integers(0, len(rows), min(spot, len(rows)))
            if not np.array_equal(be.hash_rows(np.ascontiguousarray(rows[pick])), h[pick]):
                errs.append(f"{tag}: the backend's hash differs from the mirror")
    allh = np.concatenate(hashes)
    if len(np.unique(allh)) != n:
        errs.append(f"hash structure: {n - len(np.unique(allh))} collisions among {n} variants of one row")
    return errs, n


def hash_identity():
    """Check 3, second half, over every row the checks of this process kept: distinct rows <=> distinct state_hash; grid_hash equal
    <=> (grid, grid_dim) equal."""
    errs, total = [], 0
    for (kind, H, W), chunks in CORPUS.items():
        rows = np.unique(np.concatenate(chunks), axis=0)
        total += len(rows)
        h = S.hash_rows_numpy(rows, kind, H, W)
        if len(np.unique(h[:, 0])) != len(rows):
            errs.append(f"{kind} {H}x{W}: {len(rows) - len(np.unique(h[:, 0]))} state_hash collisions among {len(rows)} distinct rows")
        P, off = H * W, 0
        for f, ln in B.row_layout(kind, P):
            if f == "grid":
                g = rows[:, off:off + P + 2]  # grid, grid_dim are neighbours in the row
            off += ln
        n_grids = len(np.unique(g, axis=0))
        pairs = np.unique(np.concatenate([g.view(np.uint8), h[:, 1:2].copy().view(np.uint8)], 1), axis=0)
        if len(np.unique(h[:, 1])) != n_grids or len(pairs) != n_grids:
            errs.append(f"{kind} {H}x{W}: grid_hash is not one-to-one with (grid, grid_dim): {len(np.unique(h[:, 1]))} hashes, {n_grids} grids")
    return errs, total


# ---- beam search: a stub venv over the oracle (check 6) and planted tasks (check 12) -----------------------------------------------
class OracleVenv:
    """What beam_search needs of a vec env — expand / transition / hash_rows — backed by the oracle and the NumPy hash, on torch CPU
    tensors.  answers [N, H, W] / adims [N, 2]: the tasks src_env indexes."""

    def __init__(self, kind, H, W, mt, ops, answers, adims):
        self.kind, self.H, self.W, self.mt, self.ops = kind, H, W, mt, ops
        self.answers, self.adims = answers, adims

    def hash_rows(self, rows):
        import torch
        return torch.from_numpy(S.hash_rows_numpy(rows.numpy(), self.kind, self.H, self.W).view(np.int64))

    def expand(self, rows, action, src_env=None):
        import torch
        from arcle_amd.engine import Expansion
        form = "bbox" if "bbox" in action else "point"
        rows_n, pay, op = rows.numpy(), action[form].numpy(), action["operation"].numpy()
        M, K = len(rows_n), len(op)
        src = np.arange(M) if src_env is None else src_env.numpy()
        w = oracle_expand(rows_n, self.answers[src], self.adims[src], self.kind, self.H, self.W, self.mt, self.ops, form,
                          np.broadcast_to(pay, (M,) + pay.shape).copy(), np.broadcast_to(op, (M, K)).copy())
        h = S.hash_rows_numpy(w["rows"].reshape(M * K, -1), self.kind, self.H, self.W).view(np.int64).reshape(M, K, 2)
        return Expansion(torch.from_numpy(w["reward"].astype(np.int32)), torch.from_numpy(w["term"].astype(np.uint8)),
                         torch.from_numpy(w["status"]), torch.from_numpy(h), torch.from_numpy(w["dense"]), self.hash_rows(rows))

    def transition(self, rows, action, src_env=None):
        import torch
        form = "bbox" if "bbox" in action else "point"
        rows_n = rows.numpy()
        src = np.arange(len(rows_n)) if src_env is None else src_env.numpy()
        orc = oracle_from_rows(rows_n, self.answers[src], self.adims[src], self.kind, self.H, self.W, self.mt, self.ops)
        r, t = orc.step(form, action[form].numpy(), action["operation"].numpy())
        orc.status()
        return torch.from_numpy(B.state_rows(orc)), torch.from_numpy(r), torch.from_numpy(t.astype(bool))


def planted_tasks(n_tasks=16, H=10, W=10, K=64, seed=2025):
    """n_tasks 10 x 10 O2ARC tasks whose answer is the input after a known sequence of 3 actions out of ONE shared set of K bbox
    actions (Color on a rectangle, Move of a rectangle, CopyO + Paste), planted so that — checked here on the oracle, exhaustively —
    no sequence of 1 or 2 actions from the set reaches the answer.  -> (inputs [n,H,W], idims, answers, adims, actions dict of numpy
    arrays, the planted sequences)."""
    rng = np.random.default_rng(seed)
    ops = O.o2arc_ops()
    bbox, op = np.zeros((K, 4), np.int32), np.zeros(K, np.int32)
    for k in range(K):
        x, y = rng.integers(0, H - 2), rng.integers(0, W - 2)
        bbox[k] = (x, y, min(H - 1, x + rng.integers(0, 3)), min(W - 1, y + rng.integers(0, 3)))
        op[k] = (rng.integers(1, 10), rng.integers(20, 24), 29, 30)[k % 4]  # Color | Move | CopyO | Paste
    tasks, tries = [], 0
    while len(tasks) < n_tasks:
        tries += 1
        assert tries < 400, "planted_tasks: could not plant enough tasks"
        inp = rng.integers(0, 10, (1, H, W)).astype(np.int8)
        idim = np.array([[H, W]], np.int8)
        seq = rng.choice(K, 3, replace=False)
        orc = B.OracleBackend(1, H, W, 3, "o2arc", ops)
        orc.set_tasks(inp, idim, inp, idim)
        orc.reset()
        root = B.state_rows(orc)
        for k in seq:
            orc.step("bbox", bbox[k:k + 1], op[k:k + 1])
        ans = orc.get("grid")
        if orc.status() or (ans == inp).all():
            continue
        # exhaustive depths 1 and 2 from the set: no grid may equal the answer
        lvl1 = oracle_expand(root, ans, idim, "o2arc", H, W, 3, ops, "bbox", bbox[None], op[None])
        if ((lvl1["dense"][..., 0] == lvl1["dense"][..., 1]) & (lvl1["status"] == 0)).any():
            continue
        rows1 = lvl1["rows"][0]
        lvl2 = oracle_expand(rows1, np.repeat(ans, K, 0), np.repeat(idim, K, 0), "o2arc", H, W, 3, ops, "bbox",
                             np.broadcast_to(bbox, (K, K, 4)).copy(), np.broadcast_to(op, (K, K)).copy())
        ok2 = lvl2["status"] == 0
        if ((lvl2["dense"][..., 0] == lvl2["dense"][..., 1]) & ok2).any():
            continue
        tasks.append((inp[0], ans[0], [int(k) for k in seq]))
    inputs = np.stack([t[0] for t in tasks])
    answers = np.stack([t[1] for t in tasks])
    dims = np.tile(np.array([[H, W]], np.int8), (n_tasks, 1))
    return inputs, dims, answers, dims.copy(), {"bbox": bbox, "operation": op}, [t[2] for t in tasks]


def replay_on_oracle(inp, idim, ans, adim, actions, seq, H=10, W=10):
    """The sequence + a Submit on the oracle from the task's initial state -> the Submit's reward."""
    ops = O.o2arc_ops()
    orc = B.OracleBackend(1, H, W, 3, "o2arc", ops)
    orc.set_tasks(inp[None], idim[None], ans[None], adim[None])
    orc.reset()
    for k in seq:
        orc.step("bbox", actions["bbox"][k:k + 1], actions["operation"][k:k + 1])
    r, _ = orc.step("bbox", np.zeros((1, 4), np.int32), np.array([len(ops) - 1], np.int32))
    return int(r[0])


# ---- one dumped case for the standalone sanitized emulator (check 7) ---------------------------------------------------------------
def dump_case(path, be, rows, ingress, pay, op, src, flags, chunk):
    """Writes the inputs of one emulated expansion in the format search_emu.cpp's main() reads."""
    rows = np.ascontiguousarray(rows, np.int8)
    M, K = rows.shape[0], op.shape[-1]
    mask = sum(1 << i for i, k in enumerate(B.PLANES[:-1]) if k in be.buf)
    hdr = np.array([0x53454152, be.H, be.W, mask, len(be.ops), be.max_trial, be.N, M, K, be.INGRESS[ingress], K if op.ndim == 2 else 0,
                    flags, rows.shape[1], int(src is not None), 1, chunk], np.int32)
    ops = np.zeros(65, np.uint32)
    ops[:len(be.ops)] = be.ops
    with open(path, "wb") as f:
        for a in (hdr, ops, be.buf["answer"], be.rec, rows, np.ascontiguousarray(pay, np.int32), np.ascontiguousarray(op, np.int32)):
            f.write(np.ascontiguousarray(a).tobytes())
        if src is not None:
            f.write(np.ascontiguousarray(src, np.int32).tobytes())
