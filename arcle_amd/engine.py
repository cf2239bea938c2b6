"""Device-resident state of a batch of ARCLE envs + the calls into libarcle_hip.so.

`EnvBatch` owns the HBM buffers (torch tensors: plumbing for device memory and streams only) in the
layout include/arcle_hip.h declares and hands their raw pointers to the C ABI.  All stepping happens
in the HIP kernels; this file contains no grid arithmetic.
"""
import collections
import contextlib
import ctypes
import gc
import os

import numpy as np
import torch

from . import _lib
from ._lib import ArcleHipError

PLANES = ["input", "grid", "selected", "clip", "object", "object_sel", "background", "answer"]
PLANE_ID = {k: i for i, k in enumerate(PLANES)}
REC_FIELDS = {  # name -> (byte offset, length) inside the 16-byte per-env record
    "input_dim": (0, 2), "grid_dim": (2, 2), "clip_dim": (4, 2), "object_dim": (6, 2), "object_pos": (8, 2),
    "trials_remain": (10, 1), "terminated": (11, 1), "active": (12, 1), "rotation_parity": (13, 1),
    "answer_dim": (14, 2),
}
KIND_PLANES = {  # which planes each env kind's state dict holds (o2arcenv.py:16-34, arcenv.py:81-89)
    "o2arc": PLANES,
    "arc": ["input", "grid", "clip", "answer"],
    "raw": ["input", "grid", "answer"],
}
STEP_AUTORESET = 1
STEP_ELIDE_SELECTED = 2
STEP_TRUNCATE = 4
STEP_RESAMPLE = 8
STEP_DENSE = 16
STEP_CONTINUE_RULE = 32
STEP_RESET_ON_SUBMIT = 64
STEP_FLAT_OBS = 128
STEP_PACK_OBS = 256
STEP_ROWS_INCREMENTAL = 512
AUG_PERMUTE, AUG_ROT90 = 1, 2
ST_BAD_OP, ST_ROTATE_DOMAIN, ST_BAD_TASK, ST_BAD_SELECTION, ST_AUG_DOMAIN = 1, 2, 4, 8, 16
ROW_TAIL = 16  # bytes of the optional step-output tail of a flat row (arcle_set_flat_output_ex)
MAX_CELLS = 1024  # ARCLE_MAX_CELLS: one 64-lane wavefront x 16 cells per lane holds a whole H x W plane (the one-wavefront-per-env kernels)
MAX_SIDE = 127    # dims travel as int8 in the per-env record (and in the reference's state dict, base.py:162-166)


def is_big_grid(H, W):
    """More than ARCLE_MAX_CELLS cells: the handle is served by the workgroup-per-env kernels (arcle_amd/csrc/arcle_big.hip)."""
    return int(H) * int(W) > MAX_CELLS


def check_grid_size(H, W):
    """The reference's constructor takes any max_grid_size (base.py:37-49) and stores the dims as int8 (base.py:162-166), so sides up to
    127 are meaningful.  H * W <= 1024 runs on the one-wavefront-per-env kernels (ARC grids are at most 30 x 30: the headline path);
    larger planes on the workgroup-per-env kernels — the same API minus what `EnvBatch.BIG_UNSUPPORTED` lists.  A side beyond 127 is
    refused here, before any device is touched; arcle_create reports the same as ARCLE_ERR_CONFIG."""
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        raise ValueError(f"max_grid_size must be positive, got ({H}, {W})")
    if H > MAX_SIDE or W > MAX_SIDE:
        raise ValueError(f"max_grid_size ({H}, {W}) is outside what the HIP path supports: H, W <= {MAX_SIDE} (grid dims are int8 in the "
                         f"state dict, as in the reference); ARC grids are at most 30 x 30")


_hip = None


@contextlib.contextmanager
def capture_guard():
    """Wrap every hipGraph capture of the package.  Python finalizers must not run while a capture is under way: an EnvBatch that
    dies at a garbage collection (an ARCVecEnv with a task sampler holds reference cycles, so it dies then and not at its last
    reference) frees its device buffers with hipFree, a synchronising call, and that invalidates the capture.  Dead objects are
    therefore collected first and the collector stays off until the capture has ended."""
    was_enabled = gc.isenabled()
    gc.collect()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


# what EnvBatch.expand_rows returns: device tensors [M, K, ...] (dense None without the dense pair; parent_hash [M, 2])
PLANE_SLACK = 1024  # readable bytes the library wants behind every plane it is given (ARCLE_PLANE_SLACK, include/arcle_hip.h)
Expansion = collections.namedtuple("Expansion", "reward term status hash dense parent_hash")


class EnvBatch:
    """n_envs envs of one kind on one GPU."""
    # what a batch of more than 1024 cells per plane (`self.big`) does not offer — the library refuses these calls with ARCLE_ERR_CONFIG
    BIG_UNSUPPORTED = ("autotune (one launch plan: returns no candidates)",)

    def __init__(self, n_envs, H, W, max_trial=-1, kind="o2arc", device=None, plane_stride=None):
        check_grid_size(H, W)
        if not torch.cuda.is_available():
            raise ArcleHipError("no HIP device visible (torch.cuda.is_available() is False); "
                                "arcle_amd has no CPU fallback")
        self.L = _lib.lib()
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        if self.device.index is None:  # "cuda" means torch's CURRENT device, not ordinal 0 (multi-GPU ranks)
            self.device = torch.device(f"cuda:{torch.cuda.current_device()}")
        self.N, self.H, self.W, self.P = int(n_envs), int(H), int(W), int(H) * int(W)
        self.big = is_big_grid(H, W)
        if plane_stride is None:
            plane_stride = int(os.environ.get("ARCLE_PLANE_STRIDE", "0")) or ((self.P + 127) & ~127)  # ARCLE_DEFAULT_PLANE_STRIDE
        self.PS = int(plane_stride)  # plane stride: one aligned dwordx4 per lane
        self.max_trial, self.kind = int(max_trial), kind
        # 16 B alignment of every plane/record row comes from torch's >=256 B allocation alignment
        # PLANE_SLACK bytes behind every plane (ARCLE_PLANE_SLACK): the row kernels request the answer plane from all 64 lanes — 1024
        # bytes from the env's plane on, whatever the plane stride — and for the last envs of a handle with a stride below 1024 that
        # is behind the plane: without the slack, behind the allocation, which may end a mapped region
        self._plane_store = {k: torch.zeros(self.N * self.PS + PLANE_SLACK, dtype=torch.int8, device=self.device) for k in KIND_PLANES[kind]}
        self.planes = {k: v[:self.N * self.PS].view(self.N, self.PS) for k, v in self._plane_store.items()}
        self.rec = torch.zeros((self.N, 16), dtype=torch.int8, device=self.device)
        self.cnt = torch.zeros((self.N, 2), dtype=torch.int32, device=self.device)
        self.reward = torch.zeros(self.N, dtype=torch.int32, device=self.device)
        self.term = torch.zeros(self.N, dtype=torch.uint8, device=self.device)
        cfg = _lib.Config(self.N, self.H, self.W, self.max_trial, self.device.index, self.PS)
        bufs = _lib.Buffers()
        for k, i in PLANE_ID.items():
            bufs.plane[i] = self.planes[k].data_ptr() if k in self.planes else None
        bufs.rec = self.rec.data_ptr()
        bufs.cnt = self.cnt.data_ptr()
        h = ctypes.c_void_p()
        rc = self.L.arcle_create(ctypes.byref(cfg), ctypes.byref(bufs), ctypes.byref(h))
        if rc != 0:
            raise ArcleHipError(f"arcle_create failed with status {rc}")
        self._h = h
        self.bits_stride = int(self.L.arcle_mask_bits_stride(h))  # bytes between the envs' rows of a bit-packed mask array (128 up to 1024 cells)
        self.n_ops = 0
        self._reward_ptr, self._term_ptr = self.reward.data_ptr(), self.term.data_ptr()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            self.L.arcle_destroy(h)
            self._h = None

    # ---- helpers ------------------------------------------------------------------------------
    def _check(self, rc, what):
        if rc != 0:
            msg = self.L.arcle_last_error(self._h)
            raise ArcleHipError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def _stream(self):
        """Raw handle of torch's CURRENT stream on this device (the private accessor is several times cheaper than building a
        Stream object per call; it is what torch's own inductor runtime uses)."""
        try:
            return torch._C._cuda_getCurrentRawStream(self.device.index)
        except AttributeError:  # pragma: no cover - older / newer torch without the private accessor
            return torch.cuda.current_stream(self.device).cuda_stream

    def sync(self, stream=None):
        """Blocks until `stream` (default: torch's current stream on this device) has drained — hipStreamSynchronize called directly
        (the latency path of the single-env class; saves the Python-side bookkeeping of torch's Stream objects)."""
        global _hip
        if _hip is None:
            _hip = ctypes.CDLL("libamdhip64.so")
            _hip.hipStreamSynchronize.argtypes = [ctypes.c_void_p]
        rc = _hip.hipStreamSynchronize(self._stream() if stream is None else stream)
        if rc != 0:
            raise ArcleHipError(f"hipStreamSynchronize failed ({rc})")

    def next_seq(self, tail_u8):
        """Arms the completion signal of the next launch that writes the row tail `tail_u8` (arcle_set_flat_seq) and returns its
        sequence number.  The tail's signal byte is cleared first: one counter serves several tail buffers (the step() row and the
        transition() row of a single env), so a stale byte of an earlier launch on THIS buffer could equal the new number — the
        launch is stream-ordered after this host write to pinned memory."""
        tail_u8[15] = 0
        self._seq = getattr(self, "_seq", 0) % 255 + 1
        rc = self.L.arcle_set_flat_seq(self._h, self._seq)
        if rc != 0:
            self._check(rc, "arcle_set_flat_seq")
        return self._seq

    def wait_tail(self, tail_u8, seq, stream=None, spins=40000):
        """Waits for the launch armed with `seq` by polling byte 15 of its row tail in PINNED host memory (`tail_u8`: a 16-element uint8
        numpy view): the kernel stores that byte last, behind a system-scope release, so the row is complete when it shows up.  A bounded
        spin (~2 ms); then the stream is synchronised instead (a hung or failed launch surfaces there)."""
        for _ in range(spins):
            if tail_u8[15] == seq:
                return
        self.sync(stream)
        if tail_u8[15] != seq:
            raise ArcleHipError("the step finished without writing its row tail")

    def plane(self, name):
        """Zero-copy [N,H,W] int8 view of a state plane (row stride PS)."""
        return self.planes[name][:, :self.P].view(self.N, self.H, self.W)

    def field(self, name):
        """Zero-copy [N,len] int8 view of a scalar field of the per-env record."""
        off, n = REC_FIELDS[name]
        return self.rec[:, off:off + n]

    # ---- configuration ------------------------------------------------------------------------
    def set_op_table(self, descs):
        arr = (ctypes.c_uint32 * len(descs))(*[int(d) for d in descs])
        self._check(self.L.arcle_set_op_table(self._h, arr, len(descs)), "arcle_set_op_table")
        self.n_ops = len(descs)
        # flag for step launches on states that only ever evolved through this library (see ARCLE_STEP_ELIDE_SELECTED)
        self.elide_flag = STEP_ELIDE_SELECTED if self.L.arcle_can_elide_selected(self._h) else 0

    def set_tasks(self, inputs, answers, env_ids=None):
        """Uploads tasks.  inputs/answers: sequences of un-padded 2-D int8 arrays (what Loader.pick yields)."""
        ids = range(self.N) if env_ids is None else list(env_ids)
        n = len(ids)
        pin = np.zeros((n, self.PS), np.int8)
        pan = np.zeros((n, self.PS), np.int8)
        dims = np.zeros((n, 4), np.int8)
        for j, (a, b) in enumerate(zip(inputs, answers)):
            a = np.asarray(a, np.int8)
            b = np.asarray(b, np.int8)
            if a.shape[0] > self.H or a.shape[1] > self.W or b.shape[0] > self.H or b.shape[1] > self.W:
                raise ValueError("task grid larger than max_grid_size")
            pin[j, :self.P].reshape(self.H, self.W)[:a.shape[0], :a.shape[1]] = a
            pan[j, :self.P].reshape(self.H, self.W)[:b.shape[0], :b.shape[1]] = b
            dims[j] = (a.shape[0], a.shape[1], b.shape[0], b.shape[1])
        idx = torch.as_tensor(list(ids), device=self.device, dtype=torch.long)
        self.planes["input"][idx] = torch.from_numpy(pin).to(self.device)
        self.planes["answer"][idx] = torch.from_numpy(pan).to(self.device)
        d = torch.from_numpy(dims).to(self.device)
        self.rec[idx, 0:2] = d[:, 0:2]
        self.rec[idx, 14:16] = d[:, 2:4]

    def set_tasks_padded(self, inp, input_dim, ans, answer_dim):
        """Uploads already padded [N,H,W] int8 arrays + [N,2] dims (numpy or torch)."""
        t = lambda x: (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(self.device, torch.int8)  # noqa: E731
        self.plane("input").copy_(t(inp))
        self.plane("answer").copy_(t(ans))
        self.field("input_dim").copy_(t(input_dim))
        self.field("answer_dim").copy_(t(answer_dim))

    def set_task_table(self, inputs, answers):
        """Packs a list of (input, answer) grid pairs (un-padded 2-D int8 arrays) into the device task table that
        `reset_from_table` indexes.  One upload; resets afterwards move no grids over PCIe."""
        T = len(inputs)
        tin = np.zeros((T, self.PS), np.int8)
        tan = np.zeros((T, self.PS), np.int8)
        din = np.zeros((T, 2), np.int8)
        dan = np.zeros((T, 2), np.int8)
        for j, (a, b) in enumerate(zip(inputs, answers)):
            a, b = np.asarray(a, np.int8), np.asarray(b, np.int8)
            if max(a.shape[0], b.shape[0]) > self.H or max(a.shape[1], b.shape[1]) > self.W:
                raise ValueError("task grid larger than max_grid_size")
            tin[j, :self.P].reshape(self.H, self.W)[:a.shape[0], :a.shape[1]] = a
            tan[j, :self.P].reshape(self.H, self.W)[:b.shape[0], :b.shape[1]] = b
            din[j], dan[j] = a.shape, b.shape
        self._table = [torch.from_numpy(x).to(self.device) for x in (tin, din, tan, dan)]  # keep alive
        self._check(self.L.arcle_set_task_table(self._h, _ptr(self._table[0]), _ptr(self._table[1]), _ptr(self._table[2]),
                                                _ptr(self._table[3]), T), "arcle_set_task_table")
        self.n_tasks = T

    def reset_from_table(self, task_idx, mask=None, aug_k=None, aug_perm=None):
        """task_idx: int32 [N] (device) indices into the task table; mask: optional uint8/bool [N].
        aug_k uint8 [N] (np.rot90 count) / aug_perm uint8 [N,10] (colour permutation): explicit augmentation per env
        (agents/env.py:31-42 of the reference)."""
        if task_idx.dtype != torch.int32 or task_idx.device != self.device or not task_idx.is_contiguous():
            task_idx = task_idx.to(device=self.device, dtype=torch.int32).contiguous()
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        if aug_k is None and aug_perm is None:
            self._check(self.L.arcle_reset_from_table(self._h, _ptr(task_idx), _ptr(m), self._stream()), "arcle_reset_from_table")
            return
        k = None if aug_k is None else torch.as_tensor(aug_k, device=self.device).to(torch.uint8).contiguous()
        pm = None
        if aug_perm is not None:
            pm = torch.zeros((self.N, 16), dtype=torch.uint8, device=self.device)
            pm[:, :10] = torch.as_tensor(aug_perm, device=self.device).to(torch.uint8)
        self._check(self.L.arcle_reset_from_table_aug(self._h, _ptr(task_idx), _ptr(m), _ptr(k), _ptr(pm), self._stream()),
                    "arcle_reset_from_table_aug")
        torch.cuda.current_stream(self.device).synchronize()  # (k / pm are temporaries)

    def set_sampler(self, pair_off, pair_cnt, seed, env_base=0, aug_flags=0):
        """Device-side task choice (arcle_set_sampler): pair_off / pair_cnt = first table entry / number of entries of
        every candidate problem.  Draws are keyed by (seed, env_base + env, episode)."""
        self._pair = [torch.as_tensor(np.asarray(x, np.int32)).to(self.device) for x in (pair_off, pair_cnt)]  # keep alive
        assert int(self._pair[1].min()) > 0, "every candidate problem needs at least one pair"
        if not hasattr(self, "episode"):
            self.episode = torch.zeros(self.N, dtype=torch.int32, device=self.device)
            self.cur_task = torch.full((self.N,), -1, dtype=torch.int32, device=self.device)
        self._check(self.L.arcle_set_sampler(self._h, _ptr(self._pair[0]), _ptr(self._pair[1]), len(pair_cnt),
                                             ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), ctypes.c_int64(int(env_base)),
                                             _ptr(self.episode), _ptr(self.cur_task), int(aug_flags)), "arcle_set_sampler")

    def reset_sampled(self, mask=None):
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        self._check(self.L.arcle_reset_sampled(self._h, _ptr(m), self._stream()), "arcle_reset_sampled")

    def set_truncation(self, step_limit):
        """ARCLE_STEP_TRUNCATE output: self.trunc[env] = action_steps >= step_limit (gymnasium TimeLimit)."""
        self.trunc = torch.zeros(self.N, dtype=torch.uint8, device=self.device)
        self._check(self.L.arcle_set_truncation(self._h, _ptr(self.trunc), int(step_limit)), "arcle_set_truncation")

    def set_dense_output(self):
        """ARCLE_STEP_DENSE output: self.dense int32 [N,2] = (matching cells, total cells) of agents/env.py:44-58."""
        self.dense = torch.zeros((self.N, 2), dtype=torch.int32, device=self.device)
        self._check(self.L.arcle_set_dense_output(self._h, _ptr(self.dense)), "arcle_set_dense_output")

    # ---- the hot path -------------------------------------------------------------------------
    def reset(self, mask=None):
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        self._check(self.L.arcle_reset(self._h, _ptr(m), self._stream()), "arcle_reset")

    def _step(self, fn, payload, op, flags):
        if op.dtype != torch.int32 or not op.is_contiguous() or op.device != self.device:
            op = op.to(device=self.device, dtype=torch.int32).contiguous()
        # (plain ints for the pointer arguments: ctypes converts them without a c_void_p object per argument)
        rc = fn(self._h, payload.data_ptr(), op.data_ptr(), self._reward_ptr, self._term_ptr, flags, self._stream())
        if rc != 0:
            self._check(rc, "arcle_step")
        return self.reward, self.term

    def step_bbox(self, bbox, op, flags=0):
        """bbox int32 [N,4] = (x1,y1,x2,y2) as BBoxWrapper.action (bbox.py:22-30); op int32 [N]."""
        if bbox.dtype != torch.int32 or not bbox.is_contiguous() or bbox.device != self.device:
            bbox = bbox.to(device=self.device, dtype=torch.int32).contiguous()
        return self._step(self.L.arcle_step_bbox, bbox, op, flags)

    def step_point(self, xy, op, flags=0):
        if xy.dtype != torch.int32 or not xy.is_contiguous() or xy.device != self.device:
            xy = xy.to(device=self.device, dtype=torch.int32).contiguous()
        return self._step(self.L.arcle_step_point, xy, op, flags)

    def step_mask(self, sel, op, flags=0):
        """sel [N,H,W] int8/bool selection masks (action['selection'])."""
        if sel.dtype == torch.bool:
            sel = sel.to(torch.int8)
        if sel.dtype != torch.int8 or not sel.is_contiguous() or sel.device != self.device:
            sel = sel.to(device=self.device, dtype=torch.int8).contiguous()
        return self._step(self.L.arcle_step_mask, sel, op, flags)

    def step_bbox5(self, act5, flags=0):
        """act5 int32 [N,5] = the BBoxWrapper action (x1, y1, x2, y2, operation) as one record per env (bbox.py:22-30): no separate
        op array.  `act5` may also be PINNED HOST memory (the kernel reads it over PCIe: no copy node in front of the step)."""
        if act5.dtype != torch.int32 or not act5.is_contiguous() or not (act5.device == self.device or act5.is_pinned()):
            act5 = act5.to(device=self.device, dtype=torch.int32).contiguous()
        self._check(self.L.arcle_step_bbox5(self._h, _ptr(act5), _ptr(self.reward), _ptr(self.term), int(flags), self._stream()),
                    "arcle_step_bbox5")
        return self.reward, self.term

    def step_bits(self, bits, op, flags=0):
        """bits uint8 [N,128]: bit-packed boolean selection masks (bit f of row e = cell f of env e; `pack_mask_bits` makes them)."""
        assert bits.dtype == torch.uint8 and bits.shape == (self.N, self.bits_stride) and bits.is_contiguous() and bits.device == self.device
        return self._step(self.L.arcle_step_bits, bits, op, flags)

    def pack_mask_bits(self, sel, out=None):
        """int8/bool [N,H,W] selection masks -> uint8 [N,128] bit-packed rows (one launch)."""
        if sel.dtype == torch.bool:
            sel = sel.view(torch.int8) if sel.is_contiguous() else sel.to(torch.int8)
        if sel.dtype != torch.int8 or not sel.is_contiguous() or sel.device != self.device:
            sel = sel.to(device=self.device, dtype=torch.int8).contiguous()
        if out is None:
            out = torch.empty((self.N, self.bits_stride), dtype=torch.uint8, device=self.device)
        self._check(self.L.arcle_pack_mask_bits(self._h, _ptr(sel), _ptr(out), self._stream()), "arcle_pack_mask_bits")
        return out

    def step_many(self, form, payload, op=None, flags=0, reward=None, term=None):
        """K step() launches enqueued by ONE call into the library (arcle_step_many): payload [K, N, ...] in the ingress form
        `form` ("mask" | "bbox" | "point" | "bbox5" | "bits"), op int32 [K, N] (None for "bbox5") -> (reward int32 [K, N],
        terminated uint8 [K, N]).  Every step is a full step; self.reward / self.term are not written."""
        K = int(payload.shape[0])
        # ("bbox5" records may live in PINNED HOST memory: the library then prefetches step t+1's records under launch t)
        assert payload.is_contiguous() and (payload.device == self.device or (form == "bbox5" and payload.is_pinned()))
        assert op is None or (op.is_contiguous() and op.dtype == torch.int32)
        if reward is None:
            reward = torch.empty((K, self.N), dtype=torch.int32, device=self.device)
        if term is None:
            term = torch.empty((K, self.N), dtype=torch.uint8, device=self.device)
        self._check(self.L.arcle_step_many(self._h, _lib.INGRESS[form], K, _ptr(payload), _ptr(op), _ptr(reward), _ptr(term), int(flags),
                                           self._stream()), "arcle_step_many")
        return reward, term

    def set_dispatch_order(self, enable=True):
        """Dispatch order on / off for this handle (arcle_set_dispatch_order).  On (default): launches of the standard 30 x 30 batch
        hand the object operations (Move / Rotate / Flip, the longest waves) to the waves that start first — every launch derives that
        from the operations it is about to execute, inside groups of 32 envs; scheduling only, results never depend on it."""
        self._check(self.L.arcle_set_dispatch_order(self._h, 1 if enable else 0), "arcle_set_dispatch_order")

    def launch_info(self, form, flags):
        """The plan a step launch with this ingress form and these flags takes (arcle_launch_info): dict(orders_itself, policy ('' or the
        letter A / B / H / J), waves_per_workgroup, autotuned)."""
        import numpy as np
        out = np.zeros(4, np.int32)
        self._check(self.L.arcle_launch_info(self._h, _lib.INGRESS[form], int(flags), out.ctypes.data), "arcle_launch_info")
        return {"orders_itself": bool(out[0]), "policy": chr(out[1]) if out[1] else "", "waves_per_workgroup": int(out[2]), "autotuned": bool(out[3])}

    def orders_itself(self, form, flags):
        return self.launch_info(form, flags)["orders_itself"]

    def autotune(self, form, payload, op, flags):
        """Times every launch plan this handle can take on the caller's own action tensors — payload [K, N, ...] / op [K, N]: K consecutive
        action batches, a representative stretch of the policy's output (a single [N, ...] batch is accepted, but one repeated batch is
        a poor sample) — and keeps the fastest for later (form, flags) launches (arcle_autotune: state saved and restored, stream
        synchronised).  Returns the candidates as a list of dicts sorted by time."""
        import numpy as np
        rep = np.zeros((16, 4), np.int32)
        K = int(payload.shape[0]) if (op is not None and op.dim() == 2) or (op is None and payload.dim() == 3) else 1
        assert payload.is_contiguous() and (op is None or op.is_contiguous())
        rc = self.L.arcle_autotune(self._h, _lib.INGRESS[form], K, _ptr(payload), _ptr(op), int(flags), rep.ctypes.data, 16, self._stream())
        if rc < 0:
            self._check(rc, "arcle_autotune")
        rows = [{"orders_itself": bool(r[0]), "policy": chr(r[1]) if r[1] else "", "waves_per_workgroup": int(r[2]), "us_per_launch": r[3] / 1e3} for r in rep[:rc]]
        return sorted(rows, key=lambda r: r["us_per_launch"])

    def hint_next_ops(self, next_op, stride=1):
        """ABI 4's one-shot hint of the NEXT step's operations.  Launches order themselves since ABI 5, so this does nothing; kept so
        that callers written against it keep running."""
        return None

    def step_bbox_ptr(self, bbox_ptr, op_ptr, flags=0, stream=0):
        """Lowest-overhead launch for rollout loops: raw device addresses (ints) of an int32 [N,4] bbox array
        and an int32 [N] op array, explicit stream handle.  Outputs land in self.reward / self.term."""
        rc = self.L.arcle_step_bbox(self._h, bbox_ptr, op_ptr, self._reward_ptr, self._term_ptr, flags, stream)
        if rc != 0:
            self._check(rc, "arcle_step_bbox")

    def rollout(self, payload, op, flags=0, point=False, mask=False, packed=None):
        """T steps in one launch.  payload int32 [T,N,4] (bbox) / [T,N,2] (point) / int8 [T,N,H,W] (mask=True), op
        int32 [T,N]; returns (reward int32 [T,N], terminated uint8 [T,N]).  Same semantics as T step_* calls.
        packed: a uint8 [T, N, packed_obs_size()] device tensor — the launch then also writes the packed observation row of EVERY step
        (grid | grid_dim | reward | terminated; STEP_PACK_OBS; unpack with EnvBatch.unpack_obs): an observation after every step although
        the state never leaves the chip between the steps."""
        T = int(op.shape[0])
        if packed is not None:
            assert packed.shape == (T, self.N, self.packed_obs_size()) and packed.dtype == torch.uint8 and packed.is_contiguous() and packed.device == self.device
            prev = getattr(self, "packed", None)
            self._check(self.L.arcle_set_packed_output(self._h, _ptr(packed)), "arcle_set_packed_output")
            try:
                return self.rollout(payload, op, int(flags) | STEP_PACK_OBS, point, mask)
            finally:
                self._check(self.L.arcle_set_packed_output(self._h, _ptr(prev)), "arcle_set_packed_output")
        op = op.to(device=self.device, dtype=torch.int32).contiguous()
        if mask:
            payload = payload.to(device=self.device, dtype=torch.int8).contiguous()
            assert payload.shape == (T, self.N, self.H, self.W)
        else:
            payload = payload.to(device=self.device, dtype=torch.int32).contiguous()
            assert payload.shape == (T, self.N, 2 if point else 4)
        assert op.shape == (T, self.N)
        reward = torch.empty((T, self.N), dtype=torch.int32, device=self.device)
        term = torch.empty((T, self.N), dtype=torch.uint8, device=self.device)
        fn = self.L.arcle_rollout_mask if mask else (self.L.arcle_rollout_point if point else self.L.arcle_rollout_bbox)
        self._check(fn(self._h, T, _ptr(payload), _ptr(op), _ptr(reward), _ptr(term), int(flags), self._stream()),
                    "arcle_rollout")
        return reward, term

    def rollout_ex(self, payload, op, flags, form, trunc=None, dense=None, rows=None, rows_filtered=False, packed=None):
        """T steps in one launch with the research env's step flags (arcle_rollout_ex): same semantics as T step_* calls with `flags`,
        every step's outputs written to caller-allocated device tensors — trunc uint8 [T,N] (STEP_TRUNCATE), dense int32 [T,N,2]
        (STEP_DENSE), rows int8 [T,N,stride] (STEP_FLAT_OBS; stride = flat_obs_size(rows_filtered) rounded up to 16, rows written in full),
        packed uint8 [T,N,packed_obs_size()] (STEP_PACK_OBS).  form "bbox" (int32 [T,N,4]) | "point" (int32 [T,N,2]) | "mask" (int8
        [T,N,H,W]); op int32 [T,N].  Every tensor is checked before anything is launched (ValueError); an output flag whose tensor is missing
        is refused by the library.  Returns (reward int32 [T,N], terminated uint8 [T,N])."""
        if form not in ("bbox", "point", "mask"):
            raise ValueError(f"rollout_ex: form must be 'bbox', 'point' or 'mask', got {form!r}")
        if not torch.is_tensor(op) or op.dim() != 2:
            raise ValueError("rollout_ex: op must be an int32 [T, N] device tensor")
        T = int(op.shape[0])
        if T <= 0:
            raise ValueError("rollout_ex: at least one step")
        N = self.N

        def check(name, t, shape, dtype):
            if not torch.is_tensor(t) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != self.device or not t.is_contiguous():
                got = (tuple(t.shape), t.dtype, str(t.device), t.is_contiguous()) if torch.is_tensor(t) else type(t).__name__
                raise ValueError(f"rollout_ex: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)} on {self.device}, got {got}")

        pay_shape = {"bbox": (T, N, 4), "point": (T, N, 2), "mask": (T, N, self.H, self.W)}[form]
        check("payload", payload, pay_shape, torch.int8 if form == "mask" else torch.int32)
        check("op", op, (T, N), torch.int32)
        flags = int(flags)
        outs = {"trunc": (trunc, STEP_TRUNCATE), "dense": (dense, STEP_DENSE), "rows": (rows, STEP_FLAT_OBS), "packed": (packed, STEP_PACK_OBS)}
        for name, (t, bit) in outs.items():
            if t is not None and not flags & bit:
                raise ValueError(f"rollout_ex: {name} given without its step flag")
        if trunc is not None:
            check("trunc", trunc, (T, N), torch.uint8)
        if dense is not None:
            check("dense", dense, (T, N, 2), torch.int32)
        stride = 0
        if rows is not None:
            stride = (self.flat_obs_size(rows_filtered) + 15) & ~15
            check("rows", rows, (T, N, stride), torch.int8)
            if rows.data_ptr() % 16:
                raise ValueError("rollout_ex: rows must be 16-byte aligned")
        if packed is not None:
            check("packed", packed, (T, N, self.packed_obs_size()), torch.uint8)
            if packed.data_ptr() % 16:
                raise ValueError("rollout_ex: packed must be 16-byte aligned")
        reward = torch.empty((T, N), dtype=torch.int32, device=self.device)
        term = torch.empty((T, N), dtype=torch.uint8, device=self.device)
        out = _lib.RolloutOut(_ptr(trunc), _ptr(dense), _ptr(rows), stride, int(bool(rows_filtered)), _ptr(packed))
        self._check(self.L.arcle_rollout_ex(self._h, _lib.INGRESS[form], T, _ptr(payload), _ptr(op), _ptr(reward), _ptr(term),
                                            ctypes.byref(out), flags, self._stream()), "arcle_rollout_ex")
        return reward, term

    def flat_obs_size(self, filtered=False):
        """Logical row length of the flattened observation (7*H*W + 14 for O2ARCv2Env; 3*H*W + 10 filtered)."""
        n = self.L.arcle_flat_obs_size(self._h, int(filtered))
        if n < 0:
            raise ArcleHipError("the FilterO2ARC subset needs the O2ARCv2Env state planes")
        return n

    def _flat_buffer(self, filtered):
        L = self.flat_obs_size(filtered)
        return torch.empty((self.N, (L + 15) & ~15), dtype=torch.int8, device=self.device), L

    def flat_obs(self, out=None, filtered=False):
        """[N, L] int8 flattened observations in Gymnasium FlattenObservation key order (agents/models/GPTPolicy.py:
        17-35 of the reference), or the FilterO2ARC subset (agents/env.py:109-126).  Returned as a view of a [N, stride]
        buffer (stride = L rounded up to 16) so that every row store is aligned; pass that buffer back as `out` to reuse it."""
        L = self.flat_obs_size(filtered)
        if out is None:
            out, _ = self._flat_buffer(filtered)
        assert out.dtype == torch.int8 and out.device == self.device and out.shape == (self.N, (L + 15) & ~15) and out.is_contiguous()
        self._check(self.L.arcle_flatten_obs(self._h, _ptr(out), out.shape[1], int(filtered), self._stream()), "arcle_flatten_obs")
        return out[:, :L]

    def set_flat_output(self, filtered=False, tail=False, host=False):
        """Installs the destination of STEP_FLAT_OBS: every step call with that flag also refreshes `self.flat` ([N, L]).
        tail=True: each row's stride ends with 16 bytes of step outputs (`self.flat_tail` int32 [N, 4] view: reward, action_steps,
        submit_count, terminated | truncated << 8 | status << 16).  host=True: the rows live in PINNED HOST memory — the step kernel
        writes them across PCIe itself, no device->host copy afterwards (single envs / small batches)."""
        L = self.flat_obs_size(filtered)
        stride = ((L + 15) & ~15) + (ROW_TAIL if tail else 0)
        if host:
            self._flat_buf = torch.zeros((self.N, stride), dtype=torch.int8).pin_memory()
        else:
            self._flat_buf = torch.zeros((self.N, stride), dtype=torch.int8, device=self.device)
        self._check(self.L.arcle_set_flat_output_ex(self._h, _ptr(self._flat_buf), stride, int(filtered), int(tail)),
                    "arcle_set_flat_output_ex")
        self.flat = self._flat_buf[:, :L]
        self.flat_tail = self._flat_buf[:, stride - ROW_TAIL:].view(torch.int32) if tail else None
        return self.flat

    # ---- state rows: checkpoint / restore and the stateless batched transition ------------------------------------------------
    def state_row_size(self):
        return self.flat_obs_size(False)

    def get_state_rows(self, out=None):
        """The state dict of every env as one row [N, L] int8 (full FlattenObservation layout) — see set_state_rows."""
        return self.flat_obs(out, False)

    def set_state_rows(self, rows, mask=None):
        """rows int8 [N, >= L] (device or pinned host; any stride) -> the resident state of the (masked) envs: the inverse of
        get_state_rows.  The task side (answer, answer_dim) and the counters are not part of a row and stay."""
        assert rows.dtype == torch.int8 and rows.dim() == 2 and rows.shape[0] == self.N and rows.stride(1) == 1
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        self._check(self.L.arcle_set_state_rows(self._h, _ptr(rows), rows.stride(0), _ptr(m), self._stream()), "arcle_set_state_rows")
        if m is not None:
            torch.cuda.current_stream(self.device).synchronize()  # (m may be a temporary)

    def transition_rows(self, rows, form, payload, op, src_env=None, out=None, tail=False, flags=0, reward=None, term=None):
        """`transition(state, action)` of the reference (o2arcenv.py:149-151) for a batch of M (state row, action) pairs, none of
        which touches the resident envs: rows int8 [M, >= L]; payload in the ingress form `form` ("mask" int8 [M,H,W] | "bbox" int32
        [M,4] | "point" int32 [M,2] | "bits" uint8 [M,128]: bit-packed masks in `step_bits`' layout); op int32 [M]; src_env int32 [M] = the resident env whose answer a Submit / the reward compares
        with (None: env r for row r).  Returns (rows_out [M, stride], reward int32 [M], terminated uint8 [M]); with tail=True the last
        16 bytes of every output row carry (reward, 1, submit counted, terminated | status << 16).  All arrays device or pinned host."""
        M = int(rows.shape[0])
        L = self.flat_obs_size(False)
        stride = ((L + 15) & ~15) + (ROW_TAIL if tail else 0)
        if out is None:
            out = torch.empty((M, stride), dtype=torch.int8, device=self.device)
        # (`out` may be the buffer `rows` views: rows_out == rows_in with equal strides is the in-place form — untouched planes stay)
        assert out.dim() == 2 and out.shape[0] == M and out.shape[1] >= stride and out.shape[1] % 16 == 0 and out.dtype == torch.int8 and out.is_contiguous()
        stride = out.shape[1]
        assert rows.dtype == torch.int8 and rows.stride(1) == 1 and payload.is_contiguous() and op.dtype == torch.int32 and op.is_contiguous()
        if form == "bits":
            assert payload.dtype == torch.uint8 and tuple(payload.shape) == (M, self.bits_stride)
        if reward is None:
            reward = torch.empty(M, dtype=torch.int32, device=self.device)
        if term is None:
            term = torch.empty(M, dtype=torch.uint8, device=self.device)
        self._check(self.L.arcle_transition_rows(self._h, M, _ptr(rows), rows.stride(0), _lib.INGRESS[form], _ptr(payload), _ptr(op),
                                                 _ptr(src_env), _ptr(out), stride, int(tail), _ptr(reward), _ptr(term), int(flags),
                                                 self._stream()), "arcle_transition_rows")
        return out, reward, term

    # ---- search on state rows: hashes, K candidate actions per row ---------------------------------------------------------------
    def hash_rows(self, rows, out=None):
        """(state_hash, grid_hash) of every state row: rows int8 [M, >= L] (any stride / alignment) -> int64 [M, 2] (the uint64
        words of arcle_hash_rows reinterpreted: torch sorts, compares and `unique`s int64).  The formula: include/arcle_hip.h;
        its NumPy mirror: arcle_amd.search.hash_rows_numpy."""
        M = int(rows.shape[0])
        assert rows.dtype == torch.int8 and rows.dim() == 2 and rows.stride(1) == 1
        if out is None:
            out = torch.empty((M, 2), dtype=torch.int64, device=self.device)
        assert out.dtype == torch.int64 and tuple(out.shape) == (M, 2) and out.is_contiguous()
        self._check(self.L.arcle_hash_rows(self._h, M, _ptr(rows), rows.stride(0), _ptr(out), self._stream()), "arcle_hash_rows")
        return out

    def expand_rows(self, rows, form, payload, op, src_env=None, dense=False, flags=0, out=None):
        """K candidate actions per state row, verdicts only (arcle_expand_rows): rows int8 [M, >= L], read only; form "bbox" | "point" |
        "bits"; payload int32 [K, 4 | 2] — "bits": uint8 [K, 128], bit-packed masks in `step_bits`' layout, what `components_rows(bits=
        True)` writes — with op int32 [K] (ONE action set applied to every row) or [M, K, ...] with op [M, K] (a set per row); src_env int32 [M] = the env whose answer row m is judged against (None: env m).  Returns an Expansion of device tensors,
        all [M, K, ...]: reward int32, term uint8, status uint8 (ARCLE_ST_* bits of that child), hash int64 [M, K, 2] (state_hash,
        grid_hash of the child row, which is never written), dense int32 [M, K, 2] (correct, total) or None, parent_hash int64 [M, 2].
        Every value equals what transition_rows + hash_rows report for the replicated (row, action) pairs.  out: an Expansion of a
        previous call with the same shapes to write into (captured graphs)."""
        assert form in ("bbox", "point", "bits"), "expand_rows takes bbox, point or bits actions"
        M = int(rows.shape[0])
        tw = {"bbox": 4, "point": 2, "bits": self.bits_stride}[form]
        assert rows.dtype == torch.int8 and rows.dim() == 2 and rows.stride(1) == 1
        assert payload.dtype == (torch.uint8 if form == "bits" else torch.int32) and payload.is_contiguous() and op.dtype == torch.int32 and op.is_contiguous()
        if payload.dim() == 2:
            K, stride = int(payload.shape[0]), 0
            assert tuple(payload.shape) == (K, tw) and tuple(op.shape) == (K,)
        else:
            K = int(payload.shape[1])
            stride = K
            assert tuple(payload.shape) == (M, K, tw) and tuple(op.shape) == (M, K)
        if out is None:
            dev = self.device
            out = Expansion(torch.empty((M, K), dtype=torch.int32, device=dev), torch.empty((M, K), dtype=torch.uint8, device=dev),
                            torch.empty((M, K), dtype=torch.uint8, device=dev), torch.empty((M, K, 2), dtype=torch.int64, device=dev),
                            torch.empty((M, K, 2), dtype=torch.int32, device=dev) if dense else None,
                            torch.empty((M, 2), dtype=torch.int64, device=dev))
        assert tuple(out.reward.shape) == (M, K) and (out.dense is not None) == bool(dense)
        self._check(self.L.arcle_expand_rows(self._h, M, _ptr(rows), rows.stride(0), K, _lib.INGRESS[form], _ptr(payload), _ptr(op), stride,
                                             _ptr(src_env), _ptr(out.reward), _ptr(out.term), _ptr(out.status), _ptr(out.hash),
                                             _ptr(out.dense), _ptr(out.parent_hash), int(flags), self._stream()), "arcle_expand_rows")
        return out

    def expand_macros(self, rows, form, payload, op, length=None, src_env=None, dense=False, flags=0, out=None):
        """K candidate MACROS per state row — sequences of up to T steps run back to back on the wave's register copy of the state —
        with one set of verdicts per macro (arcle_expand_macros).  payload [K, T, w] with op int32 [K, T] and length int32 [K] (one
        set for every row) or [M, K, T, w] with op [M, K, T] and length [M, K] (a set per row); w as in `expand_rows`; length None:
        every macro runs its T steps.  Returns an Expansion, all [M, K, ...]: reward = the steps' rewards summed, term = the last
        step's, status = the OR of the steps' status bits, dense = the pair after the last step, hash = the hash of the final row —
        what `length` in-place transition_rows calls + hash_rows report.  A length outside [1, T] runs nothing: ARCLE_ST_BAD_OP,
        the parent's hash.  out: an Expansion of a previous call with the same shapes (captured graphs)."""
        assert form in ("bbox", "point", "bits"), "expand_macros takes bbox, point or bits actions"
        M = int(rows.shape[0])
        tw = {"bbox": 4, "point": 2, "bits": self.bits_stride}[form]
        assert rows.dtype == torch.int8 and rows.dim() == 2 and rows.stride(1) == 1
        assert payload.dtype == (torch.uint8 if form == "bits" else torch.int32) and payload.is_contiguous() and op.dtype == torch.int32 and op.is_contiguous()
        if payload.dim() == 3:
            K, T, stride = int(payload.shape[0]), int(payload.shape[1]), 0
            assert tuple(payload.shape) == (K, T, tw) and tuple(op.shape) == (K, T)
            lead = (K,)
        else:
            K, T = int(payload.shape[1]), int(payload.shape[2])
            stride = K
            assert tuple(payload.shape) == (M, K, T, tw) and tuple(op.shape) == (M, K, T)
            lead = (M, K)
        if length is not None:
            assert length.dtype == torch.int32 and length.is_contiguous() and tuple(length.shape) == lead
        if out is None:
            dev = self.device
            out = Expansion(torch.empty((M, K), dtype=torch.int32, device=dev), torch.empty((M, K), dtype=torch.uint8, device=dev),
                            torch.empty((M, K), dtype=torch.uint8, device=dev), torch.empty((M, K, 2), dtype=torch.int64, device=dev),
                            torch.empty((M, K, 2), dtype=torch.int32, device=dev) if dense else None,
                            torch.empty((M, 2), dtype=torch.int64, device=dev))
        assert tuple(out.reward.shape) == (M, K) and (out.dense is not None) == bool(dense)
        self._check(self.L.arcle_expand_macros(self._h, M, _ptr(rows), rows.stride(0), K, T, _lib.INGRESS[form], _ptr(payload), _ptr(op),
                                               _ptr(length), stride, _ptr(src_env), _ptr(out.reward), _ptr(out.term), _ptr(out.status),
                                               _ptr(out.hash), _ptr(out.dense), _ptr(out.parent_hash), int(flags), self._stream()),
                    "arcle_expand_macros")
        return out

    def components_rows(self, rows=None, max_components=32, skip_color=-1, bits=False, out=None):
        """The connected components (color.py:8-30: 4-connected, same colour, inside grid_dim) of the grid of every state row, each as
        a ready-made action (arcle_components_rows): rows int8 [M, >= L] (any stride / alignment; read only), or None = the resident
        envs.  Returns (count int32 [M, 2] = (written, left), comp int32 [M, C, 8] = x0, y0, x1, y1, sx, sy, colour, cells,
        bits uint8 [M, C, 128] | None), C = max_components: components in ascending row-major order of their first cell (sx, sy),
        the seed; the box inclusive, rows x / columns y as BBoxWrapper; cells of skip_color (-1: none) belong to no component; left =
        the cells no written component holds; comp[m, k >= written] is not written.  bits: the cells in the layout of step_bits.
        out: the tuple of a previous call with the same shapes to write into (captured graphs).  Nothing of the batch is touched."""
        C = int(max_components)
        if rows is None:
            M, ptr, stride = self.N, None, 0
        else:
            assert rows.dtype == torch.int8 and rows.dim() == 2 and rows.stride(1) == 1
            M, ptr, stride = int(rows.shape[0]), _ptr(rows), rows.stride(0)
        if out is None:
            dev = self.device
            out = (torch.zeros((M, 2), dtype=torch.int32, device=dev), torch.zeros((M, C, 8), dtype=torch.int32, device=dev),
                   torch.zeros((M, C, _lib.BITS_STRIDE), dtype=torch.uint8, device=dev) if bits else None)
        count, comp, mbits = out
        assert count.dtype == torch.int32 and tuple(count.shape) == (M, 2) and count.is_contiguous()
        assert comp.dtype == torch.int32 and tuple(comp.shape) == (M, C, 8) and comp.is_contiguous()
        assert (mbits is not None) == bool(bits) and (mbits is None or (mbits.dtype == torch.uint8 and tuple(mbits.shape) == (M, C, _lib.BITS_STRIDE) and mbits.is_contiguous()))
        self._check(self.L.arcle_components_rows(self._h, M, ptr, stride, C, int(skip_color), _ptr(count), _ptr(comp), _ptr(mbits), self._stream()),
                    "arcle_components_rows")
        return out

    def objects_rows(self, rows=None, max_components=32, skip_color=-1, any_color=False, diagonal=False, bits=False, colors=False, out=None):
        """`components_rows` under a chosen notion of "object" (arcle_objects_rows): any_color — every cell inside grid_dim that is not
        of skip_color may join, so an object may have several colours (skip_color -1: a full rectangle is one object); diagonal —
        8-connected.  Neither: the components of `components_rows`, output for output.  Returns (count, comp, bits | None, colors
        uint32-as-int32 [M, C] | None): everything as `components_rows` (comp[..., 6] is the SEED's colour); colors[m, k] has bit
        v & 31 set for every cell byte v of object k — for ARC's colours the set of colours present — and is not written for
        k >= written.  out: the 4-tuple of a previous call with the same shapes.  Nothing of the batch is touched."""
        C = int(max_components)
        if rows is None:
            M, ptr, stride = self.N, None, 0
        else:
            assert rows.dtype == torch.int8 and rows.dim() == 2 and rows.stride(1) == 1
            M, ptr, stride = int(rows.shape[0]), _ptr(rows), rows.stride(0)
        if out is None:
            dev = self.device
            out = (torch.zeros((M, 2), dtype=torch.int32, device=dev), torch.zeros((M, C, 8), dtype=torch.int32, device=dev),
                   torch.zeros((M, C, _lib.BITS_STRIDE), dtype=torch.uint8, device=dev) if bits else None,
                   torch.zeros((M, C), dtype=torch.int32, device=dev) if colors else None)
        count, comp, mbits, cols = out
        assert count.dtype == torch.int32 and tuple(count.shape) == (M, 2) and count.is_contiguous()
        assert comp.dtype == torch.int32 and tuple(comp.shape) == (M, C, 8) and comp.is_contiguous()
        assert (mbits is not None) == bool(bits) and (mbits is None or (mbits.dtype == torch.uint8 and tuple(mbits.shape) == (M, C, _lib.BITS_STRIDE) and mbits.is_contiguous()))
        assert (cols is not None) == bool(colors) and (cols is None or (cols.dtype == torch.int32 and tuple(cols.shape) == (M, C) and cols.is_contiguous()))
        mode = (_lib.OBJ_ANY_COLOR if any_color else 0) | (_lib.OBJ_DIAG if diagonal else 0)
        self._check(self.L.arcle_objects_rows(self._h, M, ptr, stride, C, int(skip_color), mode, _ptr(count), _ptr(comp), _ptr(mbits), _ptr(cols),
                                              self._stream()), "arcle_objects_rows")
        return out

    def place_rows(self, rows, count, bits, src_env=None, max_dist=None, out=None):
        """Where each object of every state row best fits the answer (arcle_place_rows): rows int8 [M, >= L] (any stride / alignment;
        read only) or None = the resident envs; count int32 [M, 2] or None (every row has C objects) and bits uint8 [M, C, 128] as
        `components_rows` / `objects_rows` return them; src_env int32 [M] = the env whose answer judges row m (None: env m); max_dist
        None: no limit on |dx| + |dy|.  Returns (place int32 [M, C, 4] = dx, dy, correct at the best translation, correct at (0, 0),
        base int32 [M, 2] = the dense pair of the row's own grid): the translation (dx rows down, dy columns right; the object's box
        stays inside grid_dim) whose Move macro — select the object, Move |dx| + |dy| times — scores the most correct cells, ties to
        the nearer one, then the smaller dx, then the smaller dy; entries k >= count are not written.  The definition:
        include/arcle_hip.h; its NumPy mirror: arcle_amd.search.place_numpy.  out: the pair of a previous call with the same shapes
        (captured graphs).  Nothing of the batch is touched."""
        assert bits.dtype == torch.uint8 and bits.dim() == 3 and bits.shape[2] == _lib.BITS_STRIDE and bits.is_contiguous()
        C = int(bits.shape[1])
        if rows is None:
            M, ptr, stride = int(bits.shape[0]), None, 0
        else:
            assert rows.dtype == torch.int8 and rows.dim() == 2 and rows.stride(1) == 1
            M, ptr, stride = int(rows.shape[0]), _ptr(rows), rows.stride(0)
        assert int(bits.shape[0]) == M
        assert count is None or (count.dtype == torch.int32 and tuple(count.shape) == (M, 2) and count.is_contiguous())
        assert src_env is None or (src_env.dtype == torch.int32 and tuple(src_env.shape) == (M,) and src_env.is_contiguous())
        if out is None:
            out = (torch.zeros((M, C, 4), dtype=torch.int32, device=self.device), torch.zeros((M, 2), dtype=torch.int32, device=self.device))
        place, base = out
        assert place.dtype == torch.int32 and tuple(place.shape) == (M, C, 4) and place.is_contiguous()
        assert base is None or (base.dtype == torch.int32 and tuple(base.shape) == (M, 2) and base.is_contiguous())
        D = 0x7fffffff if max_dist is None else int(max_dist)
        self._check(self.L.arcle_place_rows(self._h, M, ptr, stride, C, _ptr(count), _ptr(bits), _ptr(src_env), D, _ptr(place), _ptr(base),
                                            self._stream()), "arcle_place_rows")
        return out

    def stamp_rows(self, rows, count, bits, src_env=None, max_dist=None, blank=True, out=None):
        """Where a COPY of each object of every state row best fits the answer (arcle_stamp_rows): rows, count, bits, src_env and
        max_dist as for `place_rows`; blank = what the Paste of the caller's op table does (True: it writes the clip's whole
        rectangle, zeros included — paste_blank, both default tables; False: the clip's positive cells only).  Returns (stamp int32
        [M, C, 4] = px, py, correct(px, py), the object's cells inside grid_dim, base int32 [M, 2] = the dense pair of the row's own
        grid): the cell (px, py) inside grid_dim, within max_dist of the object's box corner (x0, y0), at which CopyO + Paste —
        copy the object, paste with the clip's top-left corner there; the stamp may hang over the bottom and right edges — scores
        the most correct cells, ties to the nearer one, then the smaller px - x0, then the smaller py - y0; entries k >= count are
        not written; an empty bit row gives (0, 0, base correct, 0).  The definition: include/arcle_hip.h; its NumPy mirror:
        arcle_amd.search.stamp_numpy.  out: the pair of a previous call with the same shapes (captured graphs).  Nothing of the
        batch is touched."""
        assert bits.dtype == torch.uint8 and bits.dim() == 3 and bits.shape[2] == _lib.BITS_STRIDE and bits.is_contiguous()
        C = int(bits.shape[1])
        if rows is None:
            M, ptr, stride = int(bits.shape[0]), None, 0
        else:
            assert rows.dtype == torch.int8 and rows.dim() == 2 and rows.stride(1) == 1
            M, ptr, stride = int(rows.shape[0]), _ptr(rows), rows.stride(0)
        assert int(bits.shape[0]) == M
        assert count is None or (count.dtype == torch.int32 and tuple(count.shape) == (M, 2) and count.is_contiguous())
        assert src_env is None or (src_env.dtype == torch.int32 and tuple(src_env.shape) == (M,) and src_env.is_contiguous())
        if out is None:
            out = (torch.zeros((M, C, 4), dtype=torch.int32, device=self.device), torch.zeros((M, 2), dtype=torch.int32, device=self.device))
        stamp, base = out
        assert stamp.dtype == torch.int32 and tuple(stamp.shape) == (M, C, 4) and stamp.is_contiguous()
        assert base is None or (base.dtype == torch.int32 and tuple(base.shape) == (M, 2) and base.is_contiguous())
        D = 0x7fffffff if max_dist is None else int(max_dist)
        self._check(self.L.arcle_stamp_rows(self._h, M, ptr, stride, C, _ptr(count), _ptr(bits), _ptr(src_env), D, int(bool(blank)),
                                            _ptr(stamp), _ptr(base), self._stream()), "arcle_stamp_rows")
        return out

    def turn_rows(self, rows, count, bits, src_env=None, max_dist=None, turns=31, out=None):
        """Where each object of every state row best fits the answer after a rotation or a flip (arcle_turn_rows): rows, count, bits,
        src_env and max_dist as for `place_rows`; turns = the set of turns asked for (bit t = slot t: Rotate 90, 180, 270, Flip H,
        Flip V; _lib.TURN_*).  Returns (turn int32 [M, C, 5, 4] = dx, dy, correct, valid per turn, base int32 [M, 2] = the dense
        pair of the row's own grid): per turn the translation (dx rows down, dy columns right, counted from where the turn leaves
        the freshly selected object; the turned tile stays inside grid_dim) at which select + turn + |dx| + |dy| Moves score the
        most correct cells, ties to the nearer one, then the smaller dx, then the smaller dy; valid = 0 (and zeros) where the turned
        tile fits nowhere within max_dist.  Slots of turns not asked for and entries k >= count are not written (zero in a fresh
        output).  The definition: include/arcle_hip.h; its NumPy mirror: arcle_amd.search.turn_numpy.  out: the pair of a previous
        call with the same shapes (captured graphs).  Nothing of the batch is touched."""
        assert bits.dtype == torch.uint8 and bits.dim() == 3 and bits.shape[2] == _lib.BITS_STRIDE and bits.is_contiguous()
        C = int(bits.shape[1])
        if rows is None:
            M, ptr, stride = int(bits.shape[0]), None, 0
        else:
            assert rows.dtype == torch.int8 and rows.dim() == 2 and rows.stride(1) == 1
            M, ptr, stride = int(rows.shape[0]), _ptr(rows), rows.stride(0)
        assert int(bits.shape[0]) == M
        assert count is None or (count.dtype == torch.int32 and tuple(count.shape) == (M, 2) and count.is_contiguous())
        assert src_env is None or (src_env.dtype == torch.int32 and tuple(src_env.shape) == (M,) and src_env.is_contiguous())
        if out is None:
            out = (torch.zeros((M, C, 5, 4), dtype=torch.int32, device=self.device), torch.zeros((M, 2), dtype=torch.int32, device=self.device))
        turn, base = out
        assert turn.dtype == torch.int32 and tuple(turn.shape) == (M, C, 5, 4) and turn.is_contiguous()
        assert base is None or (base.dtype == torch.int32 and tuple(base.shape) == (M, 2) and base.is_contiguous())
        D = 0x7fffffff if max_dist is None else int(max_dist)
        self._check(self.L.arcle_turn_rows(self._h, M, ptr, stride, C, _ptr(count), _ptr(bits), _ptr(src_env), D, int(turns),
                                           _ptr(turn), _ptr(base), self._stream()), "arcle_turn_rows")
        return out

    def mirror_rows(self, rows, count, bits, src_env=None, max_dist=None, mirrors=7, blank=True, out=None):
        """Each object's box filled from its mirror image (arcle_mirror_rows): rows, count, bits, src_env and max_dist as for
        `place_rows`; mirrors = the set of symmetries asked for (bit s = slot s: left-right H, up-down V, the point reflection;
        _lib.MIRROR_*); blank = what the table's Paste does (True: paste_blank, both default tables).  Returns (mirror int32 [M, C, 3,
        4] = dx, dy, correct, valid per symmetry, base int32 [M, 2] = the dense pair of the row's own grid): per symmetry the source
        rectangle — the object's box moved dx rows down and dy columns right, inside grid_dim; dx = 0 under H, dy = 0 under V — whose
        flipped copy, written over the box (CopyO + Paste + Flip), scores the most correct cells, ties to the nearer one, then the
        smaller dx, then the smaller dy.  Slots of symmetries not asked for and entries k >= count are not written (zero in a fresh
        output).  The definition: include/arcle_hip.h; its NumPy mirror: arcle_amd.search.mirror_numpy.  out: the pair of a previous
        call with the same shapes (captured graphs).  Nothing of the batch is touched."""
        assert bits.dtype == torch.uint8 and bits.dim() == 3 and bits.shape[2] == _lib.BITS_STRIDE and bits.is_contiguous()
        C = int(bits.shape[1])
        if rows is None:
            M, ptr, stride = int(bits.shape[0]), None, 0
        else:
            assert rows.dtype == torch.int8 and rows.dim() == 2 and rows.stride(1) == 1
            M, ptr, stride = int(rows.shape[0]), _ptr(rows), rows.stride(0)
        assert int(bits.shape[0]) == M
        assert count is None or (count.dtype == torch.int32 and tuple(count.shape) == (M, 2) and count.is_contiguous())
        assert src_env is None or (src_env.dtype == torch.int32 and tuple(src_env.shape) == (M,) and src_env.is_contiguous())
        if out is None:
            out = (torch.zeros((M, C, 3, 4), dtype=torch.int32, device=self.device), torch.zeros((M, 2), dtype=torch.int32, device=self.device))
        mirror, base = out
        assert mirror.dtype == torch.int32 and tuple(mirror.shape) == (M, C, 3, 4) and mirror.is_contiguous()
        assert base is None or (base.dtype == torch.int32 and tuple(base.shape) == (M, 2) and base.is_contiguous())
        D = 0x7fffffff if max_dist is None else int(max_dist)
        self._check(self.L.arcle_mirror_rows(self._h, M, ptr, stride, C, _ptr(count), _ptr(bits), _ptr(src_env), D, int(mirrors),
                                             int(bool(blank)), _ptr(mirror), _ptr(base), self._stream()), "arcle_mirror_rows")
        return out

    def align_rows(self, rows=None, src_env=None, max_dist=None, sources=3, blank=True, out=None):
        """The offset at which the grid or the input of every state row best fits the answer's canvas (arcle_align_rows): rows int8
        [M, >= L] state rows (None: the resident envs, M = N, or the length of src_env / of `out`), src_env and max_dist as for
        `place_rows`; sources = the set of sources asked for (_lib.ALIGN_GRID: slot 0, the row's grid; _lib.ALIGN_INPUT: slot 1, the
        row's input); blank = what the caller's Paste does (True: paste_blank).  Returns (align int32 [M, 2, 8] = ox, oy, correct,
        total, sh, sw, ah, aw per source, base int32 [M, 2] = the dense pair of the row's own grid): the offset at which [Copy of the
        source's rectangle the canvas covers, resize_grid to answer_dim, Paste] leaves the most correct cells, ties to the nearer
        one, then the smaller ox, then the smaller oy; total = ah * aw, the child's dense total; an all-zero (ox, oy, correct,
        total) where a dim is 0.  Slots of sources not asked for are not written (zero in a fresh output).  The definition:
        include/arcle_hip.h; its NumPy mirror: arcle_amd.search.align_numpy.  out: the pair of a previous call with the same shapes
        (captured graphs).  Nothing of the batch is touched."""
        if rows is None:
            M = int(out[0].shape[0]) if out is not None else int(src_env.shape[0]) if src_env is not None else self.N
            ptr, stride = None, 0
        else:
            assert rows.dtype == torch.int8 and rows.dim() == 2 and rows.stride(1) == 1
            M, ptr, stride = int(rows.shape[0]), _ptr(rows), rows.stride(0)
        assert src_env is None or (src_env.dtype == torch.int32 and tuple(src_env.shape) == (M,) and src_env.is_contiguous())
        if out is None:
            out = (torch.zeros((M, 2, 8), dtype=torch.int32, device=self.device), torch.zeros((M, 2), dtype=torch.int32, device=self.device))
        align, base = out
        assert align.dtype == torch.int32 and tuple(align.shape) == (M, 2, 8) and align.is_contiguous()
        assert base is None or (base.dtype == torch.int32 and tuple(base.shape) == (M, 2) and base.is_contiguous())
        D = 0x7fffffff if max_dist is None else int(max_dist)
        self._check(self.L.arcle_align_rows(self._h, M, ptr, stride, _ptr(src_env), D, int(sources), int(blank), _ptr(align), _ptr(base),
                                            self._stream()), "arcle_align_rows")
        return out

    def ray_rows(self, rows, count, bits, sets, free_color=0, through=False, src_env=None, best_bits=True, out=None):
        """The lines each object of every state row casts toward the answer (arcle_ray_rows): rows, count, bits and src_env as for
        `place_rows`; sets uint8 [S] on the device, 1 <= S <= 16 = one mask of directions per candidate (bit 0..7 = N, S, W, E, NW,
        NE, SW, SE: _lib.RAY_*; a zero entry is the empty candidate); free_color = the byte (as int8) of the cells a ray may enter;
        through = True: a ray runs over every cell outside the object to the edge of grid_dim.  Returns (ray int32 [M, C, S, 4] =
        color, correct, cells, right; best int32 [M, C, 4] = set, color, correct, cells; best_bits uint8 [M, C, 128] or None; base
        int32 [M, 2] = the dense pair of the row's own grid): per object and candidate the cells its rays cover — from the object's
        own cells through free cells up to the first obstacle or the edge —, the colour c in 0..9 for which ONE `Color c` step on
        them leaves the most correct cells (ties: the smaller c), that number and the cells of the answer the step gets right; per
        object the candidate with the most correct (then the fewest cells, then the lowest index; set = -1: every candidate is
        empty) and its cells as a bit row, the "bits" selection of `expand_rows` / `transition_rows`.  Entries k >= count are not
        written; an empty candidate gives (0, base correct, 0, 0).  The definition: include/arcle_hip.h; its NumPy mirror:
        arcle_amd.search.ray_numpy.  out: the four of a previous call with the same shapes (captured graphs; `sets` is read when
        the launch runs).  Nothing of the batch is touched."""
        assert bits.dtype == torch.uint8 and bits.dim() == 3 and bits.shape[2] == _lib.BITS_STRIDE and bits.is_contiguous()
        assert sets.dtype == torch.uint8 and sets.dim() == 1 and sets.is_contiguous() and sets.device == bits.device
        C, S = int(bits.shape[1]), int(sets.shape[0])
        if rows is None:
            M, ptr, stride = int(bits.shape[0]), None, 0
        else:
            assert rows.dtype == torch.int8 and rows.dim() == 2 and rows.stride(1) == 1
            M, ptr, stride = int(rows.shape[0]), _ptr(rows), rows.stride(0)
        assert int(bits.shape[0]) == M
        assert count is None or (count.dtype == torch.int32 and tuple(count.shape) == (M, 2) and count.is_contiguous())
        assert src_env is None or (src_env.dtype == torch.int32 and tuple(src_env.shape) == (M,) and src_env.is_contiguous())
        if out is None:
            out = (torch.zeros((M, C, S, 4), dtype=torch.int32, device=self.device), torch.zeros((M, C, 4), dtype=torch.int32, device=self.device),
                   torch.zeros((M, C, _lib.BITS_STRIDE), dtype=torch.uint8, device=self.device) if best_bits else None,
                   torch.zeros((M, 2), dtype=torch.int32, device=self.device))
        ray, best, bbits, base = out
        assert ray.dtype == torch.int32 and tuple(ray.shape) == (M, C, S, 4) and ray.is_contiguous()
        assert best.dtype == torch.int32 and tuple(best.shape) == (M, C, 4) and best.is_contiguous()
        assert bbits is None or (bbits.dtype == torch.uint8 and tuple(bbits.shape) == (M, C, _lib.BITS_STRIDE) and bbits.is_contiguous())
        assert base is None or (base.dtype == torch.int32 and tuple(base.shape) == (M, 2) and base.is_contiguous())
        self._check(self.L.arcle_ray_rows(self._h, M, ptr, stride, C, _ptr(count), _ptr(bits), _ptr(src_env), _ptr(sets), S, int(free_color),
                                          int(bool(through)), _ptr(ray), _ptr(best), _ptr(bbits), _ptr(base), self._stream()), "arcle_ray_rows")
        return out

    def region_rows(self, rows, count, bits, kinds, free_color=0, through=False, src_env=None, out=None, best_bits=True):
        """The cells around and inside each object of every state row (arcle_region_rows): rows, count, bits and src_env as for
        `place_rows`; kinds uint8 [S] on the device, 1 <= S <= 16 = one region code per candidate (_lib.REGION_*: 0 none, 1 HALO4,
        2 HALO8, 3 BOX_REST, 4 BOX_FRAME, 5 INSIDE, 6 BOX, 7 SELF; the array is read on the device when the launch runs, so a code
        above 7 is not refused: it counts as 0, the empty candidate); free_color = the byte (as int8) a cell outside the object must
        hold to be painted; through = True: every cell of the region is.  Returns (region int32 [M, C, S, 4] = color, correct, cells,
        right; best int32 [M, C, 4] = index, color, correct, cells; best_bits uint8 [M, C, 128] or None; base int32 [M, 2] = the
        dense pair of the row's own grid): per object and candidate the cells of the region, the colour c in 0..9 for which ONE
        `Color c` step on them leaves the most correct cells (ties: the smaller c), that number and the cells of the answer the step
        gets right; per object the candidate with the most correct (then the fewest cells, then the lowest index; index = -1: every
        candidate is empty) and its cells as a bit row, the "bits" selection of `expand_rows` / `transition_rows`.  Entries k >=
        count are not written; an empty candidate gives (0, base correct, 0, 0).  The definition: include/arcle_hip.h; its NumPy
        mirror: arcle_amd.search.region_numpy.  out: the four of a previous call with the same shapes (captured graphs; `kinds` is
        read when the launch runs).  Nothing of the batch is touched."""
        assert bits.dtype == torch.uint8 and bits.dim() == 3 and bits.shape[2] == _lib.BITS_STRIDE and bits.is_contiguous()
        assert kinds.dtype == torch.uint8 and kinds.dim() == 1 and kinds.is_contiguous() and kinds.device == bits.device
        C, S = int(bits.shape[1]), int(kinds.shape[0])
        if rows is None:
            M, ptr, stride = int(bits.shape[0]), None, 0
        else:
            assert rows.dtype == torch.int8 and rows.dim() == 2 and rows.stride(1) == 1
            M, ptr, stride = int(rows.shape[0]), _ptr(rows), rows.stride(0)
        assert int(bits.shape[0]) == M
        assert count is None or (count.dtype == torch.int32 and tuple(count.shape) == (M, 2) and count.is_contiguous())
        assert src_env is None or (src_env.dtype == torch.int32 and tuple(src_env.shape) == (M,) and src_env.is_contiguous())
        if out is None:
            out = (torch.zeros((M, C, S, 4), dtype=torch.int32, device=self.device), torch.zeros((M, C, 4), dtype=torch.int32, device=self.device),
                   torch.zeros((M, C, _lib.BITS_STRIDE), dtype=torch.uint8, device=self.device) if best_bits else None,
                   torch.zeros((M, 2), dtype=torch.int32, device=self.device))
        region, best, bbits, base = out
        assert region.dtype == torch.int32 and tuple(region.shape) == (M, C, S, 4) and region.is_contiguous()
        assert best.dtype == torch.int32 and tuple(best.shape) == (M, C, 4) and best.is_contiguous()
        assert bbits is None or (bbits.dtype == torch.uint8 and tuple(bbits.shape) == (M, C, _lib.BITS_STRIDE) and bbits.is_contiguous())
        assert base is None or (base.dtype == torch.int32 and tuple(base.shape) == (M, 2) and base.is_contiguous())
        self._check(self.L.arcle_region_rows(self._h, M, ptr, stride, C, _ptr(count), _ptr(bits), _ptr(src_env), _ptr(kinds), S, int(free_color),
                                             int(bool(through)), _ptr(region), _ptr(best), _ptr(bbits), _ptr(base), self._stream()), "arcle_region_rows")
        return out

    def scale_rows(self, rows=None, src_env=None, sources=3, modes=7, out=None, table=False, bits=True):
        """The grid or the input of every state row zoomed, shrunk or tiled onto the answer's canvas (arcle_scale_rows): rows, src_env
        and sources as for `align_rows`; modes = the set of candidate families asked for (_lib.SCALE_ZOOM | SCALE_SHRINK |
        SCALE_TILE).  Returns (scale int32 [M, 2, 8] = cand, correct, total, colours, sh, sw, ah, aw per source; table int32 [M, 2,
        132] or None = correct of every candidate, -1 for a mode not asked for; bits uint8 [M, 2, 9, 128] or None = the best child's
        cells of colour 1 .. 9 as bit rows; base int32 [M, 2] = the dense pair of the row's own grid): the candidate — index
        (kx - 1) * 8 + (ky - 1): every cell a kx x ky block; 64 + the same: the top-left cell of every kx x ky block; 128 + t: the
        source repeated, bit 0 / 1 of t mirroring every second tile column / row — whose child leaves the most correct cells, ties
        to the lowest index; total = ah * aw, the child's dense total; cand -1 and total 0 where a dim is 0.  Slots of sources not
        asked for are not written (zero in a fresh output).  The definition: include/arcle_scale_rows.h; its NumPy mirror:
        arcle_amd.search.scale_numpy.  out: the four of a previous call with the same shapes (captured graphs).  Nothing of the
        batch is touched."""
        if rows is None:
            M = int(out[0].shape[0]) if out is not None else int(src_env.shape[0]) if src_env is not None else self.N
            ptr, stride = None, 0
        else:
            assert rows.dtype == torch.int8 and rows.dim() == 2 and rows.stride(1) == 1
            M, ptr, stride = int(rows.shape[0]), _ptr(rows), rows.stride(0)
        assert src_env is None or (src_env.dtype == torch.int32 and tuple(src_env.shape) == (M,) and src_env.is_contiguous())
        if out is None:
            out = (torch.zeros((M, 2, 8), dtype=torch.int32, device=self.device),
                   torch.zeros((M, 2, _lib.SCALE_CANDS), dtype=torch.int32, device=self.device) if table else None,
                   torch.zeros((M, 2, 9, _lib.BITS_STRIDE), dtype=torch.uint8, device=self.device) if bits else None,
                   torch.zeros((M, 2), dtype=torch.int32, device=self.device))
        scale, tab, cbits, base = out
        assert scale.dtype == torch.int32 and tuple(scale.shape) == (M, 2, 8) and scale.is_contiguous()
        assert tab is None or (tab.dtype == torch.int32 and tuple(tab.shape) == (M, 2, _lib.SCALE_CANDS) and tab.is_contiguous())
        assert cbits is None or (cbits.dtype == torch.uint8 and tuple(cbits.shape) == (M, 2, 9, _lib.BITS_STRIDE) and cbits.is_contiguous())
        assert base is None or (base.dtype == torch.int32 and tuple(base.shape) == (M, 2) and base.is_contiguous())
        self._check(self.L.arcle_scale_rows(self._h, M, ptr, stride, _ptr(src_env), int(sources), int(modes), _ptr(scale), _ptr(tab), _ptr(cbits),
                                            _ptr(base), self._stream()), "arcle_scale_rows")
        return out

    def get_plane(self, name, out=None):
        """One key of the state dict as a dense [N, H, W] int8 array (device tensor, or a pinned host tensor passed as `out`):
        arcle_get_plane, a strided copy on the current stream."""
        if out is None:
            out = torch.empty((self.N, self.H, self.W), dtype=torch.int8, device=self.device)
        assert out.dtype == torch.int8 and out.is_contiguous() and out.numel() == self.N * self.P
        self._check(self.L.arcle_get_plane(self._h, PLANE_ID[name], _ptr(out), self._stream()), "arcle_get_plane")
        return out

    def set_plane(self, name, src):
        """The inverse: dense [N, H, W] int8 (device or pinned host) -> the plane (padding untouched); the caches derived from the
        state are dropped (arcle_invalidate)."""
        assert src.dtype == torch.int8 and src.is_contiguous() and src.numel() == self.N * self.P
        self._check(self.L.arcle_set_plane(self._h, PLANE_ID[name], _ptr(src), self._stream()), "arcle_set_plane")
        self.invalidate()

    def get_state(self):
        """Checkpoint of everything that defines the batch's future: a dict of CLONED device tensors (state planes incl. the task's
        input / answer, the per-env record, the counters, and — when a sampler is installed — the per-env episode numbers and
        current task indices).  `set_state` restores it; trajectories continue bit-identically."""
        st = {"planes": {k: v.clone() for k, v in self.planes.items()}, "rec": self.rec.clone(), "cnt": self.cnt.clone()}
        if hasattr(self, "episode"):
            st["episode"], st["cur_task"] = self.episode.clone(), self.cur_task.clone()
        return st

    def invalidate(self):
        """After editing state planes behind the library's back (plain tensor writes into `planes`): drop what the library derived
        from the old state (the dense-pair cache).  Rows kept by ARCLE_STEP_ROWS_INCREMENTAL must be rewritten by the caller."""
        self._check(self.L.arcle_invalidate(self._h, self._stream()), "arcle_invalidate")

    def set_state(self, st):
        self.invalidate()
        for k, v in st["planes"].items():
            self.planes[k].copy_(v)
        self.rec.copy_(st["rec"])
        self.cnt.copy_(st["cnt"])
        if "episode" in st and hasattr(self, "episode"):
            self.episode.copy_(st["episode"])
            self.cur_task.copy_(st["cur_task"])

    def packed_obs_size(self):
        return int(self.L.arcle_packed_obs_size(self._h))

    def packed_obs(self, out=None):
        """[N, R] uint8 rows = grid | grid_dim | reward (int32 LE) | terminated | padding, R = arcle_packed_obs_size()
        (912 for 30x30): the record a central learner gathers per step (one all-gather, arcle_amd.dist)."""
        R = self.L.arcle_packed_obs_size(self._h)
        if out is None:
            out = torch.empty((self.N, R), dtype=torch.uint8, device=self.device)
        assert out.shape == (self.N, R) and out.dtype == torch.uint8 and out.is_contiguous() and out.device == self.device
        self._check(self.L.arcle_pack_obs(self._h, _ptr(self.reward), _ptr(self.term), _ptr(out), self._stream()),
                    "arcle_pack_obs")
        return out

    def set_packed_output(self, out=None):
        """Installs the destination of STEP_PACK_OBS: every step call with that flag also writes `self.packed` ([N, R] uint8 rows
        grid | grid_dim | reward | terminated) from inside the step kernel — no packing launch before the multi-GPU gather.
        `out`: a caller-owned contiguous uint8 [N, R] device tensor (e.g. one slot of a double buffer); launches already enqueued
        keep writing where they were told to (parameters are taken by value per launch)."""
        if out is None:
            out = torch.empty((self.N, self.packed_obs_size()), dtype=torch.uint8, device=self.device)
        assert out.shape == (self.N, self.packed_obs_size()) and out.dtype == torch.uint8 and out.is_contiguous() and out.device == self.device
        self.packed = out
        self._check(self.L.arcle_set_packed_output(self._h, _ptr(self.packed)), "arcle_set_packed_output")
        return self.packed

    def packed_obs_ptr(self, out_ptr, stream=0):
        """Lowest-overhead form for rollout loops: raw device address of the [N, packed_obs_size()] uint8 output."""
        rc = self.L.arcle_pack_obs(self._h, self._reward_ptr, self._term_ptr, out_ptr, stream)
        if rc != 0:
            self._check(rc, "arcle_pack_obs")

    @staticmethod
    def unpack_obs(rows, H, W):
        """(grid int8 [M,H,W], grid_dim int8 [M,2], reward int32 [M], terminated bool [M]) views/copies of packed rows."""
        P = H * W
        grid = rows[:, :P].view(torch.int8).reshape(-1, H, W)
        gdim = rows[:, P:P + 2].view(torch.int8)
        rew = rows[:, P + 2:P + 6].contiguous().view(torch.int32).reshape(-1)
        term = rows[:, P + 6] != 0
        return grid, gdim, rew, term

    # ---- status / accounting ------------------------------------------------------------------
    def status(self, clear=True):
        s = ctypes.c_uint32(0)
        self._check(self.L.arcle_get_status(self._h, ctypes.byref(s), int(clear), self._stream()), "arcle_get_status")
        return s.value

    def enable_accounting(self, on=True):
        self._check(self.L.arcle_enable_accounting(self._h, int(on)), "arcle_enable_accounting")

    def accounting_ex(self, clear=True):
        """(algorithmic bytes, issued bytes, env-steps) since the last clear — arcle_get_accounting_ex."""
        b, i, s = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self.L.arcle_get_accounting_ex(self._h, ctypes.byref(b), ctypes.byref(i), ctypes.byref(s), int(clear), self._stream()),
                    "arcle_get_accounting_ex")
        return b.value, i.value, s.value

    def accounting(self, clear=True):
        b, s = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self.L.arcle_get_accounting(self._h, ctypes.byref(b), ctypes.byref(s), int(clear), self._stream()),
                    "arcle_get_accounting")
        return b.value, s.value
