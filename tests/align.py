"""Backend-independent checks of arcle_align_rows (the offset at which the grid or the input of a state row best fits the answer's
canvas).  The counterpart of tests/turn.py; it takes tests/place.py's env arrangement (envs_for), guards and SENTINEL: every check takes
a backend — EmuAlign (tests/emu/align_emu.cpp: the kernel body of arcle_align.h lock-step on the CPU) or HipAlign (the product) — and
returns a list of mismatch strings.  The reference point is arcle_amd.search.align_numpy, which builds every child grid from the
definition and which tests/test_align_host.py pins on the oracle's own Copy + resize_grid + Paste."""
import ctypes
import os
import subprocess

import numpy as np

import backends as B
import components as CP
import place as PL
import stamp as ST
from arcle_amd import search as S
from oracle import oracle as O

EMU_DIR = CP.EMU_DIR
EMU_SRC = os.path.join(EMU_DIR, "align_emu.cpp")
EMU_HDRS = PL.EMU_HDRS + [os.path.join(B.ROOT, "arcle_amd", "csrc", f) for f in ("arcle_stamp.h", "arcle_align.h")]
SENTINEL = PL.SENTINEL
LARGE = PL.LARGE
DISTS = PL.DISTS
SIZES = PL.SIZES
ORACLE_SIZES = ((5, 5), (7, 6), (6, 9))
# per env kind: (Copy_O, Copy_I), resize_grid, Paste in the default table (O2ARCv2Env: o2arcenv.py:102-109)
ALIGN_OPS = {"o2arc": ((29, 28), 33, 30), "arc": ((21, 20), 25, 22)}
SOURCE_NAMES = ("grid", "input")
ops_for = ST.ops_for  # (the kind's default table; blank False: its Paste without paste_blank)


def child_of(src, sh, sw, ah, aw, ox, oy, blank=True):
    """G'(ox, oy) on the whole plane, cell by cell from the definition of include/arcle_hip.h — used to build ANSWERS and to describe
    cases only (the mirror under test is align_numpy, which clips and pastes, and the oracle settles the rule in
    tests/test_align_host.py)"""
    H, W = src.shape
    out = np.zeros((H, W), np.int8)
    for i in range(ah):
        for j in range(aw):
            x, y = i + ox, j + oy
            if 0 <= x < sh and 0 <= y < sw and (blank or src[x, y] > 0):
                out[i, j] = src[x, y]
    return out


# ---- the cases: a grid, an input, an answer and their dims ---------------------------------------------------------------------------
_cases = {}


def cases_of(H, W):
    """Per size (a case that a size has no room for is left out; `want` = the offsets a case was built for, per source slot):
      window grid       the answer is a window of the grid (random colours 1 .. 9: the window is unique), the input is noise
      window input      the answer is a window of the input; the grid is wrecked (all zero)
      embed             the source is smaller than the answer on both axes: it sits somewhere on a blank canvas (ox, oy <= 0)
      embed one axis    ... smaller on the rows only, wider than the answer on the columns
      cross a / b       a planted best offset with ox < 0 < oy / with oy < 0 < ox
      junk              source dims below (H, W), the plane full of bytes outside them that WOULD complete the answer if read
      negative          negative bytes in the source and in the answer: blank = 1 carries them over, blank = 0 turns them into 0,
                        which matches the answer's zeros
      foreign bit       an answer colour (8) with a bit no source byte has
      zero source       all-zero sources: every offset ties, the rule picks (0, 0)
      1x1 answer        answer_dim (1, 1)
      1x1 source        source dims (1, 1) under an answer of the plane's full size: the largest offset range
      zero dim a / b / c   grid_dim with a 0, input_dim with a 0, answer_dim with a 0: no candidate
      tie distance / ox / oy / ox before oy   periodic stripes, one tie per level of the tie rule, TIE_WANT = the offset the rule names"""
    if (H, W) in _cases:
        return _cases[(H, W)]
    rng = np.random.default_rng(5000 + 131 * H + W)
    out = []

    def add(name, grid, dim, inp, idim, answer, adim, want=None):
        out.append({"name": f"{H}x{W} {name}", "H": H, "W": W, "grid": np.asarray(grid).astype(np.int8), "dim": np.asarray(dim, np.int8),
                    "inp": np.asarray(inp).astype(np.int8), "idim": np.asarray(idim, np.int8), "answer": np.asarray(answer).astype(np.int8),
                    "adim": np.asarray(adim, np.int8), "want": want or {}})

    def noise():
        return rng.integers(1, 10, (H, W))

    def on_canvas(a, h, w):
        c = np.zeros((H, W), np.int8)
        c[:h, :w] = a[:h, :w]
        return c
    full, zero = (H, W), np.zeros((H, W), np.int8)
    ah, aw = (H + 1) // 2, (W + 1) // 2
    g = noise()
    x, y = int(rng.integers(0, H - ah + 1)), int(rng.integers(0, W - aw + 1))
    add("window grid", g, full, noise(), full, on_canvas(g[x:, y:], ah, aw), (ah, aw), {0: (x, y)})
    g = noise()
    x, y = int(rng.integers(0, H - ah + 1)), int(rng.integers(0, W - aw + 1))
    add("window input", zero, full, g, full, on_canvas(g[x:, y:], ah, aw), (ah, aw), {1: (x, y)})
    if H >= 2 and W >= 2:
        sh, sw = H // 2, W // 2
        g = on_canvas(noise(), sh, sw)
        x, y = int(rng.integers(0, H - sh + 1)), int(rng.integers(0, W - sw + 1))
        add("embed", g, (sh, sw), g, (sh, sw), child_of(g, sh, sw, H, W, -x, -y), full, {0: (-x, -y), 1: (-x, -y)})
        g = noise()
        g[sh:] = 0
        x, y = int(rng.integers(1, H - sh + 1)), int(rng.integers(0, W - aw + 1))
        add("embed one axis", g, (sh, W), g, (sh, W), child_of(g, sh, W, H, aw, -x, y), (H, aw), {0: (-x, y), 1: (-x, y)})
        g = noise()
        add("cross a", g, full, zero, full, child_of(g, H, W, H, W, -1, 1), full, {0: (-1, 1)})
        g = noise()
        add("cross b", zero, full, g, full, child_of(g, H, W, H, W, 1, -1), full, {1: (1, -1)})
    if H >= 2 or W >= 2:
        dh, dw = int(H >= 2), int(W >= 2)
        g = noise()
        add("junk", g, (H - dh, W - dw), g, (H - dh, W - dw), on_canvas(g[dh:, dw:], H - dh, W - dw), (H - dh, W - dw))
    g = rng.choice([-128, -3, -1, 0, 3, 5, 127], (H, W))
    g.flat[0], g.flat[-1] = -1, -3
    a = g.copy()
    a.flat[np.flatnonzero(g < 0)[1::2]] = 0  # (every other negative byte of the source meets a zero of the answer)
    add("negative", g, full, g, full, a, full)
    g = rng.integers(0, 4, (H, W))
    a = np.where(rng.random((H, W)) < 0.3, 8, g)
    add("foreign bit", g, full, rng.integers(0, 4, (H, W)), full, a, full)
    add("zero source", zero, full, zero, full, rng.choice([0, 0, 3], (H, W)), full, {0: (0, 0), 1: (0, 0)})
    add("1x1 answer", noise(), full, noise(), full, on_canvas(noise(), 1, 1), (1, 1))
    add("1x1 source", noise(), (1, 1), noise(), (1, 1), rng.choice([0, 3, 5], (H, W)), full)
    add("zero dim a", noise(), (0, W), noise(), full, noise(), full)
    add("zero dim b", noise(), full, noise(), (H, 0), noise(), full)
    add("zero dim c", noise(), full, noise(), full, noise(), (0, W))
    ii, jj = np.mgrid[:H, :W]
    if H >= 4:  # horizontal stripes of period 2, the answer a window of the other phase: perfect at ox = 1 and at ox = 3
        g = 1 + ii % 2
        add("tie distance", g, full, g, full, on_canvas(1 + (ii + 1) % 2, H - 3, W), (H - 3, W), {0: (1, 0), 1: (1, 0)})
    if H >= 2:  # ... the answer of the plane's size: (-1, 0) and (1, 0) both lose one row
        g = 1 + ii % 2
        add("tie ox", g, full, g, full, 1 + (ii + 1) % 2, full, {0: (-1, 0), 1: (-1, 0)})
    if W >= 2:  # vertical stripes: (0, -1) and (0, 1) both lose one column
        g = 1 + jj % 2
        add("tie oy", g, full, g, full, 1 + (jj + 1) % 2, full, {0: (0, -1), 1: (0, -1)})
    if H >= 2 and W >= 2:  # a checkerboard, the answer a window of the other phase: perfect at (0, 1) and at (1, 0)
        g = 1 + (ii + jj) % 2
        add("tie ox before oy", g, full, g, full, on_canvas(1 + (ii + jj + 1) % 2, H - 1, W - 1), (H - 1, W - 1), {0: (0, 1), 1: (0, 1)})
    _cases[(H, W)] = out
    return out


TIE_NAMES = ("tie distance", "tie ox", "tie oy", "tie ox before oy")
_mirror = {}


def mirror(case, dist, blank):
    """align_numpy of a case with both sources, computed once per (case, max_dist, blank): (align [2, 8], base (2,))"""
    key = (case["name"], dist, bool(blank))
    if key not in _mirror:
        _mirror[key] = S.align_numpy(case["grid"], case["dim"], case["inp"], case["idim"], case["answer"], case["adim"],
                                     None if dist >= LARGE else dist, 3, blank)
    return _mirror[key]


def make_rows(kind, cases, rng):
    """State rows of env kind `kind` whose grid / grid_dim / input / input_dim are the cases'; every other byte random."""
    H, W = cases[0]["H"], cases[0]["W"]
    lay = B.row_layout(kind, H * W)
    rows = rng.integers(-128, 128, (len(cases), sum(ln for _, ln in lay))).astype(np.int8)
    off = 0
    for f, ln in lay:
        key = {"grid": "grid", "grid_dim": "dim", "input": "inp", "input_dim": "idim"}.get(f)
        if key:
            rows[:, off:off + ln] = np.stack([c[key].reshape(-1) for c in cases])
        off += ln
    return rows


# ---- the backends -----------------------------------------------------------------------------------------------------------------
class _AlignParams(ctypes.Structure):  # mirror of arcle::AlignParams (arcle_amd/csrc/arcle_align.h)
    _fields_ = [("p", B._StepParams), ("max_dist", ctypes.c_int32), ("sources", ctypes.c_uint32), ("src_env", ctypes.c_void_p),
                ("align", ctypes.c_void_p), ("base", ctypes.c_void_p), ("blank", ctypes.c_int32), ("pad_", ctypes.c_int32)]


_emu = None


def emu_lib():
    global _emu
    if _emu is None:
        so = os.path.join(EMU_DIR, "libalign_emu.so")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [EMU_SRC] + EMU_HDRS):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, EMU_SRC])
        _emu = ctypes.CDLL(so)
        _emu.align_emu_run.argtypes = [ctypes.POINTER(_AlignParams), ctypes.c_int]
        assert _emu.align_emu_params_size() == ctypes.sizeof(_AlignParams), "AlignParams layout drifted"
    return _emu


class EmuAlign:
    """The emulated kernel.  fw: -1 = the instantiation the library launches for the width, 0 = FW_GENERIC at any width."""
    BACKEND = B.EmuBackend  # (a subclass may name a backend of another plane stride)
    name = "emu"

    def __init__(self, fw=-1):
        self.fw = fw

    def run(self, kind, H, W, cases, layout, dist, with_src, with_base, sources, blank, rng):
        M = len(cases)
        resident = layout == "resident"
        N, ans, adim, src, bad = PL.envs_for(cases, resident, with_src, rng)
        be = self.BACKEND(N, H, W, 3, kind, CP.OPS[kind]())
        for k in be.buf:
            be.buf[k][:] = 0x55
        be.rec[:] = 0x55
        be.buf["answer"][:, :H * W] = ans.reshape(N, -1)
        be.rec[:, 14:16] = adim
        x = _AlignParams()
        p = be._params()
        p.n_resident, p.n_envs = N, M
        if resident:
            be.buf["grid"][:M, :H * W] = np.stack([c["grid"].reshape(-1) for c in cases])
            be.buf["input"][:M, :H * W] = np.stack([c["inp"].reshape(-1) for c in cases])
            be.rec[:M, 0:2] = np.stack([c["idim"] for c in cases])
            be.rec[:M, 2:4] = np.stack([c["dim"] for c in cases])
            p.rows_in, p.rows_in_stride = None, 0
        else:
            buf, offset, stride = CP.place(make_rows(kind, cases, rng), layout)
            p.rows_in, p.rows_in_stride = buf.ctypes.data + offset, stride
        x.p = p
        self.guards = [PL._guarded((M, 2, 8)), PL._guarded((M, 2))]
        (_, align), (_, base) = self.guards
        x.max_dist, x.sources, x.blank = min(dist, 2048), sources, int(blank)
        x.src_env = None if src is None else src.ctypes.data
        x.align, x.base = align.ctypes.data, base.ctypes.data if with_base else None
        rc = emu_lib().align_emu_run(ctypes.byref(x), self.fw)
        assert rc == 0, f"align emulator reported error {rc} (divergent cross-lane op / non-uniform value)"
        return align, base, bad

    def guards_intact(self):
        return all((buf[:16] == SENTINEL).all() and (buf[-16:] == SENTINEL).all() for buf, _ in self.guards)


class HipAlign:
    """EnvBatch.align_rows on the device."""
    PLANE_STRIDE = None  # override, as HipBackend's: passed on as EnvBatch(plane_stride=)
    name = "hip"

    def __init__(self):
        import torch
        self.t = torch
        self._b = {}

    def batch(self, kind, H, W, N):
        from arcle_amd.engine import EnvBatch
        key = (kind, H, W, N)
        if key not in self._b:
            self._b[key] = EnvBatch(N, H, W, 3, kind, plane_stride=self.PLANE_STRIDE)
            self._b[key].set_op_table(CP.OPS[kind]())
        return self._b[key]

    def run(self, kind, H, W, cases, layout, dist, with_src, with_base, sources, blank, rng):
        t = self.t
        M = len(cases)
        resident = layout == "resident"
        N, ans, adim, src, bad = PL.envs_for(cases, resident, with_src, rng)
        b = self.batch(kind, H, W, N)
        b.plane("answer").copy_(t.as_tensor(ans, device=b.device))
        b.field("answer_dim").copy_(t.as_tensor(adim, device=b.device))
        rows = make_rows(kind, cases, rng)
        if resident:
            b.set_state_rows(t.as_tensor(rows, device=b.device))
            view = None
        else:
            buf, offset, stride = CP.place(rows, layout)
            dbuf = t.as_tensor(buf, device=b.device)  # (exactly the bytes of the rows: the last row ends the allocation)
            view = t.as_strided(dbuf, (M, rows.shape[1]), (stride, 1), offset)
        na = M * 16
        guard = t.full((na + M * 2 + 48,), SENTINEL, dtype=t.int32, device=b.device)
        align, base = guard[16:16 + na].view(M, 2, 8), guard[32 + na:32 + na + 2 * M].view(M, 2)
        b.align_rows(view, None if src is None else t.as_tensor(src, device=b.device), None if dist >= LARGE else dist, sources, blank,
                     out=(align, base if with_base else None))
        g = guard.cpu().numpy()
        self._ok = bool((g[:16] == SENTINEL).all() and (g[16 + na:32 + na] == SENTINEL).all() and (g[32 + na + 2 * M:] == SENTINEL).all())
        return align.cpu().numpy(), base.cpu().numpy(), bad

    def guards_intact(self):
        return self._ok


def compare(tag, got, cases, dist, with_base, sources, blank):
    """Everything exact: the eight words of every slot asked for, the base pair, SENTINEL in the slots not asked for and in an absent
    base."""
    align, base, bad = got
    errs = []
    for m, c in enumerate(cases):
        wa, wb = mirror(c, dist, blank)
        t = f"{tag} row {m} ({c['name']})"
        if m in bad:
            wa, wb = np.zeros_like(wa), (0, 0)
        for s in range(2):
            if (sources >> s) & 1:
                if not np.array_equal(align[m, s], wa[s]):
                    errs.append(f"{t}: {SOURCE_NAMES[s]} {align[m, s].tolist()} != {wa[s].tolist()}")
            elif (align[m, s] != SENTINEL).any():
                errs.append(f"{t}: the {SOURCE_NAMES[s]} slot was written though not asked for")
        if with_base and tuple(int(v) for v in base[m]) != tuple(wb):
            errs.append(f"{t}: base {base[m].tolist()} != {tuple(wb)}")
        if not with_base and (base[m] != SENTINEL).any():
            errs.append(f"{t}: base was written though not asked for")
    return errs


# size -> the runs of one backend: (kind, layout | "resident", M, max_dist, src given, base asked for, sources, blank).  Per size: every
# env kind (the offsets of grid and input differ), the three layouts and the resident form, M = 1 and 37 (None: one row per case; a
# string or a tuple of strings: the cases whose name ends with one), every max_dist of DISTS, sources 1, 2 and 3, both Pastes, src and NULL.  The emulator
# walks a row board's passes lane by lane and a flat board's offsets one by one, so its unlimited runs take one row per case (and few
# cases on the flat board); `full` (the device) adds every case without a limit under both Pastes.
def plan(H, W, full=False):
    if W > 32 or H > 64:
        runs = [("o2arc", "odd", None, 3, True, True, 3, True), ("arc", "dense", None, 1, False, True, 1, False),
                ("raw", "lib", 1, 0, False, False, 2, True), ("raw", "resident", None, 1, True, True, 3, False),
                ("o2arc", "lib", 37, 1, True, True, 2, True), ("arc", "resident", "negative", LARGE, False, True, 3, True),
                ("o2arc", "dense", 37, 1, True, False, 1, True), ("o2arc", "odd", "tie oy", LARGE, False, True, 3, False)]
        return runs + ([("o2arc", "lib", None, LARGE, True, True, 3, True), ("arc", "lib", None, LARGE, True, True, 3, False)] if full else [])
    # (an emulated row of a large row board with no limit costs seconds: there the unlimited run takes the cases whose offsets reach
    # furthest, and every case runs within 3)
    every = None if full or H * W <= 400 else ("window input", "embed one axis", "cross a", "junk", "1x1 source", "tie ox")
    runs = [("o2arc", "odd", every, LARGE, True, True, 3, True)] + ([("o2arc", "odd", None, 3, True, True, 3, True)] if every else [])
    runs += [("arc", "dense", None, 3, False, True, 1, False),
            ("raw", "lib", 1, 0, False, False, 2, True), ("raw", "resident", None, 1, True, True, 3, False),
            ("o2arc", "lib", 37, 3, True, True, 2, True), ("arc", "resident", "negative", LARGE, False, True, 3, False),
            ("o2arc", "dense", 37, 1, True, False, 1, True)]
    return runs + ([("arc", "lib", None, LARGE, True, True, 3, False)] if full else [])


def run_size(be, H, W, runs=None, full=False):
    runs = runs or plan(H, W, full)
    errs = []
    rng = np.random.default_rng(H * 1000 + W)
    for i, (kind, layout, M, dist, with_src, with_base, sources, blank) in enumerate(runs):
        cases = cases_of(H, W)
        if isinstance(M, (str, tuple)):
            cases = [c for c in cases if c["name"].endswith(M)] or cases[:1]
        elif M is not None:
            cases = PL.pad_to(cases, M) if M > 1 else cases[i % len(cases):][:1]
        tag = f"{be.name} {H}x{W} {kind} {layout} dist={dist} src={with_src} sources={sources} blank={blank}"
        got = be.run(kind, H, W, cases, layout, dist, with_src, with_base, sources, blank, rng)
        errs += compare(tag, got, cases, dist, with_base, sources, blank)
        if not be.guards_intact():
            errs.append(f"{tag}: bytes around an output buffer were written")
        if len(errs) > 10:
            break
    return errs


# ---- the oracle's side: Copy on R, resize_grid on the canvas rectangle, Paste on P ---------------------------------------------------
def case_rows(case, kind="o2arc"):
    """The state row of a freshly reset env whose input is the case's, with the case's grid and grid_dim written over the grid's -> rows [1, L]"""
    H, W = case["H"], case["W"]
    rows, _ = CP.clean_rows(kind, case["inp"][None], case["idim"][None], case["answer"][None], case["adim"][None])
    off = 0
    for f, ln in B.row_layout(kind, H * W):
        if f == "grid":
            rows[:, off:off + ln] = case["grid"].reshape(1, -1)
        elif f == "grid_dim":
            rows[:, off:off + ln] = case["dim"]
        off += ln
    return rows


def align_macro_set(case, kind, table):
    """Every candidate (source, ox, oy) of a case (from align_numpy's table: its -1 entries are outside T) as the three-step macro of
    include/arcle_hip.h on int8 masks, one flat set -> (cand int [K, 3] = (s, ox, oy), masks int8 [K, 3, H * W], op int32 [K, 3])"""
    H, W = case["H"], case["W"]
    copy_ops, resize_op, paste_op = ALIGN_OPS[kind]
    ah, aw = (min(int(v), n) for v, n in zip(case["adim"], (H, W)))
    cand = np.argwhere(table >= 0) - (0, H - 1, W - 1)
    K = len(cand)
    masks, op = np.zeros((K, 3, H, W), np.int8), np.zeros((K, 3), np.int32)
    for j, (s, ox, oy) in enumerate(cand):
        sh, sw = (max(min(int(v), n), 0) for v, n in zip(case["idim"] if s else case["dim"], (H, W)))
        masks[j, 0, max(ox, 0):min(sh, ah + ox), max(oy, 0):min(sw, aw + oy)] = 1
        masks[j, 1, :ah, :aw] = 1
        masks[j, 2, max(-ox, 0), max(-oy, 0)] = 1
        op[j] = (copy_ops[s], resize_op, paste_op)
    return cand, masks.reshape(K, 3, H * W), op


def oracle_children(case, kind, blank):
    """Every candidate's macro on the ORACLE (tests/macros.py's chained oracle, mask ingress, the kind's default table or the one whose
    Paste has no paste_blank) beside the mirror -> list of (cand (s, ox, oy), the oracle's grid, grid_dim and dense pair, the mirror's
    child grid and correct count)."""
    import macros as MC
    import search_bits as SB
    H, W = case["H"], case["W"]
    rows = case_rows(case, kind)
    _, _, table, children = S.align_numpy(case["grid"], case["dim"], case["inp"], case["idim"], case["answer"], case["adim"], None, 3, blank, full=True)
    cand, masks, op = align_macro_set(case, kind, table)
    K = len(cand)
    if not K:
        return []
    w = MC.oracle_macros(rows, case["answer"][None], case["adim"][None], kind, H, W, 3, ops_for(kind, blank), "mask", masks[None], op[None],
                         np.full((1, K), 3, np.int32))
    assert not w["status"].any(), case["name"]
    grids, gdims = SB._grids_of(w["rows"][0], kind, H, W)
    return [((int(s), int(ox), int(oy)), grids[j], gdims[j], w["dense"][0, j], children[s, ox + H - 1, oy + W - 1], int(table[s, ox + H - 1, oy + W - 1]))
            for j, (s, ox, oy) in enumerate(cand)]


# ---- planted tasks: the answer has another size than the grid --------------------------------------------------------------------
def planted_align_tasks(H=12, W=12, seed=52):
    """Eight tasks -> (inputs [8, H, W], idims [8, 2], answers [8, H, W], adims [8, 2], kinds, the planted (source slot, ox, oy)):
    three "window": the answer is a 4 x 5 window of the 10 x 10 grid, a block of random colours among distractor blocks; three "embed":
    the answer is the 5 x 4 input on a larger blank canvas at an offset; two "wiped": the answer is a window of the input, and the task
    starts after reset_grid has wiped the grid (the rows' grid is all zero: only Copy_I can help)."""
    rng = np.random.default_rng(seed)
    inputs, idims, answers, adims, kinds, plans = [], [], [], [], [], []
    for i in range(8):
        kind = ("window", "embed", "wiped")[(i >= 3) + (i >= 6)]
        g, a = np.zeros((H, W), np.int8), np.zeros((H, W), np.int8)
        if kind == "embed":
            sh, sw, ah, aw = 5, 4, int(rng.integers(7, 11)), int(rng.integers(7, 11))
            g[:sh, :sw] = rng.integers(1, 10, (sh, sw))
            x, y = int(rng.integers(1, ah - sh + 1)), int(rng.integers(1, aw - sw + 1))
            a[:ah, :aw] = child_of(g, sh, sw, ah, aw, -x, -y)[:ah, :aw]
            plan_ = (0, -x, -y)
        else:
            sh, sw, ah, aw = 10, 10, 4, 5
            g[:sh, :sw] = rng.integers(1, 10, (sh, sw)) * (rng.random((sh, sw)) < 0.7)
            x, y = int(rng.integers(1, sh - ah + 1)), int(rng.integers(1, sw - aw + 1))
            g[x:x + ah, y:y + aw] = rng.integers(1, 10, (ah, aw))
            a[:ah, :aw] = g[x:x + ah, y:y + aw]
            plan_ = (int(kind == "wiped"), x, y)
        inputs.append(g), idims.append((sh, sw)), answers.append(a), adims.append((ah, aw)), kinds.append(kind), plans.append(plan_)
    return np.stack(inputs), np.array(idims, np.int8), np.stack(answers), np.array(adims, np.int8), kinds, plans


def planted_rows(inputs, idims, answers, adims, kinds):
    """The tasks' start rows: freshly reset O2ARC envs; the "wiped" tasks one reset_grid later (op 32 on the oracle) -> rows [8, L]"""
    rows, orc = CP.clean_rows("o2arc", inputs, idims, answers, adims)
    H, W = inputs.shape[1:]
    wiped = np.array([k == "wiped" for k in kinds])
    sel = np.zeros((len(kinds), H, W), np.int8)
    op = np.where(wiped, 32, 34).astype(np.int32)  # (the others would Submit: their rows are taken from before the step)
    orc.step("mask", sel, op)
    after = B.state_rows(orc)
    rows[wiped] = after[wiped]
    return rows


def perfect_offsets(inp, idim, grid, gdim, ans, adim, blank=True):
    """The (source slot, ox, oy) whose child IS the answer, by the mirror's table"""
    align, _, table, _ = S.align_numpy(grid, gdim, inp, idim, ans, adim, None, 3, blank, full=True)
    H, W = grid.shape
    total = int(align[0, 3])
    return [tuple(int(v) for v in c - (0, H - 1, W - 1)) for c in np.argwhere(table == total)] if total else []


def align_numpy_rows(grids, gdims, inps, idims, answers, adims, max_dist, sources, blank):
    """`ARCVecEnv.align` of M states from align_numpy, on torch CPU tensors (the stub vec envs' `align`)."""
    import torch
    from arcle_amd.envs.vec import Alignments
    M = len(grids)
    al, base = np.zeros((M, 2, 8), np.int32), np.zeros((M, 2), np.int32)
    for m in range(M):
        al[m], base[m] = S.align_numpy(grids[m], gdims[m], inps[m], idims[m], answers[m], adims[m], max_dist, sources, blank)
    t = torch.from_numpy(al)
    return Alignments(t[..., 0], t[..., 1], t[..., 2], t[..., 3], t[..., 4:6], t[..., 6:8], torch.from_numpy(base))


def _field_of(rows, kind, H, W, name):
    off = 0
    for f, ln in B.row_layout(kind, H * W):
        if f == name:
            return rows[:, off:off + ln]
        off += ln


def align_venv(answers, adims, H=12, W=12):
    """The oracle-backed stub vec env of tests/place.py + `align` (align_numpy): what beam_search(propose=propose_alignments(...))
    needs, on torch CPU tensors."""
    base = type(PL.place_venv(answers, adims, H, W))

    class AlignVenv(base):
        def align(self, rows, src_env=None, max_dist=None, sources=3, blank=True):
            r = rows.numpy()
            src = np.arange(len(r)) if src_env is None else src_env.numpy()
            return align_numpy_rows(_field_of(r, self.kind, H, W, "grid").reshape(-1, H, W), _field_of(r, self.kind, H, W, "grid_dim"),
                                    _field_of(r, self.kind, H, W, "input").reshape(-1, H, W), _field_of(r, self.kind, H, W, "input_dim"),
                                    self.answers[src], self.adims[src], max_dist, sources, blank)
    return AlignVenv("o2arc", H, W, 3, O.o2arc_ops(), answers, adims)


def replay_on_oracle(row, ans, adim, seq, kind="o2arc"):
    """The (selection, op) sequence on the oracle from the state in `row` -> 1 if no step raised a status bit and the grid and grid_dim
    it leaves are the answer's, else 0"""
    import search as SR
    H, W = ans.shape
    orc = SR.oracle_from_rows(row[None], ans[None], adim[None], kind, H, W, 3, O.o2arc_ops())
    for sel, op in seq:
        assert sel.dtype == bool and sel.shape == (H, W)
        orc.step("mask", sel[None].astype(np.int8), np.array([op], np.int32))
    gd = orc.get("grid_dim")[0]
    return int(not orc.status() and np.array_equal(gd, adim) and np.array_equal(orc.get("grid")[0][:gd[0], :gd[1]], ans[:gd[0], :gd[1]]))


def searches(venv, rows, n, before=True):
    """-> (the results of propose_alignments at width 1 and depth 1 on every task, {name: the results of the proposers the library had
    at the same width and depth} — empty with before=False)"""
    import torch

    def one(prop):
        return [S.beam_search(venv, rows[i:i + 1], None, width=1, depth=1, src_env=torch.tensor([i]), propose=prop) for i in range(n)]
    aligned = one(S.propose_alignments(*ALIGN_OPS["o2arc"]))
    if not before:
        return aligned, {}
    return aligned, {"objects": one(S.propose_objects(list(PL.MOVE_OPS) + [29], list(range(10, 20)), masks=True, any_color=True, diagonal=True)),
                     "placements": one(S.propose_placements(PL.MOVE_OPS, any_color=True, diagonal=True)),
                     "stamps": one(S.propose_stamps(29, 30, any_color=True, diagonal=True)),
                     "turns": one(S.propose_turns((24, -1, 25, 26, 27), PL.MOVE_OPS, any_color=True, diagonal=True))}


# ---- one dumped case for the standalone sanitized emulator ------------------------------------------------------------------------
MAGIC = 0x414c474e


def dump_case(path, kind, H, W, cases, layout, dist, with_src, with_base, sources, blank, rng):
    """Writes one case in the format align_emu.cpp's main() reads: buffers exactly as long as the data.  -> the rows without an env"""
    P, PS = H * W, (H * W + 127) & ~127
    pmask = sum(1 << i for i, k in enumerate(B.PLANES[:-1]) if k in O.KIND_PLANES[kind])
    M = len(cases)
    resident = layout == "resident"
    N, ans, adim, src, bad = PL.envs_for(cases, resident, with_src, rng)
    answer = np.full((N, PS), 0x55, np.int8)
    answer[:, :P] = ans.reshape(N, P)
    rec = np.full((N, 16), 0x55, np.int8)
    rec[:, 14:16] = adim
    dist = min(dist, 2048)
    with open(path, "wb") as f:
        if resident:
            rec[:M, 0:2] = np.stack([c["idim"] for c in cases])
            rec[:M, 2:4] = np.stack([c["dim"] for c in cases])
            grid, inp = np.full((N, PS), 0x55, np.int8), np.full((N, PS), 0x55, np.int8)
            grid[:M, :P] = np.stack([c["grid"].reshape(-1) for c in cases])
            inp[:M, :P] = np.stack([c["inp"].reshape(-1) for c in cases])
            f.write(np.array([MAGIC, H, W, pmask, N, M, 0, dist, 1, 0, int(with_src), int(with_base), int(sources), int(blank)], np.int32).tobytes())
            f.write(answer.tobytes() + rec.tobytes() + grid.tobytes() + inp.tobytes())
        else:
            buf, offset, stride = CP.place(make_rows(kind, cases, rng), layout)
            f.write(np.array([MAGIC, H, W, pmask, N, M, stride, dist, 0, offset, int(with_src), int(with_base), int(sources), int(blank)], np.int32).tobytes())
            f.write(answer.tobytes() + rec.tobytes() + buf.tobytes())
        if with_src:
            f.write(src.tobytes())
    return bad


def parse_dump(text, M, with_base):
    """The standalone program's output -> (align, base) with SENTINEL where nothing was printed (the program prints 77s in the slots the
    kernel left alone)."""
    align, base = np.full((M, 2, 8), SENTINEL, np.int32), np.full((M, 2), SENTINEL, np.int32)
    lines = text.strip().splitlines()
    i = 0
    for m in range(M):
        if with_base:
            base[m] = [int(v) for v in lines[i].split()]
            i += 1
        for s in range(2):
            align[m, s] = [int(v) for v in lines[i].split()]
            i += 1
    assert i == len(lines)
    return align, base
