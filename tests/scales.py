"""Backend-independent checks of arcle_scale_rows (the grid or the input of a state row zoomed, shrunk or tiled onto the answer's
canvas).  The counterpart of tests/align.py, whose env arrangement (place.envs_for), guards and SENTINEL it takes: every check takes a
backend — EmuScale (tests/emu/scale_emu.cpp: the kernel body of arcle_scale.h lock-step on the CPU) or HipScale (the product) — and
returns a list of mismatch strings.  The reference point is arcle_amd.search.scale_numpy, which builds every child grid from the
definition and which tests/test_scale_host.py pins on the oracle's own resize_grid + Color macro."""
import ctypes
import os
import subprocess

import numpy as np

import align as AL
import backends as B
import components as CP
import place as PL
from arcle_amd import search as S
from oracle import oracle as O

EMU_DIR = CP.EMU_DIR
EMU_SRC = os.path.join(EMU_DIR, "scale_emu.cpp")
EMU_HDRS = AL.EMU_HDRS + [os.path.join(B.ROOT, "arcle_amd", "csrc", "arcle_scale.h")]
SENTINEL = PL.SENTINEL
SENTINEL8 = SENTINEL  # (the byte the bit rows are filled with)
# 5 x 5 and 7 x 6: every candidate against the oracle; 20 x 7: the row board under the generic width class; 7 x 12: a plane stride of
# 96; 30 x 30: the fast width; 16 x 33 and 3 x 40: the flat board
SIZES = ((5, 5), (7, 6), (20, 7), (7, 12), (30, 30), (16, 33), (3, 40))
ORACLE_SIZES = ((5, 5), (7, 6))
# per env kind: resize_grid and Color 0 .. 9 in the default table (O2ARCv2Env: o2arcenv.py:102-109)
SCALE_OPS = {"o2arc": (33, tuple(range(10))), "arc": (25, tuple(range(10)))}
SOURCE_NAMES = ("grid", "input")
CANDS = S.scale_candidates()
ZOOM, SHRINK, TILE = 0, 1, 2


def cand_of(mode, kx, ky):
    """The index of ZOOM / SHRINK (kx, ky), kx, ky in 1..8, or of TILE with mirrored tile rows (kx = 1) / columns (ky = 1)"""
    return 128 + 2 * kx + ky if mode == TILE else 64 * mode + 8 * (kx - 1) + (ky - 1)


def child_of(src, sh, sw, ah, aw, cand):
    """G' of a candidate on the whole plane, cell by cell from the definition of include/arcle_scale_rows.h — used to build ANSWERS and to
    describe cases only (the mirror under test is scale_numpy, which indexes whole rows and columns, and the oracle settles the macro
    in tests/test_scale_host.py)"""
    H, W = src.shape
    mode, kx, ky = CANDS[cand]
    out = np.zeros((H, W), np.int8)

    def at(k, t, n):
        if mode == ZOOM:
            return t // k
        if mode == SHRINK:
            return t * k
        q, r = divmod(t, n)
        return n - 1 - r if (k and q % 2) else r
    for i in range(ah):
        for j in range(aw):
            x, y = at(kx, i, sh), at(ky, j, sw)
            if 0 <= x < sh and 0 <= y < sw and 1 <= src[x, y] <= 9:
                out[i, j] = src[x, y]
    return out


# ---- the cases: a grid, an input, an answer and their dims ---------------------------------------------------------------------------
_cases = {}


def cases_of(H, W):
    """Per size, H >= 3 and W >= 5 (`want` = per source slot the candidate a case was built for, which must be PERFECT there; `unique`
    = the slots where no other candidate may be; `short` = the slots whose best child must stay below the total):
      zoom              every cell of a (H // 2) x (W // 2) grid a 2 x 2 block; the input is noise
      zoom aniso        the input zoomed by (2, 3) — (1, 2) where the plane has no room; the grid is all zero
      zoom short        a zoomed source smaller than the canvas: the rows and columns behind it read 0 (f(i) >= sh)
      shrink            the top-left cell of every 2 x 2 block of the full plane
      shrink past       a canvas one row and one column larger than the shrunk source: i * kx runs past sh
      1x1 source        a single cell at factor 8 (or as far as the plane goes) under a canvas of min(8, H) x min(8, W)
      tile flat row / column   sh = 1 with mirrored tile columns (bit 1 of t cannot matter: t = 1 ties with 3) and sw = 1 with
                        mirrored tile rows (t = 2 ties with 3)
      tile ragged       plain tiles whose size divides neither H nor W
      tile mirrored     every second tile mirrored on both axes
      junk              source dims below (H, W), the plane full of bytes outside them that WOULD complete the answer if read
      bad bytes         source bytes -128, -1, 10, 127 where the answer is 0: they are read as 0
      answer byte       answer bytes -1, 10 and 127 over the SAME source bytes: never matched
      zero source       all-zero sources: every candidate ties, candidate 0, no colour
      zero dim a / b / c   grid_dim with a 0, input_dim with a 0, answer_dim with a 0: no candidate
      tie identity      the answer IS the source: ZOOM(1, 1), SHRINK(1, 1) and TILE 0 .. 3 are all perfect; the lowest index
      constant          a one-colour source under a one-colour answer: every zoom ties
    (at H = 3 a canvas of two rows cannot tell the row factors 2 .. 8 apart: `zoom` and `shrink past` are perfect there, not unique)"""
    if (H, W) in _cases:
        return _cases[(H, W)]
    rng = np.random.default_rng(7000 + 131 * H + W)
    out = []

    def add(name, grid, dim, inp, idim, answer, adim, want=None, unique=(), short=()):
        out.append({"name": f"{H}x{W} {name}", "H": H, "W": W, "grid": np.asarray(grid).astype(np.int8), "dim": np.asarray(dim, np.int8),
                    "inp": np.asarray(inp).astype(np.int8), "idim": np.asarray(idim, np.int8), "answer": np.asarray(answer).astype(np.int8),
                    "adim": np.asarray(adim, np.int8), "want": want or {}, "unique": tuple(unique), "short": tuple(short)})

    def noise(h=H, w=W):
        """Colours 1 .. 9 on [0, h) x [0, w) of the plane, neighbours in a row and in a column different (no zoom of it is one of its
        own tilings), 0 elsewhere"""
        c = np.zeros((H, W), np.int8)
        for i in range(h):
            for j in range(w):
                bad = {int(c[i - 1, j]) if i else 0, int(c[i, j - 1]) if j else 0}
                c[i, j] = rng.choice([v for v in range(1, 10) if v not in bad])
        return c
    full, zero = (H, W), np.zeros((H, W), np.int8)
    sh, sw = H // 2, W // 2
    g = noise(sh, sw)
    add("zoom", g, (sh, sw), noise(), full, child_of(g, sh, sw, 2 * sh, 2 * sw, cand_of(ZOOM, 2, 2)), (2 * sh, 2 * sw), {0: cand_of(ZOOM, 2, 2)}, unique=(0,) if H >= 5 else ())
    kx, ky = (2, 3) if H >= 4 and W >= 6 else (1, 2)
    sh, sw = H // kx, W // ky
    g = noise(sh, sw)
    add("zoom aniso", zero, full, g, (sh, sw), child_of(g, sh, sw, kx * sh, ky * sw, cand_of(ZOOM, kx, ky)), (kx * sh, ky * sw), {1: cand_of(ZOOM, kx, ky)}, unique=(1,))
    sh, sw = (H - 1) // 2, (W - 1) // 2
    g = noise(sh, sw)
    add("zoom short", g, (sh, sw), g, (sh, sw), child_of(g, sh, sw, H, W, cand_of(ZOOM, 2, 2)), full, {0: cand_of(ZOOM, 2, 2), 1: cand_of(ZOOM, 2, 2)}, unique=(0, 1))
    g = noise()
    ah, aw = (H + 1) // 2, (W + 1) // 2
    add("shrink", g, full, noise(), full, child_of(g, H, W, ah, aw, cand_of(SHRINK, 2, 2)), (ah, aw), {0: cand_of(SHRINK, 2, 2)}, unique=(0,))
    sh, sw = H - 1, W - 1
    g = noise(sh, sw)
    ah, aw = (sh + 1) // 2 + 1, (sw + 1) // 2 + 1
    add("shrink past", zero, full, g, (sh, sw), child_of(g, sh, sw, ah, aw, cand_of(SHRINK, 2, 2)), (ah, aw), {1: cand_of(SHRINK, 2, 2)}, unique=(1,) if H >= 5 else ())
    g = noise(1, 1)
    ah, aw = min(8, H), min(8, W)
    add("1x1 source", g, (1, 1), g, (1, 1), child_of(g, 1, 1, ah, aw, cand_of(ZOOM, 8, 8)), (ah, aw), {0: cand_of(ZOOM, ah, aw), 1: cand_of(ZOOM, ah, aw)})
    g = noise(1, 3)
    while g[0, 0] == g[0, 2]:  # (a palindrome is its own mirror image)
        g = noise(1, 3)
    add("tile flat row", g, (1, 3), g, (1, 3), child_of(g, 1, 3, H, W, cand_of(TILE, 0, 1)), full, {0: cand_of(TILE, 0, 1), 1: cand_of(TILE, 0, 1)})
    g = noise(2, 1)
    add("tile flat column", g, (2, 1), g, (2, 1), child_of(g, 2, 1, H, W, cand_of(TILE, 1, 0)), full, {0: cand_of(TILE, 1, 0), 1: cand_of(TILE, 1, 0)})
    sh = next((n for n in (2, 3, 4, 5) if H % n and n < H), 2)
    sw = next((n for n in (2, 3, 4, 5) if W % n and n < W), 2)
    g = noise(sh, sw)
    add("tile ragged", g, (sh, sw), noise(), full, child_of(g, sh, sw, H, W, cand_of(TILE, 0, 0)), full, {0: cand_of(TILE, 0, 0)}, unique=(0,))
    sh, sw = max(H // 3, 2), max(W // 3, 2)
    g = noise(sh, sw)
    add("tile mirrored", zero, full, g, (sh, sw), child_of(g, sh, sw, H, W, cand_of(TILE, 1, 1)), full, {1: cand_of(TILE, 1, 1)}, unique=(1,))
    g = noise()
    add("junk", g, (H - 1, W - 1), g, (H - 1, W - 1), g, full, short=(0, 1))
    g = noise()
    a = g.copy()
    for k, v in enumerate((-128, -1, 10, 127)):
        g.flat[1 + 3 * k], a.flat[1 + 3 * k] = v, 0
    add("bad bytes", g, full, g, full, a, full, {0: 0, 1: 0})
    g = noise()
    for k, v in enumerate((-1, 10, 127)):
        g.flat[2 + 4 * k] = v
    add("answer byte", g, full, g, full, g, full, short=(0, 1))
    add("zero source", zero, full, zero, full, rng.choice([0, 0, 3], (H, W)), full)
    add("zero dim a", noise(), (0, W), noise(), full, noise(), full)
    add("zero dim b", noise(), full, noise(), (H, 0), noise(), full)
    add("zero dim c", noise(), full, noise(), full, noise(), (0, W))
    g = noise()
    add("tie identity", g, full, g, full, g, full, {0: 0, 1: 0})
    g = np.full((H, W), 4, np.int8)
    add("constant", g, full, g, full, g, full, {0: 0, 1: 0})
    _cases[(H, W)] = out
    return out


_mirror = {}


def mirror(case, modes=7):
    """scale_numpy of a case with both sources and everything it can tell, computed once per (case, modes): (scale [2, 8], base (2,),
    table [2, 132], children [2, 132, H, W])"""
    key = (case["name"], int(modes))
    if key not in _mirror:
        _mirror[key] = S.scale_numpy(case["grid"], case["dim"], case["inp"], case["idim"], case["answer"], case["adim"], 3, modes, full=True)
    return _mirror[key]


def bit_rows(child):
    """The nine bit rows of a child grid: row c - 1 = its cells of colour c in the layout of arcle_step_bits -> uint8 [9, 128]"""
    flat = np.zeros((9, 1024), np.uint8)
    for c in range(1, 10):
        flat[c - 1, :child.size] = (child == c).reshape(-1)
    return np.packbits(flat, axis=1, bitorder="little")


make_rows = AL.make_rows


# ---- the backends -----------------------------------------------------------------------------------------------------------------
class _ScaleParams(ctypes.Structure):  # mirror of arcle::ScaleParams (arcle_amd/csrc/arcle_scale.h)
    _fields_ = [("p", B._StepParams), ("sources", ctypes.c_uint32), ("modes", ctypes.c_uint32), ("src_env", ctypes.c_void_p),
                ("scale", ctypes.c_void_p), ("table", ctypes.c_void_p), ("bits", ctypes.c_void_p), ("base", ctypes.c_void_p)]


_emu = None


def emu_lib():
    global _emu
    if _emu is None:
        so = os.path.join(EMU_DIR, "libscale_emu.so")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [EMU_SRC] + EMU_HDRS):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, EMU_SRC])
        _emu = ctypes.CDLL(so)
        _emu.scale_emu_run.argtypes = [ctypes.POINTER(_ScaleParams), ctypes.c_int]
        assert _emu.scale_emu_params_size() == ctypes.sizeof(_ScaleParams), "ScaleParams layout drifted"
    return _emu


class EmuScale:
    """The emulated kernel.  fw: -1 = the instantiation the library launches for the width, 0 = FW_GENERIC at any width."""
    BACKEND = B.EmuBackend  # (a subclass may name a backend of another plane stride)
    name = "emu"

    def __init__(self, fw=-1):
        self.fw = fw

    def run(self, kind, H, W, cases, layout, with_src, with_base, sources, modes, with_table, with_bits, rng):
        M = len(cases)
        resident = layout == "resident"
        N, ans, adim, src, bad = PL.envs_for(cases, resident, with_src, rng)
        be = self.BACKEND(N, H, W, 3, kind, CP.OPS[kind]())
        for k in be.buf:
            be.buf[k][:] = 0x55
        be.rec[:] = 0x55
        be.buf["answer"][:, :H * W] = ans.reshape(N, -1)
        be.rec[:, 14:16] = adim
        x = _ScaleParams()
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
        self.guards = [PL._guarded((M, 2, 8)), PL._guarded((M, 2, S.SCALE_CANDS)), PL._guarded((M, 2, 9, 128), np.uint8), PL._guarded((M, 2))]
        (_, scale), (_, table), (_, bits), (_, base) = self.guards
        x.sources, x.modes = sources, modes
        x.src_env = None if src is None else src.ctypes.data
        x.scale, x.base = scale.ctypes.data, base.ctypes.data if with_base else None
        x.table, x.bits = table.ctypes.data if with_table else None, bits.ctypes.data if with_bits else None
        rc = emu_lib().scale_emu_run(ctypes.byref(x), self.fw)
        assert rc == 0, f"scale emulator reported error {rc} (divergent cross-lane op / non-uniform value)"
        return scale, table, bits, base, bad

    def guards_intact(self):
        return all((buf[:16] == SENTINEL).all() and (buf[-16:] == SENTINEL).all() for buf, _ in self.guards)


class HipScale:
    """EnvBatch.scale_rows on the device."""
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

    def run(self, kind, H, W, cases, layout, with_src, with_base, sources, modes, with_table, with_bits, rng):
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
        ns, nt = M * 16, M * 2 * S.SCALE_CANDS
        guard = t.full((ns + nt + M * 2 + 64,), SENTINEL, dtype=t.int32, device=b.device)
        scale = guard[16:16 + ns].view(M, 2, 8)
        table = guard[32 + ns:32 + ns + nt].view(M, 2, S.SCALE_CANDS)
        base = guard[48 + ns + nt:48 + ns + nt + 2 * M].view(M, 2)
        nb = M * 2 * 9 * 128
        guard8 = t.full((nb + 32,), SENTINEL8, dtype=t.uint8, device=b.device)
        bits = guard8[16:16 + nb].view(M, 2, 9, 128)
        b.scale_rows(view, None if src is None else t.as_tensor(src, device=b.device), sources, modes,
                     out=(scale, table if with_table else None, bits if with_bits else None, base if with_base else None))
        g, g8 = guard.cpu().numpy(), guard8.cpu().numpy()
        self._ok = bool((g[:16] == SENTINEL).all() and (g[16 + ns:32 + ns] == SENTINEL).all() and (g[32 + ns + nt:48 + ns + nt] == SENTINEL).all() and
                        (g[48 + ns + nt + 2 * M:] == SENTINEL).all() and (g8[:16] == SENTINEL8).all() and (g8[16 + nb:] == SENTINEL8).all())
        return scale.cpu().numpy(), table.cpu().numpy(), bits.cpu().numpy(), base.cpu().numpy(), bad

    def guards_intact(self):
        return self._ok


def compare(tag, got, cases, with_base, sources, modes, with_table, with_bits):
    """Everything exact: the eight words, the table row and the nine bit rows of every slot asked for, the base pair; SENTINEL in the
    slots not asked for and in an absent table, bits or base."""
    scale, table, bits, base, bad = got
    errs = []
    for m, c in enumerate(cases):
        ws, wb, wt, wch = mirror(c, modes)
        t = f"{tag} row {m} ({c['name']})"
        if m in bad:
            ws, wb, wt = np.zeros_like(ws), (0, 0), np.full_like(wt, -1)
            ws[:, 0] = -1
        for s in range(2):
            asked = bool((sources >> s) & 1)
            if asked and not np.array_equal(scale[m, s], ws[s]):
                errs.append(f"{t}: {SOURCE_NAMES[s]} {scale[m, s].tolist()} != {ws[s].tolist()}")
            if not asked and (scale[m, s] != SENTINEL).any():
                errs.append(f"{t}: the {SOURCE_NAMES[s]} slot was written though not asked for")
            if asked and with_table:
                if not np.array_equal(table[m, s], wt[s]):
                    k = int(np.flatnonzero(table[m, s] != wt[s])[0])
                    errs.append(f"{t}: {SOURCE_NAMES[s]} table[{k}] {int(table[m, s, k])} != {int(wt[s, k])}")
            elif (table[m, s] != SENTINEL).any():
                errs.append(f"{t}: the {SOURCE_NAMES[s]} table row was written though not asked for")
            if asked and with_bits:
                want = bit_rows(wch[s, ws[s, 0]]) if ws[s, 0] >= 0 else np.zeros((9, 128), np.uint8)
                if not np.array_equal(bits[m, s], want):
                    k = int(np.flatnonzero((bits[m, s] != want).any(1))[0])
                    errs.append(f"{t}: {SOURCE_NAMES[s]} bit row of colour {k + 1} differs")
            elif (bits[m, s] != SENTINEL8).any():
                errs.append(f"{t}: the {SOURCE_NAMES[s]} bit rows were written though not asked for")
        if with_base and tuple(int(v) for v in base[m]) != tuple(wb):
            errs.append(f"{t}: base {base[m].tolist()} != {tuple(wb)}")
        if not with_base and (base[m] != SENTINEL).any():
            errs.append(f"{t}: base was written though not asked for")
    return errs


# size -> the runs of one backend: (kind, layout | "resident", M, src given, base asked for, sources, modes, table, bits).  Per size:
# every env kind (the offsets of grid and input differ), the three layouts and the resident form, M = 1 and 37 (None: one row per
# case; a tuple of strings: the cases whose name ends with one), sources 1, 2 and 3, modes 1 .. 7, src and NULL, with and without the
# table, the bits and the base.  The emulator pays for every cross-lane fetch of every candidate, so its 37-row runs take the TILE
# family (four candidates) and, on the flat board, every run but the first takes few cases; `full` (the device) adds every case with
# every mode in both remaining kinds.
FEW = ("zoom aniso", "shrink past", "tile mirrored", "bad bytes", "zero dim b", "tie identity")


def plan(H, W, full=False):
    flat = W > 32 or H > 64
    few = FEW if flat else None
    runs = [("o2arc", "odd", None, True, True, 3, 7, True, True), ("arc", "dense", few, False, True, 1, 3, False, True),
            ("raw", "lib", 1, False, False, 2, 5, True, False), ("raw", "resident", few, True, True, 3, 6, True, True),
            ("o2arc", "lib", 37, True, True, 2, 4, True, True), ("arc", "resident", ("tie identity", "constant", "1x1 source"), False, True, 3, 2, True, True),
            ("o2arc", "dense", 37, True, False, 1, 4, False, False), ("arc", "lib", ("tie identity", "zoom", "shrink"), False, True, 3, 1, True, True)]
    return runs + ([("arc", "lib", None, True, True, 3, 7, True, True), ("raw", "dense", 37, False, True, 3, 7, True, True)] if full else [])


def run_size(be, H, W, runs=None, full=False):
    runs = runs or plan(H, W, full)
    errs = []
    rng = np.random.default_rng(H * 1000 + W)
    for i, (kind, layout, M, with_src, with_base, sources, modes, with_table, with_bits) in enumerate(runs):
        cases = cases_of(H, W)
        if isinstance(M, (str, tuple)):
            cases = [c for c in cases if c["name"].endswith(M)] or cases[:1]
        elif M is not None:
            cases = PL.pad_to(cases, M) if M > 1 else cases[i % len(cases):][:1]
        tag = f"{be.name} {H}x{W} {kind} {layout} src={with_src} sources={sources} modes={modes}"
        got = be.run(kind, H, W, cases, layout, with_src, with_base, sources, modes, with_table, with_bits, rng)
        errs += compare(tag, got, cases, with_base, sources, modes, with_table, with_bits)
        if not be.guards_intact():
            errs.append(f"{tag}: bytes around an output buffer were written")
        if len(errs) > 10:
            break
    return errs


# ---- the oracle's side: resize_grid on the canvas rectangle, then Color c on the child's cells of colour c ---------------------------
case_rows = AL.case_rows


def scale_macro_set(case, kind, children, slot):
    """Every candidate of one source slot of a case (children [132, H, W] of scale_numpy) as the macro of include/arcle_scale_rows.h on int8
    masks -> (masks int8 [132, 10, H * W], op int32 [132, 10], length int32 [132]): resize_grid on the canvas, then Color c on the
    child's cells of colour c for the colours present, ascending"""
    H, W = case["H"], case["W"]
    resize_op, color_ops = SCALE_OPS[kind]
    ah, aw = (min(int(v), n) for v, n in zip(case["adim"], (H, W)))
    K = len(children)
    masks, op, length = np.zeros((K, 10, H, W), np.int8), np.full((K, 10), -1, np.int32), np.ones(K, np.int32)
    for j, child in enumerate(children):
        masks[j, 0, :ah, :aw] = 1
        op[j, 0] = resize_op
        for c in range(1, 10):
            if (child == c).any():
                masks[j, length[j]] = child == c
                op[j, length[j]] = color_ops[c]
                length[j] += 1
    return masks.reshape(K, 10, H * W), op, length


def oracle_children(case, kind, slot, ops=None):
    """Every candidate's macro of one source slot on the ORACLE (tests/macros.py's chained oracle, mask ingress, the kind's default
    table unless `ops` is given) beside the mirror -> list of (cand, the oracle's grid, grid_dim and dense pair, the mirror's child
    grid and correct count); empty where the slot has no candidate."""
    import macros as MC
    import search_bits as SB
    H, W = case["H"], case["W"]
    rows = case_rows(case, kind)
    scale, _, table, children = mirror(case)
    if scale[slot, 0] < 0:
        return []
    masks, op, length = scale_macro_set(case, kind, children[slot], slot)
    w = MC.oracle_macros(rows, case["answer"][None], case["adim"][None], kind, H, W, 3, ops or CP.OPS[kind](), "mask", masks[None], op[None], length[None])
    assert not w["status"].any(), case["name"]
    grids, gdims = SB._grids_of(w["rows"][0], kind, H, W)
    return [(j, grids[j], gdims[j], w["dense"][0, j], children[slot, j], int(table[slot, j])) for j in range(len(masks))]


# ---- planted tasks: the answer is the input zoomed, shrunk or tiled ----------------------------------------------------------------
def planted_scale_tasks(H=12, W=12, seed=61):
    """Eight tasks on 12 x 12 planes -> (inputs [8, H, W], idims [8, 2], answers [8, H, W], adims [8, 2], names, the planted
    candidate): x2 and x3 zoom of 4 x 4, zoom (2, 3) of 4 x 4, /2 and /3 shrink of a block-uniform 12 x 12, a 2 x 3 plain tiling of
    4 x 4, a 2 x 2 tiling of 5 x 5 mirrored on both axes, a 1 x 2 tiling of 6 x 6 with mirrored columns.  Every source has at least 3
    colours and no symmetry (its flips and its transpose differ from it)."""
    rng = np.random.default_rng(seed)

    def source(h, w):
        while True:
            s = rng.integers(1, 10, (h, w)).astype(np.int8)
            if len(np.unique(s)) >= 3 and not np.array_equal(s, s[::-1]) and not np.array_equal(s, s[:, ::-1]) and not np.array_equal(s, s[::-1, ::-1]) \
                    and not (h == w and (np.array_equal(s, s.T) or np.array_equal(s, s[::-1, ::-1].T))) \
                    and (s[:, 1:] != s[:, :-1]).all() and (s[1:] != s[:-1]).all():
                return s
    specs = [("zoom x2", (4, 4), cand_of(ZOOM, 2, 2), (8, 8)), ("zoom x3", (4, 4), cand_of(ZOOM, 3, 3), (12, 12)), ("zoom (2, 3)", (4, 4), cand_of(ZOOM, 2, 3), (8, 12)),
             ("shrink /2", (12, 12), cand_of(SHRINK, 2, 2), (6, 6)), ("shrink /3", (12, 12), cand_of(SHRINK, 3, 3), (4, 4)),
             ("tile 2 x 3", (4, 4), cand_of(TILE, 0, 0), (8, 12)), ("tile 2 x 2 mirrored", (5, 5), cand_of(TILE, 1, 1), (10, 10)),
             ("tile 1 x 2 mirrored columns", (6, 6), cand_of(TILE, 0, 1), (6, 12))]
    inputs, idims, answers, adims, names, plans = [], [], [], [], [], []
    for name, (sh, sw), cand, (ah, aw) in specs:
        g = np.zeros((H, W), np.int8)
        if name.startswith("shrink"):  # block-uniform: every k x k block one colour
            k = CANDS[cand][1]
            g[:] = np.kron(source(sh // k, sw // k), np.ones((k, k), np.int8))
        else:
            g[:sh, :sw] = source(sh, sw)
        inputs.append(g), idims.append((sh, sw)), answers.append(child_of(g, sh, sw, ah, aw, cand)), adims.append((ah, aw)), names.append(name), plans.append(cand)
    return np.stack(inputs), np.array(idims, np.int8), np.stack(answers), np.array(adims, np.int8), names, plans


def planted_rows(inputs, idims, answers, adims):
    """The tasks' start rows: freshly reset O2ARC envs -> rows [8, L]"""
    return CP.clean_rows("o2arc", inputs, idims, answers, adims)[0]


def scale_numpy_rows(grids, gdims, inps, idims, answers, adims, sources, modes, table=False, bits=True):
    """`ARCVecEnv.scale` of M states from scale_numpy, on torch CPU tensors (the stub vec envs' `scale`)."""
    import torch
    from arcle_amd.envs.vec import scales_of
    M = len(grids)
    sc, base, tab, cb = np.zeros((M, 2, 8), np.int32), np.zeros((M, 2), np.int32), np.zeros((M, 2, S.SCALE_CANDS), np.int32), np.zeros((M, 2, 9, 128), np.uint8)
    for m in range(M):
        sc[m], base[m], t, ch = S.scale_numpy(grids[m], gdims[m], inps[m], idims[m], answers[m], adims[m], sources, modes, full=True)
        for s in range(2):
            if (sources >> s) & 1:
                tab[m, s] = t[s]
                if sc[m, s, 0] >= 0:
                    cb[m, s] = bit_rows(ch[s, sc[m, s, 0]])
    return scales_of(torch.from_numpy(sc), torch.from_numpy(tab) if table else None, torch.from_numpy(cb) if bits else None, torch.from_numpy(base))


def scale_venv(answers, adims, H=12, W=12):
    """The oracle-backed stub vec env of tests/align.py + `scale` (scale_numpy): what beam_search(propose=propose_scales(...)) needs,
    on torch CPU tensors."""
    base = type(AL.align_venv(answers, adims, H, W))

    class ScaleVenv(base):
        def scale(self, rows, src_env=None, sources=3, modes=7, table=False, bits=True):
            r = rows.numpy()
            src = np.arange(len(r)) if src_env is None else src_env.numpy()
            f = AL._field_of
            return scale_numpy_rows(f(r, self.kind, H, W, "grid").reshape(-1, H, W), f(r, self.kind, H, W, "grid_dim"),
                                    f(r, self.kind, H, W, "input").reshape(-1, H, W), f(r, self.kind, H, W, "input_dim"),
                                    self.answers[src], self.adims[src], sources, modes, table, bits)
    return ScaleVenv("o2arc", H, W, 3, O.o2arc_ops(), answers, adims)


replay_on_oracle = AL.replay_on_oracle


BEFORE = {"alignments": lambda: S.propose_alignments(*AL.ALIGN_OPS["o2arc"]),
          "objects": lambda: S.propose_objects(list(PL.MOVE_OPS) + [29], list(range(10, 20)), masks=True, any_color=True, diagonal=True),
          "placements": lambda: S.propose_placements(PL.MOVE_OPS, any_color=True, diagonal=True),
          "stamps": lambda: S.propose_stamps(29, 30, any_color=True, diagonal=True),
          "turns": lambda: S.propose_turns((24, -1, 25, 26, 27), PL.MOVE_OPS, any_color=True, diagonal=True)}


def searches(venv, rows, n, before=tuple(BEFORE)):
    """-> (the results of propose_scales at width 1 and depth 1 on every task, {name: the results of the proposers of BEFORE named in
    `before` at the same width and depth}); the oracle-backed stub env serves the first three of them"""
    import torch

    def one(prop):
        return [S.beam_search(venv, rows[i:i + 1], None, width=1, depth=1, src_env=torch.tensor([i]), propose=prop) for i in range(n)]
    return one(S.propose_scales(*SCALE_OPS["o2arc"])), {k: one(BEFORE[k]()) for k in before}


# ---- one dumped case for the standalone sanitized emulator ------------------------------------------------------------------------
MAGIC = 0x5343414c


def dump_case(path, kind, H, W, cases, layout, with_src, with_base, sources, modes, with_table, with_bits, rng):
    """Writes one case in the format scale_emu.cpp's main() reads: buffers exactly as long as the data.  -> the rows without an env"""
    P, PS = H * W, (H * W + 127) & ~127
    pmask = sum(1 << i for i, k in enumerate(B.PLANES[:-1]) if k in O.KIND_PLANES[kind])
    M = len(cases)
    resident = layout == "resident"
    N, ans, adim, src, bad = PL.envs_for(cases, resident, with_src, rng)
    answer = np.full((N, PS), 0x55, np.int8)
    answer[:, :P] = ans.reshape(N, P)
    rec = np.full((N, 16), 0x55, np.int8)
    rec[:, 14:16] = adim
    outs = int(with_table) | 2 * int(with_bits)
    with open(path, "wb") as f:
        if resident:
            rec[:M, 0:2] = np.stack([c["idim"] for c in cases])
            rec[:M, 2:4] = np.stack([c["dim"] for c in cases])
            grid, inp = np.full((N, PS), 0x55, np.int8), np.full((N, PS), 0x55, np.int8)
            grid[:M, :P] = np.stack([c["grid"].reshape(-1) for c in cases])
            inp[:M, :P] = np.stack([c["inp"].reshape(-1) for c in cases])
            f.write(np.array([MAGIC, H, W, pmask, N, M, 0, modes, 1, 0, int(with_src), int(with_base), int(sources), outs], np.int32).tobytes())
            f.write(answer.tobytes() + rec.tobytes() + grid.tobytes() + inp.tobytes())
        else:
            buf, offset, stride = CP.place(make_rows(kind, cases, rng), layout)
            f.write(np.array([MAGIC, H, W, pmask, N, M, stride, modes, 0, offset, int(with_src), int(with_base), int(sources), outs], np.int32).tobytes())
            f.write(answer.tobytes() + rec.tobytes() + buf.tobytes())
        if with_src:
            f.write(src.tobytes())
    return bad


def parse_dump(text, M, with_base, with_table, with_bits):
    """The standalone program's output -> (scale, table, bits, base) with SENTINEL where nothing was printed (the program prints 77s in
    the slots the kernel left alone)."""
    scale, base = np.full((M, 2, 8), SENTINEL, np.int32), np.full((M, 2), SENTINEL, np.int32)
    table, bits = np.full((M, 2, S.SCALE_CANDS), SENTINEL, np.int32), np.full((M, 2, 9, 128), SENTINEL8, np.uint8)
    lines = text.strip().splitlines()
    i = 0
    for m in range(M):
        if with_base:
            base[m] = [int(v) for v in lines[i].split()]
            i += 1
        for s in range(2):
            scale[m, s] = [int(v) for v in lines[i].split()]
            i += 1
            if with_table:
                table[m, s] = [int(v) for v in lines[i].split()]
                i += 1
            if with_bits:
                for c in range(9):
                    bits[m, s, c] = np.frombuffer(bytes.fromhex(lines[i].strip()), np.uint8)
                    i += 1
    assert i == len(lines)
    return scale, table, bits, base
