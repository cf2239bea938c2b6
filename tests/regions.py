"""Backend-independent checks of arcle_region_rows (the cells around and inside each object of a state row).  The counterpart of
tests/ray.py, whose pattern it follows and whose shared pieces it takes by import (its cases, and through it those of tests/place.py:
bit rows, env arrangement, guards, SENTINEL): every check takes a backend — EmuRegion (tests/emu/region_emu.cpp: the kernel body of
arcle_region.h lock-step on the CPU) or HipRegion (the product) — and returns a list of mismatch strings.  The reference point is
arcle_amd.search.region_numpy, array slices and a cell-by-cell flood straight from the definition, which tests/test_region_host.py
pins on the oracle's own Color step and on a brute-force restatement."""
import ctypes
import os
import subprocess

import numpy as np

import backends as B
import components as CP
import place as PL
import ray as RY
from arcle_amd import search as S
from oracle import oracle as O

EMU_DIR = CP.EMU_DIR
EMU_SRC = os.path.join(EMU_DIR, "region_emu.cpp")
EMU_HDRS = PL.EMU_HDRS + [os.path.join(B.ROOT, "arcle_amd", "csrc", "arcle_region.h")]
SENTINEL = PL.SENTINEL
CS = PL.CS
COLOR_OPS = tuple(range(10))  # both default tables: Color 0 .. 9
# 5 x 5, 7 x 6, 6 x 9, 20 x 7: the row board under the generic width class; 12 x 12; 30 x 30: the fast width; 32 x 32: bit 31 and 1024
# cells; 64 x 16: every lane a row; 16 x 33 (W > 32) and 65 x 15 (H > 64): the flat board
SIZES = ((5, 5), (7, 6), (6, 9), (12, 12), (20, 7), (30, 30), (32, 32), (64, 16), (16, 33), (65, 15))
ORACLE_SIZES = RY.ORACLE_SIZES
DEFAULT = tuple(S.REGION_KINDS)
# a non-default list: n_kinds = 16, zero entries, repeats, and a code above 7 (taken as 0: the array is read on the device)
KINDS16 = (0, 7, 6, 5, 4, 3, 2, 1, 5, 5, 0, 200, 2, 1, 6, 4)
KIND_LISTS = {"default": DEFAULT, "sixteen": KINDS16, "one": (5,)}
NAMES = ("edges", "full", "hollow", "diamond", "ushape", "twoholes", "nested", "whole")  # + spiral, spiral shut where H, W >= 7


# ---- the cases: those of tests/ray.py (and through it tests/place.py) and what a region adds -------------------------------------------
_cases = {}


def spiral(H, W, shut=False):
    """A one-cell-wide wall that winds from (0, 0) clockwise to the middle, one free corridor of width 1 beside it all the way: the
    corridor opens on the grid's edge at (1, 0) — nothing is inside, and a flood from the edge needs the most rounds a board of this
    size can ask for; shut=True walls that cell up, so the whole corridor is inside."""
    g = np.zeros((H, W), bool)
    x, y, dx, dy = 0, 0, 0, 1
    g[0, 0] = True

    def can(x, y, dx, dy):
        nx, ny, fx, fy = x + dx, y + dy, x + 2 * dx, y + 2 * dy
        return 0 <= nx < H and 0 <= ny < W and not g[nx, ny] and not (0 <= fx < H and 0 <= fy < W and g[fx, fy])
    while True:
        if not can(x, y, dx, dy):
            dx, dy = dy, -dx
            if not can(x, y, dx, dy):
                break
        x, y = x + dx, y + dy
        g[x, y] = True
    if shut:
        g[1, 0] = True
    return g


def cases_of(H, W):
    """The cases of RY.cases_of(H, W) (those of tests/place.py — moved, shrunk a / b, bytes with the whole-grid object and an empty
    mask, twocolour, the ties — and the rays': lines, star, dense, shape, fives) and the cases a region can get wrong (H, W >= 5):
      edges       grid_dim one below the plane on both axes, garbage bytes beyond it; one-cell objects in two corners and on each of
                  the four edges of grid_dim, and a mask with bits set OUTSIDE grid_dim
      full        grid_dim = the plane: the four corners, a bar down column 0 and one down column W - 1 (bit 31 at W = 32, lane 63
                  at H = 64, both columns a flat shift could wrap across)
      hollow      a 3 x 3 ring round a free cell          diamond    a ring whose cells touch only diagonally: it encloses
      ushape      a U open to the grid's edge: nothing is inside
      twoholes    a 3 x 5 block with two holes            nested     a 5 x 5 ring whose 3 x 3 hole holds another object
      spiral      the wall of `spiral`; spiral shut: its corridor closed (H, W >= 7)
      whole       one object that is the whole grid, grid = answer = one colour (every count is H * W: 1024 at 32 x 32), and an empty
                  bit row"""
    if (H, W) in _cases:
        return _cases[(H, W)]
    rng = np.random.default_rng(9100 + 131 * H + W)
    out = list(RY.cases_of(H, W))

    def add(name, grid, dim, answer, adim, masks):
        masks = np.asarray(masks, np.uint8).reshape(-1, H, W)[:16]
        out.append({"name": f"{H}x{W} {name}", "H": H, "W": W, "grid": grid.astype(np.int8), "dim": np.asarray(dim, np.int8),
                    "answer": answer.astype(np.int8), "adim": np.asarray(adim, np.int8), "masks": masks})

    def cell(x, y):
        m = np.zeros((H, W), bool)
        m[x, y] = True
        return m
    assert H >= 5 and W >= 5
    noise = rng.integers(0, 10, (H, W))
    # edges
    gh, gw = H - 1, W - 1
    g = rng.integers(-5, 10, (H, W))
    g[:gh, :gw] = 0
    spots = [(0, 0), (gh - 1, gw - 1), (0, gw // 2), (gh - 1, gw // 2), (gh // 2, 0), (gh // 2, gw - 1)]
    for i, (x, y) in enumerate(spots):
        g[x, y] = 1 + i
    beyond = cell(gh // 2, gw // 2)
    beyond[H - 1, :], beyond[:, W - 1] = True, True
    add("edges", g, (gh, gw), noise, (gh, gw), [cell(x, y) for x, y in spots] + [beyond])
    # full
    g = np.zeros((H, W), np.int8)
    g[0, 0], g[0, W - 1], g[H - 1, 0], g[H - 1, W - 1] = 1, 2, 3, 4
    g[2:H - 2, 0], g[2:H - 2, W - 1] = 5, 6
    add("full", g, (H, W), noise, (H, W), [g == c for c in range(1, 7)])
    # hollow
    g = np.zeros((H, W), np.int8)
    g[1:4, 1:4] = 6
    g[2, 2] = 0
    a = g.copy()
    a[2, 2] = 4
    add("hollow", g, (H, W), a, (H, W), [g == 6])
    # diamond
    g = np.zeros((H, W), np.int8)
    for x, y in ((0, 2), (1, 1), (1, 3), (2, 0), (2, 4), (3, 1), (3, 3), (4, 2)):
        g[x, y] = 2
    a = g.copy()
    for x, y in ((1, 2), (2, 1), (2, 2), (2, 3), (3, 2)):
        a[x, y] = 3
    add("diamond", g, (H, W), a, (H, W), [g == 2])
    # ushape: open towards row 0
    g = np.zeros((H, W), np.int8)
    g[0:3, 1], g[0:3, 3], g[2, 1:4] = 7, 7, 7
    a = g.copy()
    a[0:2, 2] = 1
    add("ushape", g, (H, W), a, (H, W), [g == 7])
    # twoholes
    g = np.zeros((H, W), np.int8)
    g[1:4, 0:5] = 3
    g[2, 1], g[2, 3] = 0, 0
    a = g.copy()
    a[2, 1], a[2, 3] = 8, 8
    add("twoholes", g, (H, W), a, (H, W), [g == 3])
    # nested
    g = np.zeros((H, W), np.int8)
    g[0:5, 0:5] = 6
    g[1:4, 1:4] = 0
    g[2, 2] = 9
    a = g.copy()
    a[1:4, 1:4] = 4
    add("nested", g, (H, W), a, (H, W), [g == 6, g == 9])
    if H >= 7 and W >= 7:
        for name, shut in (("spiral", False), ("spiral shut", True)):
            wall = spiral(H, W, shut)
            g = np.where(wall, 5, 0)
            add(name, g, (H, W), np.where(wall, 5, 2), (H, W), [wall])
    # whole
    g = np.full((H, W), 3, np.int8)
    add("whole", g, (H, W), g, (H, W), [np.ones((H, W), bool), np.zeros((H, W), bool)])
    _cases[(H, W)] = out
    return out


_mirror = {}


def mirror(case, kinds, free_color, through):
    """region_numpy of a case, computed once per (case, kinds, free_color, through) over all its objects: (region [n, S, 4], best
    [n, 4], base (2,), bits uint8 [n, 128] = the best candidate's cells as a bit row)"""
    key = (case["name"], tuple(kinds), int(free_color), bool(through))
    if key not in _mirror:
        reg, best, base, cells = S.region_numpy(case["grid"], case["dim"], case["answer"], case["adim"], case["masks"], kinds, free_color, bool(through), full=True)
        pick = np.stack([cells[k, b] if b >= 0 else np.zeros_like(cells[k, 0]) for k, b in enumerate(best[:, 0])]) if len(best) else cells[:, 0]
        _mirror[key] = (reg, best, base, B.pack_bits(pick))
    return _mirror[key]


# ---- the backends -----------------------------------------------------------------------------------------------------------------
class _RegionParams(ctypes.Structure):  # mirror of arcle::RegionParams (arcle_amd/csrc/arcle_region.h)
    _fields_ = [("p", B._StepParams), ("max_comp", ctypes.c_int32), ("n_kinds", ctypes.c_int32), ("count", ctypes.c_void_p),
                ("bits", ctypes.c_void_p), ("src_env", ctypes.c_void_p), ("kinds", ctypes.c_void_p), ("region", ctypes.c_void_p),
                ("best", ctypes.c_void_p), ("best_bits", ctypes.c_void_p), ("base", ctypes.c_void_p), ("free_color", ctypes.c_int32),
                ("through", ctypes.c_int32)]


_emu = None


def emu_lib():
    global _emu
    if _emu is None:
        so = os.path.join(EMU_DIR, "libregion_emu.so")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [EMU_SRC] + EMU_HDRS):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, EMU_SRC])
        _emu = ctypes.CDLL(so)
        _emu.region_emu_run.argtypes = [ctypes.POINTER(_RegionParams), ctypes.c_int]
        assert _emu.region_emu_params_size() == ctypes.sizeof(_RegionParams), "RegionParams layout drifted"
    return _emu


class EmuRegion:
    """The emulated kernel.  fw: -1 = the instantiation the library launches for the width, 0 = FW_GENERIC at any width."""
    BACKEND = B.EmuBackend  # (a subclass may name a backend of another plane stride)
    name = "emu"

    def __init__(self, fw=-1):
        self.fw = fw

    def run(self, kind, H, W, cases, layout, C, kinds, free_color, through, with_count, with_src, with_base, with_bits, rng):
        M, S_ = len(cases), len(kinds)
        resident = layout == "resident"
        N, ans, adim, src, bad = PL.envs_for(cases, resident, with_src, rng)
        be = self.BACKEND(N, H, W, 3, kind, CP.OPS[kind]())
        for k in be.buf:
            be.buf[k][:] = 0x55
        be.rec[:] = 0x55
        be.buf["answer"][:, :H * W] = ans.reshape(N, -1)
        be.rec[:, 14:16] = adim
        x = _RegionParams()
        p = be._params()
        p.n_resident, p.n_envs = N, M
        if resident:
            be.buf["grid"][:M, :H * W] = np.stack([c["grid"].reshape(-1) for c in cases])
            be.rec[:M, 2:4] = np.stack([c["dim"] for c in cases])
            p.rows_in, p.rows_in_stride = None, 0
        else:
            buf, offset, stride = CP.place(CP.make_rows(kind, cases, rng), layout)
            p.rows_in, p.rows_in_stride = buf.ctypes.data + offset, stride
        x.p = p
        count, bits = PL.bit_rows(cases, C, with_count, rng)
        kinds_a = np.array(kinds, np.uint8)
        self.guards = [PL._guarded((M, C, S_, 4)), PL._guarded((M, C, 4)), PL._guarded((M, C, B.BITS_STRIDE), np.uint8), PL._guarded((M, 2))]
        (_, reg), (_, best), (_, bbits), (_, base) = self.guards
        x.max_comp, x.n_kinds, x.free_color, x.through = C, S_, int(free_color), int(through)
        x.count, x.bits, x.src_env = count.ctypes.data if with_count else None, bits.ctypes.data, None if src is None else src.ctypes.data
        x.kinds, x.region, x.best = kinds_a.ctypes.data, reg.ctypes.data, best.ctypes.data
        x.best_bits, x.base = bbits.ctypes.data if with_bits else None, base.ctypes.data if with_base else None
        rc = emu_lib().region_emu_run(ctypes.byref(x), self.fw)
        assert rc == 0, f"region emulator reported error {rc} (divergent cross-lane op / non-uniform value)"
        return reg, best, bbits, base, bad

    def guards_intact(self):
        return all((buf[:16] == buf.dtype.type(SENTINEL)).all() and (buf[-16:] == buf.dtype.type(SENTINEL)).all() for buf, _ in self.guards)


class HipRegion:
    """EnvBatch.region_rows on the device."""
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

    def outputs(self, dev, M, C, S_):
        """SENTINEL-filled outputs, each with 16 guard elements on both sides -> (the guard buffers, the four views)"""
        t = self.t
        bufs, views = [], []
        for shape, dt in (((M, C, S_, 4), t.int32), ((M, C, 4), t.int32), ((M, C, B.BITS_STRIDE), t.uint8), ((M, 2), t.int32)):
            n = int(np.prod(shape))
            g = t.full((n + 32,), SENTINEL, dtype=dt, device=dev)
            bufs.append(g)
            views.append(g[16:16 + n].view(shape))
        return bufs, views

    def run(self, kind, H, W, cases, layout, C, kinds, free_color, through, with_count, with_src, with_base, with_bits, rng):
        t = self.t
        M = len(cases)
        resident = layout == "resident"
        N, ans, adim, src, bad = PL.envs_for(cases, resident, with_src, rng)
        b = self.batch(kind, H, W, N)
        b.plane("answer").copy_(t.as_tensor(ans, device=b.device))
        b.field("answer_dim").copy_(t.as_tensor(adim, device=b.device))
        rows = CP.make_rows(kind, cases, rng)
        if resident:
            b.set_state_rows(t.as_tensor(rows, device=b.device))
            view = None
        else:
            buf, offset, stride = CP.place(rows, layout)
            dbuf = t.as_tensor(buf, device=b.device)  # (exactly the bytes of the rows: the last row ends the allocation)
            view = t.as_strided(dbuf, (M, rows.shape[1]), (stride, 1), offset)
        count, bits = PL.bit_rows(cases, C, with_count, rng)
        bufs, (reg, best, bbits, base) = self.outputs(b.device, M, C, len(kinds))
        b.region_rows(view, t.as_tensor(count, device=b.device) if with_count else None, t.as_tensor(bits, device=b.device),
                   t.as_tensor(np.array(kinds, np.uint8), device=b.device), free_color, bool(through),
                   None if src is None else t.as_tensor(src, device=b.device), out=(reg, best, bbits if with_bits else None, base if with_base else None))
        self._ok = all(bool((g[:16] == SENTINEL).all()) and bool((g[-16:] == SENTINEL).all()) for g in bufs)
        return reg.cpu().numpy(), best.cpu().numpy(), bbits.cpu().numpy(), base.cpu().numpy(), bad

    def guards_intact(self):
        return self._ok


def compare(tag, got, cases, C, kinds, free_color, through, with_count, with_base, with_bits):
    """Everything exact: the four words of every candidate, the best slot, its bit row, the base pair, SENTINEL in the entries >= count
    and in the outputs not asked for."""
    reg, best, bbits, base, bad = got
    S_ = len(kinds)
    errs = []
    for m, c in enumerate(cases):
        wr, wb, wbase, wbits = mirror(c, kinds, free_color, through)
        n = min(C, len(wr))
        t = f"{tag} row {m} ({c['name']})"
        empty_reg, empty_best = (0, wbase[0], 0, 0), (-1, 0, wbase[0], 0)
        if m in bad:
            wr, wb, wbits, wbase = np.zeros_like(wr), np.zeros_like(wb), np.zeros_like(wbits), (0, 0)
            empty_reg, empty_best = (0, 0, 0, 0), (0, 0, 0, 0)
        if not np.array_equal(reg[m, :n], wr[:n]):
            k, s = (int(v) for v in np.argwhere((reg[m, :n] != wr[:n]).any(2))[0])
            errs.append(f"{t}: object {k} candidate {s} (kind {kinds[s]}) {reg[m, k, s].tolist()} != {wr[k, s].tolist()}")
        if not np.array_equal(best[m, :n], wb[:n]):
            k = int(np.argwhere((best[m, :n] != wb[:n]).any(1))[0, 0])
            errs.append(f"{t}: object {k} best {best[m, k].tolist()} != {wb[k].tolist()}")
        if with_bits and not np.array_equal(bbits[m, :n], wbits[:n]):
            k = int(np.argwhere((bbits[m, :n] != wbits[:n]).any(1))[0, 0])
            errs.append(f"{t}: object {k} best_bits differ from the mirror's cells of candidate {int(wb[k, 0])}")
        if not with_bits and (bbits[m] != np.uint8(SENTINEL)).any():
            errs.append(f"{t}: best_bits was written though not asked for")
        if with_count:
            if (reg[m, n:] != SENTINEL).any() or (best[m, n:] != SENTINEL).any() or (with_bits and (bbits[m, n:] != np.uint8(SENTINEL)).any()):
                errs.append(f"{t}: an entry >= count was written")
        else:  # (the slots beyond the case's masks hold empty masks: B empty)
            if (reg[m, n:] != np.array(empty_reg)).any() or (best[m, n:] != np.array(empty_best)).any() or (with_bits and bbits[m, n:].any()):
                errs.append(f"{t}: an empty mask gave {reg[m, n:].reshape(-1, 4)[:1].tolist()} / {best[m, n:][:1].tolist()}")
        if with_base and tuple(int(v) for v in base[m]) != tuple(wbase):
            errs.append(f"{t}: base {base[m].tolist()} != {tuple(wbase)}")
        if not with_base and (base[m] != SENTINEL).any():
            errs.append(f"{t}: base was written though not asked for")
    return errs


# size -> the runs of one backend: (kind, layout | "resident", M, C, kind list, free_color, through, count given, src given, base asked
# for, best_bits asked for).  Per size: every env kind, the three layouts and the resident form, M = 1 and 37 (None: one row per case),
# every C of CS, the three kind lists, both `through` values, free_color 0, 5 and -1, count and NULL, src and NULL, base and best_bits
# asked for and not.
def plan(H, W, full=False):
    runs = [("o2arc", "odd", None, 16, "default", 0, False, True, True, True, True), ("arc", "dense", None, 5, "sixteen", 0, True, False, False, True, True),
            ("raw", "lib", 1, 1, "one", 5, False, True, False, False, False), ("raw", "resident", None, 16, "sixteen", 5, False, True, True, True, True),
            ("o2arc", "lib", 37, 5, "default", 0, True, True, True, True, False), ("arc", "resident", None, 5, "one", -1, False, False, False, True, True),
            ("o2arc", "dense", 37, 1, "sixteen", 0, False, False, True, False, True)]
    return runs + ([("arc", "lib", None, 16, "default", 0, True, True, True, True, True), ("o2arc", "lib", None, 16, "sixteen", 0, False, True, True, True, True)] if full else [])


def run_size(be, H, W, runs=None, full=False):
    runs = runs or plan(H, W, full)
    errs = []
    rng = np.random.default_rng(H * 1000 + W)
    for i, (kind, layout, M, C, kindname, fc, through, with_count, with_src, with_base, with_bits) in enumerate(runs):
        cases = cases_of(H, W)
        kinds = KIND_LISTS[kindname]
        if isinstance(M, str):
            cases = [c for c in cases if c["name"].endswith(M)] or cases[:1]
        elif M is not None:
            cases = PL.pad_to(cases, M) if M > 1 else cases[i % len(cases):][:1]
        tag = f"{be.name} {H}x{W} {kind} {layout} C={C} kinds={kindname} free={fc} through={int(through)} count={with_count} src={with_src}"
        got = be.run(kind, H, W, cases, layout, C, kinds, fc, through, with_count, with_src, with_base, with_bits, rng)
        errs += compare(tag, got, cases, C, kinds, fc, through, with_count, with_base, with_bits)
        if not be.guards_intact():
            errs.append(f"{tag}: bytes around an output buffer were written")
        if len(errs) > 10:
            break
    return errs


# ---- the oracle's side: ONE Color c step on the candidate's cells -----------------------------------------------------------------------
def oracle_children(case, kinds, through, kind="o2arc", free_color=0):
    """For every object, candidate and colour c the first number of the dense pair the ORACLE reports after `Color c` on the mirror's cells of
    that candidate (mask ingress, tests/macros.py's chained oracle with macros of one step) -> (dense int [n, S, 10], -1 where the
    candidate is empty; the mirror's (reg, best, base, cells) on the grid the oracle's freshly reset env holds)."""
    import macros as MC
    import search_bits as SB
    H, W = case["H"], case["W"]
    rows, orc = CP.clean_rows(kind, case["grid"][None], case["dim"][None], case["answer"][None], case["adim"][None])
    grid = SB._grids_of(rows, kind, H, W)[0][0]
    got = S.region_numpy(grid, case["dim"], case["answer"], case["adim"], case["masks"], kinds, free_color, through, full=True)
    cells = got[3]
    n, S_ = cells.shape[:2]
    idx = [(k, s) for k in range(n) for s in range(S_) if cells[k, s].any()]
    dense = np.full((n, S_, 10), -1, np.int64)
    if idx:
        K = len(idx) * 10
        masks = np.repeat(np.stack([cells[k, s] for k, s in idx]).astype(np.int8), 10, 0).reshape(1, K, 1, H * W)
        op = np.tile(np.array(COLOR_OPS, np.int32), len(idx)).reshape(1, K, 1)
        w = MC.oracle_macros(rows, case["answer"][None], case["adim"][None], kind, H, W, 3, CP.OPS[kind](), "mask", masks, op, np.ones((1, K), np.int32))
        assert not w["status"].any(), case["name"]
        for i, (k, s) in enumerate(idx):
            dense[k, s] = w["dense"][0, 10 * i:10 * i + 10, 0]
    return dense, got


# ---- planted tasks: objects whose halo, box, frame or inside the answer paints -----------------------------------------------------------
# (kind, objects) per task
PLANTED = ((S.REGION_HALO8, 1), (S.REGION_HALO4, 2), (S.REGION_INSIDE, 1), (S.REGION_BOX_REST, 1), (S.REGION_HALO8, 3), (S.REGION_HALO4, 3),
           (S.REGION_INSIDE, 1), (S.REGION_BOX_FRAME, 2))
GAP = 2  # free cells at least between an object's box and the grid's edge, and between two boxes


def _shape(kind, rng):
    """bool [h, w]: one 4-connected object for a task of the kind, and the cells (bool [h, w]) that hold another colour"""
    other = None
    if kind == S.REGION_HALO8:  # one or two cells, or an L of three: a halo of 8 to 12 cells
        m = [np.ones((1, 1), bool), np.ones((1, 2), bool), np.array([[1, 0], [1, 1]], bool)][int(rng.integers(0, 3))]
    elif kind == S.REGION_HALO4:  # halo4 != halo8 for every shape; 4 to 7 cells against at most 3 of the object
        m = [np.ones((1, 1), bool), np.ones((2, 1), bool), np.array([[1, 1], [0, 1]], bool)][int(rng.integers(0, 3))]
    elif kind == S.REGION_INSIDE:  # a closed ring round 3 x 3 or 3 x 4 cells, one or two of them of another colour
        h, w = 5, int(rng.integers(5, 7))
        m = np.ones((h, w), bool)
        m[1:-1, 1:-1] = False
        other = np.zeros((h, w), bool)
        for c in rng.permutation((h - 2) * (w - 2))[:int(rng.integers(1, 3))]:
            other[1 + int(c) // (w - 2), 1 + int(c) % (w - 2)] = True
    elif kind == S.REGION_BOX_REST:  # an L with arms of 3 and 4: 6 cells, 6 cells of its box are free
        m = np.zeros((3, 4), bool)
        m[:, 0], m[2, :] = True, True
    else:  # BOX_FRAME round a T: the frame (14 cells) is not the halo (which holds the two free cells of the box too)
        m = np.array([[1, 1, 1], [0, 1, 0]], bool)
    if rng.integers(0, 2):
        m, other = m[::-1].copy(), (None if other is None else other[::-1].copy())
    return m, other


def planted_region_tasks(n=8, H=12, W=12, seed=12):
    """n tasks on background 0, fixed by the seed: per task the kind and the number of objects of PLANTED; every object (a `_shape`, of
    its own colour 1 .. 6) lies with its box at least GAP free cells from the grid's edge and from every other box — so that no region
    touches another object or its region, and a reg from an object runs at least GAP > 1 cells before anything stops it, further
    than any halo reaches; the answer paints the task's region of every object (region_numpy's cells, through = 1)
    with colour 7 or 8, over the one or two cells of colour 9 an INSIDE task holds.  -> (inputs [n, H, W], dims [n, 2], answers
    [n, H, W], the number of objects per task, the kind per task)"""
    rng = np.random.default_rng(seed)
    dims = np.tile(np.array([[H, W]], np.int8), (n, 1))
    inputs, answers, depths, kinds = [], [], [], []
    for _ in range(20000):
        if len(inputs) == n:
            break
        kind, want = PLANTED[len(inputs) % len(PLANTED)]
        g = np.zeros((H, W), np.int8)
        boxes, masks, ok = [], [], True
        for col in rng.permutation(6)[:want] + 1:
            m, other = _shape(kind, rng)
            h, w = m.shape
            if H - 2 * GAP - h < 0 or W - 2 * GAP - w < 0:
                ok = False
                break
            x0, y0 = int(rng.integers(GAP, H - GAP - h + 1)), int(rng.integers(GAP, W - GAP - w + 1))
            if any(x0 < b[2] + GAP and b[0] < x0 + h + GAP and y0 < b[3] + GAP and b[1] < y0 + w + GAP for b in boxes):
                ok = False
                break
            boxes.append((x0, y0, x0 + h, y0 + w))
            full = np.zeros((H, W), bool)
            full[x0:x0 + h, y0:y0 + w] = m
            g[full] = col
            if other is not None:
                g[x0:x0 + h, y0:y0 + w][other] = 9
            masks.append(full)
        if not ok:
            continue
        a = g.copy()
        cells = S.region_numpy(g, (H, W), g, (H, W), np.stack(masks), [kind], 0, True, full=True)[3]
        for k, paint in enumerate(rng.permutation(2)[:1].repeat(want) + 7):
            assert cells[k, 0].sum() >= 4
            a[cells[k, 0]] = paint
        inputs.append(g)
        answers.append(a)
        depths.append(want)
        kinds.append(kind)
    assert len(inputs) == n, "planted_region_tasks: no such tasks at this seed"
    return np.stack(inputs), dims, np.stack(answers), depths, kinds


def region_numpy_rows(grids, gdims, answers, adims, objs, kinds, free_color, through, bits=True):
    """`ARCVecEnv.regions` of M grids from region_numpy, on torch CPU tensors (the stub vec envs' `regions`)."""
    import torch
    from arcle_amd.envs.vec import Regions
    kinds = S.REGION_KINDS if kinds is None else kinds
    M, C, S_ = int(objs.bits.shape[0]), int(objs.bits.shape[1]), len(kinds)
    H, W = grids.shape[1:]
    reg, best, bb, base = np.zeros((M, C, S_, 4), np.int32), np.zeros((M, C, 4), np.int32), np.zeros((M, C, B.BITS_STRIDE), np.uint8), np.zeros((M, 2), np.int32)
    cells = np.unpackbits(objs.bits.numpy(), axis=-1, bitorder="little")[..., :H * W].reshape(M, C, H, W)
    for m in range(M):
        n = int(objs.count[m])
        r, b, base[m], sel = S.region_numpy(grids[m], gdims[m], answers[m], adims[m], cells[m, :n], kinds, free_color, through, full=True)
        reg[m, :n], best[m, :n] = r, b
        for k in range(n):
            if b[k, 0] >= 0:
                bb[m, k] = B.pack_bits(sel[k, b[k, 0]][None])[0]
    t, u = torch.from_numpy(reg), torch.from_numpy(best)
    return Regions(t[..., 0], t[..., 1], t[..., 2], t[..., 3], u[..., 0], u[..., 1], u[..., 2], u[..., 3], torch.from_numpy(bb) if bits else None,
                   torch.from_numpy(base))


def region_venv(answers, adims, H=12, W=12):
    """The oracle-backed stub vec env of tests/mirror.py (objects, place, stamp, turn, align, rays, mirror from their mirrors) +
    `regions` (region_numpy): what beam_search(propose=propose_regions(...)) and the seven earlier proposers need, on torch CPU
    tensors."""
    import mirror as MI
    import search_bits as SB
    base = type(MI.mirror_venv(answers, adims, H, W))

    class RegionVenv(base):
        def regions(self, rows, objs, kinds=None, free_color=0, through=False, bits=True, src_env=None):
            grids, gdims = SB._grids_of(rows.numpy(), self.kind, self.H, self.W)
            src = np.arange(len(grids)) if src_env is None else src_env.numpy()
            return region_numpy_rows(grids, gdims, self.answers[src], self.adims[src], objs, kinds, free_color, through, bits)
    return RegionVenv("o2arc", H, W, 3, O.o2arc_ops(), answers, adims)


def searches(venv, rows, n, depths, before=True):
    """-> (the results of propose_regions(range(10), through=True) at width 1 and depth = the task's number of objects on every task,
    {name: the results of the seven proposers the library had at the same width and depth — the argument lists of
    tests/mirror.py::searches plus propose_mirrors} — empty with before=False)"""
    import mirror as MI
    import torch

    def one(prop):
        return [S.beam_search(venv, rows[i:i + 1], None, width=1, depth=depths[i], src_env=torch.tensor([i]), propose=prop) for i in range(n)]
    painted = one(S.propose_regions(COLOR_OPS, through=True))
    if not before:
        return painted, {}
    earlier = MI.searches(venv, rows, n, depths)
    return painted, dict(earlier[1], mirrors=earlier[0])


# the planted tasks that the seven earlier proposers solve at the same width and depth (the sum over the seven): found with the
# oracle-backed stub (tests/test_region_host.py); the construction is meant to give 0
BEFORE_SOLVES = 0


# ---- one dumped case for the standalone sanitized emulator ------------------------------------------------------------------------
MAGIC = 0x5245474e


def dump_case(path, kind, H, W, cases, layout, C, kinds, free_color, through, with_count, with_src, with_base, with_bits, rng):
    """Writes one case in the format region_emu.cpp's main() reads: buffers exactly as long as the data.  -> the rows without an env"""
    P, PS = H * W, (H * W + 127) & ~127
    pmask = sum(1 << i for i, k in enumerate(B.PLANES[:-1]) if k in O.KIND_PLANES[kind])
    M = len(cases)
    resident = layout == "resident"
    N, ans, adim, src, bad = PL.envs_for(cases, resident, with_src, rng)
    answer = np.full((N, PS), 0x55, np.int8)
    answer[:, :P] = ans.reshape(N, P)
    rec = np.full((N, 16), 0x55, np.int8)
    rec[:, 14:16] = adim
    count, bits = PL.bit_rows(cases, C, with_count, rng)

    def header(stride, res, offset):
        return np.array([MAGIC, H, W, pmask, N, M, stride, C, len(kinds), int(with_count), res, offset, int(with_src), int(with_base), int(free_color),
                         int(through), int(with_bits)], np.int32).tobytes()
    with open(path, "wb") as f:
        if resident:
            rec[:M, 2:4] = np.stack([c["dim"] for c in cases])
            grid = np.full((N, PS), 0x55, np.int8)
            grid[:M, :P] = np.stack([c["grid"].reshape(-1) for c in cases])
            f.write(header(0, 1, 0) + answer.tobytes() + rec.tobytes() + grid.tobytes())
        else:
            buf, offset, stride = CP.place(CP.make_rows(kind, cases, rng), layout)
            f.write(header(stride, 0, offset) + answer.tobytes() + rec.tobytes() + buf.tobytes())
        if with_count:
            f.write(count.tobytes())
        f.write(bits.tobytes())
        if with_src:
            f.write(src.tobytes())
        f.write(np.array(kinds, np.uint8).tobytes())
    return bad


def parse_dump(text, cases, C, S_, with_count, with_base, with_bits):
    """The standalone program's output -> (reg, best, best_bits, base) with SENTINEL where nothing was printed."""
    M = len(cases)
    reg, best = np.full((M, C, S_, 4), SENTINEL, np.int32), np.full((M, C, 4), SENTINEL, np.int32)
    bbits, base = np.full((M, C, B.BITS_STRIDE), SENTINEL, np.uint8), np.full((M, 2), SENTINEL, np.int32)
    lines = text.strip().splitlines()
    i = 0
    for m, c in enumerate(cases):
        if with_base:
            base[m] = [int(v) for v in lines[i].split()]
            i += 1
        for k in range(min(C, len(c["masks"])) if with_count else C):
            for s in range(S_):
                reg[m, k, s] = [int(v) for v in lines[i].split()]
                i += 1
            best[m, k] = [int(v) for v in lines[i].split()]
            i += 1
            if with_bits:
                bbits[m, k] = np.frombuffer(bytes.fromhex(lines[i]), np.uint8)
                i += 1
    assert i == len(lines)
    return reg, best, bbits, base
