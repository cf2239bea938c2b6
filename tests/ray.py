"""Backend-independent checks of arcle_ray_rows (the lines each object of a state row casts toward the answer).  The counterpart of
tests/stamp.py, whose pattern it follows and whose shared pieces it takes from tests/place.py (cases, bit rows, env arrangement,
guards, SENTINEL): every check takes a backend — EmuRay (tests/emu/ray_emu.cpp: the kernel body of arcle_ray.h lock-step on the CPU)
or HipRay (the product) — and returns a list of mismatch strings.  The reference point is arcle_amd.search.ray_numpy, a per-cell walk
straight from the definition, which tests/test_ray_host.py pins on the oracle's own Color step."""
import ctypes
import os
import subprocess

import numpy as np

import backends as B
import components as CP
import place as PL
from arcle_amd import search as S
from oracle import oracle as O

EMU_DIR = CP.EMU_DIR
EMU_SRC = os.path.join(EMU_DIR, "ray_emu.cpp")
EMU_HDRS = PL.EMU_HDRS + [os.path.join(B.ROOT, "arcle_amd", "csrc", "arcle_ray.h")]
SENTINEL = PL.SENTINEL
CS = PL.CS
COLOR_OPS = tuple(range(10))  # both default tables: Color 0 .. 9
# one cell; one row / one column; 3 x 3; 5 x 32: shifts across the whole word; 5 x 5, 7 x 6, 6 x 9, 20 x 7: the row board under the
# generic width class; 12 x 12; 30 x 30: the fast width; 33 x 31: more than 32 rows; 64 x 16: every lane a row; 3 x 40, 16 x 33 and
# 65 x 15 (H > 64): the flat board
SIZES = ((1, 1), (1, 9), (9, 1), (3, 3), (5, 32), (5, 5), (7, 6), (6, 9), (20, 7), (12, 12), (30, 30), (33, 31), (64, 16), (3, 40), (16, 33), (65, 15))
ORACLE_SIZES = ((5, 5), (7, 6), (6, 9))
DEFAULT = tuple(S.RAY_SETS)
# a non-default set list: n_sets = 16, zero entries, every direction alone and odd mixtures
SETS16 = (0, 128, 64, 32, 16, 8, 4, 2, 1, 0x05, 0x0a, 0x50, 0xa0, 0, 0x96, 0xff)
SET_LISTS = {"default": DEFAULT, "sixteen": SETS16, "one": (0x0f,)}


# ---- the cases: those of tests/place.py and what a ray adds ---------------------------------------------------------------------------
_cases = {}


def draw(grid, seeds, dirs, gh=None, gw=None):
    """numpy: from every seed cell a line of the seed's colour in every direction of `dirs` while the cells are 0, inside (gh, gw) —
    used to build ANSWERS only (the mirror under test is ray_numpy)"""
    H, W = grid.shape
    gh, gw = H if gh is None else gh, W if gw is None else gw
    out = grid.copy()
    for x, y in seeds:
        for d in range(8):
            if (dirs >> d) & 1:
                dx, dy = S.RAY_DIRS[d]
                i, j = x + dx, y + dy
                while 0 <= i < gh and 0 <= j < gw and grid[i, j] == 0:
                    out[i, j] = grid[x, y]
                    i, j = i + dx, j + dy
    return out


def cases_of(H, W):
    """The cases of PL.cases_of(H, W) — moved, shrunk a / b (grid_dim below (H, W), a differing answer_dim), bytes (negative bytes
    under rectangles and the whole-grid object, an empty mask), twocolour, the ties — and the cases place never needed:
      lines     a blank grid with a few one-cell seeds and obstacles of a further colour; the answer holds every seed's orthogonal rays
      star      the same with the seeds' eight rays in the answer, grid_dim one below the plane on both axes
      dense     ten-colour noise, half of it background, a ten-colour answer: every ray is short, every colour board is in use
      shape     an L-shaped object, a ring around a free hole and a ring around an obstacle; the answer holds the L's N | E rays
      fives     the background is 5, not 0 (free_color = 5 lets the rays run, 0 stops them at once)
    (grids of at least 3 x 3)."""
    if (H, W) in _cases:
        return _cases[(H, W)]
    rng = np.random.default_rng(7700 + 131 * H + W)
    out = list(PL.cases_of(H, W))

    def add(name, grid, dim, answer, adim, masks):
        masks = np.asarray(masks, np.uint8).reshape(-1, H, W)[:16]
        out.append({"name": f"{H}x{W} {name}", "H": H, "W": W, "grid": grid.astype(np.int8), "dim": np.asarray(dim, np.int8),
                    "answer": answer.astype(np.int8), "adim": np.asarray(adim, np.int8), "masks": masks})
    if H >= 3 and W >= 3:
        for name, dirs, (gh, gw) in (("lines", 0x0f, (H, W)), ("star", 0xff, (H - 1, W - 1))):
            g = np.zeros((H, W), np.int8)
            cells = rng.permutation(gh * gw)[:max(3, gh * gw // 12)]
            seeds = [(int(c) // gw, int(c) % gw) for c in cells[:max(1, len(cells) // 3)]]
            for c in cells[len(seeds):]:
                g[int(c) // gw, int(c) % gw] = 8
            for i, (x, y) in enumerate(seeds):
                g[x, y] = 1 + i % 7
            n, _, _, masks = S.components_numpy(g, (gh, gw), 16, 0)
            add(name, g, (gh, gw), draw(g, seeds, dirs, gh, gw), (gh, gw), masks[:n + 1])
        g = rng.integers(0, 10, (H, W)) * (rng.random((H, W)) < 0.5)
        n, _, _, masks = S.components_numpy(g, (H, W), 16, 0)
        add("dense", g, (H, W), rng.integers(0, 10, (H, W)), (H, W), masks[:n + 1])
        g = np.zeros((H, W), np.int8)
        g[H - 1, 0] = g[H - 2, 0] = g[H - 1, 1] = 4  # the L
        masks = [g == 4]
        if H >= 7 and W >= 7:
            g[1:4, W - 4:W - 1] = 6
            g[2, W - 3] = 0  # a free hole
            g[H - 4:H - 1, W - 4:W - 1] = 7
            g[H - 3, W - 3] = 9  # a hole that is an obstacle
            masks += [g == 6, g == 7, g == 9]
        add("shape", g, (H, W), draw(g, [(H - 2, 0), (H - 1, 1), (H - 1, 0)], 0x09), (H, W), masks)
        g = np.full((H, W), 5, np.int8)
        g[H // 2, W // 2], g[0, W - 1] = 2, 3
        ans = g.copy()
        ans[H // 2, :] = 2
        add("fives", g, (H, W), ans, (H, W), [g == 2, g == 3])
    _cases[(H, W)] = out
    return out


_mirror = {}


def mirror(case, sets, free_color, through):
    """ray_numpy of a case, computed once per (case, sets, free_color, through) over all its objects: (ray [n, S, 4], best [n, 4],
    base (2,), bits uint8 [n, 128] = the best candidate's cells as a bit row)"""
    key = (case["name"], tuple(sets), int(free_color), bool(through))
    if key not in _mirror:
        ray, best, base, cells = S.ray_numpy(case["grid"], case["dim"], case["answer"], case["adim"], case["masks"], sets, free_color, bool(through), full=True)
        pick = np.stack([cells[k, b] if b >= 0 else np.zeros_like(cells[k, 0]) for k, b in enumerate(best[:, 0])]) if len(best) else cells[:, 0]
        _mirror[key] = (ray, best, base, B.pack_bits(pick))
    return _mirror[key]


# ---- the backends -----------------------------------------------------------------------------------------------------------------
class _RayParams(ctypes.Structure):  # mirror of arcle::RayParams (arcle_amd/csrc/arcle_ray.h)
    _fields_ = [("p", B._StepParams), ("max_comp", ctypes.c_int32), ("n_sets", ctypes.c_int32), ("count", ctypes.c_void_p),
                ("bits", ctypes.c_void_p), ("src_env", ctypes.c_void_p), ("sets", ctypes.c_void_p), ("ray", ctypes.c_void_p),
                ("best", ctypes.c_void_p), ("best_bits", ctypes.c_void_p), ("base", ctypes.c_void_p), ("free_color", ctypes.c_int32),
                ("through", ctypes.c_int32)]


_emu = None


def emu_lib():
    global _emu
    if _emu is None:
        so = os.path.join(EMU_DIR, "libray_emu.so")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [EMU_SRC] + EMU_HDRS):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, EMU_SRC])
        _emu = ctypes.CDLL(so)
        _emu.ray_emu_run.argtypes = [ctypes.POINTER(_RayParams), ctypes.c_int]
        assert _emu.ray_emu_params_size() == ctypes.sizeof(_RayParams), "RayParams layout drifted"
    return _emu


class EmuRay:
    """The emulated kernel.  fw: -1 = the instantiation the library launches for the width, 0 = FW_GENERIC at any width."""
    BACKEND = B.EmuBackend  # (a subclass may name a backend of another plane stride)
    name = "emu"

    def __init__(self, fw=-1):
        self.fw = fw

    def run(self, kind, H, W, cases, layout, C, sets, free_color, through, with_count, with_src, with_base, with_bits, rng):
        M, S_ = len(cases), len(sets)
        resident = layout == "resident"
        N, ans, adim, src, bad = PL.envs_for(cases, resident, with_src, rng)
        be = self.BACKEND(N, H, W, 3, kind, CP.OPS[kind]())
        for k in be.buf:
            be.buf[k][:] = 0x55
        be.rec[:] = 0x55
        be.buf["answer"][:, :H * W] = ans.reshape(N, -1)
        be.rec[:, 14:16] = adim
        x = _RayParams()
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
        sets_a = np.array(sets, np.uint8)
        self.guards = [PL._guarded((M, C, S_, 4)), PL._guarded((M, C, 4)), PL._guarded((M, C, B.BITS_STRIDE), np.uint8), PL._guarded((M, 2))]
        (_, ray), (_, best), (_, bbits), (_, base) = self.guards
        x.max_comp, x.n_sets, x.free_color, x.through = C, S_, int(free_color), int(through)
        x.count, x.bits, x.src_env = count.ctypes.data if with_count else None, bits.ctypes.data, None if src is None else src.ctypes.data
        x.sets, x.ray, x.best = sets_a.ctypes.data, ray.ctypes.data, best.ctypes.data
        x.best_bits, x.base = bbits.ctypes.data if with_bits else None, base.ctypes.data if with_base else None
        rc = emu_lib().ray_emu_run(ctypes.byref(x), self.fw)
        assert rc == 0, f"ray emulator reported error {rc} (divergent cross-lane op / non-uniform value)"
        return ray, best, bbits, base, bad

    def guards_intact(self):
        return all((buf[:16] == buf.dtype.type(SENTINEL)).all() and (buf[-16:] == buf.dtype.type(SENTINEL)).all() for buf, _ in self.guards)


class HipRay:
    """EnvBatch.ray_rows on the device."""
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

    def run(self, kind, H, W, cases, layout, C, sets, free_color, through, with_count, with_src, with_base, with_bits, rng):
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
        bufs, (ray, best, bbits, base) = self.outputs(b.device, M, C, len(sets))
        b.ray_rows(view, t.as_tensor(count, device=b.device) if with_count else None, t.as_tensor(bits, device=b.device),
                   t.as_tensor(np.array(sets, np.uint8), device=b.device), free_color, bool(through),
                   None if src is None else t.as_tensor(src, device=b.device), out=(ray, best, bbits if with_bits else None, base if with_base else None))
        self._ok = all(bool((g[:16] == SENTINEL).all()) and bool((g[-16:] == SENTINEL).all()) for g in bufs)
        return ray.cpu().numpy(), best.cpu().numpy(), bbits.cpu().numpy(), base.cpu().numpy(), bad

    def guards_intact(self):
        return self._ok


def compare(tag, got, cases, C, sets, free_color, through, with_count, with_base, with_bits):
    """Everything exact: the four words of every candidate, the best slot, its bit row, the base pair, SENTINEL in the entries >= count
    and in the outputs not asked for."""
    ray, best, bbits, base, bad = got
    S_ = len(sets)
    errs = []
    for m, c in enumerate(cases):
        wr, wb, wbase, wbits = mirror(c, sets, free_color, through)
        n = min(C, len(wr))
        t = f"{tag} row {m} ({c['name']})"
        empty_ray, empty_best = (0, wbase[0], 0, 0), (-1, 0, wbase[0], 0)
        if m in bad:
            wr, wb, wbits, wbase = np.zeros_like(wr), np.zeros_like(wb), np.zeros_like(wbits), (0, 0)
            empty_ray, empty_best = (0, 0, 0, 0), (0, 0, 0, 0)
        if not np.array_equal(ray[m, :n], wr[:n]):
            k, s = (int(v) for v in np.argwhere((ray[m, :n] != wr[:n]).any(2))[0])
            errs.append(f"{t}: object {k} set {s} (mask {sets[s]:#x}) {ray[m, k, s].tolist()} != {wr[k, s].tolist()}")
        if not np.array_equal(best[m, :n], wb[:n]):
            k = int(np.argwhere((best[m, :n] != wb[:n]).any(1))[0, 0])
            errs.append(f"{t}: object {k} best {best[m, k].tolist()} != {wb[k].tolist()}")
        if with_bits and not np.array_equal(bbits[m, :n], wbits[:n]):
            k = int(np.argwhere((bbits[m, :n] != wbits[:n]).any(1))[0, 0])
            errs.append(f"{t}: object {k} best_bits differ from the mirror's cells of set {int(wb[k, 0])}")
        if not with_bits and (bbits[m] != np.uint8(SENTINEL)).any():
            errs.append(f"{t}: best_bits was written though not asked for")
        if with_count:
            if (ray[m, n:] != SENTINEL).any() or (best[m, n:] != SENTINEL).any() or (with_bits and (bbits[m, n:] != np.uint8(SENTINEL)).any()):
                errs.append(f"{t}: an entry >= count was written")
        else:  # (the slots beyond the case's masks hold empty masks: B empty)
            if (ray[m, n:] != np.array(empty_ray)).any() or (best[m, n:] != np.array(empty_best)).any() or (with_bits and bbits[m, n:].any()):
                errs.append(f"{t}: an empty mask gave {ray[m, n:].reshape(-1, 4)[:1].tolist()} / {best[m, n:][:1].tolist()}")
        if with_base and tuple(int(v) for v in base[m]) != tuple(wbase):
            errs.append(f"{t}: base {base[m].tolist()} != {tuple(wbase)}")
        if not with_base and (base[m] != SENTINEL).any():
            errs.append(f"{t}: base was written though not asked for")
    return errs


# size -> the runs of one backend: (kind, layout | "resident", M, C, set list, free_color, through, count given, src given, base asked
# for, best_bits asked for).  Per size: every env kind, the three layouts and the resident form, M = 1 and 37 (None: one row per case),
# every C of CS, the three set lists, both `through` values, free_color 0, 5 and -1, count and NULL, src and NULL, base and best_bits
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
    for i, (kind, layout, M, C, setname, fc, through, with_count, with_src, with_base, with_bits) in enumerate(runs):
        cases = cases_of(H, W)
        sets = SET_LISTS[setname]
        if isinstance(M, str):
            cases = [c for c in cases if c["name"].endswith(M)] or cases[:1]
        elif M is not None:
            cases = PL.pad_to(cases, M) if M > 1 else cases[i % len(cases):][:1]
        tag = f"{be.name} {H}x{W} {kind} {layout} C={C} sets={setname} free={fc} through={int(through)} count={with_count} src={with_src}"
        got = be.run(kind, H, W, cases, layout, C, sets, fc, through, with_count, with_src, with_base, with_bits, rng)
        errs += compare(tag, got, cases, C, sets, fc, through, with_count, with_base, with_bits)
        if not be.guards_intact():
            errs.append(f"{tag}: bytes around an output buffer were written")
        if len(errs) > 10:
            break
    return errs


# ---- the oracle's side: ONE Color c step on the candidate's cells -----------------------------------------------------------------------
def oracle_children(case, sets, through, kind="o2arc"):
    """For every object, set and colour c the first number of the dense pair the ORACLE reports after `Color c` on the mirror's cells of
    that candidate (mask ingress, tests/macros.py's chained oracle with macros of one step) -> (dense int [n, S, 10], -1 where the
    candidate is empty; the mirror's (ray, best, base, cells) on the grid the oracle's freshly reset env holds)."""
    import macros as MC
    import search_bits as SB
    H, W = case["H"], case["W"]
    rows, orc = CP.clean_rows(kind, case["grid"][None], case["dim"][None], case["answer"][None], case["adim"][None])
    grid = SB._grids_of(rows, kind, H, W)[0][0]
    got = S.ray_numpy(grid, case["dim"], case["answer"], case["adim"], case["masks"], sets, 0, through, full=True)
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


# ---- planted tasks: one-cell seeds whose rays the answer holds ------------------------------------------------------------------------
# (directions, seeds) per task: orthogonal cross, diagonal cross, star — one seed each: two such seeds' rays cross almost anywhere —,
# N|S twice, W|E thrice, E thrice, N twice, W|E twice: parallel lines of several seeds never cross
PLANTED = ((0x0f, 1), (0xf0, 1), (0xff, 1), (0x03, 2), (0x0c, 3), (0x08, 3), (0x01, 2), (0x0c, 2))


def planted_ray_tasks(n=8, H=12, W=12, seed=6):
    """n tasks on background 0: 1 to 3 one-cell seeds of distinct colours (1 .. 7) and a few obstacle cells of colour 8; the answer holds
    every seed's rays for the task's direction set (PLANTED), stopped by the obstacles, the other seeds and the edge.  Seeds are
    placed so that no ray of one seed touches a cell another seed's rays cover or another seed itself, no obstacle sits next to a seed
    in a direction of the set, and the answer has at least 12 new cells.  -> (inputs [n, H, W], dims [n, 2], answers [n, H, W], the
    number of seeds per task)"""
    rng = np.random.default_rng(seed)
    dims = np.tile(np.array([[H, W]], np.int8), (n, 1))
    inputs, answers, depths = [], [], []
    for _ in range(20000):
        if len(inputs) == n:
            break
        dirs, want = PLANTED[len(inputs) % len(PLANTED)]
        g = np.zeros((H, W), np.int8)
        spots = rng.permutation(H * W)[:want + 4]
        seeds = [(int(c) // W, int(c) % W) for c in spots[:want]]
        for c in spots[want:]:
            g[int(c) // W, int(c) % W] = 8
        for (x, y), col in zip(seeds, rng.permutation(7)[:want] + 1):
            g[x, y] = col
        alone = [draw(g, [sd], dirs) != g for sd in seeds]
        cover = np.sum(alone, 0)
        if (cover > 1).any() or int(cover.sum()) < 12 or any(a.sum() < 2 for a in alone):
            continue  # (rays cross, too few new cells, or a seed that draws next to nothing)
        if any(abs(a[0] - b[0]) <= 1 and abs(a[1] - b[1]) <= 1 for k, a in enumerate(seeds) for b in seeds[:k]):
            continue  # (two seeds would be ONE 8-connected object)
        inputs.append(g)
        answers.append(draw(g, seeds, dirs))
        depths.append(want)
    assert len(inputs) == n, "planted_ray_tasks: no such tasks at this seed"
    return np.stack(inputs), dims, np.stack(answers), depths


def ray_numpy_rows(grids, gdims, answers, adims, objs, sets, free_color, through, bits=True):
    """`ARCVecEnv.rays` of M grids from ray_numpy, on torch CPU tensors (the stub vec envs' `rays`)."""
    import torch
    from arcle_amd.envs.vec import Rays
    sets = S.RAY_SETS if sets is None else sets
    M, C, S_ = int(objs.bits.shape[0]), int(objs.bits.shape[1]), len(sets)
    H, W = grids.shape[1:]
    ray, best, bb, base = np.zeros((M, C, S_, 4), np.int32), np.zeros((M, C, 4), np.int32), np.zeros((M, C, B.BITS_STRIDE), np.uint8), np.zeros((M, 2), np.int32)
    cells = np.unpackbits(objs.bits.numpy(), axis=-1, bitorder="little")[..., :H * W].reshape(M, C, H, W)
    for m in range(M):
        n = int(objs.count[m])
        r, b, base[m], sel = S.ray_numpy(grids[m], gdims[m], answers[m], adims[m], cells[m, :n], sets, free_color, through, full=True)
        ray[m, :n], best[m, :n] = r, b
        for k in range(n):
            if b[k, 0] >= 0:
                bb[m, k] = B.pack_bits(sel[k, b[k, 0]][None])[0]
    t, u = torch.from_numpy(ray), torch.from_numpy(best)
    return Rays(t[..., 0], t[..., 1], t[..., 2], t[..., 3], u[..., 0], u[..., 1], u[..., 2], u[..., 3], torch.from_numpy(bb) if bits else None,
                torch.from_numpy(base))


def ray_venv(answers, adims, H=12, W=12):
    """The oracle-backed stub vec env of tests/align.py (place, stamp, turn, align from their mirrors) + `rays` (ray_numpy): what
    beam_search(propose=propose_rays(...)) and the five earlier proposers need, on torch CPU tensors."""
    import align as AL
    import search_bits as SB
    import stamp as ST
    import turn as TU
    base = type(AL.align_venv(answers, adims, H, W))

    class RayVenv(base):
        def rays(self, rows, objs, sets=None, free_color=0, through=False, src_env=None, bits=True):
            grids, gdims = SB._grids_of(rows.numpy(), self.kind, self.H, self.W)
            src = np.arange(len(grids)) if src_env is None else src_env.numpy()
            return ray_numpy_rows(grids, gdims, self.answers[src], self.adims[src], objs, sets, free_color, through, bits)

        def stamp(self, rows, objs, src_env=None, max_dist=None, blank=True):
            grids, gdims = SB._grids_of(rows.numpy(), self.kind, self.H, self.W)
            src = np.arange(len(grids)) if src_env is None else src_env.numpy()
            return ST.stamp_numpy_rows(grids, gdims, self.answers[src], self.adims[src], objs, max_dist, blank)

        def turn(self, rows, objs, src_env=None, max_dist=None, turns=31):
            grids, gdims = SB._grids_of(rows.numpy(), self.kind, self.H, self.W)
            src = np.arange(len(grids)) if src_env is None else src_env.numpy()
            return TU.turn_numpy_rows(grids, gdims, self.answers[src], self.adims[src], objs, max_dist, turns)
    return RayVenv("o2arc", H, W, 3, O.o2arc_ops(), answers, adims)


def searches(venv, rows, n, depths, before=True):
    """-> (the results of propose_rays(range(10)) at width 1 and depth = the task's number of seeds on every task, {name: the results
    of the five proposers the library had at the same width and depth — the argument lists of tests/align.py::searches, with the
    Colour ops 0-9 among propose_objects' box ops} — empty with before=False)"""
    import align as AL
    import torch

    def one(prop):
        return [S.beam_search(venv, rows[i:i + 1], None, width=1, depth=depths[i], src_env=torch.tensor([i]), propose=prop) for i in range(n)]
    cast = one(S.propose_rays(COLOR_OPS))
    if not before:
        return cast, {}
    return cast, {"objects": one(S.propose_objects(list(PL.MOVE_OPS) + [29] + list(COLOR_OPS), list(range(10, 20)), masks=True, any_color=True, diagonal=True)),
                  "placements": one(S.propose_placements(PL.MOVE_OPS, any_color=True, diagonal=True)),
                  "stamps": one(S.propose_stamps(29, 30, any_color=True, diagonal=True)),
                  "turns": one(S.propose_turns((24, -1, 25, 26, 27), PL.MOVE_OPS, any_color=True, diagonal=True)),
                  "alignments": one(S.propose_alignments(*AL.ALIGN_OPS["o2arc"]))}


# ---- one dumped case for the standalone sanitized emulator ------------------------------------------------------------------------
MAGIC = 0x52415953


def dump_case(path, kind, H, W, cases, layout, C, sets, free_color, through, with_count, with_src, with_base, with_bits, rng):
    """Writes one case in the format ray_emu.cpp's main() reads: buffers exactly as long as the data.  -> the rows without an env"""
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
        return np.array([MAGIC, H, W, pmask, N, M, stride, C, len(sets), int(with_count), res, offset, int(with_src), int(with_base), int(free_color),
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
        f.write(np.array(sets, np.uint8).tobytes())
    return bad


def parse_dump(text, cases, C, S_, with_count, with_base, with_bits):
    """The standalone program's output -> (ray, best, best_bits, base) with SENTINEL where nothing was printed."""
    M = len(cases)
    ray, best = np.full((M, C, S_, 4), SENTINEL, np.int32), np.full((M, C, 4), SENTINEL, np.int32)
    bbits, base = np.full((M, C, B.BITS_STRIDE), SENTINEL, np.uint8), np.full((M, 2), SENTINEL, np.int32)
    lines = text.strip().splitlines()
    i = 0
    for m, c in enumerate(cases):
        if with_base:
            base[m] = [int(v) for v in lines[i].split()]
            i += 1
        for k in range(min(C, len(c["masks"])) if with_count else C):
            for s in range(S_):
                ray[m, k, s] = [int(v) for v in lines[i].split()]
                i += 1
            best[m, k] = [int(v) for v in lines[i].split()]
            i += 1
            if with_bits:
                bbits[m, k] = np.frombuffer(bytes.fromhex(lines[i]), np.uint8)
                i += 1
    assert i == len(lines)
    return ray, best, bbits, base
