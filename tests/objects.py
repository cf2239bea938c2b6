"""Backend-independent checks of arcle_objects_rows (arcle_components_rows under four notions of "object": same- or multi-colour, 4- or
8-connected, with an optional colour set per object).  The pattern of tests/components.py, whose make_rows / place / fixture this file
imports: every check takes a backend — EmuObjects (tests/emu/objects_emu.cpp: the kernel body of arcle_objects.h lock-step on the CPU)
or HipObjects (the product) — and returns a list of mismatch strings.

The reference has no labelling but its dfs, so the reference point of the new modes is `uf_objects` below: a union-find over
neighbouring cell pairs that shares no code with the BFS of arcle_amd.search.components_numpy.  tests/test_objects_host.py pins the
two on each other over every grid used here, and mode 0 on tests/golden/components/components.npz (the reference's own dfs)."""
import ctypes
import os
import subprocess

import numpy as np

import backends as B
import components as CP
from arcle_amd import search as S
from oracle import oracle as O

EMU_DIR = CP.EMU_DIR
EMU_SRC = os.path.join(EMU_DIR, "objects_emu.cpp")
EMU_HDRS = CP.EMU_HDRS + [os.path.join(B.ROOT, "arcle_amd", "csrc", "arcle_objects.h")]
SKIPS, SENTINEL, LAYOUTS = CP.SKIPS, CP.SENTINEL, CP.LAYOUTS
ANY, DIAG = 1, 2  # ARCLE_OBJ_ANY_COLOR, ARCLE_OBJ_DIAG
MODES = (0, ANY, DIAG, ANY | DIAG)
# the smallest shapes that reach each code path: one cell; one row / one column (DIAG must behave as 4-connected); 3 x 3 and 5 x 5;
# 20 x 7: the row board under the generic width class, rows on both sides of the lane-15/16 DPP row boundary; 30 x 30: the fast
# width; 64 x 16: all 64 lanes of the row board; 3 x 40 and 16 x 33: the flat board with W > 32; 8 x 127: the flat board at the widest W
SIZES = ((1, 1), (1, 9), (9, 1), (3, 3), (5, 5), (20, 7), (30, 30), (64, 16), (3, 40), (16, 33), (8, 127))


# ---- the independent labelling: union-find over neighbouring cell pairs -------------------------------------------------------------
def uf_objects(grid, dim, skip=-1, any_color=False, diagonal=False):
    """Every object of one grid -> (comp int32 [n, 8], masks uint8 [n, H, W], colors uint32 [n]) in ascending row-major index of
    the first cell, uncut."""
    grid = np.asarray(grid)
    H, W = grid.shape
    gh, gw = min(int(dim[0]), H), min(int(dim[1]), W)
    member = np.zeros((H, W), bool)
    member[:gh, :gw] = True
    if skip >= 0:
        member &= grid.astype(np.int64) != (int(skip) + 128) % 256 - 128
    parent = list(range(H * W))

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if diagonal else [])
    for dx, dy in steps:
        for x in range(gh - dx):
            for y in range(max(0, -dy), gw - max(0, dy)):
                if member[x, y] and member[x + dx, y + dy] and (any_color or grid[x, y] == grid[x + dx, y + dy]):
                    ra, rb = find(x * W + y), find((x + dx) * W + y + dy)
                    if ra != rb:
                        parent[max(ra, rb)] = min(ra, rb)  # the root of a set is its lowest cell: the seed
    roots = np.array([find(f) if member.flat[f] else -1 for f in range(H * W)]).reshape(H, W)
    seeds = np.unique(roots[roots >= 0])
    comp, masks, colors = np.zeros((len(seeds), 8), np.int32), np.zeros((len(seeds), H, W), np.uint8), np.zeros(len(seeds), np.uint32)
    for k, s in enumerate(seeds):
        m = roots == s
        xs, ys = np.nonzero(m)
        masks[k] = m
        comp[k] = (xs.min(), ys.min(), xs.max(), ys.max(), s // W, s % W, int(grid.flat[s]), m.sum())
        for v in np.unique(grid[m]):
            colors[k] |= np.uint32(1) << np.uint32(int(v) & 31)
    return comp, masks, colors


_mirror = {}


def mirror(case, C, skip, mode):
    """uf_objects of a case, computed once per (case, skip, mode), cut at C: (n, left, comp [n, 8], bit rows [n, 128], colors [n])"""
    key = (case["name"], case["H"], case["W"], skip, mode)
    if key not in _mirror:
        comp, masks, colors = uf_objects(case["grid"], case["dim"], skip, bool(mode & ANY), bool(mode & DIAG))
        _mirror[key] = (comp, B.pack_bits(masks) if len(masks) else np.zeros((0, B.BITS_STRIDE), np.uint8), colors)
    comp, bits, colors = _mirror[key]
    n = min(C, len(comp))
    return n, int(comp[n:, 7].sum()), comp[:n], bits[:n], colors[:n]


# ---- the grids --------------------------------------------------------------------------------------------------------------------
_cases = {}


def cases_of(H, W):
    """The fixture's grids of the size (tests/golden/components) and the generated ones: 3-colour noise; a two-colour checkerboard
    (skip -1: H * W objects 4-connected, 2 same-colour 8-connected, 1 multi-colour); the full diagonal and anti-diagonal (one cell
    per closure pass); a zig-zag staircase over every row, of two colours; cells (r, W - 1) and (r + 2, 0) only — W + 1 apart on the
    flat board, never one object; a grid_dim smaller than H x W with garbage outside; arbitrary bytes (the colour words take v & 31)."""
    if (H, W) in _cases:
        return _cases[(H, W)]
    rng = np.random.default_rng(7000 + 131 * H + W)
    full = np.array([H, W], np.int8)
    out = [dict(c) for c in CP.cases_of(H, W)] if (H, W) in CP.sizes() else []

    def add(name, g, dim=full):
        out.append({"name": f"{H}x{W} gen {name}", "H": H, "W": W, "grid": g.astype(np.int8), "dim": np.asarray(dim, np.int8)})
    add("noise3", rng.choice([0, 3, 5], (H, W)))
    xx, yy = np.mgrid[0:H, 0:W]
    add("checker35", np.where((xx + yy) % 2 == 0, 3, 5))
    n = min(H, W)
    g = np.zeros((H, W), np.int8)
    g[np.arange(n), np.arange(n)] = 5
    add("diagonal", g)
    g = np.zeros((H, W), np.int8)
    g[np.arange(n), W - 1 - np.arange(n)] = 5
    add("antidiagonal", g)
    g = np.zeros((H, W), np.int8)
    amp = max(1, min(W - 1, 3))
    tri = [abs((i + amp) % (2 * amp) - amp) if W > 1 else 0 for i in range(H)]  # columns 3 2 1 0 1 2 3 2 ...: every step is diagonal
    g[np.arange(H), tri] = np.where((np.arange(H) // 3) % 2 == 0, 5, 3)
    add("zigzag", g)
    if H >= 3:
        g = np.zeros((H, W), np.int8)
        for r in range(0, H - 2, 3):
            g[r, W - 1] = 5
            g[r + 2, 0] = 5
        add("wrap2", g)
    g = rng.integers(-128, 128, (H, W)).astype(np.int8)
    gh, gw = max(1, H - 2), max(1, W - 3)
    g[:gh, :gw] = rng.choice([0, 3, 5], (gh, gw))
    add(f"shrunk dim {gh}x{gw}", g, (gh, gw))
    add("bytes", rng.choice([-128, -1, 0, 3, 5, 37, 127], (H, W)))
    _cases[(H, W)] = out
    return out


def small(cases, mode, skip=-1, limit=40):
    """The cases of at most `limit` objects (the emulator's time goes with the number of objects; the device takes them all)."""
    return [c for c in cases if mirror(c, 1024, skip, mode)[0] <= limit]


# ---- the backends -----------------------------------------------------------------------------------------------------------------
class _ObjParams(ctypes.Structure):  # mirror of arcle::ObjParams (arcle_amd/csrc/arcle_objects.h)
    _fields_ = [("c", CP._CompParams), ("colors", ctypes.c_void_p)]


_emu = None


def emu_lib():
    global _emu
    if _emu is None:
        so = os.path.join(EMU_DIR, "libobjects_emu.so")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [EMU_SRC] + EMU_HDRS):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, EMU_SRC])
        _emu = ctypes.CDLL(so)
        _emu.objects_emu_run.argtypes = [ctypes.POINTER(_ObjParams), ctypes.c_int, ctypes.c_int]
        assert _emu.objects_emu_params_size() == ctypes.sizeof(_ObjParams), "ObjParams layout drifted"
    return _emu


def _outputs(M, C, bits, colors):
    return (np.full((M, 2), SENTINEL, np.int32), np.full((M, C, 8), SENTINEL, np.int32),
            np.full((M, C, B.BITS_STRIDE), SENTINEL, np.uint8) if bits else None, np.full((M, C), SENTINEL, np.uint32) if colors else None)


class EmuObjects:
    """The emulated kernel.  fw: -1 = the instantiation the library launches for the width, 0 = FW_GENERIC at any width."""
    BACKEND = B.EmuBackend  # (tests/strides.py: a subclass of another plane stride)
    name, limit = "emu", 40

    def __init__(self, fw=-1):
        self.fw = fw

    def _run(self, be, M, C, skip, mode, bits, colors, rows_ptr, stride):
        x = _ObjParams()
        p = be._params()
        p.n_resident, p.n_envs = be.N, M
        p.rows_in, p.rows_in_stride = rows_ptr, stride
        x.c.p = p
        out = _outputs(M, C, bits, colors)
        x.c.max_comp, x.c.skip_color = C, skip
        x.c.count, x.c.comp, x.c.bits = out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data if bits else None
        x.colors = out[3].ctypes.data if colors else None
        rc = emu_lib().objects_emu_run(ctypes.byref(x), self.fw, mode)
        assert rc == 0, f"objects emulator reported error {rc} (divergent cross-lane op / non-uniform value)"
        return out

    def rows(self, kind, H, W, rows, layout, C, skip, mode, bits, colors):
        be = self.BACKEND(2, H, W, 3, kind, CP.OPS[kind]())
        buf, offset, stride = CP.place(rows, layout)
        return self._run(be, rows.shape[0], C, skip, mode, bits, colors, buf.ctypes.data + offset, stride)

    def resident(self, kind, H, W, rows, cases, C, skip, mode, bits, colors):
        M = len(cases)
        be = self.BACKEND(M, H, W, 3, kind, CP.OPS[kind]())
        for k in be.buf:
            be.buf[k][:] = 0x55
        be.rec[:] = 0x55
        be.buf["grid"][:, :H * W] = np.stack([c["grid"].reshape(-1) for c in cases])
        be.rec[:, 2:4] = np.stack([c["dim"] for c in cases])
        return self._run(be, M, C, skip, mode, bits, colors, None, 0)


class HipObjects:
    """EnvBatch.objects_rows on the device."""
    PLANE_STRIDE = None  # override, as HipBackend's: passed on as EnvBatch(plane_stride=)
    name, limit = "hip", 1024

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

    def _out(self, b, M, C, bits, colors):
        t = self.t
        return (t.full((M, 2), SENTINEL, dtype=t.int32, device=b.device), t.full((M, C, 8), SENTINEL, dtype=t.int32, device=b.device),
                t.full((M, C, B.BITS_STRIDE), SENTINEL, dtype=t.uint8, device=b.device) if bits else None,
                t.full((M, C), SENTINEL, dtype=t.int32, device=b.device) if colors else None)

    def _np(self, out):
        out = [None if o is None else o.cpu().numpy() for o in out]
        if out[3] is not None:
            out[3] = out[3].view(np.uint32)
        return tuple(out)

    def _call(self, b, view, M, C, skip, mode, bits, colors):
        return self._np(b.objects_rows(view, C, skip, bool(mode & ANY), bool(mode & DIAG), bits, colors, out=self._out(b, M, C, bits, colors)))

    def rows(self, kind, H, W, rows, layout, C, skip, mode, bits, colors):
        t = self.t
        b = self.batch(kind, H, W, 2)
        buf, offset, stride = CP.place(rows, layout)
        M, L = rows.shape
        dbuf = t.as_tensor(buf, device=b.device)  # (exactly the bytes of the rows: the last row ends the allocation)
        return self._call(b, t.as_strided(dbuf, (M, L), (stride, 1), offset), M, C, skip, mode, bits, colors)

    def resident(self, kind, H, W, rows, cases, C, skip, mode, bits, colors):
        t = self.t
        M = len(cases)
        b = self.batch(kind, H, W, M)
        b.set_state_rows(t.as_tensor(rows, device=b.device))
        return self._call(b, None, M, C, skip, mode, bits, colors)


def compare(tag, got, cases, C, skip, mode, bits, colors):
    """Everything exact: (written, left), every descriptor, every bit row, every colours word, and the sentinels beyond `written`."""
    count, comp, mb, cw = got
    errs = []
    for m, c in enumerate(cases):
        n, left, wc, wb, wcol = mirror(c, C, skip, mode)
        t = f"{tag} row {m} ({c['name']})"
        if (int(count[m, 0]), int(count[m, 1])) != (n, left):
            errs.append(f"{t}: (written, left) {count[m].tolist()} != {(n, left)}")
            continue
        if not np.array_equal(comp[m, :n], wc):
            k = int(np.argwhere((comp[m, :n] != wc).any(1))[0, 0])
            errs.append(f"{t}: object {k} {comp[m, k].tolist()} != {wc[k].tolist()}")
        if (comp[m, n:] != SENTINEL).any():
            errs.append(f"{t}: an entry >= written was written")
        if bits:
            if not np.array_equal(mb[m, :n], wb):
                errs.append(f"{t}: bit masks differ (first: object {int(np.argwhere((mb[m, :n] != wb).any(1))[0, 0])})")
            if (mb[m, n:] != SENTINEL).any():
                errs.append(f"{t}: a bit mask >= written was written")
        if colors:
            if not np.array_equal(cw[m, :n], wcol):
                k = int(np.argwhere(cw[m, :n] != wcol)[0, 0])
                errs.append(f"{t}: colours of object {k} {int(cw[m, k]):#x} != {int(wcol[k]):#x}")
            if (cw[m, n:] != SENTINEL).any():
                errs.append(f"{t}: a colours word >= written was written")
    return errs


# (size, mode) -> the runs of one backend: (kind, C, skip, layout | "resident", bits, colors, M).  Per size and mode: every env kind
# (the grid offset differs), every C of (1, 5, 1024), every skip colour, the three layouts and the resident form, M = 1 and M = 37,
# bits and colours on and off; 30 x 30 takes the whole C x skip product.  M: None = one row per case of the size; "small" = the cases
# of at most `be.limit` objects under the run's mode and skip colour (C = 1024 writes them all; the device takes every case); an int = the cases repeated to M rows.
def plan(H, W):
    runs = [("o2arc", 1024, -1, "odd", True, True, "small"), ("arc", 5, 0, "dense", True, False, None), ("raw", 1, 3, "lib", False, True, 1),
            ("raw", 5, -1, "resident", True, True, None), ("o2arc", 1, 0, "lib", False, False, 37), ("arc", 1024, 3, "resident", False, True, "small")]
    if (H, W) == (30, 30):
        runs += [("o2arc", C, s, "lib", C == 5, s == 0, 37 if C < 1024 else "small") for C in (1, 5, 1024) for s in SKIPS]
    return runs


def run_size(be, H, W, modes=MODES, runs=None):
    errs = []
    rng = np.random.default_rng(H * 1000 + W)
    for mode in modes:
        for kind, C, skip, layout, bits, colors, M in (runs or plan(H, W)):
            cases = cases_of(H, W)
            if M == "small":
                cases = small(cases, mode, skip, be.limit)
            elif M is not None:
                cases = CP.pad_to(cases, M) if M > 1 else cases[mode:mode + 1]
            rows = CP.make_rows(kind, cases, rng)
            tag = f"{be.name} {H}x{W} mode {mode} {kind} C={C} skip={skip} {layout}"
            if layout == "resident":
                got = be.resident(kind, H, W, rows, cases, C, skip, mode, bits, colors)
            else:
                got = be.rows(kind, H, W, rows, layout, C, skip, mode, bits, colors)
            errs += compare(tag, got, cases, C, skip, mode, bits, colors)
            if len(errs) > 10:
                return errs
    return errs


# ---- planted tasks only a whole object solves: a two-colour shape, a diagonal line --------------------------------------------------
MOVE_OPS = CP.MOVE_OPS
TWO_COLOUR = (((0, 0), (0, 1), (1, 0)), ((1, 1), (2, 1), (2, 0)))  # two 3-cell parts, 4-adjacent along (1, 0)-(1, 1) and (0, 1)-(1, 1)


def planted_whole_object_tasks(n=8, H=12, W=12, seed=3):
    """n tasks on background 0, even: ONE object of two colours whose colour parts are 4-adjacent (neither part is the object);
    odd: one diagonal line of three cells of one colour.  The answer, made by the ORACLE: one Move of the whole object, selected by
    its exact cells.  -> (inputs [n, H, W], dims [n, 2], answers [n, H, W], the planted (mask bool [H, W], op) per task)"""
    rng = np.random.default_rng(seed)
    ops = O.o2arc_ops()
    dims = np.tile(np.array([[H, W]], np.int8), (n, 1))
    inputs, answers, steps = [], [], []
    while len(inputs) < n:
        i = len(inputs)
        g = np.zeros((H, W), np.int8)
        x, y = int(rng.integers(2, H - 5)), int(rng.integers(2, W - 5))
        c1, c2 = (int(c) for c in rng.permutation(np.arange(1, 10))[:2])
        if i % 2 == 0:
            for part, col in zip(TWO_COLOUR, (c1, c2)):
                for a, b in part:
                    g[x + a, y + b] = col
        else:
            flip = int(rng.integers(0, 2))
            for a in range(3):
                g[x + a, y + (2 - a if flip else a)] = c1
        mask = g != 0
        op = int(rng.choice(MOVE_OPS))
        orc = B.OracleBackend(1, H, W, 3, "o2arc", ops)
        orc.set_tasks(g[None], dims[:1], g[None], dims[:1])
        orc.reset()
        orc.step("mask", mask[None].astype(np.int8), np.array([op], np.int32))
        ans = orc.get("grid")[0]
        assert not orc.status() and (ans != 0).sum() == mask.sum() and not np.array_equal(ans, g)
        inputs.append(g)
        answers.append(ans)
        steps.append((mask, op))
    return np.stack(inputs), dims, np.stack(answers), steps


def objects_numpy(grids, gdims, max_components, skip_color, any_color, diagonal, bits, colors):
    """`ARCVecEnv.objects` of M grids from components_numpy, on torch CPU tensors (the stub vec envs' `objects`)."""
    import torch
    from arcle_amd.envs.vec import Objects
    M, C = len(grids), int(max_components)
    count, left, comp = np.zeros(M, np.int32), np.zeros(M, np.int32), np.zeros((M, C, 8), np.int32)
    mbits, cw = np.zeros((M, C, B.BITS_STRIDE), np.uint8), np.zeros((M, C), np.uint32)
    for m in range(M):
        count[m], left[m], comp[m], masks = S.components_numpy(grids[m], gdims[m], C, skip_color, any_color, diagonal)
        mbits[m] = B.pack_bits(masks)
        cw[m, :count[m]] = S.component_colors_numpy(grids[m], masks[:count[m]])
    t = torch.from_numpy(comp)
    return Objects(torch.from_numpy(count), torch.from_numpy(left), t[:, :, 0:4], t[:, :, 4:6], t[:, :, 6], t[:, :, 7],
                   torch.from_numpy(mbits) if bits else None, torch.from_numpy(cw.view(np.int32)) if colors else None)


def whole_object_searches(venv, rows, n):
    """The two searches of the demonstration on every task -> (results with the 4-connected one-colour components, results with
    multi-colour 8-connected objects): width 1, depth 1, Move ops on the objects' exact cells."""
    import torch
    narrow = [S.beam_search(venv, rows[i:i + 1], None, width=1, depth=1, src_env=torch.tensor([i]), propose=S.propose_objects(MOVE_OPS, [], masks=True))
              for i in range(n)]
    wide = [S.beam_search(venv, rows[i:i + 1], None, width=1, depth=1, src_env=torch.tensor([i]),
                          propose=S.propose_objects(MOVE_OPS, [], masks=True, any_color=True, diagonal=True)) for i in range(n)]
    return narrow, wide


# ---- one dumped case for the standalone sanitized emulator ------------------------------------------------------------------------
MAGIC = 0x4f424a53


def dump_case(path, kind, H, W, cases, C, skip, mode, bits, colors, layout, rng):
    """Writes one case in the format objects_emu.cpp's main() reads: buffers exactly as long as the data."""
    P, PS = H * W, (H * W + 127) & ~127
    mask = sum(1 << i for i, k in enumerate(B.PLANES[:-1]) if k in O.KIND_PLANES[kind])
    M = len(cases)
    rows = CP.make_rows(kind, cases, rng)
    with open(path, "wb") as f:
        if layout == "resident":
            f.write(np.array([MAGIC, H, W, mask, M, M, 0, C, skip, int(bits), 1, 0, mode, int(colors)], np.int32).tobytes())
            grid = np.full((M, PS), 0x55, np.int8)
            grid[:, :P] = np.stack([c["grid"].reshape(-1) for c in cases])
            rec = np.full((M, 16), 0x55, np.int8)
            rec[:, 2:4] = np.stack([c["dim"] for c in cases])
            f.write(grid.tobytes())
            f.write(rec.tobytes())
        else:
            buf, offset, stride = CP.place(rows, layout)
            f.write(np.array([MAGIC, H, W, mask, 2, M, stride, C, skip, int(bits), 0, offset, mode, int(colors)], np.int32).tobytes())
            f.write(buf.tobytes())


def parse_dump(text, M, C, bits, colors):
    """The standalone program's output -> (count, comp, bits, colors) with SENTINEL where nothing was printed."""
    out = _outputs(M, C, bits, colors)
    lines = text.strip().splitlines()
    i = 0
    for m in range(M):
        n, left = (int(v) for v in lines[i].split())
        i += 1
        out[0][m] = (n, left)
        for k in range(n):
            parts = lines[i].split()
            i += 1
            out[1][m, k] = [int(v) for v in parts[:8]]
            if colors:
                out[3][m, k] = int(parts[8])
            if bits:
                out[2][m, k] = np.frombuffer(bytes.fromhex(parts[-1]), np.uint8)
    return out
