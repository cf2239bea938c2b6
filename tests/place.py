"""Backend-independent checks of arcle_place_rows (where each object of a state row best fits the answer).  The pattern of
tests/objects.py, whose make_rows / place-in-a-buffer helpers this file takes from tests/components.py: every check takes a backend —
EmuPlace (tests/emu/place_emu.cpp: the kernel body of arcle_place.h lock-step on the CPU) or HipPlace (the product) — and returns a
list of mismatch strings.  The reference point is arcle_amd.search.place_numpy, which builds every child grid from the definition and
which tests/test_place_host.py pins on the oracle's own Moves."""
import ctypes
import os
import subprocess

import numpy as np

import backends as B
import components as CP
from arcle_amd import search as S
from oracle import oracle as O

EMU_DIR = CP.EMU_DIR
EMU_SRC = os.path.join(EMU_DIR, "place_emu.cpp")
EMU_HDRS = CP.EMU_HDRS + [os.path.join(B.ROOT, "arcle_amd", "csrc", "arcle_place.h")]
SENTINEL = CP.SENTINEL
MOVE_OPS = (20, 21, 22, 23)  # O2ARCv2Env's table: Move up, down, right, left
LARGE = 1 << 30
DISTS = (0, 1, 3, LARGE)
CS = (1, 5, 16)
# one cell; one row / one column; 3 x 3; 5 x 32: shifts across the whole 32-bit word; 20 x 7: the row board under the generic width
# class; 30 x 30: the fast width; 33 x 31: more than 32 rows; 64 x 16: every lane a row; 3 x 40 and 16 x 33: the flat board
SIZES = ((1, 1), (1, 9), (9, 1), (3, 3), (5, 32), (20, 7), (30, 30), (33, 31), (64, 16), (3, 40), (16, 33))
ORACLE_SIZES = ((5, 5), (7, 6), (30, 30))
TWO_COLOUR = (((0, 0), (0, 1), (1, 0)), ((1, 1), (2, 1), (2, 0)))


# ---- the cases: a grid, an answer, their dims and up to 16 object masks -------------------------------------------------------------
_cases = {}


def _paste_moved(rng, grid, masks, gh, gw):
    """An answer: every object's positive cells pasted at a random translation that keeps its box inside (gh, gw), on background 0."""
    ans = np.zeros_like(grid)
    for m in masks:
        xs, ys = np.nonzero(m)
        if not len(xs):
            continue
        dx, dy = int(rng.integers(-xs.min(), gh - xs.max())), int(rng.integers(-ys.min(), gw - ys.max()))
        keep = grid[xs, ys] > 0
        ans[xs[keep] + dx, ys[keep] + dy] = grid[xs, ys][keep]
    return ans


def cases_of(H, W):
    """moved: sparse 3-colour noise whose multi-colour 8-connected objects sit somewhere else in the answer; shrunk a / b: grid_dim
    below (H, W) with arbitrary bytes outside it and in the masks' cells outside it, answer_dim larger on one axis and smaller on the
    other, one-colour components; bytes: arbitrary bytes (negative ones, zeros) under the whole-grid object (T = {(0, 0)}), random
    rectangles and an empty mask; twocolour: one two-colour shape, moved; tie *: a one-cell object and an answer with two equally
    good placements — one per level of the tie rule (distance, dx, dy)."""
    if (H, W) in _cases:
        return _cases[(H, W)]
    rng = np.random.default_rng(9000 + 131 * H + W)
    out = []

    def add(name, grid, dim, answer, adim, masks):
        masks = np.asarray(masks, np.uint8).reshape(-1, H, W)[:16]
        out.append({"name": f"{H}x{W} {name}", "H": H, "W": W, "grid": grid.astype(np.int8), "dim": np.asarray(dim, np.int8),
                    "answer": answer.astype(np.int8), "adim": np.asarray(adim, np.int8), "masks": masks})
    g = rng.choice([0, 0, 0, 0, 0, 3, 5, 6], (H, W))
    n, _, _, masks = S.components_numpy(g, (H, W), 16, 0, True, True)
    masks = masks[:n + 1]  # (and one empty mask)
    add("moved", g, (H, W), _paste_moved(rng, g, masks, H, W), (H, W), masks)
    for tag, (da, db) in (("a", (1, -1)), ("b", (-1, 1))):
        gh, gw = max(1, H - 2), max(1, W - 3)
        g = rng.integers(-128, 128, (H, W)).astype(np.int8)
        g[:gh, :gw] = rng.choice([0, 0, 0, 3, 5], (gh, gw))
        n, _, _, masks = S.components_numpy(g, (gh, gw), 16, 0)
        masks = masks[:n + 1]
        ah, aw = min(H, max(1, gh + da)), min(W, max(1, gw + db))
        ans = np.zeros((H, W), np.int8)
        ans[:ah, :aw] = np.where(rng.random((ah, aw)) < 0.5, _paste_moved(rng, g, masks, gh, gw)[:ah, :aw], rng.choice([0, 3, 5], (ah, aw)))
        masks = masks.copy()
        outside = np.ones((H, W), bool)
        outside[:gh, :gw] = False
        masks[:, outside] = rng.integers(0, 2, (len(masks), int(outside.sum())))  # (cells outside grid_dim are ignored)
        add(f"shrunk {tag} grid {gh}x{gw} answer {ah}x{aw}", g, (gh, gw), ans, (ah, aw), masks)
    g = rng.choice([-128, -1, 0, 0, 3, 5, 37, 127], (H, W))
    masks = [np.ones((H, W), np.uint8), np.zeros((H, W), np.uint8)]
    for _ in range(6):
        x0, y0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        m = np.zeros((H, W), np.uint8)
        m[x0:x0 + int(rng.integers(1, 4)), y0:y0 + int(rng.integers(1, 5))] = 1
        masks.append(m)
    masks.append((rng.random((H, W)) < 0.1).astype(np.uint8))
    add("bytes", g, (H, W), np.roll(g, (1 if H > 1 else 0, -1 if W > 1 else 0), (0, 1)), (H, W), masks)
    if H >= 4 and W >= 4:
        g = np.zeros((H, W), np.int8)
        for part, col in zip(TWO_COLOUR, (4, 7)):
            for a, b in part:
                g[a, 1 + b] = col
        m = g != 0
        add("twocolour", g, (H, W), _paste_moved(rng, g, [m], H, W), (H, W), [m, g == 4, g == 7])
    cx, cy = H // 2, W // 2
    for name, spots in (("tie dx", ((-1, 0), (1, 0))), ("tie dy", ((0, -1), (0, 1))), ("tie distance", ((1, 0), (-2, 0))), ("tie distance y", ((0, -2), (0, 1))),
                        ("tie dx before dy", ((-1, 0), (0, -1))), ("tie dx before dy 2", ((1, 0), (0, 1))), ("tie diagonal", ((1, -1), (-1, 1)))):
        if all(0 <= cx + a < H and 0 <= cy + b < W for a, b in spots):
            g, ans = np.zeros((H, W), np.int8), np.zeros((H, W), np.int8)
            g[cx, cy] = 5
            for a, b in spots:
                ans[cx + a, cy + b] = 5
            add(name, g, (H, W), ans, (H, W), [g != 0])
    _cases[(H, W)] = out
    return out


_mirror = {}


def mirror(case, dist):
    """place_numpy of a case, computed once per (case, max_dist) over all its objects: (place [n, 4], base (2,))"""
    key = (case["name"], dist)
    if key not in _mirror:
        _mirror[key] = S.place_numpy(case["grid"], case["dim"], case["answer"], case["adim"], case["masks"], None if dist >= LARGE else dist)
    return _mirror[key]


def bit_rows(cases, C, with_count, rng):
    """-> (count int32 [M, 2], bits uint8 [M, C, 128]): every case's first C masks packed, every bit at a cell index >= H * W random
    (ignored); slots beyond the case's masks: SENTINEL bytes where `count` keeps them from being read, empty masks where it is NULL."""
    M, P = len(cases), cases[0]["H"] * cases[0]["W"]
    bits = np.full((M, C, B.BITS_STRIDE), SENTINEL if with_count else 0, np.uint8)
    count = np.zeros((M, 2), np.int32)
    for m, c in enumerate(cases):
        n = min(C, len(c["masks"]))
        count[m] = (n, 12345)
        cells = np.zeros((n, 8 * B.BITS_STRIDE), np.uint8)
        cells[:, :P] = c["masks"][:n].reshape(n, P) != 0
        cells[:, P:] = rng.integers(0, 2, (n, 8 * B.BITS_STRIDE - P))
        bits[m, :n] = np.packbits(cells, axis=1, bitorder="little")
    return count, bits


def envs_for(cases, resident, with_src, rng):
    """The envs behind M rows -> (N, answers [N, H, W], adims [N, 2], src int32 [M] | None, bad = the rows whose src names no env).
    Without src: env m = case m.  With it, rows form: env m + 1 holds row m's answer, env 0 noise, and (M > 1) the last row names
    env N; resident form (env m holds row m's grid): env (m + 1) % M holds row m's answer."""
    M, H, W = len(cases), cases[0]["H"], cases[0]["W"]
    ans, adim = np.stack([c["answer"] for c in cases]), np.stack([c["adim"] for c in cases])
    if not with_src:
        return M, ans, adim, None, []
    if resident:
        src = ((np.arange(M) + 1) % M).astype(np.int32)
        A, D = np.zeros_like(ans), np.zeros_like(adim)
        A[src], D[src] = ans, adim
        return M, A, D, src, []
    A = np.concatenate([rng.integers(0, 10, (1, H, W)).astype(np.int8), ans])
    D = np.concatenate([np.array([[H, W]], np.int8), adim])
    src = (np.arange(M) + 1).astype(np.int32)
    bad = []
    if M > 1:
        src[-1] = M + 1
        bad = [M - 1]
    return M + 1, A, D, src, bad


# ---- the backends -----------------------------------------------------------------------------------------------------------------
class _PlaceParams(ctypes.Structure):  # mirror of arcle::PlaceParams (arcle_amd/csrc/arcle_place.h)
    _fields_ = [("p", B._StepParams), ("max_comp", ctypes.c_int32), ("max_dist", ctypes.c_int32), ("count", ctypes.c_void_p),
                ("bits", ctypes.c_void_p), ("src_env", ctypes.c_void_p), ("place", ctypes.c_void_p), ("base", ctypes.c_void_p)]


_emu = None


def emu_lib():
    global _emu
    if _emu is None:
        so = os.path.join(EMU_DIR, "libplace_emu.so")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [EMU_SRC] + EMU_HDRS):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, EMU_SRC])
        _emu = ctypes.CDLL(so)
        _emu.place_emu_run.argtypes = [ctypes.POINTER(_PlaceParams), ctypes.c_int]
        assert _emu.place_emu_params_size() == ctypes.sizeof(_PlaceParams), "PlaceParams layout drifted"
    return _emu


def _guarded(shape, dtype=np.int32, guard=16):
    """A SENTINEL-filled flat buffer with `guard` elements on both sides of the array -> (buffer, the array's view)"""
    n = int(np.prod(shape))
    buf = np.full(n + 2 * guard, SENTINEL, dtype)
    return buf, buf[guard:guard + n].reshape(shape)


class EmuPlace:
    """The emulated kernel.  fw: -1 = the instantiation the library launches for the width, 0 = FW_GENERIC at any width."""
    BACKEND = B.EmuBackend  # (tests/strides.py: a subclass of another plane stride)
    name = "emu"

    def __init__(self, fw=-1):
        self.fw = fw

    def run(self, kind, H, W, cases, layout, C, dist, with_count, with_src, with_base, rng):
        M = len(cases)
        resident = layout == "resident"
        N, ans, adim, src, bad = envs_for(cases, resident, with_src, rng)
        be = self.BACKEND(N, H, W, 3, kind, CP.OPS[kind]())
        for k in be.buf:
            be.buf[k][:] = 0x55
        be.rec[:] = 0x55
        be.buf["answer"][:, :H * W] = ans.reshape(N, -1)
        be.rec[:, 14:16] = adim
        x = _PlaceParams()
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
        count, bits = bit_rows(cases, C, with_count, rng)
        self.guards = [_guarded((M, C, 4)), _guarded((M, 2))]
        (_, place), (_, base) = self.guards
        x.max_comp, x.max_dist = C, dist
        x.count, x.bits, x.src_env = count.ctypes.data if with_count else None, bits.ctypes.data, None if src is None else src.ctypes.data
        x.place, x.base = place.ctypes.data, base.ctypes.data if with_base else None
        rc = emu_lib().place_emu_run(ctypes.byref(x), self.fw)
        assert rc == 0, f"place emulator reported error {rc} (divergent cross-lane op / non-uniform value)"
        return place, base, bad

    def guards_intact(self):
        return all((buf[:16] == SENTINEL).all() and (buf[-16:] == SENTINEL).all() for buf, _ in self.guards)


class HipPlace:
    """EnvBatch.place_rows on the device."""
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

    def run(self, kind, H, W, cases, layout, C, dist, with_count, with_src, with_base, rng):
        t = self.t
        M = len(cases)
        resident = layout == "resident"
        N, ans, adim, src, bad = envs_for(cases, resident, with_src, rng)
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
        count, bits = bit_rows(cases, C, with_count, rng)
        guard = t.full((M * C * 4 + M * 2 + 48,), SENTINEL, dtype=t.int32, device=b.device)
        place, base = guard[16:16 + M * C * 4].view(M, C, 4), guard[32 + M * C * 4:32 + M * C * 4 + 2 * M].view(M, 2)
        b.place_rows(view, t.as_tensor(count, device=b.device) if with_count else None, t.as_tensor(bits, device=b.device),
                     None if src is None else t.as_tensor(src, device=b.device), None if dist >= LARGE else dist, out=(place, base if with_base else None))
        g = guard.cpu().numpy()
        self._ok = bool((g[:16] == SENTINEL).all() and (g[16 + M * C * 4:32 + M * C * 4] == SENTINEL).all() and (g[32 + M * C * 4 + 2 * M:] == SENTINEL).all())
        return place.cpu().numpy(), base.cpu().numpy(), bad

    def guards_intact(self):
        return self._ok


def compare(tag, got, cases, C, dist, with_count, with_base):
    """Everything exact: the four words of every object, the base pair, SENTINEL in the entries >= count and in an absent base."""
    place, base, bad = got
    errs = []
    for m, c in enumerate(cases):
        wp, wb = mirror(c, dist)
        n = min(C, len(wp))
        t = f"{tag} row {m} ({c['name']})"
        if m in bad:
            wp, wb = np.zeros_like(wp), (0, 0)
        if not np.array_equal(place[m, :n], wp[:n]):
            k = int(np.argwhere((place[m, :n] != wp[:n]).any(1))[0, 0])
            errs.append(f"{t}: object {k} {place[m, k].tolist()} != {wp[k].tolist()}")
        if with_count:
            if (place[m, n:] != SENTINEL).any():
                errs.append(f"{t}: an entry >= count was written")
        else:  # (the slots beyond the case's masks hold empty masks: they stay where they are and score what the grid scores)
            stay = (0, 0, 0, 0) if m in bad else (0, 0, wb[0], wb[0])
            if (place[m, n:] != np.array(stay)).any():
                errs.append(f"{t}: an empty mask gave {place[m, n:][0].tolist()} != {list(stay)}")
        if with_base and tuple(int(v) for v in base[m]) != tuple(wb):
            errs.append(f"{t}: base {base[m].tolist()} != {tuple(wb)}")
        if not with_base and (base[m] != SENTINEL).any():
            errs.append(f"{t}: base was written though not asked for")
    return errs


def pad_to(cases, M):
    return [cases[i % len(cases)] for i in range(M)]


# size -> the runs of one backend: (kind, layout | "resident", M, C, max_dist, count given, src given, base asked for).  Per size: every
# env kind (the grid offset differs), the three layouts and the resident form, M = 1 and 37 (None: one row per case; a string: the one
# case of that name), every C of CS, every max_dist of DISTS, count and NULL, src and NULL.  On the flat board the emulator walks the
# translations one by one, so there its unlimited runs take one case — the nine masks of "bytes", the tie cases have a test of their
# own — and `full` (the device) adds every case at C = 16 without a limit.
def plan(H, W, full=False):
    if W > 32 or H > 64:
        runs = [("o2arc", "odd", None, 16, 3, True, True, True), ("arc", "dense", None, 5, 1, False, False, True),
                ("raw", "lib", 1, 1, 0, True, False, False), ("raw", "resident", None, 16, 1, True, True, True),
                ("o2arc", "lib", 37, 5, 1, True, True, True), ("arc", "resident", "bytes", 16, LARGE, False, False, True),
                ("o2arc", "dense", 37, 1, 1, False, True, False)]
        return runs + ([("o2arc", "lib", None, 16, LARGE, True, True, True)] if full else [])
    return [("o2arc", "odd", None, 16, LARGE, True, True, True), ("arc", "dense", None, 5, 3, False, False, True),
            ("raw", "lib", 1, 1, 0, True, False, False), ("raw", "resident", None, 16, 1, True, True, True),
            ("o2arc", "lib", 37, 5, LARGE, True, True, True), ("arc", "resident", None, 5, LARGE, False, False, True),
            ("o2arc", "dense", 37, 1, 1, False, True, False)]


def run_size(be, H, W, runs=None, full=False):
    runs = runs or plan(H, W, full)
    errs = []
    rng = np.random.default_rng(H * 1000 + W)
    for i, (kind, layout, M, C, dist, with_count, with_src, with_base) in enumerate(runs):
        cases = cases_of(H, W)
        if isinstance(M, str):
            cases = [c for c in cases if c["name"].endswith(M)]
        elif M is not None:
            cases = pad_to(cases, M) if M > 1 else cases[i % len(cases):][:1]
        tag = f"{be.name} {H}x{W} {kind} {layout} C={C} dist={dist} count={with_count} src={with_src}"
        got = be.run(kind, H, W, cases, layout, C, dist, with_count, with_src, with_base, rng)
        errs += compare(tag, got, cases, C, dist, with_count, with_base)
        if not be.guards_intact():
            errs.append(f"{tag}: bytes around an output buffer were written")
        if len(errs) > 10:
            break
    return errs


# ---- the oracle's side: select the object, Move |dx| + |dy| times, count the correct cells ------------------------------------------
def oracle_table(case, pick, kind="o2arc"):
    """correct(dx, dy) of every object of a case, from the ORACLE, for the translations `pick(k, candidates [n, 2])` keeps of each
    object's T (max_dist unlimited) -> list per object of {(dx, dy): correct}, and the grid the oracle's freshly reset env holds.
    Driven as tests/macros.py drives it: one macro per translation — |dx| vertical Moves, then |dy| horizontal ones, the object's mask
    at step 0 and the zero mask (continue the active object) afterwards — on the chained oracle, dense[..., 0] of the last step."""
    import macros as MC
    import search_bits as SB
    H, W = case["H"], case["W"]
    ops = CP.OPS[kind]()
    rows, orc = CP.clean_rows(kind, case["grid"][None], case["dim"][None], case["answer"][None], case["adim"][None])
    grid = SB._grids_of(rows, kind, H, W)[0][0]
    _, _, table = S.place_numpy(grid, case["dim"], case["answer"], case["adim"], case["masks"], None, full=True)
    up, down, right, left = MOVE_OPS
    gh, gw = (int(v) for v in case["dim"])
    out = []
    for k, mask in enumerate(case["masks"]):
        cand = np.argwhere(table[k] >= 0) - (H - 1, W - 1)
        cand = pick(k, cand[(cand != 0).any(1)])
        res = {}
        if len(cand):
            T = int(np.abs(cand).sum(1).max())
            K = len(cand)
            pay = np.zeros((1, K, T, H, W), np.int8)
            pay[0, :, 0, :gh, :gw] = mask[:gh, :gw] != 0  # (B: the oracle is given the object's cells inside grid_dim, as arcle_objects_rows reports them)
            op = np.zeros((1, K, T), np.int32)
            for j, (dx, dy) in enumerate(cand):
                op[0, j, :abs(dx)] = up if dx < 0 else down
                op[0, j, abs(dx):abs(dx) + abs(dy)] = right if dy > 0 else left
            length = np.abs(cand).sum(1).astype(np.int32).reshape(1, K)
            w = MC.oracle_macros(rows, case["answer"][None], case["adim"][None], kind, H, W, 3, ops, "mask", pay, op, length)
            assert not w["status"].any(), (case["name"], k)
            res = {(int(dx), int(dy)): int(c) for (dx, dy), c in zip(cand, w["dense"][0, :, 0])}
        out.append(res)
    return out, grid, table


# ---- planted tasks: one sparse object 5 to 8 cells (Manhattan) from its place ---------------------------------------------------------
def planted_far_tasks(n=8, H=12, W=12, seed=21):
    """n tasks on background 0 with ONE object — a diagonal line of three or four cells of one colour (8-connected; no one-cell shift
    of it overlaps the target) — and the answer, made by the ORACLE: the object selected by its exact cells and moved |dx| times
    vertically, then |dy| times horizontally, 5 <= |dx| + |dy| <= 8, both non-zero.
    -> (inputs [n, H, W], dims [n, 2], answers [n, H, W], the (dx, dy) per task)"""
    rng = np.random.default_rng(seed)
    ops = O.o2arc_ops()
    up, down, right, left = MOVE_OPS
    dims = np.tile(np.array([[H, W]], np.int8), (n, 1))
    inputs, answers, moves = [], [], []
    while len(inputs) < n:
        ln = int(rng.integers(3, 5))
        flip = int(rng.integers(0, 2))
        x, y = int(rng.integers(0, H - ln + 1)), int(rng.integers(0, W - ln + 1))
        dist = int(rng.integers(5, 9))
        a = int(rng.integers(1, dist))
        dx, dy = a * int(rng.choice([-1, 1])), (dist - a) * int(rng.choice([-1, 1]))
        if not (0 <= x + dx and x + dx + ln <= H and 0 <= y + dy and y + dy + ln <= W):
            continue
        g = np.zeros((H, W), np.int8)
        g[x + np.arange(ln), y + (ln - 1 - np.arange(ln) if flip else np.arange(ln))] = int(rng.integers(1, 10))
        mask = g != 0
        orc = B.OracleBackend(1, H, W, 3, "o2arc", ops)
        orc.set_tasks(g[None], dims[:1], g[None], dims[:1])
        orc.reset()
        for t in range(dist):
            op = (up if dx < 0 else down) if t < abs(dx) else (right if dy > 0 else left)
            orc.step("mask", (mask if t == 0 else np.zeros_like(mask))[None].astype(np.int8), np.array([op], np.int32))
        ans = orc.get("grid")[0]
        assert not orc.status() and (ans != 0).sum() == mask.sum() and not (ans != 0)[mask].any()
        inputs.append(g)
        answers.append(ans)
        moves.append((dx, dy))
    return np.stack(inputs), dims, np.stack(answers), moves


def placement_searches(venv, rows, n, depths):
    """The two searches of the demonstration on every task -> (results of the single-step beam with the objects' exact cells at width 1
    and depth = the task's distance, results of propose_placements at width 1 and depth 1)."""
    import torch
    single = [S.beam_search(venv, rows[i:i + 1], None, width=1, depth=depths[i], src_env=torch.tensor([i]),
                            propose=S.propose_objects(list(MOVE_OPS), [], masks=True, any_color=True, diagonal=True)) for i in range(n)]
    placed = [S.beam_search(venv, rows[i:i + 1], None, width=1, depth=1, src_env=torch.tensor([i]),
                            propose=S.propose_placements(MOVE_OPS, any_color=True, diagonal=True)) for i in range(n)]
    return single, placed


def place_numpy_rows(grids, gdims, answers, adims, objs, max_dist):
    """`ARCVecEnv.place` of M grids from place_numpy, on torch CPU tensors (the stub vec envs' `place`)."""
    import torch
    from arcle_amd.envs.vec import Placements
    M, C = int(objs.bits.shape[0]), int(objs.bits.shape[1])
    H, W = grids.shape[1:]
    place, base = np.zeros((M, C, 4), np.int32), np.zeros((M, 2), np.int32)
    cells = np.unpackbits(objs.bits.numpy(), axis=-1, bitorder="little")[..., :H * W].reshape(M, C, H, W)
    for m in range(M):
        n = int(objs.count[m])
        p, base[m] = S.place_numpy(grids[m], gdims[m], answers[m], adims[m], cells[m, :n], max_dist)
        place[m, :n] = p
    t = torch.from_numpy(place)
    return Placements(t[:, :, 0], t[:, :, 1], t[:, :, 2], t[:, :, 3], torch.from_numpy(base))


def move_macro_set(case, grid, max_len=None):
    """Every translation of T (max_dist unlimited) of every object of a case as a Move macro on bit rows, one flat set: -> (owner int
    [K] = the object, cand int [K, 2] = (dx, dy), bits uint8 [K, T, 128], op int32 [K, T], length int32 [K]); (0, 0) is left out (a
    macro has at least one step).  |dx| vertical Moves, then |dy| horizontal ones; the object's cells inside grid_dim at step 0, the
    zero mask afterwards."""
    H, W = case["H"], case["W"]
    gh, gw = (int(v) for v in case["dim"])
    _, _, table = S.place_numpy(grid, case["dim"], case["answer"], case["adim"], case["masks"], None, full=True)
    up, down, right, left = MOVE_OPS
    owner, cand = [], []
    for k in range(len(case["masks"])):
        c = np.argwhere(table[k] >= 0) - (H - 1, W - 1)
        c = c[(c != 0).any(1)]
        owner += [k] * len(c)
        cand += c.tolist()
    owner, cand = np.array(owner, np.int64), np.array(cand, np.int64).reshape(-1, 2)
    K, T = len(cand), int(np.abs(cand).sum(1).max())
    inside = np.zeros_like(case["masks"])
    inside[:, :gh, :gw] = case["masks"][:, :gh, :gw] != 0
    bits = np.zeros((K, T, B.BITS_STRIDE), np.uint8)
    bits[:, 0] = B.pack_bits(inside)[owner]
    op = np.full((K, T), -1, np.int32)
    for j, (dx, dy) in enumerate(cand):
        op[j, :abs(dx)] = up if dx < 0 else down
        op[j, abs(dx):abs(dx) + abs(dy)] = right if dy > 0 else left
    return owner, cand, bits, op, np.abs(cand).sum(1).astype(np.int32), table


def place_venv(answers, adims, H=12, W=12):
    """The oracle-backed stub vec env of tests/macros.py + `objects` (components_numpy) + `place` (place_numpy): what
    beam_search(propose=propose_placements(...)) needs, on torch CPU tensors."""
    import macros as MC
    import objects as OB
    import search_bits as SB

    class PlaceVenv(MC.MacroVenv):
        def objects(self, rows, max_components=32, skip_color=-1, any_color=False, diagonal=False, bits=False, colors=False):
            grids, gdims = SB._grids_of(rows.numpy(), self.kind, self.H, self.W)
            return OB.objects_numpy(grids, gdims, max_components, skip_color, any_color, diagonal, bits, colors)

        def place(self, rows, objs, src_env=None, max_dist=None):
            grids, gdims = SB._grids_of(rows.numpy(), self.kind, self.H, self.W)
            src = np.arange(len(grids)) if src_env is None else src_env.numpy()
            return place_numpy_rows(grids, gdims, self.answers[src], self.adims[src], objs, max_dist)
    return PlaceVenv("o2arc", H, W, 3, O.o2arc_ops(), answers, adims)


# the planted tasks a single-step beam (width 1, Move ops on the objects' exact cells, depth = the task's distance) solves: found with
# the oracle-backed stub (tests/test_place_host.py) when the tasks were chosen; the device test asserts the same number
SINGLE_STEP_SOLVES = 2


# ---- one dumped case for the standalone sanitized emulator ------------------------------------------------------------------------
MAGIC = 0x504c4143


def dump_case(path, kind, H, W, cases, layout, C, dist, with_count, with_src, with_base, rng):
    """Writes one case in the format place_emu.cpp's main() reads: buffers exactly as long as the data.  -> the rows without an env"""
    P, PS = H * W, (H * W + 127) & ~127
    pmask = sum(1 << i for i, k in enumerate(B.PLANES[:-1]) if k in O.KIND_PLANES[kind])
    M = len(cases)
    resident = layout == "resident"
    N, ans, adim, src, bad = envs_for(cases, resident, with_src, rng)
    answer = np.full((N, PS), 0x55, np.int8)
    answer[:, :P] = ans.reshape(N, P)
    rec = np.full((N, 16), 0x55, np.int8)
    rec[:, 14:16] = adim
    count, bits = bit_rows(cases, C, with_count, rng)
    with open(path, "wb") as f:
        if resident:
            rec[:M, 2:4] = np.stack([c["dim"] for c in cases])
            grid = np.full((N, PS), 0x55, np.int8)
            grid[:M, :P] = np.stack([c["grid"].reshape(-1) for c in cases])
            f.write(np.array([MAGIC, H, W, pmask, N, M, 0, C, dist, int(with_count), 1, 0, int(with_src), int(with_base)], np.int32).tobytes())
            f.write(answer.tobytes() + rec.tobytes() + grid.tobytes())
        else:
            buf, offset, stride = CP.place(CP.make_rows(kind, cases, rng), layout)
            f.write(np.array([MAGIC, H, W, pmask, N, M, stride, C, dist, int(with_count), 0, offset, int(with_src), int(with_base)], np.int32).tobytes())
            f.write(answer.tobytes() + rec.tobytes() + buf.tobytes())
        if with_count:
            f.write(count.tobytes())
        f.write(bits.tobytes())
        if with_src:
            f.write(src.tobytes())
    return bad


def parse_dump(text, cases, C, with_count, with_base):
    """The standalone program's output -> (place, base) with SENTINEL where nothing was printed."""
    M = len(cases)
    place, base = np.full((M, C, 4), SENTINEL, np.int32), np.full((M, 2), SENTINEL, np.int32)
    lines = text.strip().splitlines()
    i = 0
    for m, c in enumerate(cases):
        if with_base:
            base[m] = [int(v) for v in lines[i].split()]
            i += 1
        for k in range(min(C, len(c["masks"])) if with_count else C):
            place[m, k] = [int(v) for v in lines[i].split()]
            i += 1
    assert i == len(lines)
    return place, base
