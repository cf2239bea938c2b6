"""Backend-independent checks of arcle_turn_rows (where each object of a state row best fits the answer after a rotation or a flip).
The counterpart of tests/place.py, whose cases, bit rows, env arrangement, guards and SENTINEL this file takes: every check takes a
backend — EmuTurn (tests/emu/turn_emu.cpp: the kernel body of arcle_turn.h lock-step on the CPU) or HipTurn (the product) — and returns
a list of mismatch strings.  The reference point is arcle_amd.search.turn_numpy, which builds every child grid from the definition and
which tests/test_turn_host.py pins on the oracle's own select + turn + Moves."""
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
EMU_SRC = os.path.join(EMU_DIR, "turn_emu.cpp")
EMU_HDRS = PL.EMU_HDRS + [os.path.join(B.ROOT, "arcle_amd", "csrc", f) for f in ("arcle_stamp.h", "arcle_turn.h")]
SENTINEL = PL.SENTINEL
MOVE_OPS = PL.MOVE_OPS
TURN_OPS = (24, -1, 25, 26, 27)  # O2ARCv2Env's table: Rotate 90, (no Rotate 180), Rotate 270, Flip H, Flip V
ROT180_OP = 35                   # ... and where the tests' extended table has gen_rotate(2): appended behind Submit
TURN_OPS_ALL = (24, ROT180_OP, 25, 26, 27)
TURN_NAMES = ("rot90", "rot180", "rot270", "flip H", "flip V")
ALL = 31
LARGE = PL.LARGE
DISTS = PL.DISTS
CS = PL.CS
SIZES = PL.SIZES
ORACLE_SIZES = ((5, 5), (7, 6), (6, 9))
TIE_WANT = {"tie dx": (-1, 0), "tie dy": (0, -1), "tie distance": (1, 0), "tie distance y": (0, 1), "tie dx before dy": (-1, 0),
            "tie dx before dy 2": (0, 1), "tie diagonal": (-1, 1)}


def ops_all():
    """O2ARCv2Env's table with gen_rotate(2) appended (the default table has no Rotate 180)"""
    return list(O.o2arc_ops()) + [O.desc(O.OP_ROTATE, 2)]


# ---- the cases: those of tests/place.py and what a turn adds -------------------------------------------------------------------------
_cases = {}


def corner_after(t, x0, y0, h, w):
    """(nx, ny) by the rule of include/arcle_hip.h — used to build ANSWERS and to describe cases only (the mirror under test is turn_numpy, and the
    oracle settles the rule in tests/test_turn_host.py)"""
    return ((2 * x0 + h - w) // 2, (2 * y0 + w - h) // 2) if t in (0, 2) else (x0, y0)


def _turned_answer(grid, mask, t, px, py):
    """The background with the turned tile's positive cells at corner (px, py)"""
    xs, ys = np.nonzero(mask)
    tile = np.where(mask, grid, 0)[xs.min():xs.max() + 1, ys.min():ys.max() + 1]
    tile = (np.rot90(tile, 1), np.rot90(tile, 2), np.rot90(tile, 3), tile[:, ::-1], tile[::-1])[t]
    out = np.where(mask, 0, grid)
    dst = out[px:px + tile.shape[0], py:py + tile.shape[1]]
    dst[...] = np.where(tile > 0, tile, dst)
    return out


def cases_of(H, W):
    """The cases of PL.cases_of(H, W) — moved, shrunk a / b (grid_dim below (H, W) with junk outside it, answer_dim larger on one axis
    and smaller on the other), bytes (the whole-grid object, rectangles, an empty mask), twocolour and one tie case per level of the
    tie rule (a one-cell object: every turn leaves it where it is) — and the cases only a turn needs:
      parity h x w      a filled multi-colour h x w box, (h, w) in the four parity classes, the answer holding one of its turns elsewhere
      over top / bottom / left / right   a three-cell line along an edge that a quarter turn leaves hanging over that edge: (0, 0) is
                        not a candidate; the answer holds the turned line inside the grid
      holes             a 2 x 3 box of bytes 4, -3, 0 / 0, 6, 7: a negative byte and zeros inside the box
      long              (H != W) a line as long as the longer axis: it fits under Rotate 180 and the flips only"""
    if (H, W) in _cases:
        return _cases[(H, W)]
    out = list(PL.cases_of(H, W))
    rng = np.random.default_rng(7000 + 131 * H + W)

    def add(name, grid, answer, masks):
        masks = np.asarray(masks, np.uint8).reshape(-1, H, W)[:16]
        out.append({"name": f"{H}x{W} {name}", "H": H, "W": W, "grid": grid.astype(np.int8), "dim": np.array((H, W), np.int8),
                    "answer": answer.astype(np.int8), "adim": np.array((H, W), np.int8), "masks": masks})

    def somewhere(g, m, t):
        xs, ys = np.nonzero(m)
        h, w = xs.max() - xs.min() + 1, ys.max() - ys.min() + 1
        th, tw = (w, h) if t in (0, 2) else (h, w)
        return _turned_answer(g, m, t, int(rng.integers(0, H - th + 1)), int(rng.integers(0, W - tw + 1)))
    if H >= 4 and W >= 4:
        for i, (h, w) in enumerate(((2, 2), (2, 3), (3, 2), (3, 3))):
            g = np.zeros((H, W), np.int8)
            x, y = int(rng.integers(0, H - 3)), int(rng.integers(0, W - 3))
            g[x:x + h, y:y + w] = rng.permutation([3, 5, 6, 7, 8, 9, 4, 2, 1])[:h * w].reshape(h, w)
            add(f"parity {h}x{w}", g, somewhere(g, g != 0, (0, 2, 1, 3)[i]), [g != 0])
        g = np.zeros((H, W), np.int8)
        g[1:3, 1:4] = ((4, -3, 0), (0, 6, 7))
        m = np.zeros((H, W), bool)
        m[1:3, 1:4] = True
        add("holes", g, somewhere(g, m, 2), [m])
    if H >= 3 and W >= 3:
        for name, (xs, ys) in (("over top", ((0, 0, 0), (0, 1, 2))), ("over bottom", ((H - 1,) * 3, (0, 1, 2))),
                               ("over left", ((0, 1, 2), (0, 0, 0))), ("over right", ((0, 1, 2), (W - 1,) * 3))):
            g = np.zeros((H, W), np.int8)
            g[list(xs), list(ys)] = (4, 6, 7)
            add(name, g, somewhere(g, g != 0, 0), [g != 0])
    if H != W and max(H, W) >= 3:
        g = np.zeros((H, W), np.int8)
        line = rng.choice([3, 5], max(H, W))
        line[0] = 7
        if H > W:
            g[:, 0] = line
        else:
            g[0, :] = line
        add("long", g, _turned_answer(g, g != 0, 1, 0, 0), [g != 0])
    _cases[(H, W)] = out
    return out


def facts(case):
    """What the plan test asserts the cases reach, per object with a cell inside grid_dim: (h, w, {turn: (0, 0) is a candidate},
    {turn: it has candidates at all}, the edges a quarter turn overhangs)"""
    gh, gw = (int(v) for v in case["dim"])
    out = []
    for m in case["masks"]:
        xs, ys = np.nonzero(m[:gh, :gw])
        if not len(xs):
            continue
        x0, y0, h, w = int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)
        stays, fits, over = {}, {}, set()
        for t in range(5):
            th, tw = (w, h) if t in (0, 2) else (h, w)
            nx, ny = corner_after(t, x0, y0, h, w)
            stays[t] = 0 <= nx and nx + th <= gh and 0 <= ny and ny + tw <= gw
            fits[t] = th <= gh and tw <= gw
            if fits[t]:
                over |= {e for e, c in (("top", nx < 0), ("bottom", nx + th > gh), ("left", ny < 0), ("right", ny + tw > gw)) if c}
        out.append((h, w, stays, fits, over))
    return out


_mirror = {}


def mirror(case, dist):
    """turn_numpy of a case with all five turns, computed once per (case, max_dist) over all its objects: (turn [n, 5, 4], base (2,))"""
    key = (case["name"], dist)
    if key not in _mirror:
        _mirror[key] = S.turn_numpy(case["grid"], case["dim"], case["answer"], case["adim"], case["masks"], None if dist >= LARGE else dist)
    return _mirror[key]


# ---- the backends -----------------------------------------------------------------------------------------------------------------
class _TurnParams(ctypes.Structure):  # mirror of arcle::TurnParams (arcle_amd/csrc/arcle_turn.h)
    _fields_ = [("p", B._StepParams), ("max_comp", ctypes.c_int32), ("max_dist", ctypes.c_int32), ("count", ctypes.c_void_p),
                ("bits", ctypes.c_void_p), ("src_env", ctypes.c_void_p), ("turn", ctypes.c_void_p), ("base", ctypes.c_void_p),
                ("turns", ctypes.c_uint32), ("pad_", ctypes.c_int32)]


_emu = None


def emu_lib():
    global _emu
    if _emu is None:
        so = os.path.join(EMU_DIR, "libturn_emu.so")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [EMU_SRC] + EMU_HDRS):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, EMU_SRC])
        _emu = ctypes.CDLL(so)
        _emu.turn_emu_run.argtypes = [ctypes.POINTER(_TurnParams), ctypes.c_int]
        assert _emu.turn_emu_params_size() == ctypes.sizeof(_TurnParams), "TurnParams layout drifted"
    return _emu


class EmuTurn:
    """The emulated kernel.  fw: -1 = the instantiation the library launches for the width, 0 = FW_GENERIC at any width."""
    BACKEND = B.EmuBackend  # (a subclass may name a backend of another plane stride)
    name = "emu"

    def __init__(self, fw=-1):
        self.fw = fw

    def run(self, kind, H, W, cases, layout, C, dist, with_count, with_src, with_base, turns, rng):
        M = len(cases)
        resident = layout == "resident"
        N, ans, adim, src, bad = PL.envs_for(cases, resident, with_src, rng)
        be = self.BACKEND(N, H, W, 3, kind, CP.OPS[kind]())
        for k in be.buf:
            be.buf[k][:] = 0x55
        be.rec[:] = 0x55
        be.buf["answer"][:, :H * W] = ans.reshape(N, -1)
        be.rec[:, 14:16] = adim
        x = _TurnParams()
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
        self.guards = [PL._guarded((M, C, 5, 4)), PL._guarded((M, 2))]
        (_, turn), (_, base) = self.guards
        x.max_comp, x.max_dist, x.turns = C, min(dist, 2048), turns
        x.count, x.bits, x.src_env = count.ctypes.data if with_count else None, bits.ctypes.data, None if src is None else src.ctypes.data
        x.turn, x.base = turn.ctypes.data, base.ctypes.data if with_base else None
        rc = emu_lib().turn_emu_run(ctypes.byref(x), self.fw)
        assert rc == 0, f"turn emulator reported error {rc} (divergent cross-lane op / non-uniform value)"
        return turn, base, bad

    def guards_intact(self):
        return all((buf[:16] == SENTINEL).all() and (buf[-16:] == SENTINEL).all() for buf, _ in self.guards)


class HipTurn:
    """EnvBatch.turn_rows on the device."""
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

    def run(self, kind, H, W, cases, layout, C, dist, with_count, with_src, with_base, turns, rng):
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
        nt = M * C * 20
        guard = t.full((nt + M * 2 + 48,), SENTINEL, dtype=t.int32, device=b.device)
        turn, base = guard[16:16 + nt].view(M, C, 5, 4), guard[32 + nt:32 + nt + 2 * M].view(M, 2)
        b.turn_rows(view, t.as_tensor(count, device=b.device) if with_count else None, t.as_tensor(bits, device=b.device),
                    None if src is None else t.as_tensor(src, device=b.device), None if dist >= LARGE else dist, turns,
                    out=(turn, base if with_base else None))
        g = guard.cpu().numpy()
        self._ok = bool((g[:16] == SENTINEL).all() and (g[16 + nt:32 + nt] == SENTINEL).all() and (g[32 + nt + 2 * M:] == SENTINEL).all())
        return turn.cpu().numpy(), base.cpu().numpy(), bad

    def guards_intact(self):
        return self._ok


def compare(tag, got, cases, C, dist, with_count, with_base, turns):
    """Everything exact: the four words of every slot asked for of every object, the base pair, SENTINEL in the slots not asked for, in
    the entries >= count and in an absent base."""
    turn, base, bad = got
    errs = []
    asked = np.array([(turns >> t) & 1 for t in range(5)], bool)
    for m, c in enumerate(cases):
        wt, wb = mirror(c, dist)
        n = min(C, len(wt))
        t = f"{tag} row {m} ({c['name']})"
        if m in bad:
            wt, wb = np.zeros_like(wt), (0, 0)
        if not np.array_equal(turn[m, :n][:, asked], wt[:n][:, asked]):
            k, s = (int(v) for v in np.argwhere((turn[m, :n] != wt[:n]).any(2) & asked)[0])
            errs.append(f"{t}: object {k} {TURN_NAMES[s]} {turn[m, k, s].tolist()} != {wt[k, s].tolist()}")
        if (turn[m][:, ~asked] != SENTINEL).any():
            errs.append(f"{t}: a slot that was not asked for was written")
        if with_count:
            if (turn[m, n:] != SENTINEL).any():
                errs.append(f"{t}: an entry >= count was written")
        else:  # (the slots beyond the case's masks hold empty masks: nothing turns, the grid scores what it scores)
            empty = (0, 0, 0, 0) if m in bad else (0, 0, wb[0], 1)
            if (turn[m, n:][:, asked] != np.array(empty)).any():
                errs.append(f"{t}: an empty mask gave {turn[m, n:][:, asked].reshape(-1, 4)[0].tolist()} != {list(empty)}")
        if with_base and tuple(int(v) for v in base[m]) != tuple(wb):
            errs.append(f"{t}: base {base[m].tolist()} != {tuple(wb)}")
        if not with_base and (base[m] != SENTINEL).any():
            errs.append(f"{t}: base was written though not asked for")
    return errs


# size -> the runs of one backend: (kind, layout | "resident", M, C, max_dist, count given, src given, base asked for, turns).  Per
# size: every env kind, the three layouts and the resident form, M = 1 and 37 (None: one row per case; a string: the cases whose name
# ends with it), every C of CS, every max_dist of DISTS, count and NULL, src and NULL, all five turns and each turn alone.  On the flat
# board the emulator walks the candidates one by one, so there its unlimited runs take few cases; `full` (the device) adds every case
# at C = 16 without a limit.
def plan(H, W, full=False):
    if W > 32 or H > 64:
        runs = [("o2arc", "odd", None, 16, 3, True, True, True, ALL), ("arc", "dense", None, 5, 1, False, False, True, 1),
                ("raw", "lib", 1, 1, 0, True, False, False, 2), ("raw", "resident", None, 16, 1, True, True, True, 4),
                ("o2arc", "lib", 37, 5, 1, True, True, True, 8), ("arc", "resident", "holes", 16, LARGE, False, False, True, ALL),
                ("o2arc", "dense", 37, 1, 1, False, True, False, 16), ("o2arc", "odd", "over left", 1, LARGE, True, False, True, ALL)]
        return runs + ([("o2arc", "lib", None, 16, LARGE, True, True, True, ALL)] if full else [])
    return [("o2arc", "odd", None, 16, LARGE, True, True, True, ALL), ("arc", "dense", None, 5, 3, False, False, True, 1),
            ("raw", "lib", 1, 1, 0, True, False, False, 2), ("raw", "resident", None, 16, 1, True, True, True, 4),
            ("o2arc", "lib", 37, 5, LARGE, True, True, True, 8), ("arc", "resident", None, 5, LARGE, False, False, True, 16),
            ("o2arc", "dense", 37, 1, 1, False, True, False, ALL)]


def run_size(be, H, W, runs=None, full=False):
    runs = runs or plan(H, W, full)
    errs = []
    rng = np.random.default_rng(H * 1000 + W)
    for i, (kind, layout, M, C, dist, with_count, with_src, with_base, turns) in enumerate(runs):
        cases = cases_of(H, W)
        if isinstance(M, str):
            cases = [c for c in cases if c["name"].endswith(M)] or cases[:1]
        elif M is not None:
            cases = PL.pad_to(cases, M) if M > 1 else cases[i % len(cases):][:1]
        tag = f"{be.name} {H}x{W} {kind} {layout} C={C} dist={dist} count={with_count} src={with_src} turns={turns}"
        got = be.run(kind, H, W, cases, layout, C, dist, with_count, with_src, with_base, turns, rng)
        errs += compare(tag, got, cases, C, dist, with_count, with_base, turns)
        if not be.guards_intact():
            errs.append(f"{tag}: bytes around an output buffer were written")
        if len(errs) > 10:
            break
    return errs


# ---- the oracle's side: select the object with the turn's op, Move |dx| + |dy| times, count the correct cells ------------------------
def turn_macro_set(case, grid):
    """Every candidate (t, dx, dy) of every object of a case (max_dist unlimited, from turn_numpy's table: its -1 entries are outside
    T_t) as a macro on bit rows, one flat set: -> (owner int [K] = the object, cand int [K, 3] = (t, dx, dy), bits uint8 [K, T, 128],
    op int32 [K, T], length int32 [K], the table).  Step 0 = the object's cells inside grid_dim with the turn's op of TURN_OPS_ALL,
    then |dx| vertical Moves and |dy| horizontal ones on the zero mask."""
    H, W = case["H"], case["W"]
    gh, gw = (int(v) for v in case["dim"])
    _, _, table = S.turn_numpy(grid, case["dim"], case["answer"], case["adim"], case["masks"], None, ALL, full=True)
    up, down, right, left = MOVE_OPS
    owner, cand = [], []
    for k in range(len(case["masks"])):
        c = np.argwhere(table[k] >= 0) - (0, H - 1, W - 1)
        owner += [k] * len(c)
        cand += c.tolist()
    owner, cand = np.array(owner, np.int64), np.array(cand, np.int64).reshape(-1, 3)
    K, T = len(cand), 1 + int(np.abs(cand[:, 1:]).sum(1).max()) if len(cand) else 1
    inside = np.zeros_like(case["masks"])
    inside[:, :gh, :gw] = case["masks"][:, :gh, :gw] != 0
    bits = np.zeros((K, T, B.BITS_STRIDE), np.uint8)
    if K:
        bits[:, 0] = B.pack_bits(inside)[owner]
    op = np.full((K, T), -1, np.int32)
    for j, (t, dx, dy) in enumerate(cand):
        op[j, 0] = TURN_OPS_ALL[t]
        op[j, 1:1 + abs(dx)] = up if dx < 0 else down
        op[j, 1 + abs(dx):1 + abs(dx) + abs(dy)] = right if dy > 0 else left
    return owner, cand, bits, op, (1 + np.abs(cand[:, 1:]).sum(1)).astype(np.int32), table


def oracle_table(case, kind="o2arc"):
    """correct(t, dx, dy) of every candidate of every object of a case from the ORACLE (tests/macros.py's chained oracle, mask ingress, the
    table with gen_rotate(2) appended) -> (want int32 [K], the mirror's values at the same candidates int32 [K], cand [K, 3])."""
    import macros as MC
    import search_bits as SB
    H, W = case["H"], case["W"]
    rows, orc = CP.clean_rows(kind, case["grid"][None], case["dim"][None], case["answer"][None], case["adim"][None])
    grid = SB._grids_of(rows, kind, H, W)[0][0]
    owner, cand, bits, op, length, table = turn_macro_set(case, grid)
    K, T = op.shape
    if not K:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), cand
    pay = np.unpackbits(bits, axis=-1, bitorder="little")[..., :H * W].astype(np.int8)
    w = MC.oracle_macros(rows, case["answer"][None], case["adim"][None], kind, H, W, 3, ops_all(), "mask", pay.reshape(1, K, T, H * W), op[None], length[None])
    assert not w["status"].any(), case["name"]
    return w["dense"][0, :, 0], table[owner, cand[:, 0], cand[:, 1] + H - 1, cand[:, 2] + W - 1], cand


# ---- planted tasks: one two-colour L-tetromino, turned and moved ---------------------------------------------------------------------
L_CELLS = ((0, 0), (1, 0), (2, 0), (2, 1))  # no symmetry: no translation of it equals any turn of it


def planted_turn_tasks(n=8, H=12, W=12, seed=44):
    """n tasks on background 0 with ONE object — the L-tetromino, its foot of another colour — and the answer, made by the ORACLE on the
    table with gen_rotate(2) appended: the object selected by its exact cells with a turn's op (task i takes turn i % 5), then moved
    |dx| times vertically and |dy| times horizontally, 0 <= |dx| + |dy| <= 4 (task 0 stays where the turn leaves it).
    -> (inputs [n, H, W], dims [n, 2], answers [n, H, W], the (t, dx, dy) per task)"""
    rng = np.random.default_rng(seed)
    ops = ops_all()
    up, down, right, left = MOVE_OPS
    dims = np.tile(np.array([[H, W]], np.int8), (n, 1))
    inputs, answers, plans = [], [], []
    while len(inputs) < n:
        i = len(inputs)
        t = i % 5
        x, y = int(rng.integers(2, H - 5)), int(rng.integers(2, W - 5))
        dist = i % 5 if i else 0
        a = int(rng.integers(0, dist + 1))
        dx, dy = a * int(rng.choice([-1, 1])), (dist - a) * int(rng.choice([-1, 1]))
        nx, ny = corner_after(t, x, y, 3, 2)
        if not (0 <= nx + dx and nx + dx + 3 <= H and 0 <= ny + dy and ny + dy + 3 <= W):
            continue
        g = np.zeros((H, W), np.int8)
        c1, c2 = (int(v) for v in rng.choice(np.arange(1, 10), 2, replace=False))
        for a_, b_ in L_CELLS:
            g[x + a_, y + b_] = c1
        g[x + 2, y + 1] = c2
        mask = g != 0
        orc = B.OracleBackend(1, H, W, 3, "o2arc", ops)
        orc.set_tasks(g[None], dims[:1], g[None], dims[:1])
        orc.reset()
        seq = [TURN_OPS_ALL[t]] + [up if dx < 0 else down] * abs(dx) + [right if dy > 0 else left] * abs(dy)
        for s, op in enumerate(seq):
            orc.step("mask", (mask if s == 0 else np.zeros_like(mask))[None].astype(np.int8), np.array([op], np.int32))
        ans = orc.get("grid")[0]
        assert not orc.status() and (ans != 0).sum() == 4
        inputs.append(g)
        answers.append(ans)
        plans.append((t, dx, dy))
    return np.stack(inputs), dims, np.stack(answers), plans


def turn_searches(venv, rows, n):
    """The two searches of the demonstration on every task, both at width 1 and depth 1 -> (results of propose_placements, results of
    propose_turns with every turn's op)."""
    import torch
    before = [S.beam_search(venv, rows[i:i + 1], None, width=1, depth=1, src_env=torch.tensor([i]),
                            propose=S.propose_placements(MOVE_OPS, any_color=True, diagonal=True)) for i in range(n)]
    turned = [S.beam_search(venv, rows[i:i + 1], None, width=1, depth=1, src_env=torch.tensor([i]),
                            propose=S.propose_turns(TURN_OPS_ALL, MOVE_OPS, any_color=True, diagonal=True)) for i in range(n)]
    return before, turned


def turn_numpy_rows(grids, gdims, answers, adims, objs, max_dist, turns=ALL):
    """`ARCVecEnv.turn` of M grids from turn_numpy, on torch CPU tensors (the stub vec envs' `turn`)."""
    import torch
    from arcle_amd.envs.vec import Turns
    M, C = int(objs.bits.shape[0]), int(objs.bits.shape[1])
    H, W = grids.shape[1:]
    turn, base = np.zeros((M, C, 5, 4), np.int32), np.zeros((M, 2), np.int32)
    cells = np.unpackbits(objs.bits.numpy(), axis=-1, bitorder="little")[..., :H * W].reshape(M, C, H, W)
    for m in range(M):
        n = int(objs.count[m])
        s, base[m] = S.turn_numpy(grids[m], gdims[m], answers[m], adims[m], cells[m, :n], max_dist, turns)
        turn[m, :n] = s
    t = torch.from_numpy(turn)
    return Turns(t[..., 0], t[..., 1], t[..., 2], t[..., 3], torch.from_numpy(base))


def turn_venv(answers, adims, H=12, W=12):
    """The oracle-backed stub vec env of tests/place.py + `turn` (turn_numpy), on the table with gen_rotate(2) appended: what
    beam_search(propose=propose_turns(...)) needs, on torch CPU tensors."""
    import search_bits as SB
    base = type(PL.place_venv(answers, adims, H, W))

    class TurnVenv(base):
        def turn(self, rows, objs, src_env=None, max_dist=8, turns=ALL):
            grids, gdims = SB._grids_of(rows.numpy(), self.kind, self.H, self.W)
            src = np.arange(len(grids)) if src_env is None else src_env.numpy()
            return turn_numpy_rows(grids, gdims, self.answers[src], self.adims[src], objs, max_dist, turns)
    return TurnVenv("o2arc", H, W, 3, ops_all(), answers, adims)


def replay_on_oracle(inp, dim, ans, seq):
    """The (selection, op) sequence on the oracle (the table with gen_rotate(2) appended) from the task's initial state -> 1 if no
    step raised a status bit and the grid it leaves is the answer, else 0.  (A Submit's reward cannot say so on this table: the
    reference rewards the LAST op of the table, base.py's `operation == len(operations) - 1`, which here is the appended Rotate.)"""
    H, W = inp.shape
    orc = B.OracleBackend(1, H, W, 3, "o2arc", ops_all())
    orc.set_tasks(inp[None], dim[None], ans[None], dim[None])
    orc.reset()
    for sel, op in seq:
        assert sel.dtype == bool and sel.shape == (H, W)
        orc.step("mask", sel[None].astype(np.int8), np.array([op], np.int32))
    return int(not orc.status() and np.array_equal(orc.get("grid")[0], ans) and np.array_equal(orc.get("grid_dim")[0], dim))


# the planted tasks that propose_placements solves at the same width and depth: found with the oracle-backed stub
# (tests/test_turn_host.py) when the tasks were chosen; the device test asserts the same number
BEFORE_SOLVES = 0


# ---- one dumped case for the standalone sanitized emulator ------------------------------------------------------------------------
MAGIC = 0x5455524e


def dump_case(path, kind, H, W, cases, layout, C, dist, with_count, with_src, with_base, turns, rng):
    """Writes one case in the format turn_emu.cpp's main() reads: buffers exactly as long as the data.  -> the rows without an env"""
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
    dist = min(dist, 2048)
    with open(path, "wb") as f:
        if resident:
            rec[:M, 2:4] = np.stack([c["dim"] for c in cases])
            grid = np.full((N, PS), 0x55, np.int8)
            grid[:M, :P] = np.stack([c["grid"].reshape(-1) for c in cases])
            f.write(np.array([MAGIC, H, W, pmask, N, M, 0, C, dist, int(with_count), 1, 0, int(with_src), int(with_base), int(turns)], np.int32).tobytes())
            f.write(answer.tobytes() + rec.tobytes() + grid.tobytes())
        else:
            buf, offset, stride = CP.place(CP.make_rows(kind, cases, rng), layout)
            f.write(np.array([MAGIC, H, W, pmask, N, M, stride, C, dist, int(with_count), 0, offset, int(with_src), int(with_base), int(turns)], np.int32).tobytes())
            f.write(answer.tobytes() + rec.tobytes() + buf.tobytes())
        if with_count:
            f.write(count.tobytes())
        f.write(bits.tobytes())
        if with_src:
            f.write(src.tobytes())
    return bad


def parse_dump(text, cases, C, with_count, with_base):
    """The standalone program's output -> (turn, base) with SENTINEL where nothing was printed (the program prints 77s in the slots the
    kernel left alone)."""
    M = len(cases)
    turn, base = np.full((M, C, 5, 4), SENTINEL, np.int32), np.full((M, 2), SENTINEL, np.int32)
    lines = text.strip().splitlines()
    i = 0
    for m, c in enumerate(cases):
        if with_base:
            base[m] = [int(v) for v in lines[i].split()]
            i += 1
        for k in range(min(C, len(c["masks"])) if with_count else C):
            for t in range(5):
                v = [int(x) for x in lines[i].split()]
                if v != [77] * 4:
                    turn[m, k, t] = v
                i += 1
    assert i == len(lines)
    return turn, base
