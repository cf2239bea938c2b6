"""Backend-independent checks of arcle_mirror_rows (each object's box filled from its mirror image).  The counterpart of tests/turn.py,
whose env arrangement, bit rows, guards and SENTINEL this file takes from tests/place.py as that one does: every check takes a backend —
EmuMirror (tests/emu/mirror_emu.cpp: the kernel body of arcle_mirror.h lock-step on the CPU) or HipMirror (the product) — and returns a
list of mismatch strings.  The reference point is arcle_amd.search.mirror_numpy, which builds every child grid from the definition and
which tests/test_mirror_host.py pins on the oracle's own CopyO + Paste + Flip."""
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
EMU_SRC = os.path.join(EMU_DIR, "mirror_emu.cpp")
EMU_HDRS = PL.EMU_HDRS + [os.path.join(B.ROOT, "arcle_amd", "csrc", f) for f in ("arcle_stamp.h", "arcle_turn.h", "arcle_mirror.h")]
SENTINEL = PL.SENTINEL
COPY_OP, PASTE_OP = ST.COPY_OP, ST.PASTE_OP  # O2ARCv2Env's table: CopyO, Paste (paste_blank)
FLIP_OPS = (26, 27)                          # ... Flip H, Flip V
SLOT_NAMES = ("H", "V", "point")
ALL = 7
LARGE = PL.LARGE
DISTS = PL.DISTS
CS = PL.CS
SIZES = PL.SIZES + ((5, 5), (7, 6), (6, 9), (12, 12))
ORACLE_SIZES = ((5, 5), (7, 6), (6, 9))
# the tie cases: a one-cell object at the centre (cx, cy) on an empty grid whose only two coloured cells sit at centre + spot; the answer
# holds the colour at the centre, so both spots are equally good sources
TIE_SPOTS = {"mtie dx": ((-1, 0), (1, 0)), "mtie dy": ((0, -1), (0, 1)), "mtie distance": ((1, 0), (-2, 0)), "mtie distance y": ((0, -2), (0, 1)),
             "mtie dx before dy": ((-1, 0), (0, -1)), "mtie dx before dy 2": ((1, 0), (0, 1)), "mtie diagonal": ((1, -1), (-1, 1))}


def tie_want(name, s):
    """The (dx, dy) the tie rule names in slot s: of the spots the slot allows (dx = 0 under H, dy = 0 under V) the nearer one, then the
    smaller dx, then the smaller dy; no spot allowed: every candidate scores the same and (0, 0) is the nearest."""
    ok = [(abs(a) + abs(b), a, b) for a, b in TIE_SPOTS[name] if (s != 0 or a == 0) and (s != 1 or b == 0)]
    return min(ok)[1:] if ok else (0, 0)


def ops_for(kind, blank):
    return ST.ops_for(kind, blank)


# ---- the cases: those of tests/place.py and what a mirror adds ------------------------------------------------------------------------
_cases = {}


def symmetric(rng, H, W, s, a, b, colours):
    """Noise of `colours` on H x W that is symmetric under slot s inside rows [0, 2a) x columns [0, 2b) — H: every row of the region
    reads the same from both ends (all H rows, a is ignored), V: every column (all W columns), point: the region equals its half turn —
    and plain noise elsewhere."""
    p = rng.choice(colours, (H, W))
    if s == 0:
        p[:, b:2 * b] = p[:, :b][:, ::-1]
    elif s == 1:
        p[a:2 * a] = p[:a][::-1]
    else:
        p[a:2 * a, :2 * b] = p[:a, :2 * b][::-1, ::-1]
    return p


def cases_of(H, W):
    """The cases of PL.cases_of(H, W) — moved (non-rectangular multi-colour objects: the whole box is replaced; an empty mask), shrunk a /
    b (grid_dim below (H, W) with junk outside it, answer_dim larger on one axis and smaller on the other, object cells outside
    grid_dim), bytes (the whole-grid object: only dx = dy = 0; rectangles over negative bytes and bytes above 9), twocolour, place's tie
    cases — and the cases only a mirror needs (H, W >= 4; the answer is the full pattern, the grid the pattern with the hole zeroed, the
    object the hole):
      lr / ud / pt central      left-right-, up-down- and point-symmetric noise about the central axis, a rectangular hole on one side
      lr / ud / pt off          the same about an axis (a centre) in the first third: the rest of the grid is plain noise
      edge top / bottom / left / right   a hole touching that edge: candidates exist on one side only
      wide                      a hole wider than half the grid: every source rectangle overlaps it
      lshape                    a non-rectangular hole: the whole box is replaced, cells that were right included
      odd bytes                 a pattern of bytes -128, -1, 0, 3, 37, 127, the hole filled with 5s: pos() drops the sources <= 0, and
                                with blank = 0 they are not pasted (the 5 shows through); the answer holds pos() of the pattern
      show through              zeros in the source and 7s in the hole: blank = 0 and blank = 1 differ
      mtie *                    one per level of the tie rule (TIE_SPOTS)
    (thin grids: a symmetric line with a hole along the one axis)."""
    if (H, W) in _cases:
        return _cases[(H, W)]
    out = list(PL.cases_of(H, W))
    rng = np.random.default_rng(5000 + 131 * H + W)

    def add(name, grid, answer, masks):
        masks = np.asarray(masks, np.uint8).reshape(-1, H, W)[:16]
        out.append({"name": f"{H}x{W} {name}", "H": H, "W": W, "grid": grid.astype(np.int8), "dim": np.array((H, W), np.int8),
                    "answer": answer.astype(np.int8), "adim": np.array((H, W), np.int8), "masks": masks})

    def holed(p, x0, x1, y0, y1, fill=0, cut=None):
        m = np.zeros((H, W), bool)
        m[x0:x1 + 1, y0:y1 + 1] = True
        if cut is not None:
            m[cut] = False
        return np.where(m, fill, p), m
    cols = [1, 2, 3, 4, 6]
    if H >= 4 and W >= 4:
        for s, tag in enumerate(("lr", "ud", "pt")):
            for name, (a, b) in (("central", (H // 2, W // 2)), ("off", (max(1, H // 3), max(1, W // 3)))):
                p = symmetric(rng, H, W, s, a, b, cols)
                # the hole: in the second half of the symmetric region, off the axis where there is room
                x0, y0 = (0 if s == 0 else a + (a > 2)), (0 if s == 1 else b + (b > 2))
                x1, y1 = min(x0 + 1, (H if s == 0 else 2 * a) - 1), min(y0 + 2, (W if s == 1 else 2 * b) - 1)
                g, m = holed(p, x0, x1, y0, y1)
                add(f"{tag} {name}", g, p, [m])
        pv, ph = symmetric(rng, H, W, 1, H // 2, 0, cols), symmetric(rng, H, W, 0, 0, W // 2, cols)
        for name, p, box in (("edge top", pv, (0, 0, 1, W - 2)), ("edge bottom", pv, (2 * (H // 2) - 1, 2 * (H // 2) - 1, 0, 1)),
                             ("edge left", ph, (1, H - 2, 0, 0)), ("edge right", ph, (0, 1, 2 * (W // 2) - 1, 2 * (W // 2) - 1))):
            g, m = holed(p, *box)
            add(name, g, p, [m])
        g, m = holed(ph, 1, 2, 1, W // 2 + 1)
        add("wide", g, ph, [m])
        g, m = holed(ph, 0, 2, W // 2, W // 2 + 1, cut=(0, W // 2))
        add("lshape", g, ph, [m])
        p = symmetric(rng, H, W, 0, 0, W // 2, [-128, -1, 0, 3, 37, 127])
        g, m = holed(p, 0, 1, W // 2, W // 2 + 1, fill=5)
        add("odd bytes", g, np.where(m, np.maximum(p, 0), p), [m])
        p = symmetric(rng, H, W, 2, H // 2, W // 2, [0, 0, 2, 4])
        g, m = holed(p, H // 2, H // 2 + 1, 0, 2, fill=7)
        add("show through", g, p, [m])
    elif H == 1 and W >= 4:
        p = symmetric(rng, H, W, 0, 0, W // 2, cols)
        g, m = holed(p, 0, 0, W // 2, W // 2 + 1)
        add("lr central", g, p, [m])
    elif W == 1 and H >= 4:
        p = symmetric(rng, H, W, 1, H // 2, 0, cols)
        g, m = holed(p, H // 2, H // 2 + 1, 0, 0)
        add("ud central", g, p, [m])
    cx, cy = H // 2, W // 2
    for name, spots in TIE_SPOTS.items():
        if all(0 <= cx + a < H and 0 <= cy + b < W for a, b in spots):
            g, ans = np.zeros((H, W), np.int8), np.zeros((H, W), np.int8)
            for a, b in spots:
                g[cx + a, cy + b] = 5
            ans[cx, cy] = 5
            m = np.zeros((H, W), bool)
            m[cx, cy] = True
            add(name, g, ans, [m])
    _cases[(H, W)] = out
    return out


_mirror = {}


def mirror(case, dist, blank):
    """mirror_numpy of a case with all three slots, computed once per (case, max_dist, blank) over all its objects: (mirror [n, 3, 4],
    base (2,))"""
    key = (case["name"], dist, bool(blank))
    if key not in _mirror:
        _mirror[key] = S.mirror_numpy(case["grid"], case["dim"], case["answer"], case["adim"], case["masks"], None if dist >= LARGE else dist, ALL, bool(blank))
    return _mirror[key]


# ---- the backends -----------------------------------------------------------------------------------------------------------------
class _MirrorParams(ctypes.Structure):  # mirror of arcle::MirrorParams (arcle_amd/csrc/arcle_mirror.h)
    _fields_ = [("p", B._StepParams), ("max_comp", ctypes.c_int32), ("max_dist", ctypes.c_int32), ("count", ctypes.c_void_p),
                ("bits", ctypes.c_void_p), ("src_env", ctypes.c_void_p), ("mirror", ctypes.c_void_p), ("base", ctypes.c_void_p),
                ("mirrors", ctypes.c_uint32), ("blank", ctypes.c_int32)]


_emu = None


def emu_lib():
    global _emu
    if _emu is None:
        so = os.path.join(EMU_DIR, "libmirror_emu.so")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [EMU_SRC] + EMU_HDRS):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, EMU_SRC])
        _emu = ctypes.CDLL(so)
        _emu.mirror_emu_run.argtypes = [ctypes.POINTER(_MirrorParams), ctypes.c_int]
        assert _emu.mirror_emu_params_size() == ctypes.sizeof(_MirrorParams), "MirrorParams layout drifted"
    return _emu


class EmuMirror:
    """The emulated kernel.  fw: -1 = the instantiation the library launches for the width, 0 = FW_GENERIC at any width."""
    BACKEND = B.EmuBackend  # (a subclass may name a backend of another plane stride)
    name = "emu"

    def __init__(self, fw=-1):
        self.fw = fw

    def run(self, kind, H, W, cases, layout, C, dist, with_count, with_src, with_base, mirrors, blank, rng):
        M = len(cases)
        resident = layout == "resident"
        N, ans, adim, src, bad = PL.envs_for(cases, resident, with_src, rng)
        be = self.BACKEND(N, H, W, 3, kind, CP.OPS[kind]())
        for k in be.buf:
            be.buf[k][:] = 0x55
        be.rec[:] = 0x55
        be.buf["answer"][:, :H * W] = ans.reshape(N, -1)
        be.rec[:, 14:16] = adim
        x = _MirrorParams()
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
        self.guards = [PL._guarded((M, C, 3, 4)), PL._guarded((M, 2))]
        (_, mir), (_, base) = self.guards
        x.max_comp, x.max_dist, x.mirrors, x.blank = C, min(dist, 2048), mirrors, int(blank)
        x.count, x.bits, x.src_env = count.ctypes.data if with_count else None, bits.ctypes.data, None if src is None else src.ctypes.data
        x.mirror, x.base = mir.ctypes.data, base.ctypes.data if with_base else None
        rc = emu_lib().mirror_emu_run(ctypes.byref(x), self.fw)
        assert rc == 0, f"mirror emulator reported error {rc} (divergent cross-lane op / non-uniform value)"
        return mir, base, bad

    def guards_intact(self):
        return all((buf[:16] == SENTINEL).all() and (buf[-16:] == SENTINEL).all() for buf, _ in self.guards)


class HipMirror:
    """EnvBatch.mirror_rows on the device."""
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

    def run(self, kind, H, W, cases, layout, C, dist, with_count, with_src, with_base, mirrors, blank, rng):
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
        nt = M * C * 12
        guard = t.full((nt + M * 2 + 48,), SENTINEL, dtype=t.int32, device=b.device)
        mir, base = guard[16:16 + nt].view(M, C, 3, 4), guard[32 + nt:32 + nt + 2 * M].view(M, 2)
        b.mirror_rows(view, t.as_tensor(count, device=b.device) if with_count else None, t.as_tensor(bits, device=b.device),
                      None if src is None else t.as_tensor(src, device=b.device), None if dist >= LARGE else dist, mirrors, blank,
                      out=(mir, base if with_base else None))
        g = guard.cpu().numpy()
        self._ok = bool((g[:16] == SENTINEL).all() and (g[16 + nt:32 + nt] == SENTINEL).all() and (g[32 + nt + 2 * M:] == SENTINEL).all())
        return mir.cpu().numpy(), base.cpu().numpy(), bad

    def guards_intact(self):
        return self._ok


def compare(tag, got, cases, C, dist, with_count, with_base, mirrors, blank):
    """Everything exact: the four words of every slot asked for of every object, the base pair, SENTINEL in the slots not asked for, in
    the entries >= count and in an absent base."""
    mir, base, bad = got
    errs = []
    asked = np.array([(mirrors >> s) & 1 for s in range(3)], bool)
    for m, c in enumerate(cases):
        wt, wb = mirror(c, dist, blank)
        n = min(C, len(wt))
        t = f"{tag} row {m} ({c['name']})"
        if m in bad:
            wt, wb = np.zeros_like(wt), (0, 0)
        if not np.array_equal(mir[m, :n][:, asked], wt[:n][:, asked]):
            k, s = (int(v) for v in np.argwhere((mir[m, :n] != wt[:n]).any(2) & asked)[0])
            errs.append(f"{t}: object {k} slot {SLOT_NAMES[s]} {mir[m, k, s].tolist()} != {wt[k, s].tolist()}")
        if (mir[m][:, ~asked] != SENTINEL).any():
            errs.append(f"{t}: a slot that was not asked for was written")
        if with_count:
            if (mir[m, n:] != SENTINEL).any():
                errs.append(f"{t}: an entry >= count was written")
        else:  # (the slots beyond the case's masks hold empty masks: nothing is copied, the grid scores what it scores)
            empty = (0, 0, 0, 0) if m in bad else (0, 0, wb[0], 1)
            if (mir[m, n:][:, asked] != np.array(empty)).any():
                errs.append(f"{t}: an empty mask gave {mir[m, n:][:, asked].reshape(-1, 4)[0].tolist()} != {list(empty)}")
        if with_base and tuple(int(v) for v in base[m]) != tuple(wb):
            errs.append(f"{t}: base {base[m].tolist()} != {tuple(wb)}")
        if not with_base and (base[m] != SENTINEL).any():
            errs.append(f"{t}: base was written though not asked for")
    return errs


# size -> the runs of one backend: (kind, layout | "resident", M, C, max_dist, count given, src given, base asked for, mirrors, blank).
# Per size: every env kind, the three layouts and the resident form, M = 1 and 37 (None: one row per case; a string: the cases whose
# name ends with it), every C of CS, every max_dist of DISTS, count and NULL, src and NULL, every non-empty set of slots, both Pastes —
# every case with all slots and without a distance limit once per Paste.  On the flat board the emulator walks the candidates one by
# one, so there its unlimited runs take few cases; `full` (the device) adds every case at C = 16 without a limit under both Pastes.
def plan(H, W, full=False):
    if W > 32 or H > 64:
        runs = [("o2arc", "odd", None, 16, 3, True, True, True, ALL, True), ("arc", "dense", None, 5, 1, False, False, True, 1, False),
                ("raw", "lib", 1, 1, 0, True, False, False, 2, True), ("raw", "resident", None, 16, 1, True, True, True, 4, False),
                ("o2arc", "lib", 37, 5, 1, True, True, True, 3, True), ("arc", "resident", "odd bytes", 16, LARGE, False, False, True, ALL, True),
                ("o2arc", "dense", 37, 1, 1, False, True, False, 6, False), ("o2arc", "odd", "show through", 1, LARGE, True, False, True, ALL, False),
                ("arc", "lib", None, 5, 3, True, False, True, 5, False)]
        return runs + ([("o2arc", "lib", None, 16, LARGE, True, True, True, ALL, True), ("arc", "lib", None, 16, LARGE, True, True, True, ALL, False)] if full else [])
    return [("o2arc", "odd", None, 16, LARGE, True, True, True, ALL, True), ("arc", "dense", None, 5, 3, False, False, True, 1, False),
            ("raw", "lib", 1, 1, 0, True, False, False, 2, True), ("raw", "resident", None, 16, 1, True, True, True, 4, False),
            ("o2arc", "lib", 37, 5, LARGE, True, True, True, 3, True), ("arc", "resident", None, 5, LARGE, False, False, True, 5, False),
            ("o2arc", "dense", 37, 1, 1, False, True, False, 6, False), ("arc", "lib", None, 16, LARGE, True, False, True, ALL, False)]


def run_size(be, H, W, runs=None, full=False):
    runs = runs or plan(H, W, full)
    errs = []
    rng = np.random.default_rng(H * 1000 + W)
    for i, (kind, layout, M, C, dist, with_count, with_src, with_base, mirrors, blank) in enumerate(runs):
        cases = cases_of(H, W)
        if isinstance(M, str):
            cases = [c for c in cases if c["name"].endswith(M)] or cases[:1]
        elif M is not None:
            cases = PL.pad_to(cases, M) if M > 1 else cases[i % len(cases):][:1]
        tag = f"{be.name} {H}x{W} {kind} {layout} C={C} dist={dist} count={with_count} src={with_src} mirrors={mirrors} blank={int(blank)}"
        got = be.run(kind, H, W, cases, layout, C, dist, with_count, with_src, with_base, mirrors, blank, rng)
        errs += compare(tag, got, cases, C, dist, with_count, with_base, mirrors, blank)
        if not be.guards_intact():
            errs.append(f"{tag}: bytes around an output buffer were written")
        if len(errs) > 10:
            break
    return errs


# ---- the oracle's side: CopyO on R, Paste at the box's corner, Flip(s) of the box ----------------------------------------------------
def mirror_macro_set(case, grid, blank=True):
    """Every candidate (s, dx, dy) of every object of a case (max_dist unlimited, from mirror_numpy's table: its -1 entries are no
    candidates) as a macro on int8 masks, one flat set: -> (owner int [K] = the object, cand int [K, 3] = (s, dx, dy), masks int8 [K, 4,
    H, W], op int32 [K, 4], length int32 [K], the table).  Step 0 = the rectangle R with CopyO, step 1 = the one cell (x0, y0) with
    Paste, step 2 = the box's rectangle with Flip H (slots H and point) or Flip V (slot V), step 3 (point) = the empty selection with
    Flip V."""
    H, W = case["H"], case["W"]
    gh, gw = (int(v) for v in case["dim"])
    _, _, table = S.mirror_numpy(grid, case["dim"], case["answer"], case["adim"], case["masks"], None, ALL, blank, full=True)
    owner, cand = [], []
    for k in range(len(case["masks"])):
        c = np.argwhere(table[k] >= 0) - (0, H - 1, W - 1)
        owner += [k] * len(c)
        cand += c.tolist()
    owner, cand = np.array(owner, np.int64), np.array(cand, np.int64).reshape(-1, 3)
    K = len(cand)
    masks = np.zeros((K, 4, H, W), np.int8)
    op = np.full((K, 4), -1, np.int32)
    for j, (s, dx, dy) in enumerate(cand):
        xs, ys = np.nonzero(case["masks"][owner[j]][:gh, :gw])
        x0, x1, y0, y1 = xs.min(), xs.max(), ys.min(), ys.max()
        masks[j, 0, x0 + dx:x1 + dx + 1, y0 + dy:y1 + dy + 1] = 1
        masks[j, 1, x0, y0] = 1
        masks[j, 2, x0:x1 + 1, y0:y1 + 1] = 1
        op[j, :3] = (COPY_OP, PASTE_OP, FLIP_OPS[1] if s == 1 else FLIP_OPS[0])
        if s == 2:
            op[j, 3] = FLIP_OPS[1]
    return owner, cand, masks, op, np.where(cand[:, 0] == 2, 4, 3).astype(np.int32) if K else np.zeros(0, np.int32), table


def bits_of(masks):
    """int8 masks [..., H, W] -> bit rows uint8 [..., 128]"""
    return B.pack_bits(masks.reshape((-1,) + masks.shape[-2:])).reshape(masks.shape[:-2] + (B.BITS_STRIDE,))


def oracle_children(case, blank, kind="o2arc"):
    """Every candidate of every object of a case on the ORACLE (tests/macros.py's chained oracle, mask ingress; blank False: a table whose
    Paste has arg byte 0) -> (the oracle's child grids [K, H, W] and dense pairs [K, 2], the mirror's correct at the same candidates
    [K], cand [K, 3], owner [K], the grid the freshly reset env holds)."""
    import macros as MC
    import search_bits as SB
    H, W = case["H"], case["W"]
    rows, orc = CP.clean_rows(kind, case["grid"][None], case["dim"][None], case["answer"][None], case["adim"][None])
    grid = SB._grids_of(rows, kind, H, W)[0][0]
    owner, cand, masks, op, length, table = mirror_macro_set(case, grid, blank)
    K = len(cand)
    if not K:
        return np.zeros((0, H, W), np.int8), np.zeros((0, 2), np.int32), np.zeros(0, np.int32), cand, owner, grid
    w = MC.oracle_macros(rows, case["answer"][None], case["adim"][None], kind, H, W, 3, ops_for(kind, blank), "mask", masks.reshape(1, K, 4, H * W),
                         op[None], length[None])
    assert not w["status"].any(), case["name"]
    grids, gdims = SB._grids_of(w["rows"][0], kind, H, W)
    assert (gdims == case["dim"]).all()
    return grids, w["dense"][0], table[owner, cand[:, 0], cand[:, 1] + H - 1, cand[:, 2] + W - 1], cand, owner, grid


def child_numpy(grid, mask, dim, s, dx, dy, blank):
    """The child grid of one candidate, by the definition (used to compare GRIDS with the oracle; mirror_numpy builds the same)"""
    gh, gw = int(dim[0]), int(dim[1])
    xs, ys = np.nonzero(mask[:gh, :gw])
    x0, x1, y0, y1 = xs.min(), xs.max(), ys.min(), ys.max()
    tile = grid[x0 + dx:x1 + dx + 1, y0 + dy:y1 + dy + 1]
    if not blank:
        tile = np.where(tile > 0, tile, grid[x0:x1 + 1, y0:y1 + 1])
    tile = (np.fliplr(tile), np.flipud(tile), np.flipud(np.fliplr(tile)))[s]
    out = grid.copy()
    out[x0:x1 + 1, y0:y1 + 1] = np.where(tile > 0, tile, 0)
    return out


# ---- planted tasks: a symmetric pattern with one or two rectangles punched out --------------------------------------------------------
PLANTED = ((0, 6, 1), (1, 6, 1), (2, 6, 1), (0, 4, 2), (1, 4, 2), (2, 5, 1), (0, 5, 2), (2, 4, 2))  # (slot, half-width of the region, holes)


def planted_mirror_tasks(n=8, H=12, W=12, seed=71):
    """n tasks: block noise of colours 1 .. 4 (2 x 2 blocks, so that a grid has a few dozen one-colour components) that is left-right-,
    up-down- or point-symmetric inside a region about an axis (a centre) that is central (half-width 6) or off-centre (4, 5; plain noise
    beyond it), with one or two rectangular holes of at least 6 cells zeroed in the second half of the region.  The true content of every
    hole has at least 3 colours and is not itself symmetric under the task's slot; the mirror image of every hole is intact.  The answer
    is the full pattern.  -> (inputs [n, H, W], dims [n, 2], answers [n, H, W], the list of (slot, [hole boxes (x0, y0, x1, y1)]))"""
    rng = np.random.default_rng(seed)
    dims = np.tile(np.array([[H, W]], np.int8), (n, 1))
    inputs, answers, plans = [], [], []
    while len(inputs) < n:
        s, a, holes = PLANTED[len(inputs) % len(PLANTED)]
        p = np.kron(rng.integers(1, 5, (H // 2, W // 2)), np.ones((2, 2), np.int64))
        p = np.roll(p, (int(rng.integers(0, 2)), int(rng.integers(0, 2))), (0, 1))
        if s == 0:
            p[:, a:2 * a] = p[:, :a][:, ::-1]
        elif s == 1:
            p[a:2 * a] = p[:a][::-1]
        else:
            p[a:2 * a, :2 * a] = p[:a, :2 * a][::-1, ::-1]
        g, boxes, ok = p.copy(), [], True
        taken = np.zeros((H, W), bool)
        for _ in range(holes):
            h, w = (int(v) for v in rng.choice([2, 3, 4], 2))
            lo_x, hi_x = (0, H - h) if s == 0 else (a, 2 * a - h)
            lo_y, hi_y = (0, W - w) if s == 1 else ((a, 2 * a - w) if s == 0 else (0, 2 * a - w))
            x0, y0 = int(rng.integers(lo_x, hi_x + 1)), int(rng.integers(lo_y, hi_y + 1))
            box = np.zeros((H, W), bool)
            box[x0:x0 + h, y0:y0 + w] = True
            # the hole's mirror image, and a one-cell margin around the hole so that two holes stay two components
            img = (box[:, ::-1] if s == 0 else box[::-1] if s == 1 else box[::-1, ::-1])
            img = np.roll(img, ((0 if s == 0 else 2 * a - H), (0 if s == 1 else 2 * a - W)), (0, 1))
            near = np.zeros((H, W), bool)
            near[max(x0 - 1, 0):x0 + h + 1, max(y0 - 1, 0):y0 + w + 1] = True
            content = p[x0:x0 + h, y0:y0 + w]
            flipped = (np.fliplr(content), np.flipud(content), np.flipud(np.fliplr(content)))[s]
            if h * w < 6 or (near & taken).any() or (img & (taken | box)).any() or len(set(content.ravel().tolist())) < 3 or np.array_equal(content, flipped):
                ok = False
                break
            taken |= box | img
            g[box] = 0
            boxes.append((x0, y0, x0 + h - 1, y0 + w - 1))
        if not ok:
            continue
        inputs.append(g.astype(np.int8))
        answers.append(p.astype(np.int8))
        plans.append((s, boxes))
    return np.stack(inputs), dims, np.stack(answers), plans


def mirror_numpy_rows(grids, gdims, answers, adims, objs, max_dist, mirrors=ALL, blank=True):
    """`ARCVecEnv.mirror` of M grids from mirror_numpy, on torch CPU tensors (the stub vec envs' `mirror`)."""
    import torch
    from arcle_amd.envs.vec import Mirrors
    M, C = int(objs.bits.shape[0]), int(objs.bits.shape[1])
    H, W = grids.shape[1:]
    mir, base = np.zeros((M, C, 3, 4), np.int32), np.zeros((M, 2), np.int32)
    cells = np.unpackbits(objs.bits.numpy(), axis=-1, bitorder="little")[..., :H * W].reshape(M, C, H, W)
    for m in range(M):
        n = int(objs.count[m])
        s, base[m] = S.mirror_numpy(grids[m], gdims[m], answers[m], adims[m], cells[m, :n], max_dist, mirrors, blank)
        mir[m, :n] = s
    t = torch.from_numpy(mir)
    return Mirrors(t[..., 0], t[..., 1], t[..., 2], t[..., 3], torch.from_numpy(base))


def mirror_venv(answers, adims, H=12, W=12):
    """The oracle-backed stub vec env of tests/ray.py (objects, place, stamp, turn, align, rays from their mirrors) + `mirror`
    (mirror_numpy): what beam_search(propose=propose_mirrors(...)) and the six earlier proposers need, on torch CPU tensors."""
    import ray as RY
    import search_bits as SB
    base = type(RY.ray_venv(answers, adims, H, W))

    class MirrorVenv(base):
        def mirror(self, rows, objs, src_env=None, max_dist=None, mirrors=ALL, blank=True):
            grids, gdims = SB._grids_of(rows.numpy(), self.kind, self.H, self.W)
            src = np.arange(len(grids)) if src_env is None else src_env.numpy()
            return mirror_numpy_rows(grids, gdims, self.answers[src], self.adims[src], objs, max_dist, mirrors, blank)
    return MirrorVenv("o2arc", H, W, 3, O.o2arc_ops(), answers, adims)


MAX_OBJECTS = 64  # the objects per state the mirror proposer looks at on the planted tasks: every one-colour component, the holes (0) included


def propose():
    return S.propose_mirrors(COPY_OP, PASTE_OP, FLIP_OPS, max_components=MAX_OBJECTS, skip_color=-1)


def searches(venv, rows, n, depths, before=True):
    """-> (the results of propose_mirrors at width 1 and depth = the task's number of holes on every task, {name: the results of the six
    proposers the library had at the same width and depth — the argument lists of tests/ray.py::searches plus propose_rays} — empty with
    before=False)"""
    import ray as RY
    import torch

    def one(prop):
        return [S.beam_search(venv, rows[i:i + 1], None, width=1, depth=depths[i], src_env=torch.tensor([i]), propose=prop) for i in range(n)]
    mirrored = one(propose())
    if not before:
        return mirrored, {}
    earlier = RY.searches(venv, rows, n, depths)
    return mirrored, dict(earlier[1], rays=earlier[0])


def replay_on_oracle(inp, dim, ans, seq):
    """The (selection, op) sequence on the oracle (O2ARCv2Env's table) from the task's initial state -> 1 if no step raised a status bit
    and the grid it leaves is the answer, else 0."""
    H, W = inp.shape
    orc = B.OracleBackend(1, H, W, 3, "o2arc", O.o2arc_ops())
    orc.set_tasks(inp[None], dim[None], ans[None], dim[None])
    orc.reset()
    for sel, op in seq:
        assert sel.dtype == bool and sel.shape == (H, W)
        orc.step("mask", sel[None].astype(np.int8), np.array([op], np.int32))
    return int(not orc.status() and np.array_equal(orc.get("grid")[0], ans) and np.array_equal(orc.get("grid_dim")[0], dim))


# the planted tasks that the six earlier proposers solve at the same width and depth (the sum over the six): found with the oracle-backed
# stub (tests/test_mirror_host.py) when the tasks were chosen; the device test asserts the same number
BEFORE_SOLVES = 0


# ---- one dumped case for the standalone sanitized emulator ------------------------------------------------------------------------
MAGIC = 0x4d495252


def dump_case(path, kind, H, W, cases, layout, C, dist, with_count, with_src, with_base, mirrors, blank, rng):
    """Writes one case in the format mirror_emu.cpp's main() reads: buffers exactly as long as the data.  -> the rows without an env"""
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

    def header(stride, res, offset):
        return np.array([MAGIC, H, W, pmask, N, M, stride, C, dist, int(with_count), res, offset, int(with_src), int(with_base), int(mirrors), int(blank)],
                        np.int32).tobytes()
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
    return bad


def parse_dump(text, cases, C, with_count, with_base):
    """The standalone program's output -> (mirror, base) with SENTINEL where nothing was printed (the program prints 77s in the slots
    the kernel left alone)."""
    M = len(cases)
    mir, base = np.full((M, C, 3, 4), SENTINEL, np.int32), np.full((M, 2), SENTINEL, np.int32)
    lines = text.strip().splitlines()
    i = 0
    for m, c in enumerate(cases):
        if with_base:
            base[m] = [int(v) for v in lines[i].split()]
            i += 1
        for k in range(min(C, len(c["masks"])) if with_count else C):
            for s in range(3):
                v = [int(x) for x in lines[i].split()]
                if v != [77] * 4:
                    mir[m, k, s] = v
                i += 1
    assert i == len(lines)
    return mir, base
