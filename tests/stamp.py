"""Backend-independent checks of arcle_stamp_rows (where a COPY of each object of a state row best fits the answer).  The counterpart of
tests/place.py, whose cases, bit rows, env arrangement, guards and SENTINEL this file takes: every check takes a backend — EmuStamp
(tests/emu/stamp_emu.cpp: the kernel body of arcle_stamp.h lock-step on the CPU) or HipStamp (the product) — and returns a list of
mismatch strings.  The reference point is arcle_amd.search.stamp_numpy, which builds every child grid from the definition and which
tests/test_stamp_host.py pins on the oracle's own CopyO + Paste."""
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
EMU_SRC = os.path.join(EMU_DIR, "stamp_emu.cpp")
EMU_HDRS = PL.EMU_HDRS + [os.path.join(B.ROOT, "arcle_amd", "csrc", "arcle_stamp.h")]
SENTINEL = PL.SENTINEL
COPY_OP, PASTE_OP = 29, 30  # O2ARCv2Env's table: CopyO, Paste (paste_blank)
MOVE_OPS = PL.MOVE_OPS
LARGE = PL.LARGE
DISTS = PL.DISTS
CS = PL.CS
SIZES = PL.SIZES
ORACLE_SIZES = ((5, 5), (7, 6))
TIE_WANT = {"tie dx": (-1, 0), "tie dy": (0, -1), "tie distance": (1, 0), "tie distance y": (0, 1), "tie dx before dy": (-1, 0),
            "tie dx before dy 2": (0, 1), "tie diagonal": (-1, 1)}


def ops_for(kind, blank):
    """The env kind's default table (its Paste has paste_blank); blank False: the same table with the Paste's arg byte 0."""
    ops = list(CP.OPS[kind]())
    if not blank:
        ops = [d & ~0xff00 if (d & 0xff) == 7 else d for d in ops]  # (OP_PASTE = 7: arcle_amd/actions.py)
    return ops


# ---- the cases: those of tests/place.py and what a stamp adds -------------------------------------------------------------------------
_cases = {}


def _paste(grid, mask, px, py, blank=True):
    """numpy CopyO + Paste of `mask`'s clip at (px, py) — used to build ANSWERS only (the mirror under test is stamp_numpy)"""
    H, W = grid.shape
    xs, ys = np.nonzero(mask)
    x0, x1, y0, y1 = xs.min(), xs.max(), ys.min(), ys.max()
    clip = np.where(mask, grid, 0)[x0:x1 + 1, y0:y1 + 1][:H - px, :W - py]
    out = grid.copy()
    dst = out[px:px + clip.shape[0], py:py + clip.shape[1]]
    dst[...] = clip if blank else np.where(clip > 0, clip, dst)
    return out


def cases_of(H, W):
    """The cases of PL.cases_of(H, W) — moved, shrunk a / b (grid_dim below (H, W), a differing answer_dim), bytes (negative bytes
    under rectangles and the whole-grid object, an empty mask), twocolour and one tie case per level of the tie rule (a one-cell
    object: the copy fits two cells equally well) — and the cases place never needed:
      edge right / bottom / both  an L of three cells (two colours) whose box touches the edge(s); the answer holds what a stamp that
                                  HANGS OVER that edge leaves (one column / one row / one cell of the clip)
      hollow                      a 3 x 3 ring around a cell of another colour that is not the object's: with blank = 1 the stamp at
                                  (x0, y0) zeroes it — an edit — and the answer asks for exactly that
      negative                    an object of bytes -3, 5, -128 and 0; the answer holds its blank = 1 copy elsewhere
    (thin grids: edge right at H = 1, edge bottom at W = 1, with a two-cell line)."""
    if (H, W) in _cases:
        return _cases[(H, W)]
    out = list(PL.cases_of(H, W))

    def add(name, grid, answer, masks):
        masks = np.asarray(masks, np.uint8).reshape(-1, H, W)[:16]
        out.append({"name": f"{H}x{W} {name}", "H": H, "W": W, "grid": grid.astype(np.int8), "dim": np.array((H, W), np.int8),
                    "answer": answer.astype(np.int8), "adim": np.array((H, W), np.int8), "masks": masks})
    if H >= 3 and W >= 3:
        for name, (x, y), (px, py) in (("edge right", (0, W - 2), (min(2, H - 2), W - 1)), ("edge bottom", (H - 2, 0), (H - 1, min(2, W - 2))),
                                       ("edge both", (H - 2, W - 2), (H - 1, W - 1))):
            g = np.zeros((H, W), np.int8)
            g[x, y], g[x, y + 1], g[x + 1, y] = 4, 6, 6
            add(name, g, _paste(g, g != 0, px, py), [g != 0])
        g = np.zeros((H, W), np.int8)
        g[:3, :3] = 3
        g[1, 1] = 7
        ans = g.copy()
        ans[1, 1] = 0
        add("hollow", g, ans, [g == 3, g == 7])
        g = np.zeros((H, W), np.int8)
        g[0, 0], g[0, 1], g[1, 0], g[1, 1] = -3, 5, -128, 0
        m = np.zeros((H, W), bool)
        m[:2, :2] = True
        add("negative", g, _paste(g, m, H - 2, W - 2), [m])
    elif H == 1 and W >= 3:
        g = np.zeros((H, W), np.int8)
        g[0, W - 2], g[0, W - 1] = 4, 6
        add("edge right", g, _paste(g, g != 0, 0, W - 1), [g != 0])
    elif W == 1 and H >= 3:
        g = np.zeros((H, W), np.int8)
        g[H - 2, 0], g[H - 1, 0] = 4, 6
        add("edge bottom", g, _paste(g, g != 0, H - 1, 0), [g != 0])
    _cases[(H, W)] = out
    return out


_mirror = {}


def mirror(case, dist, blank):
    """stamp_numpy of a case, computed once per (case, max_dist, blank) over all its objects: (stamp [n, 4], base (2,))"""
    key = (case["name"], dist, bool(blank))
    if key not in _mirror:
        _mirror[key] = S.stamp_numpy(case["grid"], case["dim"], case["answer"], case["adim"], case["masks"], None if dist >= LARGE else dist, bool(blank))
    return _mirror[key]


# ---- the backends -----------------------------------------------------------------------------------------------------------------
class _StampParams(ctypes.Structure):  # mirror of arcle::StampParams (arcle_amd/csrc/arcle_stamp.h)
    _fields_ = [("p", B._StepParams), ("max_comp", ctypes.c_int32), ("max_dist", ctypes.c_int32), ("count", ctypes.c_void_p),
                ("bits", ctypes.c_void_p), ("src_env", ctypes.c_void_p), ("stamp", ctypes.c_void_p), ("base", ctypes.c_void_p),
                ("blank", ctypes.c_int32), ("pad_", ctypes.c_int32)]


_emu = None


def emu_lib():
    global _emu
    if _emu is None:
        so = os.path.join(EMU_DIR, "libstamp_emu.so")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [EMU_SRC] + EMU_HDRS):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, EMU_SRC])
        _emu = ctypes.CDLL(so)
        _emu.stamp_emu_run.argtypes = [ctypes.POINTER(_StampParams), ctypes.c_int]
        assert _emu.stamp_emu_params_size() == ctypes.sizeof(_StampParams), "StampParams layout drifted"
    return _emu


class EmuStamp:
    """The emulated kernel.  fw: -1 = the instantiation the library launches for the width, 0 = FW_GENERIC at any width."""
    BACKEND = B.EmuBackend  # (a subclass may name a backend of another plane stride)
    name = "emu"

    def __init__(self, fw=-1):
        self.fw = fw

    def run(self, kind, H, W, cases, layout, C, dist, with_count, with_src, with_base, blank, rng):
        M = len(cases)
        resident = layout == "resident"
        N, ans, adim, src, bad = PL.envs_for(cases, resident, with_src, rng)
        be = self.BACKEND(N, H, W, 3, kind, CP.OPS[kind]())
        for k in be.buf:
            be.buf[k][:] = 0x55
        be.rec[:] = 0x55
        be.buf["answer"][:, :H * W] = ans.reshape(N, -1)
        be.rec[:, 14:16] = adim
        x = _StampParams()
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
        self.guards = [PL._guarded((M, C, 4)), PL._guarded((M, 2))]
        (_, stamp), (_, base) = self.guards
        x.max_comp, x.max_dist, x.blank = C, dist, int(blank)
        x.count, x.bits, x.src_env = count.ctypes.data if with_count else None, bits.ctypes.data, None if src is None else src.ctypes.data
        x.stamp, x.base = stamp.ctypes.data, base.ctypes.data if with_base else None
        rc = emu_lib().stamp_emu_run(ctypes.byref(x), self.fw)
        assert rc == 0, f"stamp emulator reported error {rc} (divergent cross-lane op / non-uniform value)"
        return stamp, base, bad

    def guards_intact(self):
        return all((buf[:16] == SENTINEL).all() and (buf[-16:] == SENTINEL).all() for buf, _ in self.guards)


class HipStamp:
    """EnvBatch.stamp_rows on the device."""
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

    def run(self, kind, H, W, cases, layout, C, dist, with_count, with_src, with_base, blank, rng):
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
        guard = t.full((M * C * 4 + M * 2 + 48,), SENTINEL, dtype=t.int32, device=b.device)
        stamp, base = guard[16:16 + M * C * 4].view(M, C, 4), guard[32 + M * C * 4:32 + M * C * 4 + 2 * M].view(M, 2)
        b.stamp_rows(view, t.as_tensor(count, device=b.device) if with_count else None, t.as_tensor(bits, device=b.device),
                     None if src is None else t.as_tensor(src, device=b.device), None if dist >= LARGE else dist, bool(blank),
                     out=(stamp, base if with_base else None))
        g = guard.cpu().numpy()
        self._ok = bool((g[:16] == SENTINEL).all() and (g[16 + M * C * 4:32 + M * C * 4] == SENTINEL).all() and (g[32 + M * C * 4 + 2 * M:] == SENTINEL).all())
        return stamp.cpu().numpy(), base.cpu().numpy(), bad

    def guards_intact(self):
        return self._ok


def compare(tag, got, cases, C, dist, with_count, with_base, blank):
    """Everything exact: the four words of every object, the base pair, SENTINEL in the entries >= count and in an absent base."""
    stamp, base, bad = got
    errs = []
    for m, c in enumerate(cases):
        ws, wb = mirror(c, dist, blank)
        n = min(C, len(ws))
        t = f"{tag} row {m} ({c['name']})"
        if m in bad:
            ws, wb = np.zeros_like(ws), (0, 0)
        if not np.array_equal(stamp[m, :n], ws[:n]):
            k = int(np.argwhere((stamp[m, :n] != ws[:n]).any(1))[0, 0])
            errs.append(f"{t}: object {k} {stamp[m, k].tolist()} != {ws[k].tolist()}")
        if with_count:
            if (stamp[m, n:] != SENTINEL).any():
                errs.append(f"{t}: an entry >= count was written")
        else:  # (the slots beyond the case's masks hold empty masks: B empty)
            empty = (0, 0, 0, 0) if m in bad else (0, 0, wb[0], 0)
            if (stamp[m, n:] != np.array(empty)).any():
                errs.append(f"{t}: an empty mask gave {stamp[m, n:][0].tolist()} != {list(empty)}")
        if with_base and tuple(int(v) for v in base[m]) != tuple(wb):
            errs.append(f"{t}: base {base[m].tolist()} != {tuple(wb)}")
        if not with_base and (base[m] != SENTINEL).any():
            errs.append(f"{t}: base was written though not asked for")
    return errs


# size -> the runs of one backend: (kind, layout | "resident", M, C, max_dist, count given, src given, base asked for, blank).  Per
# size: every env kind, the three layouts and the resident form, M = 1 and 37 (None: one row per case; a string: the one case of that
# name), every C of CS, every max_dist of DISTS, count and NULL, src and NULL, both blank values — the run over every case without a
# distance limit once per blank value.  On the flat board the emulator walks the positions one by one, so there its unlimited runs take
# one case each — "bytes" (blank = 1: negative bytes pasted) and "edge both" (blank = 0).  `full` (the device) adds every case at C = 16
# without a limit under the blank value(s) the plan has not yet run that way.
def plan(H, W, full=False):
    if W > 32 or H > 64:
        runs = [("o2arc", "odd", None, 16, 3, True, True, True, True), ("arc", "dense", None, 5, 1, False, False, True, False),
                ("raw", "lib", 1, 1, 0, True, False, False, True), ("raw", "resident", None, 16, 1, True, True, True, False),
                ("o2arc", "lib", 37, 5, 1, True, True, True, True), ("arc", "resident", "bytes", 16, LARGE, False, False, True, True),
                ("o2arc", "dense", 37, 1, 1, False, True, False, False), ("o2arc", "odd", "edge both", 1, LARGE, True, False, True, False)]
        return runs + ([("o2arc", "lib", None, 16, LARGE, True, True, True, True), ("arc", "lib", None, 16, LARGE, True, True, True, False)] if full else [])
    runs = [("o2arc", "odd", None, 16, LARGE, True, True, True, True), ("arc", "dense", None, 5, 3, False, False, True, False),
            ("raw", "lib", 1, 1, 0, True, False, False, True), ("raw", "resident", None, 16, 1, True, True, True, False),
            ("o2arc", "lib", 37, 5, LARGE, True, True, True, True), ("arc", "resident", None, 5, LARGE, False, False, True, False),
            ("o2arc", "dense", 37, 1, 1, False, True, False, False)]
    return runs + ([("arc", "lib", None, 16, LARGE, True, True, True, False)] if full else [])


def run_size(be, H, W, runs=None, full=False):
    runs = runs or plan(H, W, full)
    errs = []
    rng = np.random.default_rng(H * 1000 + W)
    for i, (kind, layout, M, C, dist, with_count, with_src, with_base, blank) in enumerate(runs):
        cases = cases_of(H, W)
        if isinstance(M, str):
            cases = [c for c in cases if c["name"].endswith(M)] or cases[:1]
        elif M is not None:
            cases = PL.pad_to(cases, M) if M > 1 else cases[i % len(cases):][:1]
        tag = f"{be.name} {H}x{W} {kind} {layout} C={C} dist={dist} count={with_count} src={with_src} blank={int(blank)}"
        got = be.run(kind, H, W, cases, layout, C, dist, with_count, with_src, with_base, blank, rng)
        errs += compare(tag, got, cases, C, dist, with_count, with_base, blank)
        if not be.guards_intact():
            errs.append(f"{tag}: bytes around an output buffer were written")
        if len(errs) > 10:
            break
    return errs


# ---- the oracle's side: CopyO on the object's cells, Paste on the one-cell selection (px, py), count the correct cells -------------------
def stamp_macro_set(case):
    """Every cell (px, py) of grid_dim for every object of a case with a cell inside grid_dim as a two-step macro — CopyO on the object's
    cells inside grid_dim, Paste on the one-cell selection (px, py) — one flat set: -> (owner int [K] = the object, cand int [K, 2] =
    (px, py), masks int8 [K, 2, H, W], op int32 [K, 2], length int32 [K])."""
    H, W = case["H"], case["W"]
    gh, gw = (int(v) for v in case["dim"])
    owner, cand = [], []
    for k, mask in enumerate(case["masks"]):
        if (mask[:gh, :gw] != 0).any():
            owner += [k] * (gh * gw)
            cand += [(px, py) for px in range(gh) for py in range(gw)]
    owner, cand = np.array(owner, np.int64), np.array(cand, np.int64).reshape(-1, 2)
    K = len(cand)
    masks = np.zeros((K, 2, H, W), np.int8)
    masks[:, 0, :gh, :gw] = case["masks"][owner][:, :gh, :gw] != 0
    masks[np.arange(K), 1, cand[:, 0], cand[:, 1]] = 1
    op = np.tile(np.array([[COPY_OP, PASTE_OP]], np.int32), (K, 1))
    return owner, cand, masks, op, np.full(K, 2, np.int32)


def oracle_table(case, blank, kind="o2arc"):
    """correct(px, py) of every object of a case for every cell of grid_dim, from the ORACLE (tests/macros.py's chained oracle, mask
    ingress; blank False: a table whose Paste has arg byte 0) -> (table int32 [n, H, W], -1 where nothing was asked, the grid the
    oracle's freshly reset env holds)."""
    import macros as MC
    import search_bits as SB
    H, W = case["H"], case["W"]
    rows, orc = CP.clean_rows(kind, case["grid"][None], case["dim"][None], case["answer"][None], case["adim"][None])
    grid = SB._grids_of(rows, kind, H, W)[0][0]
    owner, cand, masks, op, length = stamp_macro_set(case)
    K = len(cand)
    w = MC.oracle_macros(rows, case["answer"][None], case["adim"][None], kind, H, W, 3, ops_for(kind, blank), "mask",
                         masks.reshape(1, K, 2, H * W), op[None], length[None])
    assert not w["status"].any(), case["name"]
    table = np.full((len(case["masks"]), H, W), -1, np.int32)
    table[owner, cand[:, 0], cand[:, 1]] = w["dense"][0, :, 0]
    return table, grid


# ---- planted tasks: one small object, stamped once or twice into empty space -------------------------------------------------------
SHAPES = (((0, 0), (0, 1), (1, 0)), ((0, 0), (1, 0), (1, 1)), ((0, 0), (1, 1), (2, 2)), ((0, 1), (1, 0), (1, 1), (2, 1)),
          ((0, 0), (0, 1), (1, 1), (1, 2)), ((0, 0), (1, 0), (2, 0), (2, 1)))


def planted_stamp_tasks(n=8, H=12, W=12, seed=33):
    """n tasks on background 0 with ONE object — a shape of three or four cells, one colour, 8-connected — and the answer, made by the
    ORACLE: CopyO on the object's exact cells, Paste on a one-cell selection, once (the first half of the tasks) or twice (the second
    half), at positions whose stamps lie inside the grid and touch (8-neighbourhood) neither the object nor each other.
    -> (inputs [n, H, W], dims [n, 2], answers [n, H, W], the list of (px, py) per task)"""
    rng = np.random.default_rng(seed)
    ops = O.o2arc_ops()
    dims = np.tile(np.array([[H, W]], np.int8), (n, 1))
    inputs, answers, spots = [], [], []
    while len(inputs) < n:
        shape = np.array(SHAPES[int(rng.integers(0, len(SHAPES)))])
        h, w = shape.max(0) + 1
        want = 1 if len(inputs) < n // 2 else 2
        corners = [(int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))) for _ in range(want + 1)]
        if any(abs(a[0] - b[0]) <= h and abs(a[1] - b[1]) <= w for i, a in enumerate(corners) for b in corners[:i]):
            continue  # (two boxes touch or overlap)
        (x, y), targets = corners[0], corners[1:]
        g = np.zeros((H, W), np.int8)
        g[x + shape[:, 0], y + shape[:, 1]] = int(rng.integers(1, 10))
        mask = g != 0
        orc = B.OracleBackend(1, H, W, 3, "o2arc", ops)
        orc.set_tasks(g[None], dims[:1], g[None], dims[:1])
        orc.reset()
        for px, py in targets:
            one = np.zeros((1, H, W), np.int8)
            one[0, px, py] = 1
            orc.step("mask", mask[None].astype(np.int8), np.array([COPY_OP], np.int32))
            orc.step("mask", one, np.array([PASTE_OP], np.int32))
        ans = orc.get("grid")[0]
        assert not orc.status() and (ans != 0).sum() == (want + 1) * mask.sum()
        inputs.append(g)
        answers.append(ans)
        spots.append(targets)
    return np.stack(inputs), dims, np.stack(answers), spots


def stamp_searches(venv, rows, n, depths):
    """The two searches of the demonstration on every task, both at width 1 and depth = the task's number of stamps -> (results of the
    macros the library had before — the Moves on the objects' boxes and CopyO + Paste at another object's box, propose_object_macros —
    and results of propose_stamps)."""
    import torch
    before = [S.beam_search(venv, rows[i:i + 1], None, width=1, depth=depths[i], src_env=torch.tensor([i]),
                            propose=S.propose_object_macros(list(MOVE_OPS), [], [(COPY_OP, PASTE_OP)], any_color=True, diagonal=True)) for i in range(n)]
    stamped = [S.beam_search(venv, rows[i:i + 1], None, width=1, depth=depths[i], src_env=torch.tensor([i]),
                             propose=S.propose_stamps(COPY_OP, PASTE_OP, any_color=True, diagonal=True)) for i in range(n)]
    return before, stamped


def stamp_numpy_rows(grids, gdims, answers, adims, objs, max_dist, blank=True):
    """`ARCVecEnv.stamp` of M grids from stamp_numpy, on torch CPU tensors (the stub vec envs' `stamp`)."""
    import torch
    from arcle_amd.envs.vec import Stamps
    M, C = int(objs.bits.shape[0]), int(objs.bits.shape[1])
    H, W = grids.shape[1:]
    stamp, base = np.zeros((M, C, 4), np.int32), np.zeros((M, 2), np.int32)
    cells = np.unpackbits(objs.bits.numpy(), axis=-1, bitorder="little")[..., :H * W].reshape(M, C, H, W)
    for m in range(M):
        n = int(objs.count[m])
        s, base[m] = S.stamp_numpy(grids[m], gdims[m], answers[m], adims[m], cells[m, :n], max_dist, blank)
        stamp[m, :n] = s
    t = torch.from_numpy(stamp)
    return Stamps(t[:, :, 0], t[:, :, 1], t[:, :, 2], t[:, :, 3], torch.from_numpy(base))


def stamp_venv(answers, adims, H=12, W=12):
    """The oracle-backed stub vec env of tests/place.py + `stamp` (stamp_numpy): what beam_search(propose=propose_stamps(...)) needs,
    on torch CPU tensors."""
    import search_bits as SB
    base = type(PL.place_venv(answers, adims, H, W))

    class StampVenv(base):
        def stamp(self, rows, objs, src_env=None, max_dist=None, blank=True):
            grids, gdims = SB._grids_of(rows.numpy(), self.kind, self.H, self.W)
            src = np.arange(len(grids)) if src_env is None else src_env.numpy()
            return stamp_numpy_rows(grids, gdims, self.answers[src], self.adims[src], objs, max_dist, blank)
    return StampVenv("o2arc", H, W, 3, O.o2arc_ops(), answers, adims)


# the planted tasks that the macros the library had before solve at the same width and depth: found with the oracle-backed stub
# (tests/test_stamp_host.py) when the tasks were chosen; the device test asserts the same number
BEFORE_SOLVES = 0


# ---- one dumped case for the standalone sanitized emulator ------------------------------------------------------------------------
MAGIC = 0x5354414d


def dump_case(path, kind, H, W, cases, layout, C, dist, with_count, with_src, with_base, blank, rng):
    """Writes one case in the format stamp_emu.cpp's main() reads: buffers exactly as long as the data.  -> the rows without an env"""
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
    with open(path, "wb") as f:
        if resident:
            rec[:M, 2:4] = np.stack([c["dim"] for c in cases])
            grid = np.full((N, PS), 0x55, np.int8)
            grid[:M, :P] = np.stack([c["grid"].reshape(-1) for c in cases])
            f.write(np.array([MAGIC, H, W, pmask, N, M, 0, C, dist, int(with_count), 1, 0, int(with_src), int(with_base), int(blank)], np.int32).tobytes())
            f.write(answer.tobytes() + rec.tobytes() + grid.tobytes())
        else:
            buf, offset, stride = CP.place(CP.make_rows(kind, cases, rng), layout)
            f.write(np.array([MAGIC, H, W, pmask, N, M, stride, C, dist, int(with_count), 0, offset, int(with_src), int(with_base), int(blank)], np.int32).tobytes())
            f.write(answer.tobytes() + rec.tobytes() + buf.tobytes())
        if with_count:
            f.write(count.tobytes())
        f.write(bits.tobytes())
        if with_src:
            f.write(src.tobytes())
    return bad
