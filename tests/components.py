"""Backend-independent checks of arcle_components_rows (the connected components of every state row's grid as ready-made actions).
The pattern of tests/search.py: every check takes a backend — EmuComponents (tests/emu/components_emu.cpp: the kernel body of
arcle_components.h lock-step on the CPU) or HipComponents (the product) — and returns a list of mismatch strings.  The reference point is
arcle_amd.search.components_numpy, which tests/test_components_host.py pins on tests/golden/components/components.npz (the reference's own dfs)."""
import ctypes
import json
import os
import subprocess

import numpy as np

import backends as B
from arcle_amd import search as S
from oracle import oracle as O

EMU_DIR = os.path.join(B.ROOT, "tests", "emu")
EMU_SRC = os.path.join(EMU_DIR, "components_emu.cpp")
EMU_HDRS = [os.path.join(B.ROOT, "arcle_amd", "csrc", h) for h in ("arcle_wave.h", "arcle_components.h")]
SKIPS = (-1, 0, 3)
SENTINEL = 77
OPS = {"o2arc": O.o2arc_ops, "arc": O.arc_ops, "raw": O.raw_ops}
LAYOUTS = ("lib", "dense", "odd")  # the library's stride (16-byte multiple, aligned) | stride = L | an odd byte offset and stride L + 5


def skip_tag(s):
    return "m1" if s < 0 else str(s)


_fixture = None


def fixture():
    """-> list of {"name", "H", "W", "grid", "dim", "want": {skip: (comp int32 [n, 8], label int16 [H, W])}} from components.npz"""
    global _fixture
    if _fixture is None:
        z = np.load(os.path.join(B.GOLDEN_DIR, "components", "components.npz"))
        names = json.loads(str(z["names"]))
        _fixture = []
        for i, name in enumerate(names):
            g = z[f"grid_{i}"]
            _fixture.append({"name": name, "H": g.shape[0], "W": g.shape[1], "grid": g, "dim": z[f"dim_{i}"],
                             "want": {s: (z[f"comp_{i}_{skip_tag(s)}"].astype(np.int32), z[f"label_{i}_{skip_tag(s)}"]) for s in SKIPS}})
    return _fixture


def sizes():
    out = []
    for c in fixture():
        if (c["H"], c["W"]) not in out:
            out.append((c["H"], c["W"]))
    return out


_generated = {}


def generated_cases(H, W):
    """Cases of a size the fixture does not hold, in its format: 3- and 10-colour noise, a two-colour checkerboard (H * W one-cell
    components), one colour all over, a grid_dim smaller than H x W with arbitrary bytes outside it.  `want` holds components_numpy's
    descriptors (the reference of every comparison here, pinned on the fixture by tests/test_components_host.py), no label plane."""
    if (H, W) not in _generated:
        rng = np.random.default_rng(5000 + 131 * H + W)
        out = []

        def want(g, dim, skip):
            n, _, comp, _ = S.components_numpy(g, dim, 1024, skip)
            return comp[:n].astype(np.int32)

        def add(name, g, dim=(H, W)):
            g, dim = np.asarray(g).astype(np.int8), np.asarray(dim, np.int8)
            out.append({"name": f"{H}x{W} gen {name}", "H": H, "W": W, "grid": g, "dim": dim,
                        "want": {s: (want(g, dim, s), None) for s in SKIPS}})
        add("noise3", rng.choice([0, 3, 5], (H, W)))
        add("noise10", rng.integers(0, 10, (H, W)))
        xx, yy = np.mgrid[0:H, 0:W]
        add("checker35", np.where((xx + yy) % 2 == 0, 3, 5))
        add("uniform3", np.full((H, W), 3))
        g = rng.integers(-128, 128, (H, W)).astype(np.int8)
        gh, gw = max(1, H - 2), max(1, W - 3)
        g[:gh, :gw] = rng.choice([0, 3, 5], (gh, gw))
        add(f"shrunk dim {gh}x{gw}", g, (gh, gw))
        _generated[(H, W)] = out
    return _generated[(H, W)]


def cases_of(H, W):
    """The fixture's cases of the size; generated ones for a size it does not hold (tests/strides.py)."""
    return [c for c in fixture() if (c["H"], c["W"]) == (H, W)] or generated_cases(H, W)


_mirror = {}


def mirror(case, C, skip):
    """components_numpy of a fixture case, computed once per (case, C, skip) and shared; masks come bit-packed [C, 128]."""
    key = (case["name"], C, skip)
    if key not in _mirror:
        n, left, comp, masks = S.components_numpy(case["grid"], case["dim"], C, skip)
        _mirror[key] = (n, left, comp, B.pack_bits(masks[:n]) if n else np.zeros((0, B.BITS_STRIDE), np.uint8))
    return _mirror[key]


def make_rows(kind, cases, rng):
    """State rows of env kind `kind` whose grid / grid_dim are the cases'; every other byte random (an offset off by one shows)."""
    H, W = cases[0]["H"], cases[0]["W"]
    lay = B.row_layout(kind, H * W)
    L = sum(ln for _, ln in lay)
    rows = rng.integers(-128, 128, (len(cases), L)).astype(np.int8)
    off = 0
    for f, ln in lay:
        if f == "grid":
            rows[:, off:off + ln] = np.stack([c["grid"].reshape(-1) for c in cases])
        elif f == "grid_dim":
            rows[:, off:off + ln] = np.stack([c["dim"] for c in cases])
        off += ln
    return rows


def place(rows, layout):
    """-> (buffer, byte offset, stride): the rows laid out as `layout` says; the last row ENDS the buffer."""
    M, L = rows.shape
    stride, offset = {"lib": ((L + 15) & ~15, 0), "dense": (L, 0), "odd": (L + 5, 3)}[layout]
    buf = np.full(offset + (M - 1) * stride + L, 0x55, np.int8)
    view = np.lib.stride_tricks.as_strided(buf[offset:], (M, L), (stride, 1))
    view[:] = rows
    return buf, offset, stride


class _CompParams(ctypes.Structure):  # mirror of arcle::CompParams (arcle_amd/csrc/arcle_components.h)
    _fields_ = [("p", B._StepParams), ("max_comp", ctypes.c_int32), ("skip_color", ctypes.c_int32), ("count", ctypes.c_void_p),
                ("comp", ctypes.c_void_p), ("bits", ctypes.c_void_p)]


_emu = None


def emu_lib():
    global _emu
    if _emu is None:
        so = os.path.join(EMU_DIR, "libcomponents_emu.so")
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [EMU_SRC] + EMU_HDRS):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-Wno-unknown-pragmas", "-o", so, EMU_SRC])
        _emu = ctypes.CDLL(so)
        _emu.components_emu_run.argtypes = [ctypes.POINTER(_CompParams), ctypes.c_int]
        assert _emu.components_emu_params_size() == ctypes.sizeof(_CompParams), "CompParams layout drifted"
    return _emu


def _outputs(M, C, bits):
    return (np.full((M, 2), SENTINEL, np.int32), np.full((M, C, 8), SENTINEL, np.int32),
            np.full((M, C, B.BITS_STRIDE), SENTINEL, np.uint8) if bits else None)


class EmuComponents:
    """The emulated kernel.  fw: -1 = the instantiation the library launches for the width, 0 = FW_GENERIC at any width."""
    BACKEND = B.EmuBackend  # (tests/strides.py: a subclass of another plane stride)
    name = "emu"

    def __init__(self, fw=-1):
        self.fw = fw

    def _run(self, be, M, C, skip, bits, rows_ptr, stride):
        x = _CompParams()
        p = be._params()
        p.n_resident, p.n_envs = be.N, M
        p.rows_in, p.rows_in_stride = rows_ptr, stride
        x.p = p
        out = _outputs(M, C, bits)
        x.max_comp, x.skip_color = C, skip
        x.count, x.comp, x.bits = out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data if bits else None
        rc = emu_lib().components_emu_run(ctypes.byref(x), self.fw)
        assert rc == 0, f"components emulator reported error {rc} (divergent cross-lane op / non-uniform value)"
        return out

    def rows(self, kind, H, W, rows, layout, C, skip, bits):
        be = self.BACKEND(2, H, W, 3, kind, OPS[kind]())
        buf, offset, stride = place(rows, layout)
        return self._run(be, rows.shape[0], C, skip, bits, buf.ctypes.data + offset, stride)

    def resident(self, kind, H, W, rows, cases, C, skip, bits):
        M = len(cases)
        be = self.BACKEND(M, H, W, 3, kind, OPS[kind]())
        for k in be.buf:
            be.buf[k][:] = 0x55
        be.rec[:] = 0x55
        be.buf["grid"][:, :H * W] = np.stack([c["grid"].reshape(-1) for c in cases])
        be.rec[:, 2:4] = np.stack([c["dim"] for c in cases])
        return self._run(be, M, C, skip, bits, None, 0)


class HipComponents:
    """EnvBatch.components_rows on the device."""
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
            self._b[key].set_op_table(OPS[kind]())
        return self._b[key]

    def _out(self, b, M, C, bits):
        t = self.t
        return (t.full((M, 2), SENTINEL, dtype=t.int32, device=b.device), t.full((M, C, 8), SENTINEL, dtype=t.int32, device=b.device),
                t.full((M, C, B.BITS_STRIDE), SENTINEL, dtype=t.uint8, device=b.device) if bits else None)

    def _np(self, out):
        return tuple(None if o is None else o.cpu().numpy() for o in out)

    def rows(self, kind, H, W, rows, layout, C, skip, bits):
        t = self.t
        b = self.batch(kind, H, W, 2)
        buf, offset, stride = place(rows, layout)
        M, L = rows.shape
        dbuf = t.as_tensor(buf, device=b.device)  # (exactly the bytes of the rows: the last row ends the allocation)
        view = t.as_strided(dbuf, (M, L), (stride, 1), offset)
        return self._np(b.components_rows(view, C, skip, bits, out=self._out(b, M, C, bits)))

    def resident(self, kind, H, W, rows, cases, C, skip, bits):
        t = self.t
        M = len(cases)
        b = self.batch(kind, H, W, M)
        b.set_state_rows(t.as_tensor(rows, device=b.device))
        return self._np(b.components_rows(None, C, skip, bits, out=self._out(b, M, C, bits)))


def compare(tag, got, cases, C, skip, bits):
    count, comp, mb = got
    errs = []
    for m, c in enumerate(cases):
        n, left, wc, wb = mirror(c, C, skip)
        t = f"{tag} row {m} ({c['name']})"
        if (int(count[m, 0]), int(count[m, 1])) != (n, left):
            errs.append(f"{t}: (written, left) {count[m].tolist()} != {(n, left)}")
            continue
        if not np.array_equal(comp[m, :n], wc[:n]):
            k = int(np.argwhere((comp[m, :n] != wc[:n]).any(1))[0])
            errs.append(f"{t}: component {k} {comp[m, k].tolist()} != {wc[k].tolist()}")
        if (comp[m, n:] != SENTINEL).any():
            errs.append(f"{t}: an entry >= written was written")
        if bits:
            if not np.array_equal(mb[m, :n], wb):
                errs.append(f"{t}: bit masks differ (first: component {int(np.argwhere((mb[m, :n] != wb).any(1))[0])})")
            if (mb[m, n:] != SENTINEL).any():
                errs.append(f"{t}: a bit mask >= written was written")
    return errs


def pad_to(cases, M):
    return [cases[i % len(cases)] for i in range(M)]


# (size) -> the runs of one backend: (kind, C, skip, layout | "resident", bits, M).  Every env kind (the grid offset differs), every
# C, every skip colour, every layout, M = 1 and M = 37, the resident form and bits appear at every size that has another code path;
# the 30 x 30 batch takes the whole C x skip product.  M = None: one row per fixture case of the size; "small": of those, the cases
# of at most 150 components (the emulator's time goes with the number of components: the long lists run once per size).
def plan(H, W):
    if (H, W) == (30, 30):
        runs = [("o2arc", C, s, "lib", C == 32, 37) for C in (1, 5, 32) for s in SKIPS]
        runs += [("o2arc", 1024, s, "lib", False, None if s < 0 else "small") for s in SKIPS]
        runs += [("arc", 32, -1, "dense", True, None), ("raw", 5, 0, "odd", True, None), ("o2arc", 32, 0, "resident", True, None),
                 ("raw", 1024, -1, "odd", True, 1)]
        return runs
    return [("o2arc", 1024, -1, "odd", True, None), ("arc", 32, 0, "dense", True, None), ("raw", 5, 3, "lib", False, 1),
            ("raw", 1, -1, "resident", True, None), ("arc", 1024, 0, "resident", False, "small"), ("o2arc", 5, 3, "lib", True, 37)]


def run_size(be, H, W, runs=None):
    errs = []
    rng = np.random.default_rng(H * 1000 + W)
    for kind, C, skip, layout, bits, M in (runs or plan(H, W)):
        cases = cases_of(H, W)
        if M == "small":
            cases = [c for c in cases if len(c["want"][-1][0]) <= 150]
        elif M is not None:
            cases = pad_to(cases, M) if M > 1 else cases[3:4] if len(cases) > 3 else cases[:1]
        rows = make_rows(kind, cases, rng)
        tag = f"{be.name} {H}x{W} {kind} C={C} skip={skip} {layout}"
        if layout == "resident":
            got = be.resident(kind, H, W, rows, cases, C, skip, bits)
        else:
            got = be.rows(kind, H, W, rows, layout, C, skip, bits)
        errs += compare(tag, got, cases, C, skip, bits)
        if len(errs) > 10:
            break
    return errs


# ---- planted object tasks: two objects, FloodFill of one and a Move of the other --------------------------------------------------
FLOODFILL_OPS, MOVE_OPS = list(range(10, 20)), list(range(20, 24))  # O2ARCv2Env's table: FloodFill0-9, MoveU / D / R / L


def clean_rows(kind, grids, dims, answers=None, adims=None, mt=3):
    """The state rows of freshly reset envs whose input — and so grid — are `grids` [n, H, W] / `dims` [n, 2].  -> (rows, oracle)"""
    n, H, W = grids.shape
    orc = B.OracleBackend(n, H, W, mt, kind, OPS[kind]())
    orc.set_tasks(grids, dims, grids if answers is None else answers, dims if adims is None else adims)
    orc.reset()
    return B.state_rows(orc), orc


def planted_object_tasks(n=16, H=12, W=12, seed=11):
    """n tasks on H x W: two single-coloured connected objects on background 0 whose boxes do not touch (not even diagonally) and
    keep one cell off the border; the answer, made by the ORACLE: FloodFill of the first object (in row-major order of the seeds)
    to a colour neither has, at its seed, then one Move of the other object's box.  -> (inputs [n, H, W], dims [n, 2], answers,
    the planted sequences as 5-tuples (x1, y1, x2, y2, op))."""
    rng = np.random.default_rng(seed)
    ops = O.o2arc_ops()
    inputs, answers, seqs = [], [], []
    while len(inputs) < n:
        g = np.zeros((H, W), np.int8)
        boxes = []
        for _ in range(2):
            h, w = rng.integers(2, 4, 2)
            x, y = rng.integers(2, H - 2 - h), rng.integers(2, W - 2 - w)
            boxes.append((x, y, x + h - 1, y + w - 1))
        (a0, b0, a1, b1), (c0, d0, c1, d1) = boxes
        if not (a1 + 2 < c0 or c1 + 2 < a0 or b1 + 2 < d0 or d1 + 2 < b0):
            continue
        cols = rng.permutation(np.arange(1, 10))[:3]
        for (x0, y0, x1, y1), col in zip(boxes, cols[:2]):
            g[x0:x1 + 1, y0:y1 + 1] = col
            if rng.integers(0, 2):
                g[x1, y1] = 0  # an L / a notched rectangle: still one component with the same box
        cnt, left, comp, _ = S.components_numpy(g, (H, W), 4, 0)
        assert cnt == 2 and left == 0
        fill = (int(comp[0, 4]), int(comp[0, 5]), int(comp[0, 4]), int(comp[0, 5]), 10 + int(cols[2]))
        move = (int(comp[1, 0]), int(comp[1, 1]), int(comp[1, 2]), int(comp[1, 3]), int(rng.integers(20, 24)))
        dims = np.array([[H, W]], np.int8)
        orc = B.OracleBackend(1, H, W, 3, "o2arc", ops)
        orc.set_tasks(g[None], dims, g[None], dims)
        orc.reset()
        for act in (fill, move):
            orc.step("bbox", np.array([act[:4]], np.int32), np.array([act[4]], np.int32))
        ans = orc.get("grid")[0]
        if orc.status() or (ans == g).all():
            continue
        inputs.append(g)
        answers.append(ans)
        seqs.append([fill, move])
    dims = np.tile(np.array([[H, W]], np.int8), (n, 1))
    return np.stack(inputs), dims, np.stack(answers), seqs


# ---- one dumped case for the standalone sanitized emulator ------------------------------------------------------------------------
def dump_case(path, kind, H, W, cases, C, skip, bits, layout, rng):
    """Writes one case in the format components_emu.cpp's main() reads: buffers exactly as long as the data."""
    P, PS = H * W, (H * W + 127) & ~127
    mask = sum(1 << i for i, k in enumerate(B.PLANES[:-1]) if k in O.KIND_PLANES[kind])
    M = len(cases)
    rows = make_rows(kind, cases, rng)
    with open(path, "wb") as f:
        if layout == "resident":
            f.write(np.array([0x434f4d50, H, W, mask, M, M, 0, C, skip, int(bits), 1, 0], np.int32).tobytes())
            grid = np.full((M, PS), 0x55, np.int8)
            grid[:, :P] = np.stack([c["grid"].reshape(-1) for c in cases])
            rec = np.full((M, 16), 0x55, np.int8)
            rec[:, 2:4] = np.stack([c["dim"] for c in cases])
            f.write(grid.tobytes())
            f.write(rec.tobytes())
        else:
            buf, offset, stride = place(rows, layout)
            f.write(np.array([0x434f4d50, H, W, mask, 2, M, stride, C, skip, int(bits), 0, offset], np.int32).tobytes())
            f.write(buf.tobytes())


def parse_dump(text, M, C, bits):
    """The standalone program's output -> (count, comp, bits) with SENTINEL where nothing was printed."""
    out = _outputs(M, C, bits)
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
            if bits:
                out[2][m, k] = np.frombuffer(bytes.fromhex(parts[8]), np.uint8)
    return out
