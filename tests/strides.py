"""Caller-chosen plane strides (arcle_config.plane_stride, EnvBatch(plane_stride=), ARCLE_PLANE_STRIDE).  Test infrastructure only.

The default stride rounds H * W up to 128, so every other test sees plane rows that are whole cache lines, chunk counts that are
multiples of 8, bit rows that are 16-byte aligned, and padding behind the last cell that belongs to the same env.  The cases here
take the strides the ABI also accepts — any multiple of 16 with H * W <= PS <= 1024, or up to MAX_PS on a handle of more than 1024
cells — through the drivers the suite already has: `with_stride(backend_cls, ps)` gives a backend class of that stride, `run(driver,
backend_cls, ps, ...)` calls a driver with it and then checks the two invariants on EVERY backend the driver made:

  padding   bytes [H * W, PS) of every env's row of every plane are zero (the header's contract; set_state_rows and reset rely on it)
  slack     the PLANE_SLACK bytes behind every plane, filled with 0x55 when the backend is made, are unchanged: a lane at or above
            PS / 16 of the LAST env that stores anyway lands there and nowhere else (in an inner env the same mistake races with the
            neighbour's own store and can be invisible to parity)

No comparison code lives here: every comparison is the drivers' own, bit for bit against the oracle."""
import numpy as np

import backends as B
import bigcases as C
import deepstate as D
import research_model as M
import rows as R
from oracle import oracle as O

# (H, W, PS, what the stride exercises)
SMALL = (
    (30, 30, 912, "FW_FAST; 57 live lanes; the last lane holds 4 cells + 12 pad bytes; rows never line-aligned"),
    (12, 20, 240, "PS == P; 15 lanes; no padding at all"),
    (12, 20, 272, "one live lane that is all padding"),
    (12, 20, 1024, "FW_FULL with 240 cells; 49 live lanes of pure padding"),
    (7, 12, 96, "FW_GENERIC; 6 lanes"),
    (2, 100, 208, "FW_GENERIC; W > 32"),
    (5, 5, 32, "two lanes"),
    (1, 1, 16, "a single live lane"),
)
BIG = (
    (40, 40, 1600, "PS == P; 100 chunks; bit rows of 200 bytes"),
    (40, 40, 1616, "101 chunks (odd); bit rows of 202 bytes, 2-byte aligned only"),
    (33, 100, 3312, "207 chunks, odd, two per thread"),
    (100, 12, 1200, "the generic big kernel (W < 16); 75 chunks"),
    (100, 20, 2000, "the lean path with one chunk per thread by shape; 125 chunks on 128 threads"),
    (127, 127, 16144, "1009 chunks; 16 envs"),
)
CASES = SMALL + BIG
FLAG_SETS = D.FLAG_SETS  # 0 and AUTORESET | ELIDE_SELECTED
STEP_FORMS = ("mask", "bits", "bbox", "bbox5", "point")


def case_id(c):
    return f"{c[0]}x{c[1]}-ps{c[2]}"


def is_big(H, W):
    return H * W > 1024


def counts(H, W):
    """(envs, steps) of the existing deepstate case of the shape's class."""
    return (16, 48) if (H, W) == (127, 127) else (32, 48) if is_big(H, W) else (64, 64)


def step_case(H, W, flags, form):
    """The deepstate.Case whose stream is sent in ingress form `form`."""
    N, S = counts(H, W)
    return D.Case({"mask": "chain", "bits": "chain", "bbox5": "bbox"}.get(form, form), H, W, "o2arc", flags, N, S)


# ---- backends of a stride -------------------------------------------------------------------------------------------------------
def with_stride(backend_cls, ps):
    """`backend_cls` with PLANE_STRIDE = ps.  Every instance fills the slack behind its planes when it is made and is kept in the
    class's `made` list until `invariants` has looked at it."""
    class Strided(backend_cls):
        PLANE_STRIDE = ps
        made = []

        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            assert self.PS == ps, f"the backend runs at plane stride {self.PS}, not {ps}"
            self.fill_slack()
            type(self).made.append(self)

    Strided.__name__ = Strided.__qualname__ = f"{backend_cls.__name__}_ps{ps}"
    return Strided


def padding(be):
    """Bytes [H * W, PS) of every env's row of every plane are zero -> mismatch strings."""
    return [] if be.padding_is_zero() else [f"{type(be).__name__} {be.H}x{be.W}: plane padding bytes [{be.H * be.W}, {be.PS}) are not zero"]


def slack(be):
    """The PLANE_SLACK bytes behind every plane are as fill_slack() left them -> mismatch strings."""
    return [] if be.slack_intact() else [f"{type(be).__name__} {be.H}x{be.W}: the slack behind a plane was written (a store past the last env's row)"]


def invariants(cls):
    """Both invariants on every backend `cls` (of with_stride) has made since the last call."""
    made, errs = cls.made[:], []
    assert made, f"{cls.__name__}: the driver made no backend of this stride"
    del cls.made[:]
    for be in made:
        errs += padding(be) + slack(be)
    return errs


def run(driver, backend_cls, ps, *args, **kw):
    """driver(backend class of stride ps, *args, **kw) -> its mismatch strings (None: it asserts by itself) + the invariants'."""
    cls = with_stride(backend_cls, ps)
    errs = driver(cls, *args, **kw)
    return list(errs or []) + invariants(cls)


# ---- what every case runs (the drivers of the suite, unchanged) -------------------------------------------------------------------
def step(backend_cls, H, W, ps, flags, form):
    return run(D.compare, backend_cls, ps, step_case(H, W, flags, form), form)


def resets(backend_cls, H, W, ps):
    """reset, reset_from_table plain and masked (backends.task_table_compare), explicit and drawn augmentation (bigcases.aug_case)."""
    errs = run(B.task_table_compare, backend_cls, ps, H, W, 16, 7, H * 31 + W)
    return errs + run(C.aug_case, backend_cls, ps, sizes=((H, W),))


def state_rows(backend_cls, H, W, ps):
    """get_state_rows / set_state_rows round trip and arcle_pack_mask_bits."""
    errs = run(R.state_rows_roundtrip, backend_cls, ps, cases=(("o2arc", H, W),))
    return errs + run(R.mask_bits_packer, backend_cls, ps, sizes=((H, W),))


def transitions(backend_cls, H, W, ps):
    """arcle_transition_rows: rows.transition_rows on every handle, deepstate.rows_check where the shape has a ROWS case."""
    errs = run(R.transition_rows, backend_cls, ps, cases=(("o2arc", H, W, 3),))
    for case in D.ROWS_CASES:
        if (case.H, case.W) == (H, W):
            errs += run(D.rows_check, backend_cls, ps, case, forms=("mask",) if is_big(H, W) else ("mask", "bits"))
    return errs


def rollout(backend_cls, H, W, ps, T=24):
    """One rollout launch per tuple form and one of masks with every step's packed row (ARCLE_STEP_PACK_OBS)."""
    N, ops, errs = counts(H, W)[0], O.o2arc_ops(), []
    for ingress, flags, packed in (("bbox", 3, False), ("point", 0, False), ("mask", 3, True)):
        errs += run(B.rollout_compare, backend_cls, ps, "o2arc", ops, H, W, N, T, H * 7 + W, ingress=ingress, flags=flags, packed=packed)
    return errs


def research_case(H, W, stream):
    N, S = counts(H, W)
    return M.Case(stream, H, W, "resample", min(N, 32), 40)


def _research(cls, case, flags, rows, form):
    be = M.setup(cls, case, flags, rows)
    return M.compare(be, M.model_of(case, flags=flags), M.stream_of(case), flags, rows, form)


RESEARCH_FORMS = (("mask", "bits"), ("bbox", "bbox5"), ("point", "point"))  # (stream, the form it is sent in)


def research(backend_cls, H, W, ps, stream, form):
    """The research flag set — dense reward, truncation, resample with drawn augmentation, FilterO2ARC rows, incremental on the
    one-wavefront handles — against the episode model of tests/research_model.py; the point stream also writes packed rows."""
    flags = (M.RESEARCH if is_big(H, W) else M.RESEARCH_INC) | (M.PACK_OBS if stream == "point" else 0)
    return run(_research, backend_cls, ps, research_case(H, W, stream), flags, "filtered", form)


# ---- byte accounting: the closed form of tests/test_big_hip.py ----------------------------------------------------------------------
def accounting_form(H, W, PS, form, speculative=False):
    """(algorithmic, issued) bytes per env of CopyFromInput on a freshly reset (inactive) env under ELIDE_SELECTED: `issued` counts
    plane rows of PS bytes, `bytes` of H * W.
    One-wavefront handles (arcle_wave.h step_wave): two plane rows are issued — the input read, the grid written; the zero-fill of
    `selected` is elided — plus record in and out (2 x 16), counters (16), the action (20 bytes as a tuple, the H * W mask bytes, the
    128-byte bit row requested as 64 lanes x 2 bytes) and reward + terminated (5); a launch that requests the grid plane before it knows
    the op (`speculative`: arcle_launch_info names a stream policy) issued a third row, which CopyFromInput never uses.  The algorithmic figure is the op's semantic traffic,
    whatever is elided (tests/test_round3_hip.py test_kernel_counted_bytes: the same with and without the elision): three planes of
    H * W — input read, grid and `selected` written — plus record in and out and 24 bytes of action and outputs, plus a mask's H * W
    bytes or the ceil(H * W / 8) bytes of its bits.
    Workgroup-per-env handles (arcle_big.h step_body): every 16-byte access is counted: the PS / 16 chunks of the two planes and, with
    a mask or a bit row, one access per plane chunk (its 16 mask bytes, or its 2 bytes of the bit row, counted as a chunk); the scalars
    are 2 x 16 + 16 + 20 + 5 whatever the form; the algorithmic figure scales the chunks by H * W / PS."""
    P = H * W
    if is_big(H, W):
        chunks = (2 if form == "bbox" else 3) * (PS // 16)
        scal = 2 * 16 + 16 + 20 + 5
        return chunks * 16 * P // PS + scal, chunks * 16 + scal
    act = {"bbox": 20, "mask": P, "bits": 128}[form]
    return 3 * P + 2 * 16 + 24 + {"bbox": 0, "mask": P, "bits": (P + 7) // 8}[form], (3 if speculative else 2) * PS + 2 * 16 + 16 + act + 5


def _accounting(cls, H, W, form):
    N = 64
    be = cls(N, H, W, 3, "o2arc", O.o2arc_ops())
    inp = np.random.default_rng(0).integers(0, 10, (N, H, W)).astype(np.int8)
    dims = np.tile(np.array([[H, W]], np.int8), (N, 1))
    be.set_tasks(inp, dims, inp, dims)
    be.reset()
    be.start_accounting()
    op = np.full(N, 31, np.int32)
    pay = {"bbox": np.zeros((N, 4), np.int32), "mask": np.zeros((N, H, W), np.int8), "bits": np.zeros((N, be.bits_stride), np.uint8)}[form]
    be.step(form, pay, op, B.STEP_ELIDE_SELECTED)
    # which launches request the grid before they know the op (arcle_hip.hip plan_launch, policy 'A'): batches of at most
    # ARCLE_SPEC_SMALL_MAX envs — 64 here — on a one-wavefront handle that is not 30 x 30 at 1024 — none of the cases is — with tuples
    # or bit rows, never int8 masks; the emulators run the body without the request.  arcle_launch_info must say the same.
    spec = be.name == "hip" and not is_big(H, W) and form != "mask"
    if hasattr(be, "speculates"):
        assert be.speculates(form, B.STEP_ELIDE_SELECTED) == spec, f"{H}x{W} stride {be.PS} {form}: arcle_launch_info reports another plan"
    got, want = be.accounting(), tuple(N * v for v in accounting_form(H, W, be.PS, form, spec))
    return [] if got == want else [f"{H}x{W} stride {be.PS} {form}: (bytes, issued) {got}, the closed form gives {want}"]


def accounting(backend_cls, H, W, ps):
    errs = []
    for form in ("bbox", "mask", "bits"):
        errs += run(_accounting, backend_cls, ps, H, W, form)
    return errs


def plane_copies(cls, H, W):
    """arcle_set_plane / arcle_get_plane on every plane: dense [N, H, W] <-> the strided plane (hipMemcpy2D with the handle's pitch)."""
    import torch
    N = 9
    be = cls(N, H, W, 3, "o2arc", O.o2arc_ops())
    rng, errs = np.random.default_rng(H + W), []
    for name in be.b.planes:
        new = torch.from_numpy(rng.integers(0, 10, (N, H, W)).astype(np.int8))
        be.b.set_plane(name, new.cuda())
        if not torch.equal(be.b.get_plane(name).cpu(), new) or not np.array_equal(be.get(name), new.numpy()):
            errs.append(f"{H}x{W} stride {be.PS}: set_plane / get_plane of {name} do not round-trip")
    return errs


# ---- the search family (one-wavefront handles) --------------------------------------------------------------------------------------
def search_case(H, W):
    return ("o2arc", H, W, 3)


def expand_and_hash(backend_cls, H, W, ps):
    """arcle_expand_rows with tuples (search.expansion) and bit rows (search_bits.expansion), arcle_hash_rows at any row stride
    (search.hash_strides), transition_rows with bit rows (search_bits.transitions), parents with an active object
    (deepstate.expansion_check).  backend_cls: a bits backend (search_bits.EmuBitsBackend | HipBitsBackend)."""
    import search as SR
    import search_bits as SB
    cases = (search_case(H, W),)
    errs = run(SR.expansion, backend_cls, ps, cases=cases)
    errs += run(SR.hash_strides, backend_cls, ps, cases=cases)
    if H * W > 1:  # (a one-cell mask is its own filled bounding box: the share of other masks search_bits.expansion asserts on the oracle cannot be reached)
        errs += run(SB.expansion, backend_cls, ps, cases=cases)
    errs += run(SB.transitions, backend_cls, ps, cases=cases)
    return errs + run(D.expansion_check, backend_cls, ps, "o2arc", H, W, 3)


def macros(backend_cls, H, W, ps):
    """arcle_expand_macros in the three forms (macros.parity)."""
    import macros as MC
    return run(MC.parity, backend_cls, ps, cases=(search_case(H, W),))


def family_with_stride(cls, ps):
    """tests/components.py, objects.py and place.py: their Emu* class on a strided EmuBackend, their Hip* class with PLANE_STRIDE.
    -> (an instance, a function giving the invariants' mismatch strings of every backend the instance made).  The Emu* classes fill
    whole plane rows of their own backends with 0x55, padding included (garbage the kernels must not read): only the slack is
    checked there."""
    if hasattr(cls, "BACKEND"):
        be_cls = with_stride(cls.BACKEND, ps)
        inst = type(f"{cls.__name__}_ps{ps}", (cls,), {"BACKEND": be_cls})()

        def check():
            made = be_cls.made[:]
            assert made
            del be_cls.made[:]
            return [e for be in made for e in slack(be)]
        return inst, check

    class Strided(cls):
        PLANE_STRIDE = ps

        def batch(self, kind, H, W, N):
            new = (kind, H, W, N) not in self._b
            b = super().batch(kind, H, W, N)
            assert b.PS == ps
            if new:
                B.HipBatchView(b).fill_slack()
            return b

    inst = Strided()

    def check():
        assert inst._b
        return [e for b in inst._b.values() for e in padding(B.HipBatchView(b)) + slack(B.HipBatchView(b))]
    return inst, check


def objects_family(comp_cls, obj_cls, place_cls, H, W, ps):
    """arcle_components_rows, arcle_objects_rows and arcle_place_rows through run_size of their shared modules (components.py reads
    its fixture where that holds the size and generates its grids elsewhere; objects.py and place.py generate theirs for any size)."""
    import components as CP
    import objects as OB
    import place as PL
    errs = []
    for mod, cls in ((CP, comp_cls), (OB, obj_cls), (PL, place_cls)):
        inst, check = family_with_stride(cls, ps)
        errs += mod.run_size(inst, H, W) + check()
    return errs
