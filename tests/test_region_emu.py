"""The region kernel's body (arcle_amd/csrc/arcle_region.h) on the CPU wave emulator against arcle_amd.search.region_numpy — which
tests/test_region_host.py pins on the oracle's own Color step — and the sanitized standalone build of the emulator."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import backends as B
import regions as RG
from arcle_amd import search as S

K = {name: getattr(S, "REGION_" + name) for name in ("HALO4", "HALO8", "BOX_REST", "BOX_FRAME", "INSIDE", "BOX", "SELF")}
ALL = (1, 2, 3, 4, 5, 6, 7)


@pytest.mark.parametrize("H,W", RG.SIZES)
def test_emulated_kernel_equals_the_mirror(H, W):
    """Per size: the cases of tests/ray.py (those of tests/place.py and the rays' own) and the regions' own (objects in the corners and
    on the edges of a grid_dim below the plane, bits outside grid_dim, the four corners and both outer columns of the full plane, a
    hollow rectangle, a diagonal ring, an open U, two holes, a hole holding an object, the spiral and its shut twin, the whole-grid
    object, an empty bit row), in state rows of all three env kinds and the resident form; M = 1 and 37; C in {1, 5, 16}; the seven
    default kinds, 16 kinds with zeros, repeats and a code above 7, and one kind; through 0 and 1; free_color 0, 5 and -1; count,
    src_env (with a row that names no env), base and best_bits given and NULL; every word of region, best, best_bits and base exact,
    entries >= count and the bytes around every output untouched."""
    errs = RG.run_size(RG.EmuRegion(), H, W)
    assert not errs, "\n".join(errs[:10])


def test_plan_covers_every_axis():
    for H, W in RG.SIZES:
        runs = RG.plan(H, W)
        assert {r[0] for r in runs} == {"o2arc", "arc", "raw"} and {r[1] for r in runs} == {"lib", "dense", "odd", "resident"}
        assert {1, 37} <= {r[2] for r in runs} and {r[3] for r in runs} == set(RG.CS) == {1, 5, 16} and {r[4] for r in runs} == set(RG.KIND_LISTS)
        assert {r[5] for r in runs} == {0, 5, -1} and all({r[i] for r in runs} == {True, False} for i in (6, 7, 8, 9, 10))
        names = " ".join(c["name"] for c in RG.cases_of(H, W))
        assert "moved" in names and "shrunk a" in names and "bytes" in names and "lines" in names
        assert all(n in names for n in RG.NAMES) and (("spiral shut" in names) == (H >= 7 and W >= 7))
    assert RG.SIZES == ((5, 5), (7, 6), (6, 9), (12, 12), (20, 7), (30, 30), (32, 32), (64, 16), (16, 33), (65, 15))
    assert len(RG.KINDS16) == 16 and 0 in RG.KINDS16 and max(RG.KINDS16) > 7 and len(set(RG.KINDS16)) < 16 and RG.DEFAULT == ALL and len(RG.KIND_LISTS["one"]) == 1
    assert {(H > 64, W > 32) for H, W in RG.SIZES} == {(False, False), (True, False), (False, True)}  # row board, both flat-board reasons


def _one(case, through=False, free_color=0):
    """-> cells bool [n, 7, H, W] of the seven kinds and region [n, 7, 4] of a case under the mirror"""
    reg, best, base, cells = S.region_numpy(case["grid"], case["dim"], case["answer"], case["adim"], case["masks"], ALL, free_color, through, full=True)
    return cells, reg, best, base


@pytest.mark.parametrize("H,W", RG.SIZES)
def test_the_added_cases_are_what_they_claim(H, W):
    by = {c["name"].split(" ", 1)[1]: c for c in RG.cases_of(H, W)}
    i = {k: ALL.index(v) for k, v in K.items()}
    # edges: nothing leaks outside grid_dim, corner and edge objects have cut halos and frames, bits beyond grid_dim count for nothing
    c = by["edges"]
    gh, gw = (int(v) for v in c["dim"])
    assert (gh, gw) == (H - 1, W - 1)
    cells, reg, _, _ = _one(c, through=True)
    assert not cells[:, :, gh:].any() and not cells[:, :, :, gw:].any()
    assert [int(cells[0, i[k]].sum()) for k in ("HALO4", "HALO8", "BOX_FRAME", "BOX", "SELF")] == [2, 3, 3, 1, 1]  # the corner (0, 0)
    assert int(cells[1, i["HALO8"]].sum()) == 3 and all(int(cells[k, i["HALO8"]].sum()) == 5 and int(cells[k, i["HALO4"]].sum()) == 3 for k in (2, 3, 4, 5))
    assert c["masks"][6][H - 1].all() and c["masks"][6][:, W - 1].all() and int(cells[6, i["SELF"]].sum()) == 1 and int(cells[6, i["HALO8"]].sum()) == 8
    # full: column 0 and column W - 1, bit W - 1 and lane H - 1: no halo cell in the opposite column of a neighbouring row
    c = by["full"]
    cells, _, _, _ = _one(c, through=True)
    assert c["masks"][1][0, W - 1] and c["masks"][3][H - 1, W - 1] and c["masks"][4][2:H - 2, 0].all() and c["masks"][5][2:H - 2, W - 1].all()
    for k, col in ((0, 0), (2, 0), (4, 0), (1, W - 1), (3, W - 1), (5, W - 1)):
        far = W - 1 - col
        assert not cells[k, :, :, far].any() if W > 2 else True
        assert cells[k, i["HALO8"]][:, 1 if col == 0 else W - 2].any()
    assert int(cells[3, i["HALO8"]].sum()) == 3 and int(cells[1, i["HALO4"]].sum()) == 2
    # hollow / diamond: the hole(s) are inside; ushape: nothing is; twoholes: both
    cells, reg, best, base = _one(by["hollow"])
    assert np.argwhere(cells[0, i["INSIDE"]]).tolist() == [[2, 2]] and np.array_equal(cells[0, i["BOX_REST"]], cells[0, i["INSIDE"]])
    assert best[0].tolist() == [i["BOX_REST"], 4, base[0] + 1, 1]  # (equal with INSIDE: the lower index)
    cells, reg, best, base = _one(by["diamond"])
    assert sorted(np.argwhere(cells[0, i["INSIDE"]]).tolist()) == [[1, 2], [2, 1], [2, 2], [2, 3], [3, 2]] and reg[0, i["INSIDE"]].tolist() == [3, base[0] + 5, 5, 5]
    cells, _, _, _ = _one(by["ushape"])
    assert not cells[0, i["INSIDE"]].any() and cells[0, i["BOX_REST"]][0:2, 2].all() and int(cells[0, i["BOX_REST"]].sum()) == 2
    cells, reg, _, base = _one(by["twoholes"])
    assert np.argwhere(cells[0, i["INSIDE"]]).tolist() == [[2, 1], [2, 3]] and reg[0, i["INSIDE"]].tolist() == [8, base[0] + 2, 2, 2]
    # nested: the hole's object is covered under through = 1 and spared under through = 0
    c0, r0, _, base = _one(by["nested"], through=False)
    c1, r1, _, _ = _one(by["nested"], through=True)
    assert int(c1[0, i["INSIDE"]].sum()) == 9 and c1[0, i["INSIDE"]][2, 2] and int(c0[0, i["INSIDE"]].sum()) == 8 and not c0[0, i["INSIDE"]][2, 2]
    assert r1[0, i["INSIDE"]].tolist() == [4, base[0] + 9, 9, 9] and r0[0, i["INSIDE"]].tolist() == [4, base[0] + 8, 8, 8]
    # the spiral: its corridor reaches the edge — nothing inside — and is all inside once (1, 0) is shut
    if H >= 7 and W >= 7:
        cells, _, _, _ = _one(by["spiral"])
        wall = by["spiral"]["masks"][0] != 0
        assert not cells[0, i["INSIDE"]].any() and not wall[1, 0] and int((~wall).sum()) > (H * W) // 3
        assert S.components_numpy(np.where(wall, 0, 1), (H, W), 4, 0)[:2] == (1, 0)  # one corridor
        cells, _, _, _ = _one(by["spiral shut"])
        assert np.array_equal(cells[0, i["INSIDE"]], by["spiral shut"]["masks"][0] == 0)
    # whole: the box is the whole grid, the frame is empty, every count is H * W; the empty bit row gives nothing
    cells, reg, best, base = _one(by["whole"], through=True)
    assert base[0] == H * W and not cells[0, i["BOX_FRAME"]].any() and not cells[0, i["HALO8"]].any() and not cells[0, i["INSIDE"]].any()
    assert reg[0, i["BOX"]].tolist() == reg[0, i["SELF"]].tolist() == [3, H * W, H * W, H * W] and best[0].tolist() == [i["BOX"], 3, H * W, H * W]
    assert not cells[1].any() and best[1].tolist() == [-1, 0, H * W, 0]
    if (H, W) == (32, 32):
        assert reg[0, i["BOX"], 2] == 1024


def test_params_mirror():
    assert RG.emu_lib().region_emu_params_size() == ctypes.sizeof(RG._RegionParams) == ctypes.sizeof(B._StepParams) + 80


def test_generic_instantiation_at_fast_widths():
    """FW_GENERIC serves any width: at 30 x 30, 32 x 32 and 64 x 16 (where the library launches FW_FAST) it gives the same answers."""
    for (H, W), through in (((30, 30), False), ((32, 32), True), ((64, 16), True)):
        errs = RG.run_size(RG.EmuRegion(fw=0), H, W, runs=[("arc", "odd", None, 16, "default", 0, through, True, True, True, True)])
        assert not errs, "\n".join(errs[:10])


def test_a_caller_chosen_plane_stride():
    """7 x 12 at plane stride 96 (FW_GENERIC, six live lanes, 12 padding bytes of garbage): the plan's answers, and the slack behind every
    plane untouched."""
    import strides as STR
    inst, check = STR.family_with_stride(RG.EmuRegion, 96)
    errs = RG.run_size(inst, 7, 12) + check()
    assert not errs, "\n".join(errs[:10])


def test_sanitized_standalone_emulator():
    """region_emu.cpp as a program of its own under ASan + UBSan (host code only; nothing is loaded into Python), buffers exactly as
    long as the data: the row board under the fast width (30 x 30 and 32 x 32), under the generic width with a plane stride below 1024
    bytes (20 x 7) and the flat board (16 x 33 and 65 x 15), rows and resident, both `through` values, the last row / env / bit row /
    kind ending its buffer."""
    cxx = shutil.which("g++")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "region_emu")
        probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-x", "c++", "-o", os.path.join(d, "probe"), "-"],
                               input=b"int main(){return 0;}", capture_output=True) if cxx else None
        # (no skip: this is the only ASan / UBSan run of the kernel body, so a toolchain without the runtime is a failure to see)
        assert probe is not None and probe.returncode == 0, "g++ with -fsanitize=address,undefined is needed: " + (probe.stderr.decode()[-500:] if probe else "no g++")
        subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-DREGION_EMU_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-Wno-unknown-pragmas", "-o", exe, RG.EMU_SRC])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:use_sigaltstack=0", UBSAN_OPTIONS="halt_on_error=1")
        rng = np.random.default_rng(5)
        for (H, W), kind, layout, C, kindname, fc, through, with_count, with_src, with_bits in (
                ((30, 30), "o2arc", "dense", 16, "default", 0, False, True, True, True), ((32, 32), "arc", "lib", 5, "default", 0, True, True, False, True),
                ((20, 7), "raw", "odd", 5, "sixteen", 0, True, False, False, True), ((20, 7), "arc", "resident", 16, "one", 5, False, True, True, False),
                ((16, 33), "o2arc", "lib", 5, "sixteen", 0, False, True, False, True), ((65, 15), "arc", "resident", 3, "default", 0, True, False, True, True)):
            cases = RG.cases_of(H, W)
            cases = cases[1:4] + [c for c in cases if c["name"].split(" ", 1)[1] in RG.NAMES + ("spiral", "spiral shut", "dense")]
            kinds = RG.KIND_LISTS[kindname]
            case = os.path.join(d, "case.bin")
            bad = RG.dump_case(case, kind, H, W, cases, layout, C, kinds, fc, through, with_count, with_src, True, with_bits, rng)
            run = subprocess.run([exe, case], capture_output=True, text=True, env=env, timeout=600)
            assert run.returncode == 0, run.stderr[-2000:]
            reg, best, bbits, base = RG.parse_dump(run.stdout, cases, C, len(kinds), with_count, True, with_bits)
            errs = RG.compare(f"sanitized {H}x{W} {kind} {layout}", (reg, best, bbits, base, bad), cases, C, kinds, fc, through, with_count, True, with_bits)
            assert not errs, "\n".join(errs[:10])
