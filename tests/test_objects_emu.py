"""The objects kernel's body (arcle_amd/csrc/arcle_objects.h) on the CPU wave emulator against the union-find labelling of tests/objects.py
— which tests/test_objects_host.py pins on components_numpy and, in mode 0, on the reference's dfs — and the sanitized standalone build
of the emulator."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import components as CP
import objects as OB


@pytest.mark.parametrize("H,W", OB.SIZES)
def test_emulated_kernel_equals_the_mirror(H, W):
    """Per size, all four modes: the fixture's grids of the size and the generated ones (noise, checkerboard, diagonals, staircase,
    the W + 1 wrap pair, a shrunk grid_dim, arbitrary bytes) in state rows of all three env kinds; C in {1, 5, 1024}; skip_color in
    {-1, 0, 3}; the three row layouts and the resident form; M = 1 and 37; bits and colours; entries >= written untouched."""
    errs = OB.run_size(OB.EmuObjects(), H, W)
    assert not errs, "\n".join(errs[:10])


def test_params_mirror_and_the_old_struct():
    """ObjParams is CompParams + one pointer; CompParams is what the components emulator says it is."""
    assert OB.emu_lib().objects_emu_params_size() == ctypes.sizeof(OB._ObjParams) == ctypes.sizeof(CP._CompParams) + 8
    assert CP.emu_lib().components_emu_params_size() == ctypes.sizeof(CP._CompParams)


def test_mode_0_is_the_components_kernel_output_for_output():
    """wave_objects_row<FW, 0> against wave_components_row<FW> on the same rows: count, comp and bits byte for byte."""
    for (H, W), kind, layout in (((30, 30), "o2arc", "odd"), ((20, 7), "arc", "dense"), ((16, 33), "raw", "lib")):
        cases = OB.small(OB.cases_of(H, W), 0, 0)
        rows = CP.make_rows(kind, cases, np.random.default_rng(3))
        for C in (5, 1024):
            old = CP.EmuComponents().rows(kind, H, W, rows, layout, C, 0, True)
            new = OB.EmuObjects().rows(kind, H, W, rows, layout, C, 0, 0, True, True)
            assert all(np.array_equal(a, b) for a, b in zip(old, new[:3])), (H, W, C)


def test_generic_instantiation_at_fast_widths():
    """FW_GENERIC serves any width: at 30 x 30 and 64 x 16 (where the library launches FW_FAST) it gives the same lists in every mode."""
    for H, W in ((30, 30), (64, 16)):
        errs = OB.run_size(OB.EmuObjects(fw=0), H, W, runs=[("arc", 1024, 0, "odd", True, True, "small")])
        assert not errs, "\n".join(errs[:10])


def test_a_diagonal_never_wraps_on_the_flat_board():
    """Cells (r, W - 1) and (r + 2, 0) only, W + 1 apart in flat index: one-cell objects in every mode, at every flat-board size."""
    be = OB.EmuObjects()
    for H, W in ((3, 40), (16, 33), (8, 127)):
        case = [c for c in OB.cases_of(H, W) if c["name"].endswith("wrap2")]
        rows = CP.make_rows("o2arc", case, np.random.default_rng(0))
        for mode in OB.MODES:
            count, comp, _, _ = be.rows("o2arc", H, W, rows, "lib", 1024, 0, mode, False, False)
            n = int(count[0, 0])
            assert n == 2 * len(range(0, H - 2, 3)) and int(count[0, 1]) == 0 and (comp[0, :n, 7] == 1).all(), (H, W, mode)


def test_sanitized_standalone_emulator():
    """objects_emu.cpp as a program of its own under ASan + UBSan (host code only; nothing is loaded into Python), buffers exactly as
    long as the data: one case per board type and more — the row board under the fast width (30 x 30), under the generic width with a
    plane stride below 1024 bytes (5 x 5, 20 x 7) and the flat board (16 x 33), rows and resident, the last row / env ending its buffer."""
    cxx = shutil.which("g++")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "objects_emu")
        probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-x", "c++", "-o", os.path.join(d, "probe"), "-"],
                               input=b"int main(){return 0;}", capture_output=True) if cxx else None
        if probe is None or probe.returncode != 0:
            pytest.skip("g++ has no sanitizer runtime")
        subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-DOBJECTS_EMU_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-Wno-unknown-pragmas", "-o", exe, OB.EMU_SRC])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:use_sigaltstack=0", UBSAN_OPTIONS="halt_on_error=1")
        rng = np.random.default_rng(5)
        for (H, W), kind, layout, C, skip, mode in (((30, 30), "o2arc", "dense", 5, 0, 3), ((5, 5), "raw", "odd", 1024, -1, 2), ((5, 5), "arc", "resident", 5, 0, 1),
                                                    ((20, 7), "raw", "resident", 1024, 3, 3), ((16, 33), "o2arc", "lib", 1024, 0, 3),
                                                    ((16, 33), "arc", "resident", 5, -1, 0)):
            cases = OB.small(OB.cases_of(H, W), mode, skip) if C == 1024 else OB.cases_of(H, W)
            case = os.path.join(d, "case.bin")
            OB.dump_case(case, kind, H, W, cases, C, skip, mode, True, True, layout, rng)
            run = subprocess.run([exe, case], capture_output=True, text=True, env=env, timeout=600)
            assert run.returncode == 0, run.stderr[-2000:]
            got = OB.parse_dump(run.stdout, len(cases), C, True, True)
            errs = OB.compare(f"sanitized {H}x{W} {kind} {layout} mode {mode}", got, cases, C, skip, mode, True, True)
            assert not errs, "\n".join(errs[:10])
