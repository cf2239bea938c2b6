"""The scale kernel's body (arcle_amd/csrc/arcle_scale.h) on the CPU wave emulator against arcle_amd.search.scale_numpy — which
tests/test_scale_host.py pins on the oracle's own resize_grid + Color macro — and the sanitized standalone build of the emulator."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import backends as B
import scales as SC


@pytest.mark.parametrize("H,W", SC.SIZES)
def test_emulated_kernel_equals_the_mirror(H, W):
    """Per size: unique perfect zooms, shrinks and tilings, an anisotropic zoom, sources that end before the canvas does, a 1 x 1 source,
    flat tiles under both mirror bits, ragged tilings, junk outside the source's dims, source and answer bytes outside 0..9, all-zero
    sources, dims of 0 and the ties, in state rows of all three env kinds and the resident form; M = 1 and 37; sources 1, 2 and 3; modes
    1 .. 7; src_env given (with a row that names no env) and NULL; every word of scale, table, bits and base exact; slots not asked for
    and the bytes around every output untouched."""
    errs = SC.run_size(SC.EmuScale(), H, W)
    assert not errs, "\n".join(errs[:10])


def test_plan_covers_every_axis():
    for H, W in SC.SIZES:
        runs = SC.plan(H, W)
        assert {r[0] for r in runs} == {"o2arc", "arc", "raw"} and {r[1] for r in runs} == {"lib", "dense", "odd", "resident"}
        assert {1, 37} <= {r[2] for r in runs} and {r[3] for r in runs} == {True, False} and {r[4] for r in runs} == {True, False}
        assert {r[5] for r in runs} == {1, 2, 3} and {r[6] for r in runs} == {1, 2, 3, 4, 5, 6, 7}
        assert {r[7] for r in runs} == {True, False} and {r[8] for r in runs} == {True, False}
        assert any(r[2] is None and r[5] == 3 and r[6] == 7 and r[7] and r[8] for r in runs)  # every case, everything asked for
        full = SC.plan(H, W, True)
        assert sum(r[2] is None and r[5] == 3 and r[6] == 7 for r in full) >= 2 and any(r[2] == 37 and r[6] == 7 for r in full)


def test_params_mirror():
    assert SC.emu_lib().scale_emu_params_size() == ctypes.sizeof(SC._ScaleParams) == ctypes.sizeof(B._StepParams) + 48


def test_generic_instantiation_at_fast_widths():
    """FW_GENERIC serves any width: at 30 x 30 (where the library launches FW_FAST) it gives the same answers."""
    errs = SC.run_size(SC.EmuScale(fw=0), 30, 30, runs=[("arc", "odd", None, True, True, 3, 7, True, True)])
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("H,W,ps", ((7, 12, 96), (20, 7, 240)))
def test_a_caller_chosen_plane_stride(H, W, ps):
    """7 x 12 at plane stride 96 (FW_GENERIC, six live lanes, 12 padding bytes of garbage) and 20 x 7 at 240: the plan's answers, and
    the slack behind every plane untouched."""
    import strides as STR
    inst, check = STR.family_with_stride(SC.EmuScale, ps)
    errs = SC.run_size(inst, H, W) + check()
    assert not errs, "\n".join(errs[:10])


def test_sanitized_standalone_emulator():
    """scale_emu.cpp as a program of its own under ASan + UBSan (host code only; nothing is loaded into Python), buffers exactly as long
    as the data: the row board under the fast width (30 x 30), under the generic width with a plane stride below 1024 bytes (20 x 7)
    and the flat board (16 x 33 and 3 x 40), rows and resident, both sources and single ones, every mode, with and without table and
    bits, the last row / env ending its buffer; the cases include the sources that end before the canvas, the 1 x 1 source (row indices
    up to 8 times the lane), the flat tiles and the dims of 0."""
    cxx = shutil.which("g++")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "scale_emu")
        probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-x", "c++", "-o", os.path.join(d, "probe"), "-"],
                               input=b"int main(){return 0;}", capture_output=True) if cxx else None
        if probe is None or probe.returncode != 0:
            pytest.skip("g++ has no sanitizer runtime")
        subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-DSCALE_EMU_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-Wno-unknown-pragmas", "-o", exe, SC.EMU_SRC])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:use_sigaltstack=0", UBSAN_OPTIONS="halt_on_error=1")
        rng = np.random.default_rng(5)
        for (H, W), kind, layout, with_src, sources, modes, with_table, with_bits in (
                ((30, 30), "o2arc", "dense", True, 3, 7, True, True), ((20, 7), "raw", "odd", False, 1, 3, False, True),
                ((20, 7), "arc", "resident", True, 3, 6, True, False), ((16, 33), "o2arc", "lib", False, 3, 7, True, True),
                ((3, 40), "arc", "resident", True, 2, 5, True, True)):
            cases = [c for c in SC.cases_of(H, W) if c["name"].endswith(("zoom short", "shrink past", "1x1 source", "tile flat row", "tile mirrored", "bad bytes",
                                                                         "zero dim a", "zero dim c"))]
            case = os.path.join(d, "case.bin")
            bad = SC.dump_case(case, kind, H, W, cases, layout, with_src, True, sources, modes, with_table, with_bits, rng)
            run = subprocess.run([exe, case], capture_output=True, text=True, env=env, timeout=600)
            assert run.returncode == 0, run.stderr[-2000:]
            scale, table, bits, base = SC.parse_dump(run.stdout, len(cases), True, with_table, with_bits)
            errs = SC.compare(f"sanitized {H}x{W} {kind} {layout}", (scale, table, bits, base, bad), cases, True, sources, modes, with_table, with_bits)
            assert not errs, "\n".join(errs[:10])
