"""The components kernel's body (arcle_amd/csrc/arcle_components.h) on the CPU wave emulator against arcle_amd.search.components_numpy
— which tests/test_components_host.py pins on the reference's dfs — and the sanitized standalone build of the emulator."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import components as CP


@pytest.mark.parametrize("H,W", CP.sizes())
def test_emulated_kernel_equals_the_mirror(H, W):
    """Every fixture grid of the size in state rows of all three env kinds; C in {1, 5, 32, 1024}; skip_color in {-1, 0, 3}; rows at the
    library's stride, densely packed and from an odd byte offset; M = 1 and 37; the resident form; bits; entries >= written untouched."""
    errs = CP.run_size(CP.EmuComponents(), H, W)
    assert not errs, "\n".join(errs[:10])


def test_plan_covers_every_axis():
    for H, W in CP.sizes():
        runs = CP.plan(H, W)
        assert {r[0] for r in runs} == {"o2arc", "arc", "raw"} and any(r[3] == "resident" for r in runs) and any(r[4] for r in runs)
        if (H, W) != (30, 30):
            assert {r[1] for r in runs} >= {1, 5, 32, 1024} and {r[2] for r in runs} == set(CP.SKIPS)
    runs = CP.plan(30, 30)
    assert {(r[1], r[2]) for r in runs} >= {(C, s) for C in (1, 5, 32, 1024) for s in CP.SKIPS}
    assert {r[3] for r in runs} == {"lib", "dense", "odd", "resident"} and {1, 37} <= {r[5] for r in runs}


def test_checkerboard_cut_and_complete():
    """900 one-cell components: C = 32 writes 32 and leaves 868; C = 1024 writes all 900 and leaves 0."""
    case = [c for c in CP.fixture() if c["name"] == "30x30 checker dim 30x30"]
    be = CP.EmuComponents()
    rows = CP.make_rows("o2arc", case, np.random.default_rng(0))
    for C, want in ((32, (32, 868)), (1024, (900, 0))):
        count, comp, _ = be.rows("o2arc", 30, 30, rows, "lib", C, -1, False)
        assert tuple(count[0]) == want
        assert not CP.compare("checker", (count, comp, None), case, C, -1, False)


def test_generic_instantiation_at_fast_widths():
    """FW_GENERIC serves any width: at 30 x 30 and 40 x 20 (where the library launches FW_FAST) it gives the same lists."""
    for H, W in ((30, 30), (40, 20)):
        errs = CP.run_size(CP.EmuComponents(fw=0), H, W, runs=[("arc", 32, 0, "odd", True, None)])
        assert not errs, "\n".join(errs[:10])


def test_sanitized_standalone_emulator():
    """components_emu.cpp as a program of its own under ASan + UBSan (host code only), buffers exactly as long as the data: the 12 x 12
    and 5 x 5 cases (plane stride below 1024 bytes) with the last row / the last env at the end of its buffer."""
    cxx = shutil.which("g++")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "components_emu")
        probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-x", "c++", "-o", os.path.join(d, "probe"), "-"],
                               input=b"int main(){return 0;}", capture_output=True) if cxx else None
        if probe is None or probe.returncode != 0:
            pytest.skip("g++ has no sanitizer runtime")
        subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-DCOMPONENTS_EMU_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-Wno-unknown-pragmas", "-o", exe, CP.EMU_SRC])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:use_sigaltstack=0", UBSAN_OPTIONS="halt_on_error=1")
        rng = np.random.default_rng(5)
        for (H, W), kind, layout, C, skip in (((12, 12), "o2arc", "dense", 32, -1), ((12, 12), "raw", "resident", 5, 0), ((5, 5), "raw", "odd", 1024, 0),
                                              ((5, 5), "arc", "resident", 32, -1), ((5, 5), "o2arc", "lib", 5, 3)):
            cases = CP.cases_of(H, W)
            case = os.path.join(d, "case.bin")
            CP.dump_case(case, kind, H, W, cases, C, skip, True, layout, rng)
            run = subprocess.run([exe, case], capture_output=True, text=True, env=env, timeout=600)
            assert run.returncode == 0, run.stderr[-2000:]
            got = CP.parse_dump(run.stdout, len(cases), C, True)
            errs = CP.compare(f"sanitized {H}x{W} {kind} {layout}", got, cases, C, skip, True)
            assert not errs, "\n".join(errs[:10])
