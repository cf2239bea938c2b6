"""The place kernel's body (arcle_amd/csrc/arcle_place.h) on the CPU wave emulator against arcle_amd.search.place_numpy — which
tests/test_place_host.py pins on the oracle's own Moves — and the sanitized standalone build of the emulator."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import backends as B
import place as PL


@pytest.mark.parametrize("H,W", PL.SIZES)
def test_emulated_kernel_equals_the_mirror(H, W):
    """Per size: moved noise, shrunk grid_dim with answer_dim larger / smaller per axis, arbitrary bytes under the whole-grid object,
    rectangles and an empty mask, the two-colour shape and the tie cases, in state rows of all three env kinds and the resident form;
    M = 1 and 37; C in {1, 5, 16}; max_dist in {0, 1, 3, large}; count given and NULL; src_env given (with a row that names no env) and
    NULL; every word of place and base exact, entries >= count and the bytes around every output untouched."""
    errs = PL.run_size(PL.EmuPlace(), H, W)
    assert not errs, "\n".join(errs[:10])


def test_plan_covers_every_axis():
    for H, W in PL.SIZES:
        runs = PL.plan(H, W)
        assert {r[0] for r in runs} == {"o2arc", "arc", "raw"} and {r[1] for r in runs} == {"lib", "dense", "odd", "resident"}
        assert {1, 37} <= {r[2] for r in runs} and {r[4] for r in PL.plan(H, W, True)} == set(PL.DISTS) and {r[3] for r in runs} == set(PL.CS) and {r[4] for r in runs} == set(PL.DISTS)
        assert {r[5] for r in runs} == {True, False} and {r[6] for r in runs} == {True, False} and {r[7] for r in runs} == {True, False}
        names = " ".join(c["name"] for c in PL.cases_of(H, W))
        assert "moved" in names and "shrunk a" in names and "bytes" in names and ((H < 2 and W < 2) or "tie" in names)


def test_params_mirror():
    assert PL.emu_lib().place_emu_params_size() == ctypes.sizeof(PL._PlaceParams) == ctypes.sizeof(B._StepParams) + 48


def test_generic_instantiation_at_fast_widths():
    """FW_GENERIC serves any width: at 30 x 30 and 64 x 16 (where the library launches FW_FAST) it gives the same answers."""
    for H, W in ((30, 30), (64, 16)):
        errs = PL.run_size(PL.EmuPlace(fw=0), H, W, runs=[("arc", "odd", None, 16, PL.LARGE, True, True, True)])
        assert not errs, "\n".join(errs[:10])


def test_symmetric_answers_pin_every_level_of_the_tie_rule():
    """The tie cases alone, row board and flat board, unlimited and cut at distance 1: (dx, dy) is the mirror's, and the mirror's is
    the one tests/test_place_host.py spells out."""
    for H, W in ((20, 7), (30, 30), (16, 33)):
        cases = [c for c in PL.cases_of(H, W) if " tie" in c["name"]]
        assert len(cases) == 7
        for dist in (1, 3 if W > 32 else PL.LARGE):  # (farther than the farthest answer cell of a tie case, 2, either way)
            be = PL.EmuPlace()
            got = be.run("o2arc", H, W, cases, "lib", 1, dist, True, False, True, np.random.default_rng(0))
            errs = PL.compare(f"ties {H}x{W} dist {dist}", got, cases, 1, dist, True, True)
            assert not errs and be.guards_intact(), "\n".join(errs[:10])


def test_sanitized_standalone_emulator():
    """place_emu.cpp as a program of its own under ASan + UBSan (host code only; nothing is loaded into Python), buffers exactly as
    long as the data: the row board under the fast width (30 x 30), under the generic width with a plane stride below 1024 bytes
    (20 x 7) and the flat board (16 x 33), rows and resident, the last row / env / bit row ending its buffer."""
    cxx = shutil.which("g++")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "place_emu")
        probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-x", "c++", "-o", os.path.join(d, "probe"), "-"],
                               input=b"int main(){return 0;}", capture_output=True) if cxx else None
        if probe is None or probe.returncode != 0:
            pytest.skip("g++ has no sanitizer runtime")
        subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-DPLACE_EMU_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-Wno-unknown-pragmas", "-o", exe, PL.EMU_SRC])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:use_sigaltstack=0", UBSAN_OPTIONS="halt_on_error=1")
        rng = np.random.default_rng(5)
        for (H, W), kind, layout, C, dist, with_count, with_src in (((30, 30), "o2arc", "dense", 16, PL.LARGE, True, True), ((20, 7), "raw", "odd", 5, 3, False, False),
                                                                   ((20, 7), "arc", "resident", 16, PL.LARGE, True, True), ((16, 33), "o2arc", "lib", 5, 3, True, False),
                                                                   ((16, 33), "arc", "resident", 1, PL.LARGE, False, True)):
            cases = PL.cases_of(H, W)[1:6]  # (shrunk a / b, bytes, the two-colour shape, a tie)
            case = os.path.join(d, "case.bin")
            bad = PL.dump_case(case, kind, H, W, cases, layout, C, dist, with_count, with_src, True, rng)
            run = subprocess.run([exe, case], capture_output=True, text=True, env=env, timeout=600)
            assert run.returncode == 0, run.stderr[-2000:]
            place, base = PL.parse_dump(run.stdout, cases, C, with_count, True)
            errs = PL.compare(f"sanitized {H}x{W} {kind} {layout}", (place, base, bad), cases, C, dist, with_count, True)
            assert not errs, "\n".join(errs[:10])
