"""The ray kernel's body (arcle_amd/csrc/arcle_ray.h) on the CPU wave emulator against arcle_amd.search.ray_numpy — which
tests/test_ray_host.py pins on the oracle's own Color step — and the sanitized standalone build of the emulator."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import backends as B
import ray as RY


@pytest.mark.parametrize("H,W", RY.SIZES)
def test_emulated_kernel_equals_the_mirror(H, W):
    """Per size: the cases of tests/place.py (moved noise, shrunk grid_dim with answer_dim larger / smaller per axis, arbitrary bytes
    under the whole-grid object, rectangles and an empty mask, the two-colour shape, the ties) and the rays' own (seeds and obstacles
    with their lines in the answer, grid_dim below the plane, ten-colour noise, an L and two rings, a background of 5), in state rows
    of all three env kinds and the resident form; M = 1 and 37; C in {1, 5, 16}; the 13 default sets, 16 sets with zero entries and one
    set; through 0 and 1; free_color 0, 5 and -1; count, src_env (with a row that names no env), base and best_bits given and NULL;
    every word of ray, best, best_bits and base exact, entries >= count and the bytes around every output untouched."""
    errs = RY.run_size(RY.EmuRay(), H, W)
    assert not errs, "\n".join(errs[:10])


def test_plan_covers_every_axis():
    for H, W in RY.SIZES:
        runs = RY.plan(H, W)
        assert {r[0] for r in runs} == {"o2arc", "arc", "raw"} and {r[1] for r in runs} == {"lib", "dense", "odd", "resident"}
        assert {1, 37} <= {r[2] for r in runs} and {r[3] for r in runs} == set(RY.CS) and {r[4] for r in runs} == set(RY.SET_LISTS)
        assert {r[5] for r in runs} == {0, 5, -1} and all({r[i] for r in runs} == {True, False} for i in (6, 7, 8, 9, 10))
        names = " ".join(c["name"] for c in RY.cases_of(H, W))
        assert "moved" in names and "shrunk a" in names and "bytes" in names
        if H >= 3 and W >= 3:
            assert all(n in names for n in ("lines", "star", "dense", "shape", "fives"))
    assert len(RY.SETS16) == 16 and 0 in RY.SETS16 and len(RY.DEFAULT) == 13
    assert {(H > 64, W > 32) for H, W in RY.SIZES} == {(False, False), (True, False), (False, True)}  # row board, both flat-board reasons


def test_the_added_cases_are_what_they_claim():
    """lines / star: the best candidate of a seed is the set the answer was drawn with, and it gains; fives: nothing moves at
    free_color 0, the row is drawn at 5; shape: the L's best is N | E... or a superset that scores the same with fewer cells."""
    for H, W in ((7, 6), (12, 12), (30, 30), (16, 33)):
        by = {c["name"].split(" ", 1)[1]: c for c in RY.cases_of(H, W)}
        for name, want in (("lines", 0x0f), ("star", 0xff)):
            ray, best, base, _ = RY.mirror(by[name], RY.DEFAULT, 0, False)
            seeds = [k for k in range(len(best)) if by[name]["masks"][k].any() and by[name]["grid"][by[name]["masks"][k] != 0][0] != 8]
            assert seeds and any(best[k, 2] > base[0] for k in seeds)
            assert sum(best[k, 2] > base[0] and RY.DEFAULT[best[k, 0]] == want for k in seeds) >= 1, (H, W, name)
        r0, b0, base, _ = RY.mirror(by["fives"], RY.DEFAULT, 0, False)
        r5, b5, _, _ = RY.mirror(by["fives"], RY.DEFAULT, 5, False)
        assert (b0[:, 0] == -1).all() and b5[0].tolist() == [9, 2, base[0] + W - 1, W - 1]  # W|E: the whole row
        ray, best, base, _ = RY.mirror(by["shape"], RY.DEFAULT, 0, False)
        assert best[0, 2] > base[0]


def test_params_mirror():
    assert RY.emu_lib().ray_emu_params_size() == ctypes.sizeof(RY._RayParams) == ctypes.sizeof(B._StepParams) + 80


def test_generic_instantiation_at_fast_widths():
    """FW_GENERIC serves any width: at 30 x 30 and 64 x 16 (where the library launches FW_FAST) it gives the same answers."""
    for (H, W), through in (((30, 30), False), ((64, 16), True)):
        errs = RY.run_size(RY.EmuRay(fw=0), H, W, runs=[("arc", "odd", None, 16, "default", 0, through, True, True, True, True)])
        assert not errs, "\n".join(errs[:10])


def test_a_caller_chosen_plane_stride():
    """7 x 12 at plane stride 96 (FW_GENERIC, six live lanes, 12 padding bytes of garbage): the plan's answers, and the slack behind every
    plane untouched."""
    import strides as STR
    inst, check = STR.family_with_stride(RY.EmuRay, 96)
    errs = RY.run_size(inst, 7, 12) + check()
    assert not errs, "\n".join(errs[:10])


def test_sanitized_standalone_emulator():
    """ray_emu.cpp as a program of its own under ASan + UBSan (host code only; nothing is loaded into Python), buffers exactly as long
    as the data: the row board under the fast width (30 x 30), under the generic width with a plane stride below 1024 bytes (20 x 7)
    and the flat board (16 x 33 and 65 x 15), rows and resident, both `through` values, the last row / env / bit row / set ending
    its buffer."""
    cxx = shutil.which("g++")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "ray_emu")
        probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-x", "c++", "-o", os.path.join(d, "probe"), "-"],
                               input=b"int main(){return 0;}", capture_output=True) if cxx else None
        # (no skip: this is the only ASan / UBSan run of the kernel body, so a toolchain without the runtime is a failure to see)
        assert probe is not None and probe.returncode == 0, "g++ with -fsanitize=address,undefined is needed: " + (probe.stderr.decode()[-500:] if probe else "no g++")
        subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-DRAY_EMU_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-Wno-unknown-pragmas", "-o", exe, RY.EMU_SRC])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:use_sigaltstack=0", UBSAN_OPTIONS="halt_on_error=1")
        rng = np.random.default_rng(5)
        for (H, W), kind, layout, C, setname, fc, through, with_count, with_src, with_bits in (
                ((30, 30), "o2arc", "dense", 16, "default", 0, False, True, True, True), ((20, 7), "raw", "odd", 5, "sixteen", 0, True, False, False, True),
                ((20, 7), "arc", "resident", 16, "one", 5, False, True, True, False), ((16, 33), "o2arc", "lib", 5, "sixteen", 0, False, True, False, True),
                ((65, 15), "arc", "resident", 3, "default", 0, True, False, True, True)):
            cases = RY.cases_of(H, W)
            cases = cases[1:4] + [c for c in cases if c["name"].endswith(("lines", "star", "dense", "shape", "fives"))]
            sets = RY.SET_LISTS[setname]
            case = os.path.join(d, "case.bin")
            bad = RY.dump_case(case, kind, H, W, cases, layout, C, sets, fc, through, with_count, with_src, True, with_bits, rng)
            run = subprocess.run([exe, case], capture_output=True, text=True, env=env, timeout=600)
            assert run.returncode == 0, run.stderr[-2000:]
            ray, best, bbits, base = RY.parse_dump(run.stdout, cases, C, len(sets), with_count, True, with_bits)
            errs = RY.compare(f"sanitized {H}x{W} {kind} {layout}", (ray, best, bbits, base, bad), cases, C, sets, fc, through, with_count, True, with_bits)
            assert not errs, "\n".join(errs[:10])
