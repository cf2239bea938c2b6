"""The mirror kernel's body (arcle_amd/csrc/arcle_mirror.h) on the CPU wave emulator against arcle_amd.search.mirror_numpy — which
tests/test_mirror_host.py pins on the oracle's own CopyO + Paste + Flip — and the sanitized standalone build of the emulator."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import backends as B
import mirror as MI


@pytest.mark.parametrize("H,W", MI.SIZES)
def test_emulated_kernel_equals_the_mirror(H, W):
    """Per size: the cases of tests/place.py (moved noise, shrunk grid_dim with answer_dim larger / smaller per axis, arbitrary bytes
    under the whole-grid object, rectangles and an empty mask, the two-colour shape) and the mirror's own (symmetric noise with a hole,
    axis central and off-centre, boxes on every edge, a box wider than half the grid, a non-rectangular hole, bytes below 0 and above 9,
    a hole whose old cells show through under blank = 0, the tie cases), in state rows of all three env kinds and the resident form;
    M = 1 and 37; C in {1, 5, 16}; max_dist in {0, 1, 3, large}; count given and NULL; src_env given (with a row that names no env) and
    NULL; every non-empty set of slots; both Pastes; every word of every slot asked for and base exact; slots not asked for, entries >=
    count and the bytes around every output untouched."""
    errs = MI.run_size(MI.EmuMirror(), H, W)
    assert not errs, "\n".join(errs[:10])


def test_plan_covers_every_axis():
    for H, W in MI.SIZES:
        runs = MI.plan(H, W)
        assert {r[0] for r in runs} == {"o2arc", "arc", "raw"} and {r[1] for r in runs} == {"lib", "dense", "odd", "resident"}
        assert {1, 37} <= {r[2] for r in runs} and {r[3] for r in runs} == set(MI.CS) and {r[4] for r in runs} == set(MI.DISTS)
        assert {r[5] for r in runs} == {True, False} and {r[6] for r in runs} == {True, False} and {r[7] for r in runs} == {True, False}
        assert {r[8] for r in runs} == set(range(1, 8)) and {r[9] for r in runs} == {True, False}
        for blank in (True, False):
            assert any(r[8] == MI.ALL and r[4] == MI.LARGE and r[9] == blank for r in runs)
            assert any(r[8] == MI.ALL and r[4] == MI.LARGE and r[2] is None and r[3] == 16 and r[9] == blank for r in MI.plan(H, W, True))  # every case, no limit
    assert set(MI.SIZES) >= set(MI.ORACLE_SIZES) | {(12, 12), (30, 30), (16, 33), (3, 40)} and len(set(MI.SIZES)) == len(MI.SIZES)


def test_params_mirror():
    assert MI.emu_lib().mirror_emu_params_size() == ctypes.sizeof(MI._MirrorParams) == ctypes.sizeof(B._StepParams) + 56


def test_generic_instantiation_at_fast_widths():
    """FW_GENERIC serves any width: at 30 x 30 and 64 x 16 (where the library launches FW_FAST) it gives the same answers."""
    for H, W in ((30, 30), (64, 16)):
        errs = MI.run_size(MI.EmuMirror(fw=0), H, W, runs=[("arc", "odd", None, 16, MI.LARGE, True, True, True, MI.ALL, True),
                                                           ("o2arc", "lib", None, 5, 3, False, False, True, MI.ALL, False)])
        assert not errs, "\n".join(errs[:10])


def test_a_caller_chosen_plane_stride():
    """7 x 12 at plane stride 96 (FW_GENERIC, six live lanes, 12 padding bytes of garbage): the plan's answers, and the slack behind every
    plane untouched."""
    import strides as STR
    inst, check = STR.family_with_stride(MI.EmuMirror, 96)
    errs = MI.run_size(inst, 7, 12) + check()
    assert not errs, "\n".join(errs[:10])


def test_symmetric_sources_pin_every_level_of_the_tie_rule():
    """The tie cases alone (a one-cell hole, two equally good source cells), row board and flat board, both Pastes, unlimited and cut at
    distance 1: every slot's (dx, dy) is the mirror's, and unlimited it is the source the tie rule names for that slot."""
    for H, W in ((20, 7), (30, 30), (16, 33)):
        cases = [c for c in MI.cases_of(H, W) if " mtie" in c["name"]]
        assert len(cases) == 7
        for dist, blank in ((1, True), (MI.LARGE, True), (MI.LARGE, False)):
            be = MI.EmuMirror()
            got = be.run("o2arc", H, W, cases, "lib", 1, dist, True, False, True, MI.ALL, blank, np.random.default_rng(0))
            errs = MI.compare(f"ties {H}x{W} dist {dist}", got, cases, 1, dist, True, True, MI.ALL, blank)
            assert not errs and be.guards_intact(), "\n".join(errs[:10])
            if dist == MI.LARGE:
                for c, m in zip(cases, got[0]):
                    for s in range(3):
                        assert (int(m[0, s, 0]), int(m[0, s, 1])) == MI.tie_want(c["name"].split(" ", 1)[1], s), (c["name"], s)


def test_sanitized_standalone_emulator():
    """mirror_emu.cpp as a program of its own under ASan + UBSan (host code only; nothing is loaded into Python), buffers exactly as
    long as the data: the row board under the fast width (30 x 30), under the generic width with a plane stride below 1024 bytes
    (20 x 7) and the flat board (16 x 33), rows and resident, all slots and subsets, both Pastes, the last row / env / bit row ending its
    buffer; the cases include the holes on every edge."""
    cxx = shutil.which("g++")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "mirror_emu")
        probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-x", "c++", "-o", os.path.join(d, "probe"), "-"],
                               input=b"int main(){return 0;}", capture_output=True) if cxx else None
        if probe is None or probe.returncode != 0:
            pytest.skip("g++ has no sanitizer runtime")
        subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-DMIRROR_EMU_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-Wno-unknown-pragmas", "-o", exe, MI.EMU_SRC])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:use_sigaltstack=0", UBSAN_OPTIONS="halt_on_error=1")
        rng = np.random.default_rng(5)
        for (H, W), kind, layout, C, dist, with_count, with_src, mirrors, blank in (
                ((30, 30), "o2arc", "dense", 5, MI.LARGE, True, True, MI.ALL, True), ((20, 7), "raw", "odd", 5, 3, False, False, 5, False),
                ((20, 7), "arc", "resident", 16, MI.LARGE, True, True, MI.ALL, False), ((16, 33), "o2arc", "lib", 5, 1, True, False, MI.ALL, True),
                ((16, 33), "arc", "resident", 1, 3, False, True, 6, False)):
            cases = MI.cases_of(H, W)
            cases = cases[1:4] + [c for c in cases if " edge " in c["name"] or c["name"].endswith(("wide", "lshape", "odd bytes", "show through", "pt off"))]
            case = os.path.join(d, "case.bin")
            bad = MI.dump_case(case, kind, H, W, cases, layout, C, dist, with_count, with_src, True, mirrors, blank, rng)
            run = subprocess.run([exe, case], capture_output=True, text=True, env=env, timeout=600)
            assert run.returncode == 0, run.stderr[-2000:]
            mir, base = MI.parse_dump(run.stdout, cases, C, with_count, True)
            errs = MI.compare(f"sanitized {H}x{W} {kind} {layout}", (mir, base, bad), cases, C, dist, with_count, True, mirrors, blank)
            assert not errs, "\n".join(errs[:10])
