"""The stamp kernel's body (arcle_amd/csrc/arcle_stamp.h) on the CPU wave emulator against arcle_amd.search.stamp_numpy — which
tests/test_stamp_host.py pins on the oracle's own CopyO + Paste — and the sanitized standalone build of the emulator."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import backends as B
import place as PL
import stamp as ST


@pytest.mark.parametrize("H,W", ST.SIZES)
def test_emulated_kernel_equals_the_mirror(H, W):
    """Per size: the cases of tests/place.py (moved noise, shrunk grid_dim with answer_dim larger / smaller per axis, arbitrary bytes
    under the whole-grid object, rectangles and an empty mask, the two-colour shape, the tie cases) and the stamp's own (objects on the
    right / bottom edge and in the corner whose best stamp hangs over it, the hollow box, negative bytes), in state rows of all three
    env kinds and the resident form; M = 1 and 37; C in {1, 5, 16}; max_dist in {0, 1, 3, large}; count given and NULL; src_env given
    (with a row that names no env) and NULL; blank 1 and 0; every word of stamp and base exact, entries >= count and the bytes around
    every output untouched."""
    errs = ST.run_size(ST.EmuStamp(), H, W)
    assert not errs, "\n".join(errs[:10])


def test_plan_covers_every_axis():
    for H, W in ST.SIZES:
        runs = ST.plan(H, W)
        assert {r[0] for r in runs} == {"o2arc", "arc", "raw"} and {r[1] for r in runs} == {"lib", "dense", "odd", "resident"}
        assert {1, 37} <= {r[2] for r in runs} and {r[3] for r in runs} == set(ST.CS) and {r[4] for r in runs} == set(ST.DISTS)
        assert {r[5] for r in runs} == {True, False} and {r[6] for r in runs} == {True, False} and {r[7] for r in runs} == {True, False}
        assert {r[8] for r in runs} == {True, False} and {r[8] for r in runs if r[4] == ST.LARGE} == {True, False}
        full = ST.plan(H, W, True)
        assert {r[8] for r in full if r[4] == ST.LARGE and r[2] is None and r[3] == 16} == {True, False}  # every case, no limit, both Pastes
        names = " ".join(c["name"] for c in ST.cases_of(H, W))
        assert "moved" in names and "shrunk a" in names and "bytes" in names and ((H < 2 and W < 2) or "tie" in names)
        if H >= 3 and W >= 3:
            assert all(n in names for n in ("edge right", "edge bottom", "edge both", "hollow", "negative"))


def test_the_added_cases_are_what_they_claim():
    """The best stamp of each edge case hangs over the edge it names; the hollow box's best blank = 1 stamp is (x0, y0) itself with one
    more correct cell than the grid (and gains nothing with blank = 0); the negative object's copy counts its negative bytes only
    with blank = 1."""
    for H, W in ((5, 5), (20, 7), (30, 30), (16, 33)):
        by = {c["name"].split(" ", 1)[1]: c for c in ST.cases_of(H, W)}
        for name, over_x, over_y in (("edge right", False, True), ("edge bottom", True, False), ("edge both", True, True)):
            for blank in (True, False):
                (px, py, cor, cells), (base, _) = ST.mirror(by[name], ST.LARGE, blank)[0][0], ST.mirror(by[name], ST.LARGE, blank)[1]
                assert cells == 3 and cor > base and (px + 2 > H) == over_x and (py + 2 > W) == over_y, (H, W, name, blank)
        (s1, (base, _)), (s0, _) = ST.mirror(by["hollow"], ST.LARGE, True), ST.mirror(by["hollow"], ST.LARGE, False)
        assert s1[0].tolist() == [0, 0, base + 1, 8] and s0[0].tolist() == [0, 0, base, 8]
        (n1, (base, _)), (n0, _) = ST.mirror(by["negative"], ST.LARGE, True), ST.mirror(by["negative"], ST.LARGE, False)
        assert n1[0].tolist() == [H - 2, W - 2, base + 3, 4] and n0[0, 2] == base + 1
    assert PL.cases_of(5, 5) is not ST.cases_of(5, 5) and len(PL.cases_of(5, 5)) + 5 == len(ST.cases_of(5, 5))


def test_params_mirror():
    assert ST.emu_lib().stamp_emu_params_size() == ctypes.sizeof(ST._StampParams) == ctypes.sizeof(B._StepParams) + 56


def test_generic_instantiation_at_fast_widths():
    """FW_GENERIC serves any width: at 30 x 30 and 64 x 16 (where the library launches FW_FAST) it gives the same answers."""
    for (H, W), blank in (((30, 30), True), ((64, 16), False)):
        errs = ST.run_size(ST.EmuStamp(fw=0), H, W, runs=[("arc", "odd", None, 16, ST.LARGE, True, True, True, blank)])
        assert not errs, "\n".join(errs[:10])


def test_a_caller_chosen_plane_stride():
    """7 x 12 at plane stride 96 (FW_GENERIC, six live lanes, 12 padding bytes of garbage): the plan's answers, and the slack behind every
    plane untouched."""
    import strides as STR
    inst, check = STR.family_with_stride(ST.EmuStamp, 96)
    errs = ST.run_size(inst, 7, 12) + check()
    assert not errs, "\n".join(errs[:10])


def test_symmetric_answers_pin_every_level_of_the_tie_rule():
    """The tie cases alone (a one-cell object; its copy fits two cells of the answer equally well), row board and flat board, both
    Pastes, unlimited and cut at distance 1: (px, py) is the mirror's, and unlimited it is the cell the tie rule names."""
    for H, W in ((20, 7), (30, 30), (16, 33)):
        cases = [c for c in ST.cases_of(H, W) if " tie" in c["name"]]
        assert len(cases) == 7
        for blank in (True, False):
            for dist in (1, ST.LARGE):
                be = ST.EmuStamp()
                got = be.run("o2arc", H, W, cases, "lib", 1, dist, True, False, True, blank, np.random.default_rng(0))
                errs = ST.compare(f"ties {H}x{W} dist {dist}", got, cases, 1, dist, True, True, blank)
                assert not errs and be.guards_intact(), "\n".join(errs[:10])
                if dist == ST.LARGE:
                    for c, s in zip(cases, got[0]):
                        dx, dy = ST.TIE_WANT[c["name"].split(" ", 1)[1]]
                        assert (int(s[0, 0]), int(s[0, 1])) == (H // 2 + dx, W // 2 + dy), c["name"]


def test_sanitized_standalone_emulator():
    """stamp_emu.cpp as a program of its own under ASan + UBSan (host code only; nothing is loaded into Python), buffers exactly as
    long as the data: the row board under the fast width (30 x 30), under the generic width with a plane stride below 1024 bytes
    (20 x 7) and the flat board (16 x 33), rows and resident, both Pastes, the last row / env / bit row ending its buffer; the cases
    include the stamps that hang over the bottom and right edges."""
    cxx = shutil.which("g++")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "stamp_emu")
        probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-x", "c++", "-o", os.path.join(d, "probe"), "-"],
                               input=b"int main(){return 0;}", capture_output=True) if cxx else None
        if probe is None or probe.returncode != 0:
            pytest.skip("g++ has no sanitizer runtime")
        subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-DSTAMP_EMU_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-Wno-unknown-pragmas", "-o", exe, ST.EMU_SRC])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:use_sigaltstack=0", UBSAN_OPTIONS="halt_on_error=1")
        rng = np.random.default_rng(5)
        for (H, W), kind, layout, C, dist, with_count, with_src, blank in (
                ((30, 30), "o2arc", "dense", 16, ST.LARGE, True, True, True), ((20, 7), "raw", "odd", 5, 3, False, False, False),
                ((20, 7), "arc", "resident", 16, ST.LARGE, True, True, False), ((16, 33), "o2arc", "lib", 5, 3, True, False, True),
                ((16, 33), "arc", "resident", 1, ST.LARGE, False, True, False)):
            cases = ST.cases_of(H, W)
            cases = cases[1:5] + [c for c in cases if " edge" in c["name"] or c["name"].endswith(("hollow", "negative"))]
            case = os.path.join(d, "case.bin")
            bad = ST.dump_case(case, kind, H, W, cases, layout, C, dist, with_count, with_src, True, blank, rng)
            run = subprocess.run([exe, case], capture_output=True, text=True, env=env, timeout=600)
            assert run.returncode == 0, run.stderr[-2000:]
            stamp, base = PL.parse_dump(run.stdout, cases, C, with_count, True)
            errs = ST.compare(f"sanitized {H}x{W} {kind} {layout}", (stamp, base, bad), cases, C, dist, with_count, True, blank)
            assert not errs, "\n".join(errs[:10])
