"""The turn kernel's body (arcle_amd/csrc/arcle_turn.h) on the CPU wave emulator against arcle_amd.search.turn_numpy — which
tests/test_turn_host.py pins on the oracle's own select + turn + Moves — and the sanitized standalone build of the emulator."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import backends as B
import place as PL
import turn as TU


@pytest.mark.parametrize("H,W", TU.SIZES)
def test_emulated_kernel_equals_the_mirror(H, W):
    """Per size: the cases of tests/place.py (moved noise, shrunk grid_dim with answer_dim larger / smaller per axis, arbitrary bytes
    under the whole-grid object, rectangles and an empty mask, the two-colour shape, the tie cases) and the turn's own (the four parity
    classes, lines a quarter turn leaves hanging over each edge, a box with a negative byte and zeros, a line that fits under some
    turns only), in state rows of all three env kinds and the resident form; M = 1 and 37; C in {1, 5, 16}; max_dist in {0, 1, 3,
    large}; count given and NULL; src_env given (with a row that names no env) and NULL; all five turns and each alone; every word of
    every slot asked for and base exact; slots not asked for, entries >= count and the bytes around every output untouched."""
    errs = TU.run_size(TU.EmuTurn(), H, W)
    assert not errs, "\n".join(errs[:10])


def test_plan_covers_every_axis():
    for H, W in TU.SIZES:
        runs = TU.plan(H, W)
        assert {r[0] for r in runs} == {"o2arc", "arc", "raw"} and {r[1] for r in runs} == {"lib", "dense", "odd", "resident"}
        assert {1, 37} <= {r[2] for r in runs} and {r[3] for r in runs} == set(TU.CS) and {r[4] for r in runs} == set(TU.DISTS)
        assert {r[5] for r in runs} == {True, False} and {r[6] for r in runs} == {True, False} and {r[7] for r in runs} == {True, False}
        assert {r[8] for r in runs} == {TU.ALL, 1, 2, 4, 8, 16}
        assert any(r[8] == TU.ALL and r[4] == TU.LARGE for r in runs)
        assert any(r[8] == TU.ALL and r[4] == TU.LARGE and r[2] is None and r[3] == 16 for r in TU.plan(H, W, True))  # every case, no limit


def test_the_cases_reach_what_a_turn_can_meet():
    """All four parity classes of (h, w); a tile that a quarter turn leaves overhanging each of the four edges, so that (0, 0) is no
    candidate; an object that fits under some turns only (and, on the one-row / one-column grids, quarter turns without any
    candidate); a multi-colour object with a negative byte and a zero inside its box; grid_dim below (H, W) with junk outside it;
    answer_dim larger on one axis and smaller on the other; an empty mask; the whole-grid object; one tie per level of the tie rule."""
    for H, W in TU.SIZES:
        cases = TU.cases_of(H, W)
        names = " ".join(c["name"] for c in cases)
        facts = [f for c in cases for f in TU.facts(c)]
        assert any(not (c["masks"][k][:c["dim"][0], :c["dim"][1]]).any() for c in cases for k in range(len(c["masks"]))), "an empty mask"
        assert any(c["masks"][k].all() for c in cases for k in range(len(c["masks"]))), "the whole-grid object"
        shrunk = [c for c in cases if c["dim"].tolist() != [H, W]]
        if H > 2 and W > 3:
            assert shrunk and all((c["grid"][c["dim"][0]:] != 0).any() or (c["grid"][:, c["dim"][1]:] != 0).any() for c in shrunk), "junk outside grid_dim"
        if H >= 4 and W >= 4:  # (below that an axis of grid_dim is 1 and the answer cannot be smaller on it)
            assert any(c["adim"][0] > c["dim"][0] and c["adim"][1] < c["dim"][1] for c in shrunk) and any(c["adim"][0] < c["dim"][0] and c["adim"][1] > c["dim"][1] for c in shrunk)
            assert {(h % 2, w % 2) for h, w, *_ in facts} == {(0, 0), (0, 1), (1, 0), (1, 1)}
            hole = [c for c in cases if c["name"].endswith("holes")][0]
            inside = hole["grid"][hole["masks"][0] != 0]
            assert (inside < 0).any() and (inside == 0).any() and len(set(inside[inside > 0].tolist())) >= 2
            assert sum(" tie" in c["name"] for c in cases) == 7 and all(f" {n}" in names for n in TU.TIE_WANT)
        if H >= 3 and W >= 3:
            over = set()
            for h, w, stays, fits, edges in facts:
                over |= {e for e in edges if not stays[0]}
            assert over == {"top", "bottom", "left", "right"}, (H, W, over)
        if H != W and max(H, W) >= 3:
            assert any(fits[1] and fits[3] and fits[4] and not fits[0] and not fits[2] for _, _, _, fits, _ in facts), "fits under some turns only"
    # the mirror agrees about the overhang: (0, 0) is no candidate of the quarter turn, so its best candidate is at least one Move away
    for c in TU.cases_of(20, 7):
        if " over " in c["name"]:
            t, _ = TU.mirror(c, TU.LARGE)
            assert t[0, 0, 3] == 1 and abs(t[0, 0, 0]) + abs(t[0, 0, 1]) >= 1 and TU.mirror(c, 0)[0][0, 0].tolist() == [0, 0, 0, 0], c["name"]
    # (1, 9) and (9, 1): a quarter turn of anything longer than one cell has no candidate at all
    for H, W in ((1, 9), (9, 1)):
        long = [c for c in TU.cases_of(H, W) if c["name"].endswith("long")][0]
        t, _ = TU.mirror(long, TU.LARGE)
        assert t[0, :, 3].tolist() == [0, 1, 0, 1, 1]
    assert PL.cases_of(5, 5) is not TU.cases_of(5, 5) and len(TU.cases_of(5, 5)) > len(PL.cases_of(5, 5))


def test_params_mirror():
    assert TU.emu_lib().turn_emu_params_size() == ctypes.sizeof(TU._TurnParams) == ctypes.sizeof(B._StepParams) + 56


def test_generic_instantiation_at_fast_widths():
    """FW_GENERIC serves any width: at 30 x 30 and 64 x 16 (where the library launches FW_FAST) it gives the same answers."""
    for H, W in ((30, 30), (64, 16)):
        errs = TU.run_size(TU.EmuTurn(fw=0), H, W, runs=[("arc", "odd", None, 16, TU.LARGE, True, True, True, TU.ALL)])
        assert not errs, "\n".join(errs[:10])


def test_a_caller_chosen_plane_stride():
    """7 x 12 at plane stride 96 (FW_GENERIC, six live lanes, 12 padding bytes of garbage): the plan's answers, and the slack behind every
    plane untouched."""
    import strides as STR
    inst, check = STR.family_with_stride(TU.EmuTurn, 96)
    errs = TU.run_size(inst, 7, 12) + check()
    assert not errs, "\n".join(errs[:10])


def test_symmetric_answers_pin_every_level_of_the_tie_rule():
    """The tie cases alone (a one-cell object, which every turn leaves where it is; two cells of the answer fit it equally well), row
    board and flat board, unlimited and cut at distance 1: every turn's (dx, dy) is the mirror's, and unlimited it is the translation the
    tie rule names."""
    for H, W in ((20, 7), (30, 30), (16, 33)):
        cases = [c for c in TU.cases_of(H, W) if " tie" in c["name"]]
        assert len(cases) == 7
        for dist in (1, TU.LARGE):
            be = TU.EmuTurn()
            got = be.run("o2arc", H, W, cases, "lib", 1, dist, True, False, True, TU.ALL, np.random.default_rng(0))
            errs = TU.compare(f"ties {H}x{W} dist {dist}", got, cases, 1, dist, True, True, TU.ALL)
            assert not errs and be.guards_intact(), "\n".join(errs[:10])
            if dist == TU.LARGE:
                for c, s in zip(cases, got[0]):
                    for t in range(5):
                        assert (int(s[0, t, 0]), int(s[0, t, 1])) == TU.TIE_WANT[c["name"].split(" ", 1)[1]], (c["name"], t)


def test_sanitized_standalone_emulator():
    """turn_emu.cpp as a program of its own under ASan + UBSan (host code only; nothing is loaded into Python), buffers exactly as
    long as the data: the row board under the fast width (30 x 30), under the generic width with a plane stride below 1024 bytes
    (20 x 7) and the flat board (16 x 33), rows and resident, all turns and single ones, the last row / env / bit row ending its
    buffer; the cases include the tiles that a quarter turn leaves hanging over every edge."""
    cxx = shutil.which("g++")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "turn_emu")
        probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-x", "c++", "-o", os.path.join(d, "probe"), "-"],
                               input=b"int main(){return 0;}", capture_output=True) if cxx else None
        if probe is None or probe.returncode != 0:
            pytest.skip("g++ has no sanitizer runtime")
        subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-DTURN_EMU_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-Wno-unknown-pragmas", "-o", exe, TU.EMU_SRC])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:use_sigaltstack=0", UBSAN_OPTIONS="halt_on_error=1")
        rng = np.random.default_rng(5)
        for (H, W), kind, layout, C, dist, with_count, with_src, turns in (
                ((30, 30), "o2arc", "dense", 5, TU.LARGE, True, True, TU.ALL), ((20, 7), "raw", "odd", 5, 3, False, False, 5),
                ((20, 7), "arc", "resident", 16, TU.LARGE, True, True, TU.ALL), ((16, 33), "o2arc", "lib", 5, 1, True, False, TU.ALL),
                ((16, 33), "arc", "resident", 1, 3, False, True, 26)):
            cases = TU.cases_of(H, W)
            cases = cases[1:4] + [c for c in cases if " over " in c["name"] or c["name"].endswith(("holes", "long", "parity 2x3"))]
            case = os.path.join(d, "case.bin")
            bad = TU.dump_case(case, kind, H, W, cases, layout, C, dist, with_count, with_src, True, turns, rng)
            run = subprocess.run([exe, case], capture_output=True, text=True, env=env, timeout=600)
            assert run.returncode == 0, run.stderr[-2000:]
            turn, base = TU.parse_dump(run.stdout, cases, C, with_count, True)
            errs = TU.compare(f"sanitized {H}x{W} {kind} {layout}", (turn, base, bad), cases, C, dist, with_count, True, turns)
            assert not errs, "\n".join(errs[:10])
