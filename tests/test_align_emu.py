"""The align kernel's body (arcle_amd/csrc/arcle_align.h) on the CPU wave emulator against arcle_amd.search.align_numpy — which
tests/test_align_host.py pins on the oracle's own Copy + resize_grid + Paste — and the sanitized standalone build of the emulator."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import align as AL
import backends as B
from arcle_amd import search as S


@pytest.mark.parametrize("H,W", AL.SIZES)
def test_emulated_kernel_equals_the_mirror(H, W):
    """Per size: windows of the grid and of the input, embeddings on both axes and on one, offsets of mixed sign, junk outside the
    source's dims, negative bytes, an answer colour with a foreign bit, all-zero sources, 1 x 1 answers and sources, dims of 0 and the
    tie cases, in state rows of all three env kinds and the resident form; M = 1 and 37; max_dist in {0, 1, 3, large}; sources 1, 2 and
    3; both Pastes; src_env given (with a row that names no env) and NULL; every word of every slot asked for and base exact; slots not
    asked for and the bytes around every output untouched."""
    errs = AL.run_size(AL.EmuAlign(), H, W)
    assert not errs, "\n".join(errs[:10])


def test_plan_covers_every_axis():
    for H, W in AL.SIZES:
        runs = AL.plan(H, W)
        assert {r[0] for r in runs} == {"o2arc", "arc", "raw"} and {r[1] for r in runs} == {"lib", "dense", "odd", "resident"}
        assert {1, 37} <= {r[2] for r in runs} and {r[3] for r in runs} == set(AL.DISTS)
        assert {r[4] for r in runs} == {True, False} and {r[5] for r in runs} == {True, False}
        assert {r[6] for r in runs} == {1, 2, 3} and {r[7] for r in runs} == {True, False}
        assert any(r[6] == 3 and r[3] == AL.LARGE and r[7] for r in runs) and any(r[6] == 3 and r[3] == AL.LARGE and not r[7] for r in runs)
        full = AL.plan(H, W, True)  # every case, no limit, under both Pastes
        assert any(r[6] == 3 and r[3] == AL.LARGE and r[2] is None and r[7] for r in full) and any(r[6] == 3 and r[3] == AL.LARGE and r[2] is None and not r[7] for r in full)


def _one(cases, suffix):
    return [c for c in cases if c["name"].endswith(suffix)][0]


def test_the_cases_reach_what_an_alignment_can_meet():
    """What tests/align.py::cases_of promises, from the cases themselves and from the mirror: a unique perfect window of the grid, and
    of the input under an all-zero grid; a source smaller than the answer on both axes and on one only; best offsets with ox < 0 < oy
    and oy < 0 < ox; source dims below (H, W) with junk outside them that would complete the answer if read; negative bytes that
    blank = 1 matches and blank = 0 turns into matches of the answer's zeros; an answer colour with a bit no source byte has; all-zero
    sources, for which the rule picks (0, 0); a 1 x 1 answer; a 1 x 1 source under a full-size answer, the largest offset range; dims
    of 0; one tie per level of the tie rule, each with the offset the rule names."""
    for H, W in AL.SIZES:
        cases = AL.cases_of(H, W)
        names = [c["name"].split(" ", 1)[1] for c in cases]
        assert len(set(names)) == len(names)
        for c in cases:  # every offset a case was built for is the mirror's, under both Pastes
            for blank in (True, False):
                al, _ = AL.mirror(c, AL.LARGE, blank)
                for s, want in c["want"].items():
                    assert (int(al[s, 0]), int(al[s, 1])) == want, (c["name"], s, al[s].tolist())
        wg, wi = _one(cases, "window grid"), _one(cases, "window input")
        assert not wi["grid"].any() and wi["inp"].all()
        for c, s in ((wg, 0), (wi, 1)):
            al, _, table, _ = S.align_numpy(c["grid"], c["dim"], c["inp"], c["idim"], c["answer"], c["adim"], full=True)
            assert al[s, 2] == al[s, 3] > 0 and (table[s] == al[s, 3]).sum() == 1, (c["name"], "a unique perfect window")
            assert al[1 - s, 2] < al[1 - s, 3]
        assert AL.mirror(_one(cases, "zero source"), AL.LARGE, True)[0][:, :2].tolist() == [[0, 0], [0, 0]]
        one_a, one_s = _one(cases, "1x1 answer"), _one(cases, "1x1 source")
        assert one_a["adim"].tolist() == [1, 1] and one_s["dim"].tolist() == [1, 1] and one_s["adim"].tolist() == [H, W]
        _, _, table, _ = S.align_numpy(one_s["grid"], one_s["dim"], one_s["inp"], one_s["idim"], one_s["answer"], one_s["adim"], full=True)
        assert (table[0] >= 0).sum() == H * W and table[0, 0, 0] >= 0  # ox down to -(H - 1), oy down to -(W - 1)
        for suffix, s in (("zero dim a", 0), ("zero dim b", 1), ("zero dim c", 0), ("zero dim c", 1)):
            c = _one(cases, suffix)
            al, _ = AL.mirror(c, AL.LARGE, True)
            assert al[s, :4].tolist() == [0, 0, 0, 0] and 0 in al[s, 4:].tolist(), c["name"]
        if H * W >= 9:  # (fewer cells cannot hold every kind of byte)
            neg = _one(cases, "negative")
            assert (neg["grid"] < 0).any() and (neg["answer"] < 0).any() and ((neg["grid"] < 0) & (neg["answer"] == 0)).any()
            a1, a0 = AL.mirror(neg, AL.LARGE, True)[0], AL.mirror(neg, AL.LARGE, False)[0]
            hit = [AL.child_of(neg["grid"], H, W, H, W, 0, 0, blank) == neg["answer"] for blank in (True, False)]
            assert (hit[0] & ~hit[1]).any() and (hit[1] & ~hit[0]).any(), "cells only blank = 1 matches, and cells only blank = 0 matches"
            assert a1[0, 2] >= hit[0].sum() and a0[0, 2] >= hit[1].sum()
            fb = _one(cases, "foreign bit")
            assert (fb["answer"] == 8).any() and not ((fb["grid"] | fb["inp"]) & 8).any()
        if H >= 2 or W >= 2:
            j = _one(cases, "junk")
            sh, sw = (int(v) for v in j["dim"])
            assert (sh, sw) != (H, W) and ((j["grid"][sh:] != 0).any() or (j["grid"][:, sw:] != 0).any())
            al, _ = AL.mirror(j, AL.LARGE, True)
            read = AL.child_of(j["grid"], H, W, int(j["adim"][0]), int(j["adim"][1]), int(H >= 2), int(W >= 2))  # (what reading the junk would give)
            assert np.array_equal(read, j["answer"]) and al[0, 2] < al[0, 3], "the junk would complete the answer; without it nothing does"
        if H >= 2 and W >= 2:
            e, e1 = _one(cases, "embed"), _one(cases, "embed one axis")
            assert (e["dim"] < e["adim"]).all() and e1["dim"][0] < e1["adim"][0] and e1["dim"][1] > e1["adim"][1]
            assert _one(cases, "cross a")["want"] == {0: (-1, 1)} and _one(cases, "cross b")["want"] == {1: (1, -1)}
            for c in (e, e1, _one(cases, "cross a"), _one(cases, "cross b")):
                al, _ = AL.mirror(c, AL.LARGE, True)
                assert all(al[s, 2] == al[s, 3] for s in c["want"]), c["name"]
        if H >= 4 and W >= 2:
            assert set(AL.TIE_NAMES) <= set(names)
            wants = {"tie distance": (1, 0), "tie ox": (-1, 0), "tie oy": (0, -1), "tie ox before oy": (0, 1)}  # the offset the rule names
            for name, want in wants.items():
                c = _one(cases, name)
                assert c["want"] == {0: want, 1: want}
                al, _, table, _ = S.align_numpy(c["grid"], c["dim"], c["inp"], c["idim"], c["answer"], c["adim"], full=True)
                best = np.argwhere(table[0] == al[0, 2]) - (H - 1, W - 1)
                assert len(best) >= 2 and want in [tuple(b) for b in best.tolist()], (c["name"], best.tolist())
                other = [tuple(b) for b in best.tolist() if tuple(b) != want]
                key = lambda o: (abs(o[0]) + abs(o[1]), o[0], o[1])
                level = {"tie distance": lambda o: key(o)[0] > key(want)[0], "tie ox": lambda o: key(o)[0] == key(want)[0] and o[0] > want[0],
                         "tie oy": lambda o: key(o)[:2] == key(want)[:2] and o[1] > want[1],
                         "tie ox before oy": lambda o: key(o)[0] == key(want)[0] and o[0] > want[0] and o[1] < want[1]}[name]
                assert any(level(o) for o in other), (c["name"], other)


def test_params_mirror():
    assert AL.emu_lib().align_emu_params_size() == ctypes.sizeof(AL._AlignParams) == ctypes.sizeof(B._StepParams) + 40


def test_generic_instantiation_at_fast_widths():
    """FW_GENERIC serves any width: at 30 x 30 and 64 x 16 (where the library launches FW_FAST) it gives the same answers."""
    for H, W in ((30, 30), (64, 16)):
        errs = AL.run_size(AL.EmuAlign(fw=0), H, W, runs=[("arc", "odd", ("window grid", "cross b", "junk", "tie oy"), AL.LARGE, True, True, 3, True),
                                                         ("o2arc", "lib", None, 3, True, True, 3, False)])
        assert not errs, "\n".join(errs[:10])


def test_a_caller_chosen_plane_stride():
    """7 x 12 at plane stride 96 (FW_GENERIC, six live lanes, 12 padding bytes of garbage): the plan's answers, and the slack behind every
    plane untouched."""
    import strides as STR
    inst, check = STR.family_with_stride(AL.EmuAlign, 96)
    errs = AL.run_size(inst, 7, 12) + check()
    assert not errs, "\n".join(errs[:10])


def test_flat_board_without_a_limit():
    """The flat board's whole offset range (3 x 40 and 16 x 33: 395 and 2015 offsets for a full-size pair), every case at 3 x 40 and
    the far-reaching ones at 16 x 33, under both Pastes."""
    errs = AL.run_size(AL.EmuAlign(), 3, 40, runs=[("o2arc", "lib", None, AL.LARGE, True, True, 3, True), ("arc", "dense", None, AL.LARGE, False, True, 3, False)])
    errs += AL.run_size(AL.EmuAlign(), 16, 33, runs=[("o2arc", "odd", ("window input", "cross a", "junk", "1x1 source", "tie ox before oy"), AL.LARGE, True, True, 3, True)])
    assert not errs, "\n".join(errs[:10])


def test_sanitized_standalone_emulator():
    """align_emu.cpp as a program of its own under ASan + UBSan (host code only; nothing is loaded into Python), buffers exactly as
    long as the data: the row board under the fast width (30 x 30), under the generic width with a plane stride below 1024 bytes
    (20 x 7) and the flat board (16 x 33), rows and resident, both sources and single ones, both Pastes, the last row / env ending its
    buffer; the cases include the offsets of mixed sign, the 1 x 1 source (the widest range) and the dims of 0."""
    cxx = shutil.which("g++")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "align_emu")
        probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-x", "c++", "-o", os.path.join(d, "probe"), "-"],
                               input=b"int main(){return 0;}", capture_output=True) if cxx else None
        if probe is None or probe.returncode != 0:
            pytest.skip("g++ has no sanitizer runtime")
        subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-DALIGN_EMU_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-Wno-unknown-pragmas", "-o", exe, AL.EMU_SRC])
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:use_sigaltstack=0", UBSAN_OPTIONS="halt_on_error=1")
        rng = np.random.default_rng(5)
        for (H, W), kind, layout, dist, with_src, sources, blank in (
                ((30, 30), "o2arc", "dense", AL.LARGE, True, 3, True), ((20, 7), "raw", "odd", 3, False, 1, False),
                ((20, 7), "arc", "resident", AL.LARGE, True, 3, False), ((16, 33), "o2arc", "lib", 3, False, 3, True),
                ((16, 33), "arc", "resident", 1, True, 2, False)):
            cases = [c for c in AL.cases_of(H, W) if c["name"].endswith(("window input", "cross a", "cross b", "negative", "1x1 source", "zero dim a", "zero dim c"))]
            case = os.path.join(d, "case.bin")
            bad = AL.dump_case(case, kind, H, W, cases, layout, dist, with_src, True, sources, blank, rng)
            run = subprocess.run([exe, case], capture_output=True, text=True, env=env, timeout=600)
            assert run.returncode == 0, run.stderr[-2000:]
            align, base = AL.parse_dump(run.stdout, len(cases), True)
            errs = AL.compare(f"sanitized {H}x{W} {kind} {layout}", (align, base, bad), cases, dist, True, sources, blank)
            assert not errs, "\n".join(errs[:10])
