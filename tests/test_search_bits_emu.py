"""Bit-packed selection masks in the search kernels (arcle_search.h wave_expand_row<INGRESS_BITS, FW>, arcle_wave.h
wave_transition_row<INGRESS_BITS, FW>) on the CPU wave emulator against the oracle stepped with the unpacked int8 masks, and the
sanitized standalone build of the emulator."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import backends as B
import search as SR
import search_bits as SB


def test_bit_row_expansion_equals_oracle():
    errs = SB.expansion(SB.EmuBitsBackend)
    assert not errs, "\n".join(errs[:10])


def test_rectangle_bit_rows_equal_the_bbox_expansion():
    errs = SB.rectangles(SB.EmuBitsBackend)
    assert not errs, "\n".join(errs[:10])


def test_chunk_boundaries_do_not_matter():
    errs = SB.chunks(SB.EmuBitsBackend)
    assert not errs, "\n".join(errs[:10])


def test_bit_row_transitions_equal_oracle_and_expansion():
    errs = SB.transitions(SB.EmuBitsBackend)
    assert not errs, "\n".join(errs[:10])


def test_bit_row_transitions_under_every_flag():
    errs = SB.flagged_transitions(SB.EmuBitsBackend)
    assert not errs, "\n".join(errs[:10])


def test_bits_beyond_the_grid_are_ignored():
    errs = SB.stray_bits(SB.EmuBitsBackend)
    assert not errs, "\n".join(errs[:10])


def test_sanitized_standalone_emulator():
    """search_bits_emu.cpp as a program of its own under ASan + UBSan (host code only): one dumped case in, the outputs out; `sel` is
    exactly M * K * 128 bytes, so a read past an action's bit row is a finding."""
    cxx = shutil.which("g++")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "search_bits_emu")
        probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-x", "c++", "-o", os.path.join(d, "probe"), "-"],
                               input=b"int main(){return 0;}", capture_output=True) if cxx else None
        if probe is None or probe.returncode != 0:
            pytest.skip("g++ has no sanitizer runtime")
        subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-DSEARCH_BITS_EMU_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-Wno-unknown-pragmas", "-o", exe, SB.EMU_SRC])
        kind, H, W, mt = "o2arc", 7, 12, -1
        be, orc, rng, ops, rows, _, _ = SB.mix_case(SB.EmuBitsBackend, kind, H, W, mt)
        src = rng.integers(0, 8, 8).astype(np.int32)
        grids, gdims = SB._grids_of(rows, kind, H, W)
        bits = B.pack_bits(SB.mask_mix(rng, grids, gdims, 12, H, W).reshape(-1, H, W)).reshape(8, 12, SB.STRIDE)
        op = rng.integers(0, len(ops), (8, 12)).astype(np.int32)
        op[0, 1] = len(ops) + 1
        want = be.expand_rows(rows, "bits", bits, op, src_env=src, chunk=5)
        case = os.path.join(d, "case.bin")
        SB.dump_case(case, be, rows, bits, op, src, SR.STEP_DENSE, 5)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:use_sigaltstack=0", UBSAN_OPTIONS="halt_on_error=1")
        run = subprocess.run([exe, case], capture_output=True, text=True, env=env, timeout=600)
        assert run.returncode == 0, run.stderr[-2000:]
        got = np.array([[int(v) for v in line.split()] for line in run.stdout.strip().splitlines()], dtype=np.uint64).reshape(8, 12, 7)
        assert np.array_equal(got[..., 0].astype(np.int32), want["reward"]) and np.array_equal(got[..., 1], want["term"])
        assert np.array_equal(got[..., 2], want["status"]) and np.array_equal(got[..., 3:5], want["hash"])
        assert np.array_equal(got[..., 5:7].astype(np.int32), want["dense"])


def test_bit_rows_at_the_fast_widths():
    """20 x 24 and 16 x 16 at the default stride: the FW_FAST kernels with 32 and 16 live lanes"""
    errs = SB.expansion(SB.EmuBitsBackend, cases=SR.FAST_CASES) + SB.transitions(SB.EmuBitsBackend, cases=SR.FAST_CASES)
    assert not errs, "\n".join(errs[:10])
