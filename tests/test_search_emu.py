"""The search kernels' bodies (arcle_amd/csrc/arcle_search.h) on the CPU wave emulator against the oracle and the NumPy mirror of the
hash: expansion, hash identity and structure, and the sanitized standalone build of the emulator."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import backends as B
import search as SR
from arcle_amd import search as S


def test_expansion_equals_oracle():
    errs = SR.expansion(SR.EmuSearchBackend)
    assert not errs, "\n".join(errs[:10])


def test_chunk_boundaries_do_not_matter():
    """One wave per action, one wave per row, and chunks in between give the same outputs."""
    kind, H, W, mt = "o2arc", 12, 12, 1
    be, orc, rng, ops = SR.case_pair(SR.EmuSearchBackend, kind, H, W, mt)
    rows = B.state_rows(orc)
    pay, op = SR.draw_actions(rng, "bbox", 24, H, W, len(ops))
    ref = be.expand_rows(rows, "bbox", pay, op, chunk=24)
    for chunk in (1, 7, 23):
        got = be.expand_rows(rows, "bbox", pay, op, chunk=chunk)
        for k in ref:
            assert np.array_equal(got[k], ref[k]), (chunk, k)


def test_hash_rows_any_stride_and_alignment():
    errs = SR.hash_strides(SR.EmuSearchBackend)
    assert not errs, "\n".join(errs[:10])


def test_hash_structure():
    errs, n = SR.hash_structure(SR.EmuSearchBackend)
    assert n > 200000
    assert not errs, "\n".join(errs[:10])


def test_hash_identity_over_the_corpus():
    """Runs after the tests above (file order): every distinct row they kept has its own state_hash; grid_hash <=> (grid, grid_dim)."""
    if not SR.CORPUS:
        SR.expansion(SR.EmuSearchBackend, cases=SR.CASES[2:3])
    errs, total = SR.hash_identity()
    print(f"hash identity over {total} distinct rows")
    assert not errs, "\n".join(errs[:10])


def test_mirror_ignores_everything_but_content():
    """The mirror reads exactly the L bytes of a row: bytes behind it (padding, a tail) do not count."""
    _, orc, _, _ = SR.case_pair(B.OracleBackend, "arc", 30, 30, 3)
    rows = B.state_rows(orc)
    padded = np.concatenate([rows, np.full((len(rows), 9), 0x55, np.int8)], 1)
    assert np.array_equal(S.hash_rows_numpy(rows, "arc", 30, 30), S.hash_rows_numpy(padded, "arc", 30, 30))


def test_sanitized_standalone_emulator():
    """search_emu.cpp as a program of its own under ASan + UBSan (host code only): one dumped expansion case in, the outputs out."""
    cxx = shutil.which("g++")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "search_emu")
        probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-x", "c++", "-o", os.path.join(d, "probe"), "-"],
                               input=b"int main(){return 0;}", capture_output=True) if cxx else None
        if probe is None or probe.returncode != 0:
            pytest.skip("g++ has no sanitizer runtime")
        subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-DSEARCH_EMU_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-Wno-unknown-pragmas", "-o", exe, SR.EMU_SRC])
        kind, H, W, mt = "o2arc", 7, 12, -1
        be, orc, rng, ops = SR.case_pair(SR.EmuSearchBackend, kind, H, W, mt)
        rows = B.state_rows(orc)
        src = rng.integers(0, 8, 8).astype(np.int32)
        pay, op = SR.draw_actions(rng, "bbox", 8 * 12, H, W, len(ops))
        pay, op = pay.reshape(8, 12, 4), op.reshape(8, 12)
        op[0, 1] = len(ops) + 1
        want = be.expand_rows(rows, "bbox", pay, op, src_env=src, chunk=5)
        case = os.path.join(d, "case.bin")
        SR.dump_case(case, be, rows, "bbox", pay, op, src, SR.STEP_DENSE, 5)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:use_sigaltstack=0", UBSAN_OPTIONS="halt_on_error=1")
        run = subprocess.run([exe, case], capture_output=True, text=True, env=env, timeout=600)
        assert run.returncode == 0, run.stderr[-2000:]
        got = np.array([[int(v) for v in line.split()] for line in run.stdout.strip().splitlines()], dtype=np.uint64).reshape(8, 12, 7)
        assert np.array_equal(got[..., 0].astype(np.int32), want["reward"]) and np.array_equal(got[..., 1], want["term"])
        assert np.array_equal(got[..., 2], want["status"]) and np.array_equal(got[..., 3:5], want["hash"])
        assert np.array_equal(got[..., 5:7].astype(np.int32), want["dense"])


def test_expansion_and_hash_at_the_fast_widths():
    """20 x 24 and 16 x 16 at the default stride: the FW_FAST kernels with 32 and 16 live lanes"""
    errs = SR.expansion(SR.EmuSearchBackend, cases=SR.FAST_CASES) + SR.hash_strides(SR.EmuSearchBackend, cases=SR.FAST_CASES)
    assert not errs, "\n".join(errs[:10])
