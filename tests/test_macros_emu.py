"""arcle_expand_macros' wave body on the lock-step CPU emulator (tests/emu/macro_emu.cpp) against the chained oracle: the checks of
tests/macros.py that need no GPU."""
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import backends as B
import macros as MC
import search as SR


@pytest.mark.parametrize("case", SR.CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_macro_expansion_equals_the_chained_oracle_emu(case):
    errs = MC.parity(MC.EmuMacroBackend, cases=(case,))
    assert not errs, "\n".join(errs[:10])


def test_macros_under_reset_on_submit_equal_the_reference_traces_emu():
    errs = MC.reset_on_submit(MC.EmuMacroBackend)
    assert not errs, "\n".join(errs[:10])


def test_one_step_macros_are_expand_rows_emu():
    errs = MC.single_steps(MC.EmuMacroBackend)
    assert not errs, "\n".join(errs[:10])


def test_macro_chunk_boundaries_emu():
    errs = MC.chunks(MC.EmuMacroBackend)
    assert not errs, "\n".join(errs[:10])


@pytest.mark.parametrize("form", ["bbox", "bits"])
def test_sanitized_standalone_emulator(form):
    """macro_emu.cpp as a program of its own under ASan + UBSan (host code only): one dumped case in, the outputs out.  `sel`, `op`
    and `len` are exactly as long as the contract says, so a request past a macro's last step, past the set or past the lengths —
    the prefetch of the next step under the current op is where that would come from — is a finding."""
    cxx = shutil.which("g++")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "macro_emu")
        probe = subprocess.run([cxx, "-fsanitize=address,undefined", "-static-libasan", "-x", "c++", "-o", os.path.join(d, "probe"), "-"],
                               input=b"int main(){return 0;}", capture_output=True) if cxx else None
        if probe is None or probe.returncode != 0:
            pytest.skip("g++ has no sanitizer runtime")
        subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-DMACRO_EMU_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                               "-static-libasan", "-Wno-unknown-pragmas", "-o", exe, MC.EMU_SRC])
        kind, H, W, mt = "o2arc", 7, 12, -1
        be, orc, rng, ops = SR.case_pair(MC.EmuMacroBackend, kind, H, W, mt)
        rows = B.state_rows(orc)
        src = rng.integers(0, 8, 8).astype(np.int32)
        M, K, T = 8, 12, MC.T_MACROS
        _, _, pay, op, length = MC.draw_macros(rng, form, rows, (M, K), kind, H, W, len(ops))
        op[0, 1, 1] = len(ops) + 1
        length[0, 4], length[M - 1, K - 1], length[M - 1, K - 2] = 0, T + 1, T  # (the last macros of the set: nothing behind them)
        want = be.expand_macros(rows, form, pay, op, length, src_env=src, chunk=5)
        case = os.path.join(d, "case.bin")
        MC.dump_case(case, be, rows, form, pay, op, length, src, SR.STEP_DENSE, 5)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:use_sigaltstack=0", UBSAN_OPTIONS="halt_on_error=1")
        run = subprocess.run([exe, case], capture_output=True, text=True, env=env, timeout=600)
        assert run.returncode == 0, run.stderr[-2000:]
        got = np.array([[int(v) for v in line.split()] for line in run.stdout.strip().splitlines()], dtype=np.uint64).reshape(M, K, 7)
        assert np.array_equal(got[..., 0].astype(np.int32), want["reward"]) and np.array_equal(got[..., 1], want["term"])
        assert np.array_equal(got[..., 2], want["status"]) and np.array_equal(got[..., 3:5], want["hash"])
        assert np.array_equal(got[..., 5:7].astype(np.int32), want["dense"])


@pytest.mark.parametrize("case", SR.FAST_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_macro_expansion_at_the_fast_widths(case):
    """20 x 24 and 16 x 16 at the default stride: the FW_FAST kernel with 32 and 16 live lanes"""
    errs = MC.parity(MC.EmuMacroBackend, cases=(case,))
    assert not errs, "\n".join(errs[:10])
