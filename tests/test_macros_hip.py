"""arcle_expand_macros / ARCVecEnv.expand_macros / transition_macros / beam_search with macro candidates on the MI355X: the checks of
tests/macros.py through the product, materialisation against expansion, the refusals, graph capture, and the stamp tasks through
ARCVecEnv with the same results as on the oracle-backed stub."""
import numpy as np
import pytest
import torch

import backends as B
import macros as MC
import search as SR
from arcle_amd import search as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", SR.CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_macro_expansion_equals_the_chained_oracle_hip(case):
    errs = MC.parity(MC.HipMacroBackend, cases=(case,))
    assert not errs, "\n".join(errs[:10])


def test_macros_under_reset_on_submit_equal_the_reference_traces_hip():
    errs = MC.reset_on_submit(MC.HipMacroBackend)
    assert not errs, "\n".join(errs[:10])


def test_one_step_macros_are_expand_rows_hip():
    errs = MC.single_steps(MC.HipMacroBackend)
    assert not errs, "\n".join(errs[:10])


def test_macro_chunk_boundaries_hip():
    errs = MC.chunks(MC.HipMacroBackend)
    assert not errs, "\n".join(errs[:10])


# ---- the stamp tasks through ARCVecEnv ------------------------------------------------------------------------------------------------
_STAMP = {}


def _stamp():
    if not _STAMP:
        from arcle_amd.envs import ARCVecEnv, O2ARCv2Env
        from arcle_amd.loaders import SyntheticLoader
        inputs, dims, answers, steps = MC.stamp_tasks()
        venv = ARCVecEnv(O2ARCv2Env, 8, SyntheticLoader(n_tasks=2, max_size=(10, 10)), max_grid_size=(10, 10), max_trial=3)
        venv.batch.set_tasks_padded(inputs, dims, answers, dims)
        venv.batch.reset()
        _STAMP.update(tasks=(inputs, dims, answers, steps), venv=venv, rows=venv.state_rows().clone())
    return _STAMP


def test_transition_macros_agrees_with_expand_macros():
    p = _stamp()
    venv, rows = p["venv"], p["rows"]
    assert np.array_equal(rows.cpu().numpy(), MC.stamp_rows(*p["tasks"][:3]))
    rng = np.random.default_rng(12)
    M, K, T = 8, 6, MC.T_MACROS
    _, _, pay, op, length = MC.draw_macros(rng, "bbox", None, (M, K), "o2arc", 10, 10, 35)
    length[0, 0], length[1, 0] = 0, T + 1
    op[2, 1, 0] = 40
    dev = rows.device
    pay_t, op_t, len_t = torch.as_tensor(pay, device=dev), torch.as_tensor(op, device=dev), torch.as_tensor(length, device=dev)
    for lens in (len_t, None):
        act = {"bbox": pay_t, "operation": op_t}
        if lens is not None:
            act["length"] = lens
        ex = venv.expand_macros(rows, act)
        changed = 0
        for k in range(K):
            one = {"bbox": pay_t[:, k].contiguous(), "operation": op_t[:, k].contiguous()}
            if lens is not None:
                one["length"] = lens[:, k].contiguous()
            out, r, t = venv.transition_macros(rows, one)
            assert out.shape == rows.shape and torch.equal(r, ex.reward[:, k]) and torch.equal(t, ex.term[:, k] != 0), (k, lens is None)
            assert torch.equal(venv.hash_rows(out.contiguous()), ex.hash[:, k]), (k, lens is None)
            changed += int((out != rows).any(1).sum())
        assert changed >= M * K // 2  # (the comparison is not one of untouched rows)
    assert torch.equal(rows, venv.state_rows())  # nothing of the env's own state moved
    venv.batch.status(True)  # (the row kernel's status bits are sticky: the planted bad op)


def test_macros_solve_the_stamp_tasks_as_on_the_oracle_stub():
    p = _stamp()
    inputs, dims, answers, steps = p["tasks"]
    singles, macros = MC.stamp_searches(p["venv"], p["rows"], 8)
    stub = MC.MacroVenv("o2arc", 10, 10, 3, O.o2arc_ops(), answers, dims)
    s_singles, s_macros = MC.stamp_searches(stub, p["rows"].cpu(), 8)
    assert [r.sequence for r in singles] == [None] * 8
    for n in range(8):
        assert macros[n].sequence is not None and len(macros[n].sequence) == 2
        assert macros[n] == s_macros[n] and singles[n] == s_singles[n], (n, macros[n], s_macros[n], singles[n], s_singles[n])
        assert MC.replay_steps_on_oracle(inputs[n], dims[n], answers[n], macros[n].sequence) == 1
    p["venv"].check_errors()


def test_planes_carry_the_slack_the_row_kernels_read_into():
    """The row kernels request the answer plane from all 64 lanes — 1024 bytes from the env's plane on — so a handle with a plane
    stride below 1024 owns ARCLE_PLANE_SLACK bytes behind every plane; an in-place Submit on the LAST env of such a handle (the
    step that reads the answer) runs inside them."""
    from arcle_amd import engine
    p = _stamp()
    b = p["venv"].batch
    assert engine.PLANE_SLACK == 1024 and b.PS == 128
    for k, t in b.planes.items():
        store = b._plane_store[k]
        assert t.data_ptr() == store.data_ptr() and store.numel() == b.N * b.PS + engine.PLANE_SLACK and t.is_contiguous()
    dev = p["rows"].device
    act = {"bbox": torch.zeros((1, 1, 4), dtype=torch.int32, device=dev), "operation": torch.full((1, 1), 34, dtype=torch.int32, device=dev)}
    out, r, t = p["venv"].transition_macros(p["rows"][7:8], act, torch.tensor([7], dtype=torch.int32, device=dev))
    assert int(r[0]) == 0 and not bool(t[0]) and out.shape == (1, p["rows"].shape[1])
    p["venv"].batch.status(True)


# ---- the C entry point's refusals ------------------------------------------------------------------------------------------------------
def test_refusals_return_their_codes_and_write_nothing():
    from arcle_amd import _lib
    from arcle_amd.engine import EnvBatch
    L = _lib.lib()
    ERR_ARG, ERR_CONFIG, MASK, BBOX, BBOX5, BITS = -1, -2, 0, 1, 3, 4
    be, orc, rng, ops = SR.case_pair(MC.HipMacroBackend, "o2arc", 12, 12, 1)
    dev, M, K, T = be.b.device, 8, 4, 2
    rows = torch.as_tensor(B.state_rows(orc), device=dev)
    sel = torch.zeros(M * K * T * 144 + 2, dtype=torch.uint8, device=dev)  # (large enough for any form asked below)
    op = torch.zeros((M, K, T), dtype=torch.int32, device=dev)
    outs = [torch.full((M, K, 4), 0x77, dtype=torch.uint8, device=dev), torch.full((M, K), 0x77, dtype=torch.uint8, device=dev),
            torch.full((M, K), 0x77, dtype=torch.uint8, device=dev), torch.full((M, K, 16), 0x77, dtype=torch.uint8, device=dev),
            torch.full((M, K, 8), 0x77, dtype=torch.uint8, device=dev), torch.full((M, 16), 0x77, dtype=torch.uint8, device=dev)]

    def expand(h, r, ingress, sel_ptr, max_len=T, flags=0):
        return L.arcle_expand_macros(h, M, r.data_ptr(), r.stride(0), K, max_len, ingress, sel_ptr, op.data_ptr(), None, K, None, outs[0].data_ptr(),
                                     outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), outs[4].data_ptr(), outs[5].data_ptr(), flags, None)
    assert sel.data_ptr() % 2 == 0
    assert expand(be.b._h, rows, MASK, sel.data_ptr()) == ERR_ARG          # int8 masks are not served
    assert expand(be.b._h, rows, BBOX5, sel.data_ptr()) == ERR_ARG
    assert expand(be.b._h, rows, BITS, sel.data_ptr() + 1) == ERR_ARG      # a bit row is read as uint16 words: 2-byte aligned
    assert expand(be.b._h, rows, BBOX, sel.data_ptr(), max_len=0) == ERR_ARG
    assert expand(be.b._h, rows, BBOX, sel.data_ptr(), flags=1) == ERR_ARG   # ARCLE_STEP_AUTORESET: a foreign flag
    assert expand(be.b._h, rows, BBOX, sel.data_ptr(), flags=32) == ERR_ARG  # ARCLE_STEP_CONTINUE_RULE: not served for macros
    with pytest.raises(_lib.ArcleHipError, match="2-byte aligned"):
        be.b.expand_macros(rows, "bits", sel[1:1 + M * K * T * 128].reshape(M, K, T, 128), op)
    big = EnvBatch(M, 40, 40, 3, "o2arc")
    big.set_op_table(O.o2arc_ops())
    big_rows = big.get_state_rows()
    assert expand(big._h, big_rows, BBOX, sel.data_ptr()) == ERR_CONFIG    # big grids stay refused
    with pytest.raises(_lib.ArcleHipError, match="1024"):
        big.expand_macros(big_rows, "bbox", torch.zeros((2, T, 4), dtype=torch.int32, device=dev), torch.zeros((2, T), dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    assert all(bool((t == 0x77).all()) for t in outs), "a refused call wrote to its outputs"
    assert be.b.status(False) == 0 and big.status(False) == 0
    # ... and the same arrays are served when asked properly
    assert expand(be.b._h, rows, BBOX, sel.data_ptr()) == 0
    torch.cuda.synchronize()
    assert not bool((outs[3] == 0x77).all())
    assert be.b.status(False) == 0


def test_expand_macros_in_a_captured_graph():
    be, orc, rng, ops = SR.case_pair(MC.HipMacroBackend, "o2arc", 30, 30, 3)
    dev = be.b.device
    base = B.state_rows(orc)
    M, K = len(base), MC.K_MACROS
    _, _, pay, op, length = MC.draw_macros(rng, "bbox", base, (M, K), "o2arc", 30, 30, len(ops))
    rows, pay, op, length = (torch.as_tensor(a, device=dev) for a in (base, pay, op, length))
    ref = be.b.expand_macros(rows, "bbox", pay, op, length, dense=True)
    torch.cuda.synchronize()
    out = type(ref)(*[torch.zeros_like(t) for t in ref])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):  # (one launch: a single-branch graph)
        be.b.expand_macros(rows, "bbox", pay, op, length, dense=True, out=out)
    for _ in range(2):
        for t in out:
            t.fill_(0x33)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, ref):
            assert torch.equal(a, b)


@pytest.mark.parametrize("case", SR.FAST_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_macro_expansion_at_the_fast_widths_hip(case):
    """20 x 24 and 16 x 16 at the default stride: the FW_FAST kernel with 32 and 16 live lanes"""
    errs = MC.parity(MC.HipMacroBackend, cases=(case,))
    assert not errs, "\n".join(errs[:10])
