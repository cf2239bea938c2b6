"""arcle_expand_rows / arcle_hash_rows / beam_search on the MI355X: the checks of tests/search.py through the product, expansion
against the row kernel at a size users run, graph capture, and beam search on planted tasks judged by an oracle replay."""
import numpy as np
import pytest
import torch

import backends as B
import search as SR
from arcle_amd import search as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def test_expansion_equals_oracle_hip():
    errs = SR.expansion(SR.HipSearchBackend)
    assert not errs, "\n".join(errs[:10])


def test_hash_rows_any_stride_and_alignment_hip():
    errs = SR.hash_strides(SR.HipSearchBackend)
    assert not errs, "\n".join(errs[:10])


def test_hash_structure_and_identity_hip():
    errs, n = SR.hash_structure(SR.HipSearchBackend, spot=200)
    assert n > 200000 and not errs, "\n".join(errs[:10])
    if len(SR.CORPUS) < 2:
        SR.expansion(SR.HipSearchBackend, cases=SR.CASES[1:2])
    errs, total = SR.hash_identity()
    assert not errs, "\n".join(errs[:10])
    # ... and the device agrees with the mirror on every distinct row of the corpus
    for (kind, H, W), chunks in SR.CORPUS.items():
        rows = np.unique(np.concatenate(chunks), axis=0)[:20000]
        be = SR.HipSearchBackend(8, H, W, 3, kind, O.KIND_OPS[kind]())
        assert np.array_equal(be.hash_rows(rows), S.hash_rows_numpy(rows, kind, H, W)), (kind, H, W)


def _frontier(n=8192, M=1024, seed=3):
    """M state rows drawn from an n-env 30 x 30 O2ARC batch after 10 random steps, and the env each came from."""
    import bench
    dev = torch.device("cuda:0")
    batch = bench.make_batch(dev, n)
    bbox, op = bench.make_actions(10, n, 2000)
    sh = torch.cuda.current_stream(dev).cuda_stream
    for i in range(10):
        batch.step_bbox_ptr(torch.as_tensor(bbox[i], device=dev).data_ptr(), torch.as_tensor(op[i], device=dev).data_ptr(), 0, sh)
        torch.cuda.synchronize(dev)
    batch.status(True)
    g = torch.Generator().manual_seed(seed)
    src = torch.randperm(n, generator=g)[:M].to(torch.int32).to(dev)
    rows = batch.get_state_rows().index_select(0, src.long()).contiguous()
    return batch, rows, src


def _action_set(K, per_row_M=None, seed=0):
    rng = np.random.default_rng(seed)
    n = K * (per_row_M or 1)
    op = (np.arange(n) % 35).astype(np.int32)  # K = 35: every op once
    a, b = rng.integers(0, 30, (n, 2)), rng.integers(0, 30, (n, 2))
    bbox = np.concatenate([a, np.minimum(29, a + (b % 6))], 1).astype(np.int32)  # one random rectangle each
    if per_row_M:
        return torch.from_numpy(bbox.reshape(per_row_M, K, 4)).cuda(), torch.from_numpy(op.reshape(per_row_M, K)).cuda()
    return torch.from_numpy(bbox).cuda(), torch.from_numpy(op).cuda()


def _by_row_kernel(batch, rows, src, bbox, op):
    """The parent commit's way: replicate, arcle_transition_rows with the dense pair (at most n_envs rows per launch: the dense output
    is per env), arcle_hash_rows of the rows it wrote."""
    M, K = rows.shape[0], op.shape[-1]
    n = batch.N
    batch.set_dense_output()
    rep = torch.arange(M, device=rows.device).repeat_interleave(K)
    pay = (bbox if bbox.dim() == 3 else bbox.expand(M, K, 4)).reshape(M * K, 4).contiguous()
    opf = (op if op.dim() == 2 else op.expand(M, K)).reshape(M * K).contiguous()
    out = {"reward": [], "term": [], "status": [], "hash": [], "dense": []}
    for s in range(0, M * K, n):
        r = rep[s:s + n]
        rows_out, rw, tm = batch.transition_rows(rows.index_select(0, r), "bbox", pay[s:s + n].contiguous(), opf[s:s + n].contiguous(),
                                                 src.index_select(0, r).contiguous(), tail=True, flags=SR.STEP_DENSE)
        torch.cuda.synchronize()
        L = batch.state_row_size()
        tail = rows_out[:, -16:].contiguous().view(torch.int32)
        out["reward"].append(rw.clone()), out["term"].append(tm.clone()), out["status"].append(((tail[:, 3] >> 16) & 0xff).to(torch.uint8))
        out["hash"].append(batch.hash_rows(rows_out[:, :L]).clone()), out["dense"].append(batch.dense[:len(r)].clone())
    return {k: torch.cat(v).reshape((M, K) + tuple(v[0].shape[1:])) for k, v in out.items()}


@pytest.mark.parametrize("K,per_row", [(35, False), (256, False), (35, True)])
def test_expand_equals_the_row_kernel_at_scale(K, per_row):
    batch, rows, src = _frontier()
    bbox, op = _action_set(K, rows.shape[0] if per_row else None, seed=K)
    ex = batch.expand_rows(rows, "bbox", bbox, op, src, dense=True)
    assert batch.status(False) == 0  # expansion is speculation: the sticky word stays clear whatever the children raised
    want = _by_row_kernel(batch, rows, src, bbox, op)
    batch.status(True)  # (the row kernel's bad-selection / domain bits are sticky: it is not speculation)
    assert torch.equal(ex.reward, want["reward"]) and torch.equal(ex.term, want["term"])
    assert torch.equal(ex.status, want["status"])
    assert torch.equal(ex.dense, want["dense"])
    assert torch.equal(ex.hash, want["hash"])
    assert torch.equal(ex.parent_hash, batch.hash_rows(rows))
    print(f"K={K}: {int((ex.hash[:, :, 0] != ex.parent_hash[:, None, 0]).sum())} of {ex.reward.numel()} children differ from their parent, "
          f"{int((ex.status != 0).sum())} with a status bit, {int(ex.reward.sum())} rewards")


def test_expand_in_a_captured_graph():
    batch, rows, src = _frontier(M=512)
    bbox, op = _action_set(64, seed=5)
    ref = batch.expand_rows(rows, "bbox", bbox, op, src, dense=True)
    torch.cuda.synchronize()
    out = type(ref)(*[None if t is None else torch.zeros_like(t) for t in ref])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        batch.expand_rows(rows, "bbox", bbox, op, src, dense=True, out=out)
    for _ in range(3):
        for t in out:
            t.fill_(0x33)
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, ref):
            assert torch.equal(a, b)


def test_expand_refuses_what_it_does_not_serve():
    from arcle_amd.engine import EnvBatch
    from arcle_amd._lib import ArcleHipError
    big = EnvBatch(4, 40, 40, 3, "o2arc")
    big.set_op_table(O.o2arc_ops())
    rows = big.get_state_rows()
    with pytest.raises(ArcleHipError, match="1024"):
        big.expand_rows(rows, "bbox", torch.zeros((2, 4), dtype=torch.int32).cuda(), torch.zeros(2, dtype=torch.int32).cuda())


# ---- beam search on planted tasks --------------------------------------------------------------------------------------------------
_PLANTED = {}


def _planted():
    if not _PLANTED:
        from arcle_amd.envs import ARCVecEnv, O2ARCv2Env
        from arcle_amd.loaders import SyntheticLoader
        tasks = SR.planted_tasks(16)
        inputs, idims, answers, adims, actions, seqs = tasks
        venv = ARCVecEnv(O2ARCv2Env, 16, SyntheticLoader(n_tasks=2, max_size=(10, 10)), max_grid_size=(10, 10), max_trial=3)
        venv.batch.set_tasks_padded(inputs, idims, answers, adims)
        venv.batch.reset()
        acts = {"bbox": torch.from_numpy(actions["bbox"]).cuda(), "operation": torch.from_numpy(actions["operation"]).cuda()}
        _PLANTED.update(tasks=tasks, venv=venv, rows=venv.state_rows().clone(), acts=acts)
    return _PLANTED


def test_beam_search_exhaustive_solves_every_planted_task():
    p = _planted()
    inputs, idims, answers, adims, actions, seqs = p["tasks"]
    counts = []
    for n in range(16):
        res = S.beam_search(p["venv"], p["rows"][n:n + 1], p["acts"], width=4096, depth=3, src_env=torch.tensor([n]))
        assert res.sequence is not None, f"task {n}: no sequence from an exhaustive search"
        assert SR.replay_on_oracle(inputs[n], idims[n], answers[n], adims[n], actions, res.sequence) == 1, (n, res.sequence, seqs[n])
        counts.append(res.counts)
    p["counts"] = counts
    p["venv"].check_errors()


def test_beam_search_pruned_returns_only_real_solutions():
    p = _planted()
    inputs, idims, answers, adims, actions, seqs = p["tasks"]
    solved = 0
    for n in range(16):
        res = S.beam_search(p["venv"], p["rows"][n:n + 1], p["acts"], width=64, depth=4, src_env=torch.tensor([n]))
        if res.sequence is not None:
            assert SR.replay_on_oracle(inputs[n], idims[n], answers[n], adims[n], actions, res.sequence) == 1, (n, res.sequence)
            solved += 1
    print(f"pruned beam (width 64, depth 4): {solved} of 16 planted tasks solved")


def test_beam_search_counts_equal_the_oracle_stub():
    p = _planted()
    inputs, idims, answers, adims, actions, seqs = p["tasks"]
    if "counts" not in p:
        test_beam_search_exhaustive_solves_every_planted_task()
    stub = SR.OracleVenv("o2arc", 10, 10, 3, O.o2arc_ops(), answers, adims)
    rows = p["rows"].cpu()
    acts = {k: v.cpu() for k, v in p["acts"].items()}
    for n in range(16):
        res = S.beam_search(stub, rows[n:n + 1], acts, width=4096, depth=3, src_env=torch.tensor([n]))
        assert res.counts == p["counts"][n], (n, res.counts, p["counts"][n])


def test_expansion_and_hash_at_the_fast_widths_hip():
    """20 x 24 and 16 x 16 at the default stride: the FW_FAST kernels with 32 and 16 live lanes"""
    errs = SR.expansion(SR.HipSearchBackend, cases=SR.FAST_CASES) + SR.hash_strides(SR.HipSearchBackend, cases=SR.FAST_CASES)
    assert not errs, "\n".join(errs[:10])
