"""Elided plane stores (arcle_wave.h Wave::store_if) on the MI355X: the adversarial streams of tests/adversarial.py — every env from
garbage planes installed through arcle_set_state_rows — on the real kernel at the headline batch (8192 envs: the self-ordering lean
instantiation) and at a streaming-plan size (40 960), compared with the oracle field by field; and the kernel's own byte accounting on
bench.py's c3 stream: the algorithmic figure is the parent's, the issued figure (16 B per lane that stored) well below it."""
import pytest

import adversarial as A
import backends as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu

HOT = O.STEP_AUTORESET | B.STEP_ELIDE_SELECTED


@pytest.mark.parametrize("N", [8192, 40960])
@pytest.mark.parametrize("flags", [0, B.STEP_ELIDE_SELECTED, HOT])
def test_adversarial_c3_mix_hip(N, flags):
    errs = A.adversarial_compare(B.HipBackend, O.o2arc_ops(), 30, 30, N=N, S=12, seed=N + flags, flags=flags, restate_every=6)
    assert not errs, "\n".join(errs[:10])


def test_adversarial_object_ops_hip():
    """Object operations only, garbage re-installed every 4 steps."""
    w = [0] * 20 + [1] * 8 + [0] * 7
    for flags in (0, HOT):
        errs = A.adversarial_compare(B.HipBackend, O.o2arc_ops(), 30, 30, N=8192, S=12, seed=17 + flags, flags=flags, op_weights=w,
                                     restate_every=4)
        assert not errs, "\n".join(errs[:10])


def test_adversarial_exotic_and_int8_masks_hip():
    from oracle import refdriver as RD
    errs = A.adversarial_compare(B.HipBackend, RD.variant_table("o2arc_exotic")[1], 30, 30, N=8192, S=10, seed=3,
                                 op_weights=[1] * 20 + [4] * 8 + [2] * 7)
    assert not errs, "\n".join(errs[:10])
    for flags in (0, HOT):
        errs = A.adversarial_compare(B.HipBackend, O.o2arc_ops(), 30, 30, N=2048, S=8, seed=5 + flags, flags=flags, int8_masks=True)
        assert not errs, "\n".join(errs[:10])


# bench.py's c3 stream (make_batch seed 1000, make_actions seed 2000), 40 warm-up launches, then 40 counted launches: the figures of
# the parent commit, whose kernel stored every plane it wrote in full (arcle_get_accounting_ex, summed over the 40 launches)
PARENT_ALG_BYTES = 860071396
PARENT_ISSUED_BYTES = 790694912


def test_accounting_on_bench_stream():
    import torch
    import bench
    dev = torch.device("cuda:0")
    n, K, W = 8192, 40, 40
    batch = bench.make_batch(dev, n)
    bbox, op = bench.make_actions(K + W, n, 2000)
    bb, oo = torch.as_tensor(bbox, device=dev), torch.as_tensor(op, device=dev)
    FL = batch.elide_flag | bench.STEP_AUTORESET
    assert FL == HOT
    sh = torch.cuda.current_stream(dev).cuda_stream
    for i in range(W):
        batch.step_bbox_ptr(bb[i].data_ptr(), oo[i].data_ptr(), FL, sh)
    torch.cuda.synchronize(dev)
    batch.enable_accounting(True)
    batch.accounting_ex(clear=True)
    for i in range(W, W + K):
        batch.step_bbox_ptr(bb[i].data_ptr(), oo[i].data_ptr(), FL, sh)
    torch.cuda.synchronize(dev)
    alg, issued, steps = batch.accounting_ex(clear=True)
    batch.enable_accounting(False)
    assert steps == K * n
    assert alg == PARENT_ALG_BYTES  # the algorithmic (semantic) count does not move
    assert issued < 0.9 * PARENT_ISSUED_BYTES, (issued, PARENT_ISSUED_BYTES)  # measured: 666.0 MB vs 790.7 MB
