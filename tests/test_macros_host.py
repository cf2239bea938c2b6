"""The macro side of arcle_amd.search on the host, over the oracle-backed stub vec env of tests/macros.py: run_macros (what
ARCVecEnv.transition_macros runs), object_macros, and beam_search with macro candidates on the stamp tasks — which the single-step
beam cannot solve."""
import numpy as np
import torch

import macros as MC
from arcle_amd import search as S
from oracle import oracle as O


def test_transition_macros_host_logic_equals_the_chained_oracle():
    errs = MC.materialisation_host()
    assert not errs, "\n".join(errs[:10])


def _stub():
    inputs, dims, answers, steps = MC.stamp_tasks()
    venv = MC.MacroVenv("o2arc", 10, 10, 3, O.o2arc_ops(), answers, dims)
    return inputs, dims, answers, steps, venv, torch.from_numpy(MC.stamp_rows(inputs, dims, answers))


def test_object_macros_layout():
    inputs, dims, answers, steps, venv, rows = _stub()
    C = 4
    comp = venv.components(rows, max_components=C, skip_color=0)
    assert comp.count.tolist() == [3] * 8  # marker, marker, plus — in row-major order of their seeds
    single = S.object_actions(comp, [MC.COPY_O], [5])
    mac = S.object_macros(comp, [MC.COPY_O], [5], [(MC.COPY_O, MC.PASTE), (7, 8)])
    K1, K = 2 * C, 2 * C + 2 * C * C
    assert mac["bbox"].shape == (8, K, 2, 4) and mac["operation"].shape == (8, K, 2) and mac["length"].shape == (8, K)
    assert mac["bbox"].dtype == torch.int32 and mac["operation"].dtype == torch.int32 and mac["length"].dtype == torch.int32
    # the singles first, as macros of length 1
    assert torch.equal(mac["bbox"][:, :K1, 0], single["bbox"]) and torch.equal(mac["operation"][:, :K1, 0], single["operation"])
    assert (mac["length"][:, :K1] == 1).all()
    # then every ordered pair (i, j), i-major, with every (op_a, op_b)
    box = comp.box.to(torch.int32)
    for i in range(C):
        for j in range(C):
            for q, (oa, ob) in enumerate(((MC.COPY_O, MC.PASTE), (7, 8))):
                k = K1 + (i * C + j) * 2 + q
                if i != j and i < 3 and j < 3:
                    assert torch.equal(mac["bbox"][:, k, 0], box[:, i]) and torch.equal(mac["bbox"][:, k, 1], box[:, j])
                    assert mac["operation"][:, k].tolist() == [[oa, ob]] * 8 and mac["length"][:, k].tolist() == [2] * 8
                else:
                    assert (mac["operation"][:, k, 0] == -1).all() and (mac["length"][:, k] == 1).all()
    # without pairs: T = 1
    one = S.object_macros(comp, [MC.COPY_O], [5], [])
    assert one["bbox"].shape == (8, K1, 1, 4) and torch.equal(one["operation"][:, :, 0], single["operation"])


def test_macros_solve_the_stamp_tasks_the_single_step_beam_cannot():
    inputs, dims, answers, steps, venv, rows = _stub()
    singles, macros = MC.stamp_searches(venv, rows, 8)
    # a lone CopyO changes only the clip: the dense score is the parent's, the width cut keeps the Copy of the first object
    assert [r.sequence for r in singles] == [None] * 8
    for n, res in enumerate(macros):
        assert res.sequence is not None and len(res.sequence) == 2, (n, res)
        assert [tuple(s) for s in res.sequence] == steps[n], (n, res.sequence, steps[n])
        assert MC.replay_steps_on_oracle(inputs[n], dims[n], answers[n], res.sequence) == 1, (n, res.sequence)
        assert res.counts == [(16 * 16, res.counts[0][1], 0)] and res.root == 0


def test_shared_macro_set_returns_indices():
    inputs, dims, answers, steps, venv, rows = _stub()
    n = 2
    a, b = steps[n]
    bbox = np.array([[(0, 0, 0, 0), (0, 0, 0, 0)], [a[:4], b[:4]], [b[:4], a[:4]]], np.int32)
    op = np.array([[MC.PASTE, MC.PASTE], [a[4], b[4]], [b[4], a[4]]], np.int32)
    acts = {"bbox": torch.from_numpy(bbox), "operation": torch.from_numpy(op), "length": torch.tensor([1, 2, 2], dtype=torch.int32)}
    res = S.beam_search(venv, rows[n:n + 1], acts, width=4, depth=2, src_env=torch.tensor([n]))
    assert res.sequence == [1] and res.counts[0][0] == 3
