"""The host side of the object proposals: components_numpy against the reference's dfs (tests/golden/components/components.npz), object_actions,
and beam_search(propose=...) on a stub vec env backed by the oracle (torch CPU tensors; no GPU)."""
import numpy as np
import pytest
import torch

import backends as B
import components as CP
import search as SR
from arcle_amd import search as S
from arcle_amd.envs.vec import Components
from oracle import oracle as O


@pytest.mark.parametrize("skip", CP.SKIPS)
def test_components_numpy_equals_the_reference_dfs(skip):
    """Descriptors, order, masks and `left` of every fixture grid; a cut list (C = 5) is the prefix, and `left` the cells of the rest."""
    for c in CP.fixture():
        want, label = c["want"][skip]
        n, left, comp, masks = S.components_numpy(c["grid"], c["dim"], 1024, skip)
        assert (n, left) == (len(want), 0), c["name"]
        assert np.array_equal(comp[:n], want), c["name"]
        assert not comp[n:].any() and not masks[n:].any()
        got_label = np.full(label.shape, -1, np.int16)
        for k in range(n):
            assert (got_label[masks[k] != 0] == -1).all()
            got_label[masks[k] != 0] = k
        assert np.array_equal(got_label, label), c["name"]
        n5, left5, comp5, masks5 = S.components_numpy(c["grid"], c["dim"], 5, skip)
        assert n5 == min(5, len(want)) and np.array_equal(comp5[:n5], want[:n5]) and left5 == int(want[n5:, 7].sum()), c["name"]
        assert np.array_equal(masks5[:n5], masks[:n5])


def test_fixture_covers_what_the_issue_lists():
    by_name = {c["name"]: c for c in CP.fixture()}
    assert len(by_name["30x30 one dim 30x30"]["want"][-1][0]) == 1
    assert len(by_name["30x30 checker dim 30x30"]["want"][-1][0]) == 900
    assert len(by_name["8x127 altcols dim 8x127"]["want"][-1][0]) == 127
    assert {(30, 30), (32, 32), (12, 12), (5, 5), (1, 1), (64, 16), (40, 20), (127, 8), (100, 10), (8, 127), (25, 40)} == set(CP.sizes())
    # wrap: (i, W-1) and (i+1, 0) are two one-cell components of colour 5
    for name in ("30x30 wrap", "25x40 wrap dim 25x40"):
        comp = by_name[name]["want"][-1][0]
        assert (comp[comp[:, 6] == 5][:, 7] == 1).all() and (comp[:, 6] == 5).sum() >= 2
    # cells outside grid_dim join nothing and are not counted
    c = by_name["30x30 outside dim 7x9"]
    assert int(c["want"][-1][0][:, 7].sum()) == 7 * 9 and (c["want"][-1][1][7:, :] == -1).all() and (c["want"][-1][1][:, 9:] == -1).all()


def _components_of(grids, dims, C, skip):
    M = len(grids)
    count, left, comp = np.zeros(M, np.int32), np.zeros(M, np.int32), np.zeros((M, C, 8), np.int32)
    for m in range(M):
        count[m], left[m], comp[m], _ = S.components_numpy(grids[m], dims[m], C, skip)
    t = torch.from_numpy(comp)
    return Components(torch.from_numpy(count), torch.from_numpy(left), t[:, :, 0:4], t[:, :, 4:6], t[:, :, 6], t[:, :, 7], None)


def test_object_actions_shapes_padding_and_seed_boxes():
    cases = [c for c in CP.cases_of(12, 12) if "sparse" in c["name"] or "one" in c["name"] or "diagonal" in c["name"]]
    C = 6
    comp = _components_of([c["grid"] for c in cases], [c["dim"] for c in cases], C, 0)
    box_ops, seed_ops = [20, 21, 24], [10, 15]
    a = S.object_actions(comp, box_ops, seed_ops)
    M, per = len(cases), 5
    assert tuple(a["bbox"].shape) == (M, C * per, 4) and a["bbox"].dtype == torch.int32 and a["bbox"].is_contiguous()
    assert tuple(a["operation"].shape) == (M, C * per) and a["operation"].dtype == torch.int32
    bb, op = a["bbox"].reshape(M, C, per, 4).numpy(), a["operation"].reshape(M, C, per).numpy()
    assert int(comp.count.min()) < C <= int(comp.count.max()) + 5  # both full and padded rows are in the batch
    for m in range(M):
        n = int(comp.count[m])
        assert (op[m, n:] == -1).all() and (op[m, :n] == np.array(box_ops + seed_ops)).all()
        for k in range(n):
            assert (bb[m, k, :3] == comp.box[m, k].numpy()).all()
            sx, sy = comp.seed[m, k].tolist()
            assert (bb[m, k, 3:] == np.array([sx, sy, sx, sy])).all()


class ObjectVenv(SR.OracleVenv):
    """SR.OracleVenv with a candidate set PER ROW and `components`: what beam_search(propose=...) needs of a vec env.  Slots with
    operation -1 are answered as the device answers them — ARCLE_ST_BAD_OP, the child is its parent — without asking the oracle."""

    def expand(self, rows, action, src_env=None):
        from arcle_amd.engine import Expansion
        pay, op = action["bbox"].numpy(), action["operation"].numpy()
        assert pay.ndim == 3
        M, K = op.shape
        rows_n = rows.numpy()
        src = np.arange(M) if src_env is None else src_env.numpy()
        pad = op < 0
        w = SR.oracle_expand(rows_n, self.answers[src], self.adims[src], self.kind, self.H, self.W, self.mt, self.ops, "bbox",
                             np.where(pad[..., None], 0, pay).astype(np.int32), np.where(pad, 0, op).astype(np.int32))
        w["status"][pad] = SR.ST_BAD_OP
        w["rows"][pad] = np.broadcast_to(rows_n[:, None, :], w["rows"].shape)[pad]
        h = S.hash_rows_numpy(w["rows"].reshape(M * K, -1), self.kind, self.H, self.W).view(np.int64).reshape(M, K, 2)
        return Expansion(torch.from_numpy(w["reward"].astype(np.int32)), torch.from_numpy(w["term"].astype(np.uint8)),
                         torch.from_numpy(w["status"]), torch.from_numpy(h), torch.from_numpy(w["dense"]), self.hash_rows(rows))

    def components(self, rows, max_components=32, skip_color=-1, bits=False):
        P, off = self.H * self.W, 0
        for f, ln in B.row_layout(self.kind, P):
            if f == "grid":
                g = rows.numpy()[:, off:off + P + 2]
            off += ln
        return _components_of(g[:, :P].reshape(-1, self.H, self.W), g[:, P:], max_components, skip_color)


def test_beam_search_with_object_proposals_solves_the_planted_task():
    inputs, dims, answers, seqs = CP.planted_object_tasks(3)
    rows, _ = CP.clean_rows("o2arc", inputs, dims, answers, dims)
    venv = ObjectVenv("o2arc", 12, 12, 3, O.o2arc_ops(), answers, dims)
    propose = S.propose_objects(CP.MOVE_OPS, CP.FLOODFILL_OPS, max_components=3, skip_color=0)
    for n in range(len(inputs)):
        res = S.beam_search(venv, torch.from_numpy(rows[n:n + 1]), None, width=16, depth=2, src_env=torch.tensor([n]), propose=propose)
        assert res.sequence is not None and len(res.sequence) == 2 and res.root == 0, n
        assert all(len(a) == 5 for a in res.sequence)
        _, orc = CP.clean_rows("o2arc", inputs[n:n + 1], dims[n:n + 1], answers[n:n + 1], dims[n:n + 1])
        for a in res.sequence:
            orc.step("bbox", np.array([a[:4]], np.int32), np.array([a[4]], np.int32))
        assert np.array_equal(orc.get("grid")[0], answers[n]), (n, res.sequence, seqs[n])
        assert res.counts[0][0] == 3 * 14 and len(res.counts) == 2


# what beam_search returned on the parent commit for the three planted tasks of tests/test_search_host.py (seed 7, the 12 kept actions,
# width 144 and width 5, depth 3): (sequence, counts, root) twice per task, recorded from that commit; the additive `propose` argument must not move any of it
PARENT_RESULTS = [([5, 9, 11], [(12, 9, 9), (108, 51, 51), (612, 236, 0)], 0, [5, 9, 11], [(12, 9, 5), (60, 33, 5), (60, 34, 0)], 0),
                  ([7, 1, 11], [(12, 9, 9), (108, 77, 77), (924, 501, 0)], 0, [7, 11, 1], [(12, 9, 5), (60, 45, 5), (60, 39, 0)], 0),
                  ([0, 1, 8], [(12, 9, 9), (108, 63, 63), (756, 352, 0)], 0, [0, 1, 8], [(12, 9, 5), (60, 38, 5), (60, 38, 0)], 0)]


def test_beam_search_without_propose_is_the_parent_commits():
    import test_search_host as TH
    tasks = TH.tasks3()
    inputs, idims, answers, adims, actions, seqs = tasks
    venv, roots = TH._venv(tasks), TH._roots(tasks)
    got = []
    for n in range(len(inputs)):
        rng = np.random.default_rng(n)
        others = [k for k in rng.permutation(64) if k not in seqs[n]][:9]
        keep = sorted(others + seqs[n])
        res = S.beam_search(venv, roots[n:n + 1], TH._actions(tasks, keep), width=144, depth=3, src_env=torch.tensor([n]))
        pruned = S.beam_search(venv, roots[n:n + 1], TH._actions(tasks, keep), width=5, depth=3, src_env=torch.tensor([n]))
        got.append((res.sequence, [tuple(c) for c in res.counts], res.root, pruned.sequence, [tuple(c) for c in pruned.counts], pruned.root))
    print(got)
    assert got == PARENT_RESULTS
