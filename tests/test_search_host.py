"""beam_search's host logic — dedup, the visited set, integer ranking, tie-break, the returned sequence — on a stub vec env backed by
the oracle and the NumPy hash (torch CPU tensors; no GPU), and the planted-task generator the GPU test uses."""
import numpy as np
import torch

import backends as B
import search as SR
from arcle_amd import search as S
from oracle import oracle as O

H = W = 10


def _venv(tasks):
    inputs, idims, answers, adims, actions, seqs = tasks
    return SR.OracleVenv("o2arc", H, W, 3, O.o2arc_ops(), answers, adims)


def _roots(tasks):
    inputs, idims, answers, adims, actions, seqs = tasks
    orc = B.OracleBackend(len(inputs), H, W, 3, "o2arc", O.o2arc_ops())
    orc.set_tasks(inputs, idims, answers, adims)
    orc.reset()
    return torch.from_numpy(B.state_rows(orc))


def _actions(tasks, keep=None):
    a = tasks[4]
    idx = np.arange(len(a["operation"])) if keep is None else np.asarray(keep)
    return {"bbox": torch.from_numpy(a["bbox"][idx]), "operation": torch.from_numpy(a["operation"][idx])}


TASKS = None


def tasks3():
    global TASKS
    if TASKS is None:
        TASKS = SR.planted_tasks(3, seed=7)
    return TASKS


def test_planted_tasks_are_three_deep():
    inputs, idims, answers, adims, actions, seqs = tasks3()
    for n in range(len(inputs)):
        assert SR.replay_on_oracle(inputs[n], idims[n], answers[n], adims[n], actions, seqs[n]) == 1
        for cut in (seqs[n][:2], seqs[n][:1], []):
            assert SR.replay_on_oracle(inputs[n], idims[n], answers[n], adims[n], actions, cut) == 0


def test_beam_search_finds_the_planted_sequence_in_a_small_set():
    """A candidate set of 12 actions that contains the planted three: exhaustive width, the returned sequence replays to reward 1 on
    the oracle, and the counts obey their bounds."""
    tasks = tasks3()
    inputs, idims, answers, adims, actions, seqs = tasks
    venv, roots = _venv(tasks), _roots(tasks)
    for n in range(len(inputs)):
        rng = np.random.default_rng(n)
        others = [k for k in rng.permutation(64) if k not in seqs[n]][:9]
        keep = sorted(others + seqs[n])
        res = S.beam_search(venv, roots[n:n + 1], _actions(tasks, keep), width=144, depth=3, src_env=torch.tensor([n]))
        assert res.sequence is not None and len(res.sequence) == 3 and res.root == 0
        seq = [keep[k] for k in res.sequence]
        assert SR.replay_on_oracle(inputs[n], idims[n], answers[n], adims[n], actions, seq) == 1
        (e1, d1, k1), (e2, d2, k2), (e3, d3, k3) = res.counts
        assert e1 == 12 and d1 <= 12 and k1 == d1 and e2 == 12 * k1 and d2 <= e2 and k2 == d2 and e3 == 12 * k2 and k3 == 0
        again = S.beam_search(venv, roots[n:n + 1], _actions(tasks, keep), width=144, depth=3, src_env=torch.tensor([n]))
        assert again == res  # deterministic
        assert S.beam_search(venv, roots[n:n + 1], _actions(tasks, keep), width=144, depth=2, src_env=torch.tensor([n])).sequence is None


class _Scripted:
    """A venv whose expansion is a table: checks the host logic of one depth in isolation."""

    def __init__(self, status, hash_, dense, parent_hash):
        from arcle_amd.engine import Expansion
        M, K = status.shape
        self.ex = Expansion(torch.zeros((M, K), dtype=torch.int32), torch.zeros((M, K), dtype=torch.uint8), status,
                            torch.stack([hash_, hash_], 2), dense, torch.stack([parent_hash, parent_hash], 1))
        self.transitions = []

    def hash_rows(self, rows):
        return self.ex.parent_hash

    def expand(self, rows, action, src_env=None):
        return self.ex

    def transition(self, rows, action, src_env=None):
        self.transitions.append((rows.clone(), action["operation"].clone(), src_env.clone()))
        return rows[:0], None, None  # (an empty frontier ends the search after this depth)


def test_one_depth_dedup_ranking_and_tie_break():
    # 2 parents (hashes 100, 200), 5 actions.  Children: status bit; hash == parent; seen (== the other root); duplicates inside the batch
    status = torch.tensor([[0, 8, 0, 0, 0], [0, 0, 0, 0, 1]], dtype=torch.uint8)
    hash_ = torch.tensor([[100, 7, 200, 11, 12], [11, 13, 14, 12, 15]], dtype=torch.int64)
    #         (0,0) = parent  (0,1) status  (0,2) seen root  (0,3) h11  (0,4) h12 | (1,0) dup of 11  (1,1) h13  (1,2) h14  (1,3) dup of 12  (1,4) status
    dense = torch.tensor([[[0, 0], [9, 9], [9, 10], [1, 2], [2, 4]], [[9, 10], [3, 6], [2, 3], [9, 10], [9, 9]]], dtype=torch.int32)
    v = _Scripted(status, hash_, dense, torch.tensor([100, 200], dtype=torch.int64))
    rows = torch.arange(2, dtype=torch.int8).reshape(2, 1)
    acts = {"bbox": torch.zeros((5, 4), dtype=torch.int32), "operation": torch.arange(5, dtype=torch.int32)}
    res = S.beam_search(v, rows, acts, width=3, depth=2, src_env=torch.tensor([4, 5]))
    # distinct new states: children 3 (h11), 4 (h12), 6 (h13), 7 (h14); scores 1/2, 2/4, 3/6, 2/3 -> 7 first, then the three-way tie
    # by child index: 3, 4 (6 is cut)
    assert res.sequence is None and res.counts == [(10, 4, 3)]
    (prow, pop, psrc), = v.transitions
    assert prow.reshape(-1).tolist() == [0, 0, 1] and pop.tolist() == [3, 4, 2] and psrc.tolist() == [4, 4, 5]


def test_goal_is_the_lowest_child_with_correct_equal_total():
    status = torch.zeros((2, 3), dtype=torch.uint8)
    hash_ = torch.tensor([[1, 2, 3], [4, 5, 6]], dtype=torch.int64)
    dense = torch.tensor([[[1, 2], [0, 0], [1, 2]], [[5, 6], [6, 6], [6, 6]]], dtype=torch.int32)
    v = _Scripted(status, hash_, dense, torch.tensor([100, 200], dtype=torch.int64))
    acts = {"point": torch.zeros((3, 2), dtype=torch.int32), "operation": torch.arange(3, dtype=torch.int32)}
    res = S.beam_search(v, torch.zeros((2, 1), dtype=torch.int8), acts, width=8, depth=3)
    assert res.sequence == [1] and res.root == 1 and res.counts == [(6, 6, 0)]  # (0, 0) = "no dense term" is no goal


def test_integer_ranking_key_orders_like_the_fractions():
    from fractions import Fraction
    rng = np.random.default_rng(0)
    t = rng.integers(1, 16130, 4000)
    c = (rng.random(4000) * (t + 1)).astype(np.int64)
    key = (torch.from_numpy(c) << 32) // torch.from_numpy(t)
    order = np.argsort(-key.numpy(), kind="stable")
    fr = [Fraction(int(a), int(b)) for a, b in zip(c, t)]
    want = sorted(range(4000), key=lambda i: (-fr[i], i))
    assert order.tolist() == want
