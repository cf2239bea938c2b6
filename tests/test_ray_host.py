"""arcle_amd.search.ray_numpy — the mirror every ray test compares against — pinned on the oracle's own Color step, the fill rules on
hand-made grids, ray_actions / propose_rays, and the planted tasks on the oracle-backed stub vec env.  No GPU."""
import numpy as np
import pytest
import torch

import align as AL
import components as CP
import objects as OB
import ray as RY
from arcle_amd import search as S
from arcle_amd.envs.vec import Rays

N_, S_, W_, E_, NW_, NE_, SW_, SE_ = 1, 2, 4, 8, 16, 32, 64, 128


def cast(grid, mask, sets, answer=None, dim=None, adim=None, free_color=0, through=False):
    grid = np.asarray(grid, np.int8)
    answer = grid if answer is None else np.asarray(answer, np.int8)
    ray, best, base, cells = S.ray_numpy(grid, grid.shape if dim is None else dim, answer, answer.shape if adim is None else adim, np.asarray(mask)[None], sets,
                                         free_color, through, full=True)
    return ray[0], best[0], base, cells[0]


@pytest.mark.parametrize("kind", ("o2arc", "arc"))
@pytest.mark.parametrize("H,W", RY.ORACLE_SIZES)
def test_mirror_equals_the_oracles_color_step(H, W, kind):
    """Every case of the size (grid_dim below the plane in the shrunk cases), every object, each of the 13 default sets, both `through`
    values, all ten colours: the oracle runs `Color c` on the mirror's cells of the candidate; the dense pair's first number for the
    reported colour is `correct`, the reported colour is the first arg-max over the ten children, and the children's differences are
    the differences of the answer's colour counts under the cells (`right`)."""
    seen = 0
    for case in RY.cases_of(H, W):
        gh, gw = (int(v) for v in case["dim"])
        mh, mw = min(gh, int(case["adim"][0])), min(gw, int(case["adim"][1]))
        for through in (False, True):
            dense, (ray, best, base, cells) = RY.oracle_children(case, RY.DEFAULT, through, kind)
            for k in range(len(ray)):
                for s in range(len(RY.DEFAULT)):
                    color, correct, n, right = (int(v) for v in ray[k, s])
                    if n == 0:
                        assert (dense[k, s] == -1).all() and (color, correct, right) == (0, base[0], 0), (case["name"], k, s)
                        continue
                    assert not cells[k, s][gh:].any() and not cells[k, s][:, gw:].any() and int(cells[k, s].sum()) == n
                    d = dense[k, s]
                    assert correct == d[color] and color == int(np.argmax(d)), (case["name"], through, k, s, ray[k, s], d)
                    under = case["answer"][:mh, :mw][cells[k, s][:mh, :mw]]
                    freq = np.array([(under == c).sum() for c in range(10)])
                    assert right == freq[color] and np.array_equal(d - d[color], freq - right), (case["name"], through, k, s)
                    seen += 1
    assert seen > 100


def test_a_ray_stops_in_front_of_an_obstacle_and_runs_over_it_with_through():
    g = np.zeros((5, 7), np.int8)
    g[2, 1], g[2, 4] = 3, 8
    ray, best, base, cells = cast(g, g == 3, [E_, W_, N_ | S_])
    assert np.argwhere(cells[0]).tolist() == [[2, 2], [2, 3]] and np.argwhere(cells[1]).tolist() == [[2, 0]]
    assert np.argwhere(cells[2]).tolist() == [[0, 1], [1, 1], [3, 1], [4, 1]]
    ray, best, base, cells = cast(g, g == 3, [E_], through=True)
    assert np.argwhere(cells[0]).tolist() == [[2, 2], [2, 3], [2, 4], [2, 5], [2, 6]]
    # painting over the obstacle costs the cell that was right: base - 1 + the zeros under the ray (the answer is the grid itself)
    assert ray[0].tolist() == [0, 35 - 1, 5, 4] and base == (35, 35)


def test_no_ray_wraps_into_the_next_row_or_column():
    H, W = 4, 5
    g = np.zeros((H, W), np.int8)
    g[1, W - 1] = 2  # on the right edge
    _, _, _, cells = cast(g, g == 2, [E_, NE_, SE_, W_])
    assert not cells[0].any() and not cells[1].any() and not cells[2].any() and np.argwhere(cells[3]).tolist() == [[1, 0], [1, 1], [1, 2], [1, 3]]
    g = np.zeros((H, W), np.int8)
    g[2, 0] = 2  # on the left edge
    _, _, _, cells = cast(g, g == 2, [W_, NW_, SW_, S_ | N_])
    assert not cells[0].any() and not cells[1].any() and not cells[2].any() and np.argwhere(cells[3]).tolist() == [[0, 0], [1, 0], [3, 0]]
    g = np.zeros((H, W), np.int8)
    g[0, 2], g[H - 1, 1] = 2, 3  # top and bottom edges
    _, _, _, cells = cast(g, g == 2, [N_, NW_, NE_])
    assert not cells.any()
    _, _, _, cells = cast(g, g == 3, [S_, SW_, SE_, NE_])
    assert not cells[:3].any() and np.argwhere(cells[3]).tolist() == [[0, 4], [1, 3], [2, 2]]


def test_no_cell_at_or_beyond_grid_dim():
    g = np.zeros((6, 6), np.int8)
    g[1, 1] = 4
    g[4:, :], g[:, 3:] = 0, 0  # (free bytes beyond grid_dim: still not entered)
    ray, _, base, cells = cast(g, g == 4, [0xff], dim=(4, 3), adim=(4, 3))
    assert not cells[0][4:].any() and not cells[0][:, 3:].any()
    assert sorted(np.argwhere(cells[0]).tolist()) == sorted([[0, 1], [2, 1], [3, 1], [1, 0], [1, 2], [0, 0], [0, 2], [2, 0], [2, 2]])
    m = np.zeros((6, 6), bool)
    m[1, 1] = m[5, 5] = m[1, 4] = True  # the mask's cells outside grid_dim are ignored: nothing starts there
    ray2, _, _, cells2 = cast(g, m, [0xff], dim=(4, 3), adim=(4, 3))
    assert np.array_equal(cells2, cells) and np.array_equal(ray2, ray)


def test_an_l_shape_casts_from_every_top_cell_but_not_through_its_own_cells():
    g = np.zeros((6, 6), np.int8)
    g[3, 1] = g[4, 1] = g[4, 2] = g[4, 3] = 4  # an L: a column of two on a row of three
    _, _, _, cells = cast(g, g == 4, [N_, E_, S_])
    assert sorted(np.argwhere(cells[0]).tolist()) == sorted([[0, 1], [1, 1], [2, 1], [0, 2], [1, 2], [2, 2], [3, 2], [0, 3], [1, 3], [2, 3], [3, 3]])
    assert sorted(np.argwhere(cells[1]).tolist()) == sorted([[3, 2], [3, 3], [3, 4], [3, 5], [4, 4], [4, 5]])  # (3, 1)'s ray is not cut by the L itself: it runs beside it
    assert sorted(np.argwhere(cells[2]).tolist()) == [[5, 1], [5, 2], [5, 3]]
    ring = np.zeros((6, 6), np.int8)
    ring[1:4, 1:4] = 6
    ring[2, 2] = 0
    _, _, _, cells = cast(ring, ring == 6, [E_])
    assert sorted(np.argwhere(cells[0]).tolist()) == sorted([[1, 4], [1, 5], [2, 2], [2, 4], [2, 5], [3, 4], [3, 5]])  # the free hole is crossed
    ring[2, 2] = 9
    _, _, _, cells = cast(ring, ring == 6, [E_])
    assert [2, 2] not in np.argwhere(cells[0]).tolist() and int(cells[0].sum()) == 6  # an obstacle in the hole is not


def test_free_color_empty_objects_and_zero_sets():
    g = np.full((4, 6), 5, np.int8)
    g[1, 1], g[1, 4] = 2, 0
    ray, best, base, cells = cast(g, g == 2, [E_], free_color=5)
    assert np.argwhere(cells[0]).tolist() == [[1, 2], [1, 3]]  # the 0 is an obstacle now
    ray, best, base, cells = cast(g, g == 2, [E_], free_color=0)
    assert not cells.any() and ray[0].tolist() == [0, base[0], 0, 0] and best.tolist() == [-1, 0, base[0], 0]
    g2 = g.copy()
    g2[1, 2] = -3
    _, _, _, cells = cast(g2, g2 == 2, [E_, W_], free_color=-3)
    assert np.argwhere(cells[0]).tolist() == [[1, 2]] and not cells[1].any()
    _, _, _, cells = cast(g2, g2 == 2, [E_], free_color=253)  # (the same byte as int8)
    assert np.argwhere(cells[0]).tolist() == [[1, 2]]
    ray, best, base, cells = cast(g, np.zeros_like(g), list(S.RAY_SETS), free_color=5)  # empty B
    assert not cells.any() and (ray == np.array([0, base[0], 0, 0])).all() and best.tolist() == [-1, 0, base[0], 0]
    ray, best, base, cells = cast(g, g == 2, [0, W_, 0], free_color=5)  # zero sets are empty candidates, not errors
    assert ray[0].tolist() == [0, base[0], 0, 0] == ray[2].tolist() and ray[1, 2] == 1 and best[0] == 1


def test_tie_rules_for_colour_and_best():
    g = np.zeros((3, 7), np.int8)
    g[1, 3] = 1
    ans = g.copy()
    ans[1, :3], ans[1, 4:] = (7, 4, 4), (4, 7, 7)  # west: 7 4 4; east: 4 7 7
    ray, best, base, _ = cast(g, g == 1, [W_, E_, W_ | E_, N_, S_ | N_], answer=ans)
    assert ray[0].tolist() == [4, base[0] + 2, 3, 2] and ray[1].tolist() == [7, base[0] + 2, 3, 2]
    assert ray[2].tolist() == [4, base[0] + 3, 6, 3]  # 4 and 7 three times each: the smaller colour
    assert best.tolist() == [2, 4, base[0] + 3, 6]
    ray, best, base, _ = cast(g, g == 1, [W_ | E_ | N_, W_ | E_, E_ | W_], answer=ans)
    assert [r[1] for r in ray.tolist()] == [base[0] + 3 - 1] + [base[0] + 3] * 2  # (N paints a cell that was right)
    assert best.tolist() == [1, 4, base[0] + 3, 6]  # equal correct and cells: the lower set
    ray, best, base, _ = cast(g, g == 1, [W_ | E_ | S_ | N_, N_], answer=np.where(ans == 0, 4, ans))
    assert ray[0].tolist() == [4, base[0] + 5, 8, 5] and ray[1].tolist() == [4, base[0] + 1, 1, 1] and best[0] == 0
    ans2 = g.copy()
    ans2[1, 4] = 4
    ray, best, base, _ = cast(g, g == 1, [E_ | N_, E_], answer=ans2, through=False)
    # both leave exactly the base's correct cells (Color 0 repaints what was 0): the candidate with fewer cells wins
    assert ray[1].tolist() == [0, base[0], 3, 2] and best.tolist() == [1, 0, base[0], 3]


def _objs_and_rays(sets=None):
    cases = [c for c in RY.cases_of(7, 6) if c["dim"].tolist() == [7, 6]]
    grids, dims = np.stack([c["grid"] for c in cases]), np.stack([c["dim"] for c in cases])
    objs = OB.objects_numpy(grids, dims, 6, 0, True, True, True, False)
    rays = RY.ray_numpy_rows(grids, dims, np.stack([c["answer"] for c in cases]), np.stack([c["adim"] for c in cases]), objs, sets, 0, False)
    return cases, objs, rays


def test_ray_actions_shapes_padding_and_drop_rule():
    cases, objs, rays = _objs_and_rays()
    assert isinstance(rays, Rays) and Rays._fields == ("color", "correct", "cells", "right", "best_set", "best_color", "best_correct", "best_cells", "best_bits", "base")
    M, C = len(cases), 6
    assert tuple(rays.color.shape) == (M, C, 13) and tuple(rays.best_set.shape) == (M, C) and tuple(rays.best_bits.shape) == (M, C, 128)
    ops = [40 + c for c in range(10)]
    act = S.ray_actions(objs, rays, ops)
    assert set(act) == {"bits", "operation"} and tuple(act["bits"].shape) == (M, C, 128) and act["bits"].dtype == torch.uint8
    assert tuple(act["operation"].shape) == (M, C) and act["operation"].dtype == torch.int32
    real = 0
    for m in range(M):
        for k in range(C):
            if k >= int(objs.count[m]) or int(rays.best_set[m, k]) < 0 or int(rays.best_correct[m, k]) <= int(rays.base[m, 0]):
                assert int(act["operation"][m, k]) == -1 and not act["bits"][m, k].any(), (m, k)
                continue
            real += 1
            assert int(act["operation"][m, k]) == 40 + int(rays.best_color[m, k]) and torch.equal(act["bits"][m, k], rays.best_bits[m, k])
            assert int(S.unpack_bits(act["bits"][m, k], 7, 6).sum()) == int(rays.best_cells[m, k]) > 0
    assert 2 <= real < M * C


def test_propose_rays_singles_first_then_the_rays():
    inputs, dims, answers, depths = RY.planted_ray_tasks(3)
    rows = torch.from_numpy(CP.clean_rows("o2arc", inputs, dims, answers, dims)[0])
    venv = RY.ray_venv(answers, dims)
    prop = S.propose_rays(range(10), box_ops=[3, 25], seed_ops=[12], max_components=8)
    assert prop.wants_src is True
    cand = prop(venv, rows, torch.arange(3, dtype=torch.int32))
    objs = venv.components(rows, max_components=8, skip_color=0, bits=True)
    single = S.object_actions(objs, [3, 25], [12], masks=True)
    K1 = 8 * 3
    assert set(cand) == {"bits", "operation"} and tuple(cand["bits"].shape) == (3, K1 + 8, 128) and tuple(cand["operation"].shape) == (3, K1 + 8)
    assert torch.equal(cand["bits"][:, :K1], single["bits"]) and torch.equal(cand["operation"][:, :K1], single["operation"])
    for i in range(3):
        n = int(objs.count[i])
        assert bool((cand["operation"][i, K1 + n:] == -1).all()) and not cand["bits"][i, K1 + n:].any()
        seeds = [k for k in range(n) if int(objs.color[i, k]) != 8]
        assert len(seeds) == depths[i] and all(int(cand["operation"][i, K1 + k]) == int(objs.color[i, k]) for k in seeds)  # Color <the seed's colour>
    only = S.propose_rays(range(10), max_components=8)(venv, rows, None)
    assert all(torch.equal(only[k], cand[k][:, K1:]) for k in only)
    none = S.propose_rays(range(10), sets=[0, 0], max_components=8)(venv, rows, None)
    assert bool((none["operation"] == -1).all()) and not none["bits"].any()


def test_beam_search_draws_the_planted_lines():
    """Eight planted 12 x 12 tasks — 1 to 3 one-cell seeds whose rays (cross, diagonal cross, star, N|S, W|E, E) the answer holds,
    stopped by obstacles: propose_rays(range(10)) at width 1 and depth = the number of seeds solves all eight, one Color step per
    seed, and the steps replay to the answer on the oracle.  The five proposers the library had solve none at the same width and
    depth: none of their steps adds more cells than an object already has (a copy doubles at most: 1 + 2 + 4 over three steps),
    and every answer holds at least 12 new cells."""
    inputs, dims, answers, depths = RY.planted_ray_tasks(8)
    assert sorted(set(depths)) == [1, 2, 3] and all(int(((a != 0) & (g == 0)).sum()) >= 12 for g, a in zip(inputs, answers))
    rows_np = CP.clean_rows("o2arc", inputs, dims, answers, dims)[0]
    rows = torch.from_numpy(rows_np)
    venv = RY.ray_venv(answers, dims)
    cast_, before = RY.searches(venv, rows, 8, depths)
    assert sum(r.sequence is not None for r in cast_) == 8
    assert set(before) == {"objects", "placements", "stamps", "turns", "alignments"}
    assert {name: sum(r.sequence is not None for r in res) for name, res in before.items()} == {name: 0 for name in before}
    for i, r in enumerate(cast_):
        assert r.root == 0 and len(r.sequence) == depths[i], i
        assert sorted(op for _, op in r.sequence) == sorted(int(v) for v in np.unique(inputs[i]) if v not in (0, 8)), i
        assert AL.replay_on_oracle(rows_np[i], answers[i], dims[i], r.sequence) == 1, i
