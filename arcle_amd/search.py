"""Search over ARCLE action sequences on top of `ARCVecEnv.expand`: the NumPy mirror of the device's state hash, a plain beam
search, and the objects of a grid as candidate actions (`components_numpy`: the host mirror of arcle_components_rows;
`object_actions` / `propose_objects`: its descriptors as a per-state action set for `beam_search(propose=...)` — the objects'
bounding boxes, or with masks=True their exact cells as bit rows; `pack_bits` / `unpack_bits`: that layout in torch), and where each
object best fits the answer (`place_numpy`: the host mirror of arcle_place_rows; `placement_macros` / `propose_placements`: the
best translation of every object as ONE Move macro), and where a COPY of each object best fits it (`stamp_numpy`: the host mirror of
arcle_stamp_rows; `stamp_macros` / `propose_stamps`: the best paste position of every object as ONE CopyO + Paste macro), and the
lines each object casts toward the answer (`ray_numpy`: the host mirror of arcle_ray_rows; `ray_actions` / `propose_rays`: the best
set of rays of every object as ONE Color step), and the cells around and inside each object (`region_numpy`: the host mirror of
arcle_region_rows; `region_actions` / `propose_regions`: the best halo, box, frame or inside of every object as ONE Color step), and the grid or the
input zoomed, shrunk or tiled onto the answer's canvas (`scale_numpy`: the host mirror of arcle_scale_rows; `scale_macros` /
`propose_scales`: the best candidate of every source as ONE resize_grid + Color macro).

The hash is defined in include/arcle_hip.h (next to arcle_hash_rows) and computed on the device by arcle_amd/csrc/arcle_search.h;
`hash_rows_numpy` restates it on the host — the same arrangement as arcle_amd/sampling.py for the device RNG — and is what the tests
pin the device against."""
import collections

import numpy as np
import torch

# enum arcle_plane ids of the planes a state row carries, in the row's (FlattenObservation) order, and the record byte every scalar
# field of the row lands in (ARCLE_REC_*)
_PLANE_ID = {"input": 0, "grid": 1, "selected": 2, "clip": 3, "object": 4, "object_sel": 5, "background": 6}
BITS_STRIDE = 128  # bytes of a bit-packed selection mask (ARCLE_MAX_CELLS / 8)
_REC_OFF = {"input_dim": 0, "grid_dim": 2, "clip_dim": 4, "object_dim": 6, "object_pos": 8, "trials_remain": 10, "terminated": 11,
            "active": 12, "rotation_parity": 13}


def row_layout(kind, P):
    """(field, bytes) of a full state row of env kind "o2arc" | "arc" | "raw" with P = H * W cells, in row order."""
    lay = []
    if kind != "raw":
        lay += [("clip", P), ("clip_dim", 2)]
    lay += [("grid", P), ("grid_dim", 2), ("input", P), ("input_dim", 2)]
    if kind == "o2arc":
        lay += [("active", 1), ("background", P), ("object", P), ("object_dim", 2), ("object_pos", 2), ("object_sel", P),
                ("rotation_parity", 1), ("selected", P)]
    lay += [("terminated", 1), ("trials_remain", 1)]
    return lay


def _fa(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x85EBCA6B)
    x = x ^ (x >> np.uint32(13))
    x = x * np.uint32(0xC2B2AE35)
    return x ^ (x >> np.uint32(16))


def _fb(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def _terms(d, tag):
    """(A, B) term sums over the last axis of the dwords d [n, m] under the tags tag [m] (uint32, wrapping)."""
    with np.errstate(over="ignore"):
        a = _fa(d ^ (tag * np.uint32(0x9E3779B1)))
        b = _fb(d + tag * np.uint32(0x85EBCA77))
        return a.sum(1, dtype=np.uint32), b.sum(1, dtype=np.uint32)


def hash_rows_numpy(rows, kind, H, W):
    """(state_hash, grid_hash) of state rows, uint64 [n, 2]: the formula of include/arcle_hip.h.  rows: int8 / uint8 [n, >= L]."""
    rows = np.ascontiguousarray(np.asarray(rows)).view(np.uint8)
    n, P = rows.shape[0], H * W
    nd = (P + 3) // 4
    A, B = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    GA, GB = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    rec = np.zeros((n, 16), np.uint8)
    off = 0
    for f, ln in row_layout(kind, P):
        seg = rows[:, off:off + ln]
        off += ln
        if f in _PLANE_ID:
            padded = np.zeros((n, 4 * nd), np.uint8)
            padded[:, :P] = seg
            d = padded.view("<u4")
            tag = (np.uint32((_PLANE_ID[f] + 1) * 256) + np.arange(nd, dtype=np.uint32)).astype(np.uint32)
            a, b = _terms(d, tag)
            with np.errstate(over="ignore"):
                A, B = A + a, B + b
            if f == "grid":
                GA, GB = a, b
        else:
            rec[:, _REC_OFF[f]:_REC_OFF[f] + ln] = seg
    w = rec.view("<u4")
    a, b = _terms(w, np.uint32(0x0F00) + np.arange(4, dtype=np.uint32))
    ga, gb = _terms(w[:, :1] & np.uint32(0xFFFF0000), np.array([0x0E00], np.uint32))
    with np.errstate(over="ignore"):
        A, B, GA, GB = A + a, B + b, GA + ga, GB + gb
    out = np.empty((n, 2), np.uint64)
    out[:, 0] = A.astype(np.uint64) | (B.astype(np.uint64) << np.uint64(32))
    out[:, 1] = GA.astype(np.uint64) | (GB.astype(np.uint64) << np.uint64(32))
    return out


# sequence: the action indices (into the candidate set) of the first solution found, or None; root: the row of `rows` it starts
# from; counts: per depth (children expanded, distinct new states among them, states kept for the next depth)
BeamResult = collections.namedtuple("BeamResult", "sequence counts root")


def beam_search(venv, rows, actions, width, depth, src_env=None, propose=None):
    """Beam search over sequences drawn from ONE candidate action set, scored by the dense pair (correct cells / total cells).

    venv: anything with `expand(rows, action, src_env)`, `transition(rows, action, src_env)` and `hash_rows(rows)` as ARCVecEnv has
    them; rows int8 [M0, L] start states; actions = {"bbox": int32 [K,4] | "point": int32 [K,2] | "bits": uint8 [K,128] (bit-packed
    masks, `pack_bits`), "operation": int32 [K]}; src_env int32 [M0] = the env whose answer judges row m (default: env m).  Per depth: expand every frontier state by every action; drop
    children with a status bit and children whose state equals their parent's; drop states already seen (in an earlier depth, or
    twice in this one: the lowest child index stays); if a child's grid IS the answer (correct == total: exactly when a Submit
    would pay — with unequal dims the total exceeds the common rectangle — so the candidate set needs no Submit) return the action
    indices that lead to the lowest such child; else keep the `width` best by correct / total, ties to the lower child index, and
    materialise only those with `transition`.  Every tensor lives on rows.device.

    propose: a callable `propose(venv, frontier_rows) -> {"bbox": int32 [M, K, 4], "operation": int32 [M, K]}` called at every
    depth for a candidate set PER STATE (`propose_objects`: the connected components of each state's grid); `actions` may then be
    None, and BeamResult.sequence is the list of the 5-tuples (x1, y1, x2, y2, op) themselves — BBoxWrapper actions; an index into
    a per-state set names nothing.  Slots with operation -1 are padding: their children carry a status bit and are dropped.
    A propose that carries the attribute `wants_src = True` is called as `propose(venv, frontier_rows, src_env)`, src_env int32 [M] = the
    env whose answer judges each frontier row (`propose_placements` looks at the answer); every other propose gets two arguments.
    A propose that returns {"bits": uint8 [M, K, 128], "operation": ...} (`propose_objects(masks=True)`: each object's exact cells)
    makes the sequence a list of (selection, op), selection a bool NumPy array [H, W] (H, W = venv.H, venv.W): what the reference's
    `step({"selection": selection, "operation": op})` takes.

    Macro candidates — a "length" key in `actions` ({form: [K, T, w], "operation": [K, T], "length": [K]}) or in what `propose`
    returns ([M, K, T, w], [M, K, T], [M, K]: `propose_object_macros`) — are sequences of up to T steps judged as ONE candidate: they
    are expanded through `venv.expand_macros` and the kept ones materialised through `venv.transition_macros`, so a step whose own
    effect the dense pair cannot see (a Copy before its Paste) is not lost at the width cut.  `counts` still counts children.  With
    one shared set the sequence stays a list of indices into it; with `propose` it lists the PRIMITIVE steps in order, the first
    `length` of every macro, in the forms above."""
    dev = rows.device

    def payload_of(a):
        form = "bbox" if "bbox" in a else "point" if "point" in a else "bits"
        return form, a[form].to(device=dev, dtype=torch.uint8 if form == "bits" else torch.int32).contiguous()
    macro, length = False, None  # (macro candidates: decided by the "length" key of the first candidate set)
    if propose is None:
        form, pay = payload_of(actions)
        op = actions["operation"].to(device=dev, dtype=torch.int32).contiguous()
        macro = "length" in actions
        if macro:
            length = actions["length"].to(device=dev, dtype=torch.int32).contiguous()
            assert pay.dim() == 3 and op.dim() == 2 and length.dim() == 1, "beam_search takes one set of macros for every state"
        else:
            assert pay.dim() == 2 and op.dim() == 1, "beam_search takes one candidate set for every state"
        K = int(op.shape[0])
    M0 = int(rows.shape[0])
    src = (torch.arange(M0, device=dev) if src_env is None else src_env.to(dev)).to(torch.int32)
    root = torch.arange(M0, device=dev)
    # the actions behind every frontier state: indices into the one set, or (propose) the payloads and ops themselves, [M, depth, ...]
    path, path_op = (torch.empty((M0, 0), dtype=torch.int64, device=dev), None) if propose is None else (None, torch.empty((M0, 0), dtype=torch.int32, device=dev))
    seen = venv.hash_rows(rows)[:, 0].clone()
    frontier, counts = rows, []
    for _ in range(depth):
        M = int(frontier.shape[0])
        if M == 0:
            break
        if propose is not None:
            cand = propose(venv, frontier, src) if getattr(propose, "wants_src", False) else propose(venv, frontier)
            form, pay = payload_of(cand)
            assert form != "point", "propose returns bbox or bits candidates"
            op = cand["operation"].to(device=dev, dtype=torch.int32).contiguous()
            assert path is None or macro == ("length" in cand), "propose returns macros at every depth or at none"
            macro = "length" in cand
            if macro:
                length = cand["length"].to(device=dev, dtype=torch.int32).contiguous()
                assert pay.dim() == 4 and op.dim() == 3 and length.dim() == 2 and pay.shape[0] == M, "propose returns a set of macros per frontier row"
                if path is None:  # a macro's slot in the path: its T steps' payloads side by side, [M, depth, T * w]
                    path = torch.empty((M0, 0, pay.shape[2] * pay.shape[3]), dtype=pay.dtype, device=dev)
                    path_op = torch.empty((M0, 0, pay.shape[2]), dtype=torch.int32, device=dev)
                    path_len = torch.empty((M0, 0), dtype=torch.int32, device=dev)
            else:
                assert pay.dim() == 3 and op.dim() == 2 and pay.shape[0] == M, "propose returns a candidate set per frontier row"
            K = int(op.shape[1])
            if path is None:  # (shaped by the first candidate set: 4 int32 of a box, or the bytes of a bit row)
                path = torch.empty((M0, 0, pay.shape[2]), dtype=pay.dtype, device=dev)
        if macro:
            ex = venv.expand_macros(frontier, {form: pay, "operation": op, "length": length}, src)
        else:
            ex = venv.expand(frontier, {form: pay, "operation": op}, src)
        h = ex.hash[:, :, 0]
        ok = (ex.status == 0) & (h != ex.parent_hash[:, :1])
        idx = torch.nonzero(ok.reshape(-1)).reshape(-1)  # child index m * K + k, ascending
        hh = h.reshape(-1)[idx]
        new = ~torch.isin(hh, seen)
        idx, hh = idx[new], hh[new]
        order = torch.argsort(hh, stable=True)  # equal hashes: in child order
        hs = hh[order]
        first = torch.ones_like(hs, dtype=torch.bool)
        first[1:] = hs[1:] != hs[:-1]
        idx = torch.sort(idx[order[first]]).values
        hh = h.reshape(-1)[idx]
        seen = torch.cat([seen, hh])
        d2 = ex.dense.reshape(-1, 2)[idx].to(torch.int64)
        c, t = d2[:, 0], d2[:, 1]
        parent, k = idx // K, idx % K
        if propose is None:
            step_pay, step_op, step = pay.index_select(0, k), op.index_select(0, k), k.reshape(-1, 1)
            if macro:
                step_len = length.index_select(0, k)
        elif macro:  # the survivors' macros, gathered from their parents' sets: [n, T, w], [n, T], [n]
            T = int(op.shape[2])
            step_pay, step_op = pay.reshape(-1, T, pay.shape[3]).index_select(0, idx), op.reshape(-1, T).index_select(0, idx)
            step_len = length.reshape(-1).index_select(0, idx)
            step = step_pay.reshape(-1, 1, T * pay.shape[3])
        else:  # the survivors' actions, gathered from their parents' sets
            step_pay, step_op = pay.reshape(-1, pay.shape[2]).index_select(0, idx), op.reshape(-1).index_select(0, idx)
            step = step_pay.unsqueeze(1)
        goal = (c == t) & (t > 0)
        if bool(goal.any()):
            g = int(torch.nonzero(goal)[0])
            counts.append((M * K, int(idx.numel()), 0))
            if propose is None:
                seq = path[parent[g]].tolist() + [int(k[g])]
            elif macro:  # the primitive steps: the first `length` of every macro on the way, in order
                T, w_ = int(op.shape[2]), int(pay.shape[3])
                sels = torch.cat([path[parent[g]], step[g]], 0).reshape(-1, T, w_)
                ops = torch.cat([path_op[parent[g]], step_op[g:g + 1]], 0)
                lens = torch.cat([path_len[parent[g]], step_len[g:g + 1]], 0).tolist()
                took = [(d, t) for d, n in enumerate(lens) for t in range(n)]
                if form == "bbox":
                    seq = [tuple(sels[d, t].tolist()) + (int(ops[d, t]),) for d, t in took]
                else:
                    cells = unpack_bits(sels, venv.H, venv.W).cpu().numpy()
                    seq = [(cells[d, t], int(ops[d, t])) for d, t in took]
            else:
                sels, ops = torch.cat([path[parent[g]], step[g]], 0), torch.cat([path_op[parent[g]], step_op[g:g + 1]], 0).tolist()
                if form == "bbox":
                    seq = [tuple(a) + (o,) for a, o in zip(sels.tolist(), ops)]
                else:
                    seq = list(zip(unpack_bits(sels, venv.H, venv.W).cpu().numpy(), ops))
            return BeamResult(seq, counts, int(root[parent[g]]))
        # correct / total as an integer key: floor(c * 2^32 / t).  Two different fractions with totals below 2^16 differ by at least
        # 1 / (t1 * t2) > 2^-32, so their keys differ in the same direction; equal fractions give equal keys
        key = (c << 32) // torch.clamp(t, min=1)
        best = torch.argsort(key, descending=True, stable=True)[:width]
        best = torch.sort(best).values  # (kept states stay in child order: the next depth's child indices are deterministic)
        parent = parent[best]
        counts.append((M * K, int(idx.numel()), int(best.numel())))
        if best.numel() == 0:
            break
        src_next = src.index_select(0, parent)
        if macro:
            frontier, _, _ = venv.transition_macros(frontier.index_select(0, parent), {form: step_pay.index_select(0, best), "operation": step_op.index_select(0, best),
                                                                                      "length": step_len.index_select(0, best)}, src_next)
        else:
            frontier, _, _ = venv.transition(frontier.index_select(0, parent), {form: step_pay.index_select(0, best), "operation": step_op.index_select(0, best)},
                                             src_next)
        path = torch.cat([path.index_select(0, parent), step.index_select(0, best)], 1)
        if propose is not None and macro:
            path_op = torch.cat([path_op.index_select(0, parent), step_op.index_select(0, best).unsqueeze(1)], 1)
            path_len = torch.cat([path_len.index_select(0, parent), step_len.index_select(0, best).reshape(-1, 1)], 1)
        elif propose is not None:
            path_op = torch.cat([path_op.index_select(0, parent), step_op.index_select(0, best).reshape(-1, 1)], 1)
        root, src = root.index_select(0, parent), src_next
    return BeamResult(None, counts, None)


# ---- the objects of a grid as candidate actions ------------------------------------------------------------------------------------
def components_numpy(grid, grid_dim, max_components, skip_color=-1, any_color=False, diagonal=False):
    """The connected components of ONE grid as arcle_components_rows reports them (include/arcle_hip.h) — the host mirror the tests
    pin the device against, and pin against the reference's `dfs` (color.py:8-30): 4-connected cells of the same colour inside
    grid_dim, in ascending row-major index of their first cell (the seed); cells of `skip_color` (-1: none) belong to no component.
    grid int8 [H, W]; -> (count, left, comp int32 [C, 8] = x0, y0, x1, y1, sx, sy, colour, cells (rows >= count zero),
    masks uint8 [C, H, W]), left = the cells inside grid_dim, not of skip_color, in no written component.
    any_color / diagonal: the objects of arcle_objects_rows instead — cells of any colour but skip_color join / the eight neighbours
    of a cell count, not four; the colour reported is the seed's (`component_colors_numpy` gives the set)."""
    grid = np.asarray(grid)
    H, W = grid.shape
    gh, gw = min(int(grid_dim[0]), H), min(int(grid_dim[1]), W)
    C = int(max_components)
    todo = np.zeros((H, W), bool)
    todo[:gh, :gw] = True
    if skip_color >= 0:
        todo &= grid.astype(np.int64) != ((int(skip_color) + 128) % 256 - 128)
    comp, masks, n = np.zeros((C, 8), np.int32), np.zeros((C, H, W), np.uint8), 0
    for sx in range(gh):
        for sy in range(gw):
            if not todo[sx, sy] or n >= C:
                continue
            col = grid[sx, sy]
            queue, cells = collections.deque([(sx, sy)]), []
            todo[sx, sy] = False
            while queue:
                x, y = queue.popleft()
                cells.append((x, y))
                for xn, yn in _STRAIGHTS + (_DIAGONALS if diagonal else ()):
                    xn, yn = x + xn, y + yn
                    if 0 <= xn < gh and 0 <= yn < gw and todo[xn, yn] and (any_color or grid[xn, yn] == col):
                        todo[xn, yn] = False
                        queue.append((xn, yn))
            xs, ys = np.array(cells).T
            masks[n, xs, ys] = 1
            comp[n] = (xs.min(), ys.min(), xs.max(), ys.max(), sx, sy, int(col), len(cells))
            n += 1
    return n, int(todo.sum()), comp, masks


_STRAIGHTS, _DIAGONALS = ((-1, 0), (1, 0), (0, -1), (0, 1)), ((-1, -1), (-1, 1), (1, -1), (1, 1))


def component_colors_numpy(grid, masks):
    """The `colors` words of arcle_objects_rows for the masks uint8 [n, H, W] `components_numpy` returned: bit v & 31 for the byte v
    (taken as unsigned) of every cell of the object.  -> uint32 [n]"""
    bit = np.uint32(1) << (np.asarray(grid).astype(np.uint8) & 31).astype(np.uint32)
    return np.array([np.bitwise_or.reduce(bit[np.asarray(m) != 0], initial=np.uint32(0)) for m in masks], np.uint32).reshape(len(masks))


def pack_bits(masks):
    """Selection masks [..., H, W] (bool, or int8: truthy = non-zero) -> uint8 [..., 128] bit rows on the masks' device: bit f & 7 of
    byte f >> 3 is cell f = row * W + col — the layout of `step_bits`, `components(bits=True)` and the "bits" form of `expand` /
    `transition`.  (arcle_pack_mask_bits does the same for exactly the handle's N envs; a search packs M * K masks.)"""
    lead, P = tuple(masks.shape[:-2]), int(masks.shape[-2]) * int(masks.shape[-1])
    assert P <= 8 * BITS_STRIDE, "pack_bits: grids of at most 1024 cells"
    flat = torch.zeros(lead + (8 * BITS_STRIDE,), dtype=torch.uint8, device=masks.device)
    flat[..., :P] = (masks != 0).reshape(lead + (P,))
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=masks.device)
    return (flat.reshape(lead + (BITS_STRIDE, 8)) * w).sum(-1, dtype=torch.uint8)  # (eight distinct bits: the byte sum cannot carry)


def unpack_bits(bits, H, W):
    """The inverse of pack_bits: uint8 [..., 128] bit rows -> bool [..., H, W] (bits at cell indices >= H * W are dropped)."""
    sh = torch.arange(8, dtype=torch.int32, device=bits.device)
    cells = ((bits.to(torch.int32).unsqueeze(-1) >> sh) & 1).reshape(tuple(bits.shape[:-1]) + (-1,))
    return cells[..., :H * W].reshape(tuple(bits.shape[:-1]) + (H, W)).to(torch.bool)


def object_actions(comp, box_ops, seed_ops, masks=False):
    """The components of M states (`ARCVecEnv.components`: count [M], box [M, C, 4], seed [M, C, 2]) as a candidate set per state:
    {"bbox": int32 [M, K, 4], "operation": int32 [M, K]}, K = C * (len(box_ops) + len(seed_ops)).  Component k contributes its box
    with every op of box_ops (Move / Rotate / Flip / Copy want the box of a shape), then its seed as the 1 x 1 box (sx, sy, sx, sy)
    with every op of seed_ops (a 1 x 1 rectangle is what FloodFill accepts).  The slots of components k >= count get operation -1:
    expansion reports ARCLE_ST_BAD_OP for such a child alone, and beam_search drops children with a status bit.  Pure indexing on the
    device: no host synchronisation.
    masks=True (needs comp.bits, `components(bits=True)`): {"bits": uint8 [M, K, 128], "operation": int32 [M, K]} — component k's
    exact cells with every op of box_ops (a box selects whatever else lies inside it), then the one-bit mask of its seed with every
    op of seed_ops (FloodFill acts only on a selection of one cell); the slots of components k >= count get a zero mask."""
    box, seed, count = comp.box, comp.seed, comp.count
    M, C = int(box.shape[0]), int(box.shape[1])
    dev = box.device
    ops = torch.as_tensor(list(box_ops) + list(seed_ops), dtype=torch.int32, device=dev)
    nb, ns = len(box_ops), len(seed_ops)
    per = nb + ns
    bb = torch.cat([box.reshape(M, C, 1, 4).expand(M, C, nb, 4), torch.cat([seed, seed], 2).reshape(M, C, 1, 4).expand(M, C, ns, 4)], 2)
    there = (torch.arange(C, device=dev).reshape(1, C) < count.reshape(M, 1)).reshape(M, C, 1)
    op = torch.where(there, ops.reshape(1, 1, per), torch.full((), -1, dtype=torch.int32, device=dev))
    if masks:
        assert comp.bits is not None, "object_actions(masks=True) needs the components' bit masks (components(bits=True))"
        cells = torch.where(there, comp.bits, torch.zeros((), dtype=torch.uint8, device=dev))  # (entries >= count were never written)
        # the seed is the component's first cell in row-major order: the lowest set bit of its row
        first = (cells != 0).to(torch.uint8).argmax(-1, keepdim=True)
        v = cells.gather(-1, first).to(torch.int32)
        one = torch.zeros_like(cells).scatter_(-1, first, (v & -v).to(torch.uint8))
        S_ = int(cells.shape[-1])
        mb = torch.cat([cells.reshape(M, C, 1, S_).expand(M, C, nb, S_), one.reshape(M, C, 1, S_).expand(M, C, ns, S_)], 2)
        return {"bits": mb.reshape(M, C * per, S_).contiguous(), "operation": op.reshape(M, C * per).to(torch.int32).contiguous()}
    bb = torch.where(there.reshape(M, C, 1, 1), bb.to(torch.int32), torch.zeros((), dtype=torch.int32, device=dev))  # (entries >= count were never written)
    return {"bbox": bb.reshape(M, C * per, 4).contiguous(), "operation": op.reshape(M, C * per).to(torch.int32).contiguous()}


def propose_objects(box_ops, seed_ops, max_components=16, skip_color=0, masks=False, any_color=False, diagonal=False):
    """A `propose` for beam_search: at every depth the connected components of each frontier state's grid (`venv.components`, one
    launch) with box_ops on their boxes and seed_ops on their seeds (`object_actions`); masks=True: on their exact cells, as bit
    rows, instead of their boxes.  any_color / diagonal: the multi-colour / 8-connected objects of `venv.objects` instead."""
    box_ops, seed_ops = list(box_ops), list(seed_ops)

    def propose(venv, rows):
        if any_color or diagonal:
            comp = venv.objects(rows, max_components=max_components, skip_color=skip_color, any_color=any_color, diagonal=diagonal, bits=bool(masks))
        else:
            comp = venv.components(rows, max_components=max_components, skip_color=skip_color, bits=True) if masks else \
                venv.components(rows, max_components=max_components, skip_color=skip_color)
        return object_actions(comp, box_ops, seed_ops, masks)
    return propose


def run_macros(transition, rows, action, src_env=None):
    """One macro per row, materialised: `rows` [M, L] after each row's own macro — action = {form: [M, T, w], "operation": [M, T],
    "length": [M] (optional: every row runs T steps)} — by T calls of `transition(rows_t, action_t, src_t) -> (rows, reward, term)`
    (`ARCVecEnv.transition`'s signature), call t over the rows that still have a step at position t.  -> (rows, reward int32 [M] =
    the steps' rewards summed, terminated bool [M] = the last step's).  A length outside [1, T] runs nothing, as `expand_macros`
    reports it.  The gathers are bounded by the beam width: this is how a search materialises its survivors, not its hot path."""
    form = "bbox" if "bbox" in action else "point" if "point" in action else "bits"
    pay, op, length = action[form], action["operation"], action.get("length")
    M, T = int(op.shape[0]), int(op.shape[1])
    cur = rows.clone()
    reward = torch.zeros(M, dtype=torch.int32, device=rows.device)
    term = torch.zeros(M, dtype=torch.bool, device=rows.device)
    for t in range(T):
        if length is None:
            out, r, tm = transition(cur, {form: pay[:, t].contiguous(), "operation": op[:, t].contiguous()}, src_env)
            cur, reward, term = out, reward + r.to(torch.int32), tm.to(torch.bool)
            continue
        idx = torch.nonzero((length > t) & (length <= T)).reshape(-1)
        if idx.numel() == 0:
            break
        out, r, tm = transition(cur.index_select(0, idx), {form: pay[:, t].index_select(0, idx), "operation": op[:, t].index_select(0, idx)},
                                None if src_env is None else src_env.index_select(0, idx))
        cur[:, :out.shape[1]].index_copy_(0, idx, out.to(cur.dtype))
        reward.index_add_(0, idx, r.to(torch.int32))
        term.index_copy_(0, idx, tm.to(torch.bool))
    return cur, reward, term


def object_macros(comp, box_ops, seed_ops, pair_ops):
    """The components of M states as a set of MACROS per state (T = 2 when pair_ops is not empty, else 1): {"bbox": int32 [M, K, T, 4],
    "operation": int32 [M, K, T], "length": int32 [M, K]}.  First the singles of `object_actions(comp, box_ops, seed_ops)`, in its
    order, as macros of length 1; then for every ordered pair of components (i, j), i-major, and every (op_a, op_b) of pair_ops the
    macro [op_a on box i, op_b on box j] of length 2 — CopyO on one object's box, Paste at another's; a selection-setting op, then
    an object op — K = C * (len(box_ops) + len(seed_ops)) + C * C * len(pair_ops).  Pair slots with i == j or a component >= count
    get operation -1 at step 0 and length 1: one ARCLE_ST_BAD_OP child, dropped by beam_search.  Boxes only.  Pure indexing on the
    device: no host synchronisation."""
    single = object_actions(comp, box_ops, seed_ops)
    box, count = comp.box, comp.count
    M, C = int(box.shape[0]), int(box.shape[1])
    dev = box.device
    T = 2 if len(pair_ops) else 1
    K1, npair = int(single["operation"].shape[1]), len(pair_ops)
    bb1 = torch.zeros((M, K1, T, 4), dtype=torch.int32, device=dev)
    bb1[:, :, 0] = single["bbox"]
    op1 = torch.full((M, K1, T), -1, dtype=torch.int32, device=dev)
    op1[:, :, 0] = single["operation"]
    len1 = torch.ones((M, K1), dtype=torch.int32, device=dev)
    if not npair:
        return {"bbox": bb1, "operation": op1, "length": len1}
    po = torch.as_tensor(list(pair_ops), dtype=torch.int32, device=dev).reshape(npair, 2)
    ar = torch.arange(C, device=dev)
    there = ar.reshape(1, C) < count.reshape(M, 1)
    ok = (there.reshape(M, C, 1) & there.reshape(M, 1, C) & (ar.reshape(C, 1) != ar.reshape(1, C)).reshape(1, C, C)).reshape(M, C, C, 1)
    b32 = box.to(torch.int32)
    bb2 = torch.stack([b32.reshape(M, C, 1, 1, 4).expand(M, C, C, npair, 4), b32.reshape(M, 1, C, 1, 4).expand(M, C, C, npair, 4)], 4)
    bb2 = torch.where(ok.reshape(M, C, C, 1, 1, 1), bb2, torch.zeros((), dtype=torch.int32, device=dev))
    op2 = torch.where(ok.reshape(M, C, C, 1, 1), po.reshape(1, 1, 1, npair, 2), torch.full((), -1, dtype=torch.int32, device=dev))
    len2 = torch.where(ok, torch.full((), 2, dtype=torch.int32, device=dev), torch.ones((), dtype=torch.int32, device=dev)).expand(M, C, C, npair)
    K2 = C * C * npair
    return {"bbox": torch.cat([bb1, bb2.reshape(M, K2, 2, 4)], 1).contiguous(), "operation": torch.cat([op1, op2.reshape(M, K2, 2)], 1).contiguous(),
            "length": torch.cat([len1, len2.reshape(M, K2)], 1).contiguous()}


def propose_object_macros(box_ops, seed_ops, pair_ops, max_components=16, skip_color=0, any_color=False, diagonal=False):
    """A `propose` for beam_search that returns macros: at every depth the components of each frontier state's grid (`venv.components`,
    one launch) as `object_macros` arranges them — the singles of `propose_objects`, then every (op_a, op_b) of pair_ops on every
    ordered pair of objects' boxes as ONE candidate of two steps.  any_color / diagonal: the objects of `venv.objects` instead."""
    box_ops, seed_ops, pair_ops = list(box_ops), list(seed_ops), [tuple(p) for p in pair_ops]

    def propose(venv, rows):
        if any_color or diagonal:
            return object_macros(venv.objects(rows, max_components=max_components, skip_color=skip_color, any_color=any_color, diagonal=diagonal),
                                 box_ops, seed_ops, pair_ops)
        return object_macros(venv.components(rows, max_components=max_components, skip_color=skip_color), box_ops, seed_ops, pair_ops)
    return propose


# ---- where each object best fits the answer ----------------------------------------------------------------------------------------
def place_numpy(grid, grid_dim, answer, answer_dim, masks, max_dist=None, full=False):
    """The best translation of every object of ONE grid as arcle_place_rows reports it (include/arcle_hip.h) — the host mirror, straight
    from the definition: every child grid is built and counted.  grid, answer int8 [H, W]; masks [n, H, W] (truthy = the object's
    cells; cells outside grid_dim are ignored); max_dist None: no limit.  -> (place int32 [n, 4] = dx, dy, correct(best), correct(0, 0),
    base (correct, total) of the grid itself); full=True adds table int32 [n, 2H - 1, 2W - 1]: correct(dx, dy) at [dx + H - 1,
    dy + W - 1], -1 outside T.  The child of (dx, dy): the object's cells zeroed, then its POSITIVE cells pasted dx rows down and dy
    columns right — what select + |dx| + |dy| Moves leave (object.py:60-138, 218-243); the candidates keep the object's box inside
    grid_dim; ties go to the smaller |dx| + |dy|, then the smaller dx, then the smaller dy."""
    grid, answer = np.asarray(grid).astype(np.int8), np.asarray(answer).astype(np.int8)
    H, W = grid.shape
    gh, gw = min(int(grid_dim[0]), H), min(int(grid_dim[1]), W)
    ah, aw = min(int(answer_dim[0]), H), min(int(answer_dim[1]), W)
    mh, mw = min(gh, ah), min(gw, aw)
    D = 2 * (H + W) if max_dist is None else int(max_dist)
    total = mh * mw + (abs(ah * aw - gh * gw) if (gh <= ah) == (gw <= aw) else abs(gh - ah) * mw + abs(gw - aw) * mh)
    base = (int((grid[:mh, :mw] == answer[:mh, :mw]).sum()), total)
    masks = np.asarray(masks).reshape(-1, H, W)
    n = masks.shape[0]
    place = np.zeros((n, 4), np.int32)
    table = np.full((n, 2 * H - 1, 2 * W - 1), -1, np.int32)
    for k in range(n):
        B = np.zeros((H, W), bool)
        B[:gh, :gw] = masks[k, :gh, :gw] != 0
        back = np.where(B, 0, grid)
        xs, ys = np.nonzero(B & (grid > 0))
        cols = grid[xs, ys]
        bx, by = np.nonzero(B)
        x0, x1, y0, y1 = (bx.min(), bx.max(), by.min(), by.max()) if len(bx) else (0, gh - 1, 0, gw - 1)
        best = None
        for dx in range(max(-x0, -D), min(gh - 1 - x1, D) + 1) if len(bx) else (0,):
            for dy in range(max(-y0, -D), min(gw - 1 - y1, D) + 1) if len(bx) else (0,):
                if abs(dx) + abs(dy) > D:
                    continue
                child = back.copy()
                child[xs + dx, ys + dy] = cols
                c = int((child[:mh, :mw] == answer[:mh, :mw]).sum())
                table[k, dx + H - 1, dy + W - 1] = c
                key = (-c, abs(dx) + abs(dy), dx, dy)
                if best is None or key < best:
                    best = key
        place[k] = (best[2], best[3], -best[0], table[k, H - 1, W - 1])
    return (place, base, table) if full else (place, base)


def placement_macros(objs, placements, move_ops, max_len):
    """The best translation of every object (`ARCVecEnv.place` -> Placements) as ONE Move macro per object: {"bits": uint8 [M, C, T, 128],
    "operation": int32 [M, C, T], "length": int32 [M, C]}, T = max_len.  Macro k is |dx| vertical Moves, then |dy| horizontal ones;
    move_ops = (up, down, right, left) op indices — dx < 0 moves up, dy > 0 right (dirX / dirY of gen_move).  Step 0 carries the
    object's bit row (objs.bits); every later step the zero mask, which continues the active object (object.py:102-107).  Slots with
    k >= count, (dx, dy) == (0, 0), correct <= stay (the move gains nothing) or |dx| + |dy| > T get operation -1 at step 0 and length
    1: one ARCLE_ST_BAD_OP child, dropped by beam_search.  Pure indexing on the device: no host synchronisation."""
    assert objs.bits is not None, "placement_macros needs the objects' bit rows (bits=True)"
    dev = objs.bits.device
    M, C, S_ = (int(v) for v in objs.bits.shape)
    T = int(max_len)
    up, down, right, left = (int(o) for o in move_ops)
    dx, dy = placements.dx.to(torch.int32), placements.dy.to(torch.int32)
    nv, nh = dx.abs(), dy.abs()
    there = torch.arange(C, device=dev).reshape(1, C) < objs.count.reshape(M, 1)
    ok = there & ((nv + nh) > 0) & ((nv + nh) <= T) & (placements.correct > placements.stay)
    t = torch.arange(T, device=dev, dtype=torch.int32).reshape(1, 1, T)
    vert = torch.where(dx < 0, up, down).to(torch.int32).reshape(M, C, 1)
    horiz = torch.where(dy > 0, right, left).to(torch.int32).reshape(M, C, 1)
    minus = torch.full((), -1, dtype=torch.int32, device=dev)
    op = torch.where(t < nv.reshape(M, C, 1), vert, torch.where(t < (nv + nh).reshape(M, C, 1), horiz, minus))
    op = torch.where(ok.reshape(M, C, 1), op, minus)
    length = torch.where(ok, nv + nh, torch.ones((), dtype=torch.int32, device=dev)).to(torch.int32)
    bits = torch.zeros((M, C, T, S_), dtype=torch.uint8, device=dev)
    bits[:, :, 0] = torch.where(ok.reshape(M, C, 1), objs.bits, torch.zeros((), dtype=torch.uint8, device=dev))
    return {"bits": bits, "operation": op.to(torch.int32).contiguous(), "length": length.contiguous()}


def propose_placements(move_ops, box_ops=(), seed_ops=(), max_dist=8, max_components=16, skip_color=0, any_color=False, diagonal=False):
    """A `propose` for beam_search that answers "where does this object belong?": at every depth the objects of each frontier state's
    grid (`venv.objects` / `venv.components` with their bit rows), first the singles of `object_actions(masks=True)` — box_ops on the
    objects' exact cells, seed_ops on their seeds — as macros of length 1, then for every object ONE macro of up to max_dist Moves to
    the translation at which it fits the answer best (`venv.place`, one launch; `placement_macros`), K = C * (len(box_ops) +
    len(seed_ops) + 1), T = max(max_dist, 1).  move_ops = (up, down, right, left).  It looks at the answer of each row's env, so it
    carries `wants_src = True` and beam_search calls it with (venv, rows, src_env)."""
    move_ops, box_ops, seed_ops = tuple(int(o) for o in move_ops), list(box_ops), list(seed_ops)
    T = max(int(max_dist), 1)

    def propose(venv, rows, src_env=None):
        if any_color or diagonal:
            objs = venv.objects(rows, max_components=max_components, skip_color=skip_color, any_color=any_color, diagonal=diagonal, bits=True)
        else:
            objs = venv.components(rows, max_components=max_components, skip_color=skip_color, bits=True)
        pm = placement_macros(objs, venv.place(rows, objs, src_env, max_dist), move_ops, T)
        if not box_ops and not seed_ops:
            return pm
        single = object_actions(objs, box_ops, seed_ops, masks=True)
        M, K1 = (int(v) for v in single["operation"].shape)
        dev = single["bits"].device
        b1 = torch.zeros((M, K1, T, int(single["bits"].shape[-1])), dtype=torch.uint8, device=dev)
        b1[:, :, 0] = single["bits"]
        o1 = torch.full((M, K1, T), -1, dtype=torch.int32, device=dev)
        o1[:, :, 0] = single["operation"]
        return {"bits": torch.cat([b1, pm["bits"]], 1).contiguous(), "operation": torch.cat([o1, pm["operation"]], 1).contiguous(),
                "length": torch.cat([torch.ones((M, K1), dtype=torch.int32, device=dev), pm["length"]], 1).contiguous()}
    propose.wants_src = True
    return propose


# ---- where a copy of each object best fits the answer ------------------------------------------------------------------------------
def stamp_numpy(grid, grid_dim, answer, answer_dim, masks, max_dist=None, blank=True, full=False):
    """The best paste position of a copy of every object of ONE grid as arcle_stamp_rows reports it (include/arcle_hip.h) — the host
    mirror, straight from the definition: every child grid is built and counted.  grid, answer int8 [H, W]; masks [n, H, W] (truthy =
    the object's cells; cells outside grid_dim are ignored); max_dist None: no limit; blank = what Paste does (True: the clip's whole
    rectangle is written; False: its positive cells only).  -> (stamp int32 [n, 4] = px, py, correct(px, py), the cells of B, base
    (correct, total) of the grid itself); full=True adds table int32 [n, H, W]: correct(px, py), -1 outside T.  The child of (px,
    py): the clip — the object's box cut out of the grid, the box's cells outside the object as 0 (object.py:291-312) — written with
    its top-left corner at (px, py), cut at the plane's H x W (object.py:340-341); the candidates are the cells of grid_dim within
    max_dist of the box's corner (x0, y0); ties go to the smaller |dx| + |dy|, (dx, dy) = (px - x0, py - y0), then the smaller dx,
    then the smaller dy.  An empty object: (0, 0, base correct, 0) and a table of -1."""
    grid, answer = np.asarray(grid).astype(np.int8), np.asarray(answer).astype(np.int8)
    H, W = grid.shape
    gh, gw = min(int(grid_dim[0]), H), min(int(grid_dim[1]), W)
    ah, aw = min(int(answer_dim[0]), H), min(int(answer_dim[1]), W)
    mh, mw = min(gh, ah), min(gw, aw)
    D = 2 * (H + W) if max_dist is None else int(max_dist)
    total = mh * mw + (abs(ah * aw - gh * gw) if (gh <= ah) == (gw <= aw) else abs(gh - ah) * mw + abs(gw - aw) * mh)
    base = (int((grid[:mh, :mw] == answer[:mh, :mw]).sum()), total)
    masks = np.asarray(masks).reshape(-1, H, W)
    n = masks.shape[0]
    stamp = np.zeros((n, 4), np.int32)
    table = np.full((n, H, W), -1, np.int32)
    for k in range(n):
        B = np.zeros((H, W), bool)
        B[:gh, :gw] = masks[k, :gh, :gw] != 0
        bx, by = np.nonzero(B)
        if not len(bx):
            stamp[k] = (0, 0, base[0], 0)
            continue
        x0, x1, y0, y1 = bx.min(), bx.max(), by.min(), by.max()
        clip = np.where(B, grid, 0)[x0:x1 + 1, y0:y1 + 1]
        best = None
        for px in range(gh):
            for py in range(gw):
                if abs(px - x0) + abs(py - y0) > D:
                    continue
                child = grid.copy()
                part = clip[:H - px, :W - py]
                dst = child[px:px + part.shape[0], py:py + part.shape[1]]
                dst[...] = part if blank else np.where(part > 0, part, dst)
                c = int((child[:mh, :mw] == answer[:mh, :mw]).sum())
                table[k, px, py] = c
                key = (-c, abs(px - x0) + abs(py - y0), px - x0, py - y0)
                if best is None or key < best:
                    best = key
        stamp[k] = (x0 + best[2], y0 + best[3], -best[0], len(bx))
    return (stamp, base, table) if full else (stamp, base)


def stamp_macros(objs, stamps, copy_op, paste_op, W):
    """The best paste position of a copy of every object (`ARCVecEnv.stamp` -> Stamps) as ONE two-step macro per object: {"bits": uint8
    [M, C, 2, 128], "operation": int32 [M, C, 2], "length": int32 [M, C]}.  Step 0 is the object's bit row (objs.bits) with copy_op
    (CopyO), step 1 the one-bit row of cell (px, py) — bit px * W + py, W = the plane's width — with paste_op.  Slots with k >= count
    or correct <= base[0] (the stamp gains nothing) get operation -1 at step 0 and length 1: one ARCLE_ST_BAD_OP child, dropped by
    beam_search.  Pure indexing on the device: no host synchronisation."""
    assert objs.bits is not None, "stamp_macros needs the objects' bit rows (bits=True)"
    dev = objs.bits.device
    M, C, S_ = (int(v) for v in objs.bits.shape)
    there = torch.arange(C, device=dev).reshape(1, C) < objs.count.reshape(M, 1)
    ok = there & (stamps.correct > stamps.base[:, 0].reshape(M, 1))
    zero = torch.zeros((), dtype=torch.uint8, device=dev)
    pair = torch.where(torch.arange(2, device=dev).reshape(1, 1, 2) == 0, int(copy_op), int(paste_op)).to(torch.int32)
    op = torch.where(ok.reshape(M, C, 1), pair, torch.full((), -1, dtype=torch.int32, device=dev))
    length = torch.where(ok, torch.full((), 2, dtype=torch.int32, device=dev), torch.ones((), dtype=torch.int32, device=dev))
    cell = (stamps.px.to(torch.int64) * int(W) + stamps.py.to(torch.int64)).clamp(0, 8 * S_ - 1)
    one = torch.zeros((M, C, S_), dtype=torch.uint8, device=dev)
    one.scatter_(-1, (cell >> 3).reshape(M, C, 1), (torch.ones((), dtype=torch.int64, device=dev) << (cell & 7)).to(torch.uint8).reshape(M, C, 1))
    bits = torch.stack([objs.bits, one], 2)
    bits = torch.where(ok.reshape(M, C, 1, 1), bits, zero)
    return {"bits": bits.contiguous(), "operation": op.to(torch.int32).contiguous(), "length": length.to(torch.int32).contiguous()}


def propose_stamps(copy_op, paste_op, box_ops=(), seed_ops=(), max_dist=None, max_components=16, skip_color=0, any_color=False, diagonal=False,
                   blank=True):
    """A `propose` for beam_search that answers "where does a copy of this object belong?": at every depth the objects of each
    frontier state's grid (`venv.objects` / `venv.components` with their bit rows), first the singles of `object_actions(masks=True)`
    — box_ops on the objects' exact cells, seed_ops on their seeds — as macros of length 1, then for every object ONE macro of two
    steps, copy_op on the object and paste_op at the cell where the copy fits the answer best (`venv.stamp`, one launch;
    `stamp_macros`), K = C * (len(box_ops) + len(seed_ops) + 1), T = 2.  blank must say what paste_op does in the caller's table
    (True: paste_blank, both default tables).  It looks at the answer of each row's env, so it carries `wants_src = True` and
    beam_search calls it with (venv, rows, src_env)."""
    copy_op, paste_op, box_ops, seed_ops = int(copy_op), int(paste_op), list(box_ops), list(seed_ops)

    def propose(venv, rows, src_env=None):
        if any_color or diagonal:
            objs = venv.objects(rows, max_components=max_components, skip_color=skip_color, any_color=any_color, diagonal=diagonal, bits=True)
        else:
            objs = venv.components(rows, max_components=max_components, skip_color=skip_color, bits=True)
        sm = stamp_macros(objs, venv.stamp(rows, objs, src_env, max_dist, blank), copy_op, paste_op, venv.W)
        if not box_ops and not seed_ops:
            return sm
        single = object_actions(objs, box_ops, seed_ops, masks=True)
        M, K1 = (int(v) for v in single["operation"].shape)
        dev = single["bits"].device
        b1 = torch.zeros((M, K1, 2, int(single["bits"].shape[-1])), dtype=torch.uint8, device=dev)
        b1[:, :, 0] = single["bits"]
        o1 = torch.full((M, K1, 2), -1, dtype=torch.int32, device=dev)
        o1[:, :, 0] = single["operation"]
        return {"bits": torch.cat([b1, sm["bits"]], 1).contiguous(), "operation": torch.cat([o1, sm["operation"]], 1).contiguous(),
                "length": torch.cat([torch.ones((M, K1), dtype=torch.int32, device=dev), sm["length"]], 1).contiguous()}
    propose.wants_src = True
    return propose


# ---- where each object best fits the answer after a rotation or a flip -------------------------------------------------------------
TURN_ROT90, TURN_ROT180, TURN_ROT270, TURN_FLIP_H, TURN_FLIP_V = 1, 2, 4, 8, 16  # ARCLE_TURN_*: slot t of the output <-> bit t


def _turned(tile, t):
    return (np.rot90(tile, 1), np.rot90(tile, 2), np.rot90(tile, 3), np.fliplr(tile), np.flipud(tile))[t]


def turn_numpy(grid, grid_dim, answer, answer_dim, masks, max_dist=None, turns=31, full=False):
    """The best translation of every object of ONE grid after each of the five turns, as arcle_turn_rows reports it
    (include/arcle_hip.h) — the host mirror, straight from the definition: every child grid is built with np.rot90 / np.fliplr /
    np.flipud and counted.  grid, answer int8 [H, W]; masks [n, H, W] (truthy = the object's cells; cells outside grid_dim are
    ignored); max_dist None: no limit; turns = the mask of the turns asked for (bit t = slot t: rot90, rot180, rot270, flip H, flip
    V).  -> (turn int32 [n, 5, 4] = dx, dy, correct, valid — zeros in the slots not asked for —, base (correct, total) of the grid
    itself); full=True adds table int32 [n, 5, 2H - 1, 2W - 1]: correct(t, dx, dy) at [dx + H - 1, dy + W - 1], -1 outside T_t.
    The child of (t, dx, dy): the object's cells zeroed, then the POSITIVE cells of the turned h' x w' tile (the object's box, 0
    outside the object) written with its corner at (nx + dx, ny + dy), (nx, ny) = the corner at which the turn leaves a freshly
    selected object (object.py:186-207: the box's corner for rot180 and the flips, (floor((2 x0 + h - w) / 2), floor((2 y0 + w - h) /
    2)) for the quarter turns) — what select + turn + |dx| + |dy| Moves leave; the candidates keep the turned tile inside grid_dim;
    ties go to the smaller |dx| + |dy|, then the smaller dx, then the smaller dy.  No candidate: (0, 0, 0, 0); an empty object:
    (0, 0, base correct, 1)."""
    grid, answer = np.asarray(grid).astype(np.int8), np.asarray(answer).astype(np.int8)
    H, W = grid.shape
    gh, gw = min(int(grid_dim[0]), H), min(int(grid_dim[1]), W)
    ah, aw = min(int(answer_dim[0]), H), min(int(answer_dim[1]), W)
    mh, mw = min(gh, ah), min(gw, aw)
    D = 2 * (H + W) if max_dist is None else int(max_dist)
    total = mh * mw + (abs(ah * aw - gh * gw) if (gh <= ah) == (gw <= aw) else abs(gh - ah) * mw + abs(gw - aw) * mh)
    base = (int((grid[:mh, :mw] == answer[:mh, :mw]).sum()), total)
    masks = np.asarray(masks).reshape(-1, H, W)
    n = masks.shape[0]
    turn = np.zeros((n, 5, 4), np.int32)
    table = np.full((n, 5, 2 * H - 1, 2 * W - 1), -1, np.int32)
    for k in range(n):
        B = np.zeros((H, W), bool)
        B[:gh, :gw] = masks[k, :gh, :gw] != 0
        bx, by = np.nonzero(B)
        for t in range(5):
            if not (int(turns) >> t) & 1:
                continue
            if not len(bx):
                turn[k, t] = (0, 0, base[0], 1)
                continue
            x0, x1, y0, y1 = int(bx.min()), int(bx.max()), int(by.min()), int(by.max())
            h, w = x1 - x0 + 1, y1 - y0 + 1
            back = np.where(B, 0, grid)
            tile = _turned(np.where(B, grid, 0)[x0:x1 + 1, y0:y1 + 1], t)
            th, tw = tile.shape
            nx, ny = ((2 * x0 + h - w) // 2, (2 * y0 + w - h) // 2) if t in (0, 2) else (x0, y0)
            ti, tj = np.nonzero(tile > 0)
            cols = tile[ti, tj]
            best = None
            for px in range(0, gh - th + 1):
                for py in range(0, gw - tw + 1):
                    dx, dy = px - nx, py - ny
                    if abs(dx) + abs(dy) > D:
                        continue
                    child = back.copy()
                    child[px + ti, py + tj] = cols
                    c = int((child[:mh, :mw] == answer[:mh, :mw]).sum())
                    table[k, t, dx + H - 1, dy + W - 1] = c
                    key = (-c, abs(dx) + abs(dy), dx, dy)
                    if best is None or key < best:
                        best = key
            if best is not None:
                turn[k, t] = (best[2], best[3], -best[0], 1)
    return (turn, base, table) if full else (turn, base)


def turn_macros(objs, turns, turn_ops, move_ops, max_len):
    """The best turn + translation of every object (`ARCVecEnv.turn` -> Turns) as ONE macro per object: {"bits": uint8 [M, C, T, 128],
    "operation": int32 [M, C, T], "length": int32 [M, C]}, T = max_len.  turn_ops = the op indices of rot90, rot180, rot270, flip H,
    flip V in the caller's table, -1 where it has none (O2ARCv2Env: (24, -1, 25, 26, 27)); move_ops = (up, down, right, left).  Per
    object the best valid turn that has an op: more correct, then fewer steps, then the lower slot.  Step 0 is the object's bit row
    (objs.bits) with the turn's op; then |dx| vertical and |dy| horizontal Moves on the zero mask, which continues the active object
    (object.py:102-107), as `placement_macros` lays them out.  Slots with k >= count, no valid turn, correct <= base[0] (the turn gains
    nothing) or 1 + |dx| + |dy| > T get operation -1 at step 0 and length 1: one ARCLE_ST_BAD_OP child, dropped by beam_search.  Pure
    indexing on the device: no host synchronisation."""
    assert objs.bits is not None, "turn_macros needs the objects' bit rows (bits=True)"
    dev = objs.bits.device
    M, C, S_ = (int(v) for v in objs.bits.shape)
    T = int(max_len)
    up, down, right, left = (int(o) for o in move_ops)
    tops = torch.as_tensor([int(o) for o in turn_ops], dtype=torch.int32, device=dev).reshape(1, 1, 5)
    steps = turns.dx.to(torch.int64).abs() + turns.dy.to(torch.int64).abs()
    usable = (turns.valid != 0) & (tops >= 0)
    score = turns.correct.to(torch.int64) * 4096 - steps * 8 - torch.arange(5, device=dev).reshape(1, 1, 5)
    score = torch.where(usable, score, torch.full((), -1, dtype=torch.int64, device=dev))
    pick = score.argmax(-1, keepdim=True)
    dx, dy = turns.dx.gather(-1, pick).reshape(M, C).to(torch.int32), turns.dy.gather(-1, pick).reshape(M, C).to(torch.int32)
    correct = turns.correct.gather(-1, pick).reshape(M, C)
    top = tops.expand(M, C, 5).gather(-1, pick).reshape(M, C, 1)
    nv, nh = dx.abs(), dy.abs()
    there = torch.arange(C, device=dev).reshape(1, C) < objs.count.reshape(M, 1)
    ok = there & usable.any(-1) & (correct > turns.base[:, 0].reshape(M, 1)) & ((1 + nv + nh) <= T)
    t = torch.arange(T, device=dev, dtype=torch.int32).reshape(1, 1, T)
    vert = torch.where(dx < 0, up, down).to(torch.int32).reshape(M, C, 1)
    horiz = torch.where(dy > 0, right, left).to(torch.int32).reshape(M, C, 1)
    minus = torch.full((), -1, dtype=torch.int32, device=dev)
    op = torch.where(t == 0, top, torch.where(t <= nv.reshape(M, C, 1), vert, torch.where(t <= (nv + nh).reshape(M, C, 1), horiz, minus)))
    op = torch.where(ok.reshape(M, C, 1), op, minus)
    length = torch.where(ok, 1 + nv + nh, torch.ones((), dtype=torch.int32, device=dev)).to(torch.int32)
    bits = torch.zeros((M, C, T, S_), dtype=torch.uint8, device=dev)
    bits[:, :, 0] = torch.where(ok.reshape(M, C, 1), objs.bits, torch.zeros((), dtype=torch.uint8, device=dev))
    return {"bits": bits, "operation": op.to(torch.int32).contiguous(), "length": length.contiguous()}


def propose_turns(turn_ops, move_ops, box_ops=(), seed_ops=(), max_dist=8, max_components=16, skip_color=0, any_color=False, diagonal=False):
    """A `propose` for beam_search that answers "where does this object belong once it is rotated or mirrored?": at every depth the
    objects of each frontier state's grid (`venv.objects` / `venv.components` with their bit rows), first the singles of
    `object_actions(masks=True)` — box_ops on the objects' exact cells, seed_ops on their seeds — as macros of length 1, then for every
    object ONE macro: the turn and the up to max_dist Moves after it that fit the answer best (`venv.turn`, one launch; `turn_macros`),
    K = C * (len(box_ops) + len(seed_ops) + 1), T = 1 + max_dist.  turn_ops = (rot90, rot180, rot270, flip H, flip V) op indices, -1
    where the table has none: only the turns that have an op are asked for.  It looks at the answer of each row's env, so it carries
    `wants_src = True` and beam_search calls it with (venv, rows, src_env)."""
    turn_ops, move_ops, box_ops, seed_ops = tuple(int(o) for o in turn_ops), tuple(int(o) for o in move_ops), list(box_ops), list(seed_ops)
    assert len(turn_ops) == 5 and any(o >= 0 for o in turn_ops), "turn_ops: five op indices, at least one of them >= 0"
    T = 1 + int(max_dist)
    want = sum(1 << t for t, o in enumerate(turn_ops) if o >= 0)

    def propose(venv, rows, src_env=None):
        if any_color or diagonal:
            objs = venv.objects(rows, max_components=max_components, skip_color=skip_color, any_color=any_color, diagonal=diagonal, bits=True)
        else:
            objs = venv.components(rows, max_components=max_components, skip_color=skip_color, bits=True)
        tm = turn_macros(objs, venv.turn(rows, objs, src_env, max_dist, want), turn_ops, move_ops, T)
        if not box_ops and not seed_ops:
            return tm
        single = object_actions(objs, box_ops, seed_ops, masks=True)
        M, K1 = (int(v) for v in single["operation"].shape)
        dev = single["bits"].device
        b1 = torch.zeros((M, K1, T, int(single["bits"].shape[-1])), dtype=torch.uint8, device=dev)
        b1[:, :, 0] = single["bits"]
        o1 = torch.full((M, K1, T), -1, dtype=torch.int32, device=dev)
        o1[:, :, 0] = single["operation"]
        return {"bits": torch.cat([b1, tm["bits"]], 1).contiguous(), "operation": torch.cat([o1, tm["operation"]], 1).contiguous(),
                "length": torch.cat([torch.ones((M, K1), dtype=torch.int32, device=dev), tm["length"]], 1).contiguous()}
    propose.wants_src = True
    return propose


# ---- the offset at which the grid or the input best fits the answer's canvas ------------------------------------------------------
ALIGN_GRID, ALIGN_INPUT = 1, 2  # ARCLE_ALIGN_*: slot s of the output <-> bit s


def align_numpy(grid, grid_dim, inp, input_dim, answer, answer_dim, max_dist=None, sources=3, blank=True, full=False):
    """The best offset of the grid and of the input of ONE state on the answer's canvas as arcle_align_rows reports it
    (include/arcle_hip.h) — the host mirror, straight from the definition: every child grid is built and counted.  grid, inp, answer
    int8 [H, W]; max_dist None: no limit; sources = ALIGN_GRID | ALIGN_INPUT; blank = what Paste does (True: the clip's whole
    rectangle is written; False: its positive cells only).  -> (align int32 [2, 8] = ox, oy, correct, total, sh, sw, ah, aw per
    source — slot 0 the grid, slot 1 the input; the slot of a source not asked for stays zero —, base (correct, total) of the grid
    itself); full=True adds table int32 [2, 2H - 1, 2W - 1]: correct(ox, oy) at [ox + H - 1, oy + W - 1], -1 outside T, and children
    int8 [2, 2H - 1, 2W - 1, H, W]: the child grid of every candidate on the whole plane.  The child of (ox, oy): the all-zero ah x aw
    grid resize_grid leaves, with the clip — the source's rectangle [max(ox, 0), min(sh, ah + ox)) x [max(oy, 0), min(sw, aw + oy)) —
    written with its corner at (max(-ox, 0), max(-oy, 0)); the candidates are -ah < ox < sh, -aw < oy < sw within max_dist; ties go to
    the smaller |ox| + |oy|, then the smaller ox, then the smaller oy.  A dim of 0: (0, 0, 0, 0, sh, sw, ah, aw)."""
    grid, inp, answer = (np.asarray(a).astype(np.int8) for a in (grid, inp, answer))
    H, W = grid.shape
    gh, gw = min(int(grid_dim[0]), H), min(int(grid_dim[1]), W)
    ah, aw = min(int(answer_dim[0]), H), min(int(answer_dim[1]), W)
    mh, mw = min(gh, ah), min(gw, aw)
    D = 2 * (H + W) if max_dist is None else int(max_dist)
    total = mh * mw + (abs(ah * aw - gh * gw) if (gh <= ah) == (gw <= aw) else abs(gh - ah) * mw + abs(gw - aw) * mh)
    base = (int((grid[:mh, :mw] == answer[:mh, :mw]).sum()), total)
    align = np.zeros((2, 8), np.int32)
    table = np.full((2, 2 * H - 1, 2 * W - 1), -1, np.int32)
    children = np.zeros((2, 2 * H - 1, 2 * W - 1, H, W), np.int8) if full else None
    for s, (src, dim) in enumerate(((grid, grid_dim), (inp, input_dim))):
        if not (int(sources) >> s) & 1:
            continue
        sh, sw = max(min(int(dim[0]), H), 0), max(min(int(dim[1]), W), 0)
        best = None
        some = min(sh, sw, ah, aw) >= 1  # (a dim of 0: T is empty)
        for ox in range(1 - ah, sh) if some else ():
            for oy in range(1 - aw, sw):
                if abs(ox) + abs(oy) > D:
                    continue
                clip = src[max(ox, 0):min(sh, ah + ox), max(oy, 0):min(sw, aw + oy)]
                child = np.zeros((H, W), np.int8)
                px, py = max(-ox, 0), max(-oy, 0)
                child[px:px + clip.shape[0], py:py + clip.shape[1]] = clip if blank else np.where(clip > 0, clip, 0)
                c = int((child[:ah, :aw] == answer[:ah, :aw]).sum())
                table[s, ox + H - 1, oy + W - 1] = c
                if full:
                    children[s, ox + H - 1, oy + W - 1] = child
                key = (-c, abs(ox) + abs(oy), ox, oy)
                if best is None or key < best:
                    best = key
        align[s] = (best[2], best[3], -best[0], ah * aw, sh, sw, ah, aw) if best is not None else (0, 0, 0, 0, sh, sw, ah, aw)
    return (align, base, table, children) if full else (align, base)


def _rect_bits(x1, x2, y1, y2, H, W):
    """The bit rows (`pack_bits`) of the inclusive rectangles rows [x1, x2] x columns [y1, y2], tensors of one shape [...]: uint8 [..., 128]"""
    dev = x1.device
    r = torch.arange(H, device=dev).reshape(H, 1)
    c = torch.arange(W, device=dev).reshape(1, W)
    x1, x2, y1, y2 = (v.to(torch.int64).reshape(tuple(v.shape) + (1, 1)) for v in (x1, x2, y1, y2))
    return pack_bits((r >= x1) & (r <= x2) & (c >= y1) & (c <= y2))


def align_macros(alignments, copy_ops, resize_op, paste_op, H, W):
    """The best offset of every source (`ARCVecEnv.align` -> Alignments) as ONE three-step macro per source: {"bits": uint8 [M, 2, 3, 128],
    "operation": int32 [M, 2, 3], "length": int32 [M, 2]}.  Step 0 is the source's rectangle R = [max(ox, 0), min(sh, ah + ox)) x
    [max(oy, 0), min(sw, aw + oy)) with the source's Copy — copy_ops = (Copy_O index, Copy_I index): slot 0 copies from the grid, slot
    1 from the input —, step 1 the canvas rectangle (0, 0)..(ah - 1, aw - 1) with resize_op (resize_grid), step 2 the one-bit row of
    P = (max(-ox, 0), max(-oy, 0)) with paste_op; H, W = the plane's size.  A slot with total == 0 (not asked for, or no candidate) or
    that does not beat the row's own ratio — correct * base_total <= base_correct * total, in integers: this drops the identity, the
    grid at (0, 0) under equal dims — gets operation -1 at step 0 and length 1: one ARCLE_ST_BAD_OP child, dropped by beam_search.
    Built on the device from the eight words of each slot with `pack_bits`: no host synchronisation."""
    a = alignments
    dev = a.ox.device
    M = int(a.ox.shape[0])
    ox, oy = a.ox.to(torch.int64), a.oy.to(torch.int64)
    sh, sw = a.src_dim[..., 0].to(torch.int64), a.src_dim[..., 1].to(torch.int64)
    ah, aw = a.ans_dim[..., 0].to(torch.int64), a.ans_dim[..., 1].to(torch.int64)
    zero = torch.zeros_like(ox)
    bc, bt = a.base[:, 0].to(torch.int64).reshape(M, 1), a.base[:, 1].to(torch.int64).reshape(M, 1)
    ok = (a.total > 0) & (a.correct.to(torch.int64) * bt > bc * a.total.to(torch.int64))
    px, py = torch.maximum(-ox, zero), torch.maximum(-oy, zero)
    bits = torch.stack([_rect_bits(torch.maximum(ox, zero), torch.minimum(sh, ah + ox) - 1, torch.maximum(oy, zero), torch.minimum(sw, aw + oy) - 1, H, W),
                        _rect_bits(zero, ah - 1, zero, aw - 1, H, W), _rect_bits(px, px, py, py, H, W)], 2)
    bits = torch.where(ok.reshape(M, 2, 1, 1), bits, torch.zeros((), dtype=torch.uint8, device=dev))
    copy = torch.as_tensor([int(copy_ops[0]), int(copy_ops[1])], dtype=torch.int32, device=dev).reshape(1, 2)
    op = torch.stack([copy.expand(M, 2), torch.full((M, 2), int(resize_op), dtype=torch.int32, device=dev),
                      torch.full((M, 2), int(paste_op), dtype=torch.int32, device=dev)], 2)
    op = torch.where(ok.reshape(M, 2, 1), op, torch.full((), -1, dtype=torch.int32, device=dev))
    length = torch.where(ok, torch.full((), 3, dtype=torch.int32, device=dev), torch.ones((), dtype=torch.int32, device=dev))
    return {"bits": bits.contiguous(), "operation": op.to(torch.int32).contiguous(), "length": length.to(torch.int32).contiguous()}


def propose_alignments(copy_ops, resize_op, paste_op, blank=True, sources=3, max_dist=None, box_ops=(), seed_ops=(), max_components=16, skip_color=0,
                       any_color=False, diagonal=False):
    """A `propose` for beam_search that answers "at which offset does the grid, or the input, fit the answer's canvas?" — the one
    proposer whose children have another grid_dim than their parent: at every depth, for each frontier state, ONE macro of three steps
    per source asked for — the source's Copy on the rectangle the canvas covers, resize_op (resize_grid) to the answer's dims, paste_op
    at the corner (`venv.align`, one launch; `align_macros`): K = 2, T = 3.  copy_ops = (Copy_O index, Copy_I index); blank must say
    what paste_op does in the caller's table (True: paste_blank, both default tables).  With box_ops / seed_ops the singles of
    `object_actions(masks=True)` on the objects of each state's grid come first, as macros of length 1, the way `propose_placements`
    puts them: K = C * (len(box_ops) + len(seed_ops)) + 2.  It looks at the answer of each row's env, so it carries `wants_src = True`
    and beam_search calls it with (venv, rows, src_env)."""
    copy_ops, resize_op, paste_op = tuple(int(o) for o in copy_ops), int(resize_op), int(paste_op)
    box_ops, seed_ops = list(box_ops), list(seed_ops)

    def propose(venv, rows, src_env=None):
        am = align_macros(venv.align(rows, src_env, max_dist, sources, blank), copy_ops, resize_op, paste_op, venv.H, venv.W)
        if not box_ops and not seed_ops:
            return am
        if any_color or diagonal:
            objs = venv.objects(rows, max_components=max_components, skip_color=skip_color, any_color=any_color, diagonal=diagonal, bits=True)
        else:
            objs = venv.components(rows, max_components=max_components, skip_color=skip_color, bits=True)
        single = object_actions(objs, box_ops, seed_ops, masks=True)
        M, K1 = (int(v) for v in single["operation"].shape)
        dev = single["bits"].device
        b1 = torch.zeros((M, K1, 3, int(single["bits"].shape[-1])), dtype=torch.uint8, device=dev)
        b1[:, :, 0] = single["bits"]
        o1 = torch.full((M, K1, 3), -1, dtype=torch.int32, device=dev)
        o1[:, :, 0] = single["operation"]
        return {"bits": torch.cat([b1, am["bits"]], 1).contiguous(), "operation": torch.cat([o1, am["operation"]], 1).contiguous(),
                "length": torch.cat([torch.ones((M, K1), dtype=torch.int32, device=dev), am["length"]], 1).contiguous()}
    propose.wants_src = True
    return propose


# ---- the lines each object casts toward the answer ---------------------------------------------------------------------------------
# bit d of a direction mask (ARCLE_RAY_*) -> (dx, dy): N, S, W, E, NW, NE, SW, SE; x runs along rows
RAY_DIRS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))
# the default candidates of `ARCVecEnv.rays` / `propose_rays`: the eight single directions, N|S, W|E, the orthogonal four, the diagonal
# four, all eight
RAY_SETS = (1, 2, 4, 8, 16, 32, 64, 128, 3, 12, 15, 240, 255)


def ray_numpy(grid, grid_dim, answer, answer_dim, masks, sets=None, free_color=0, through=False, full=False):
    """The rays of every object of ONE grid as arcle_ray_rows reports them (include/arcle_hip.h) — the host mirror, straight from the
    definition and deliberately not a bit-board algorithm: from every cell of the object a walk in every direction, cell by cell.
    grid, answer int8 [H, W]; masks [n, H, W] (truthy = the object's cells; cells outside grid_dim are ignored); sets: direction masks
    (bit 0..7 = N, S, W, E, NW, NE, SW, SE; None: RAY_SETS); free_color: the byte (as int8) a ray may enter; through=True: a ray
    enters every cell of grid_dim outside the object.  -> (ray int32 [n, S, 4] = color, correct, cells, right; best int32 [n, 4] =
    set, color, correct, cells; base (correct, total) of the grid itself); full=True adds cells bool [n, S, H, W]: every candidate's
    selection.  A walk starts at a cell of B, takes the next cell while it lies inside grid_dim, is not in B and (through, or its byte
    is free_color), and stops at the first that is not.  color = the c in 0..9 most frequent in the answer under the candidate's cells
    inside the common rectangle (ties: the smaller c), right = that frequency, correct = the correct cells of the grid with those
    cells painted c.  An empty candidate: (0, base correct, 0, 0).  best: the most correct among the non-empty candidates, then the
    fewest cells, then the lowest set; none: (-1, 0, base correct, 0)."""
    grid, answer = np.asarray(grid).astype(np.int8), np.asarray(answer).astype(np.int8)
    H, W = grid.shape
    gh, gw = min(int(grid_dim[0]), H), min(int(grid_dim[1]), W)
    ah, aw = min(int(answer_dim[0]), H), min(int(answer_dim[1]), W)
    mh, mw = min(gh, ah), min(gw, aw)
    total = mh * mw + (abs(ah * aw - gh * gw) if (gh <= ah) == (gw <= aw) else abs(gh - ah) * mw + abs(gw - aw) * mh)
    base = (int((grid[:mh, :mw] == answer[:mh, :mw]).sum()), total)
    sets = [int(s) & 255 for s in (RAY_SETS if sets is None else sets)]
    fc = (int(free_color) + 128) % 256 - 128
    masks = np.asarray(masks).reshape(-1, H, W)
    n, S_ = masks.shape[0], len(sets)
    ray, best = np.zeros((n, S_, 4), np.int32), np.zeros((n, 4), np.int32)
    cells = np.zeros((n, S_, H, W), bool)
    for k in range(n):
        B = np.zeros((H, W), bool)
        B[:gh, :gw] = masks[k, :gh, :gw] != 0
        per_dir = np.zeros((8, H, W), bool)
        for x, y in np.argwhere(B):
            for d, (dx, dy) in enumerate(RAY_DIRS):
                i, j = x + dx, y + dy
                while 0 <= i < gh and 0 <= j < gw and not B[i, j] and (through or grid[i, j] == fc):
                    per_dir[d, i, j] = True
                    i, j = i + dx, j + dy
        top = None
        for s, m in enumerate(sets):
            R = np.zeros((H, W), bool)
            for d in range(8):
                if (m >> d) & 1:
                    R |= per_dir[d]
            cells[k, s] = R
            if not R.any():
                ray[k, s] = (0, base[0], 0, 0)
                continue
            under = answer[:mh, :mw][R[:mh, :mw]]
            freq = [int((under == c).sum()) for c in range(10)]
            color = int(np.argmax(freq))  # (the first maximum: the smaller c)
            child = grid.copy()
            child[R] = color
            ray[k, s] = (color, int((child[:mh, :mw] == answer[:mh, :mw]).sum()), int(R.sum()), freq[color])
            key = (-int(ray[k, s, 1]), int(ray[k, s, 2]), s)
            if top is None or key < top:
                top = key
        best[k] = (-1, 0, base[0], 0) if top is None else (top[2], ray[k, top[2], 0], -top[0], top[1])
    return (ray, best, base, cells) if full else (ray, best, base)


def ray_actions(objs, rays, color_ops):
    """The best ray candidate of every object (`ARCVecEnv.rays` -> Rays, with its bit rows) as ONE single-step candidate per object:
    {"bits": uint8 [M, C, 128] = rays.best_bits, "operation": int32 [M, C] = color_ops[best_color]} — color_ops[c] = the index of
    `Color c` in the caller's op table, c = 0..9.  Slots with k >= count, without a candidate (best_set < 0) or whose step would not
    gain (best_correct <= base correct) get operation -1 and a zero bit row: an ARCLE_ST_BAD_OP child, dropped by beam_search.  Pure
    indexing on the device: no host synchronisation."""
    assert rays.best_bits is not None, "ray_actions needs the candidates' bit rows (rays(bits=True))"
    dev = rays.best_bits.device
    M, C = (int(v) for v in rays.best_set.shape)
    ops = torch.as_tensor(list(color_ops), dtype=torch.int32, device=dev)
    assert int(ops.numel()) == 10, "color_ops: the ten Color ops, color_ops[c] paints c"
    there = torch.arange(C, device=dev).reshape(1, C) < objs.count.reshape(M, 1)
    ok = there & (rays.best_set >= 0) & (rays.best_correct > rays.base[:, 0].reshape(M, 1))
    op = torch.where(ok, ops[rays.best_color.clamp(0, 9).to(torch.int64)], torch.full((), -1, dtype=torch.int32, device=dev))
    bits = torch.where(ok.reshape(M, C, 1), rays.best_bits, torch.zeros((), dtype=torch.uint8, device=dev))
    return {"bits": bits.contiguous(), "operation": op.to(torch.int32).contiguous()}


def propose_rays(color_ops, sets=None, free_color=0, through=False, box_ops=(), seed_ops=(), max_components=16, skip_color=0, any_color=False,
                 diagonal=False):
    """A `propose` for beam_search that answers "which lines does this object cast?": at every depth the objects of each frontier
    state's grid (`venv.objects` / `venv.components` with their bit rows), first the singles of `object_actions(masks=True)` — box_ops
    on the objects' exact cells, seed_ops on their seeds — then for every object ONE step: `Color c` on the cells of its best set of
    rays (`venv.rays`, one launch; `ray_actions`), K = C * (len(box_ops) + len(seed_ops) + 1).  color_ops[c] = the index of `Color c`
    in the env's op table (both default tables: range(10)); sets, free_color, through as for `ARCVecEnv.rays`.  These are single
    steps: beam_search takes them through `venv.expand` / `venv.transition`.  It looks at the answer of each row's env, so it carries
    `wants_src = True` and beam_search calls it with (venv, rows, src_env)."""
    color_ops, box_ops, seed_ops = [int(o) for o in color_ops], list(box_ops), list(seed_ops)

    def propose(venv, rows, src_env=None):
        if any_color or diagonal:
            objs = venv.objects(rows, max_components=max_components, skip_color=skip_color, any_color=any_color, diagonal=diagonal, bits=True)
        else:
            objs = venv.components(rows, max_components=max_components, skip_color=skip_color, bits=True)
        ra = ray_actions(objs, venv.rays(rows, objs, sets, free_color, through, src_env), color_ops)
        if not box_ops and not seed_ops:
            return ra
        single = object_actions(objs, box_ops, seed_ops, masks=True)
        return {"bits": torch.cat([single["bits"], ra["bits"]], 1).contiguous(), "operation": torch.cat([single["operation"], ra["operation"]], 1).contiguous()}
    propose.wants_src = True
    return propose


# ---- each object's box filled from its mirror image ---------------------------------------------------------------------------------
MIRROR_H, MIRROR_V, MIRROR_POINT = 1, 2, 4  # ARCLE_MIRROR_*: slot s of the output <-> bit s


def _flipped(tile, s):
    return (np.fliplr(tile), np.flipud(tile), np.flipud(np.fliplr(tile)))[s]


def mirror_numpy(grid, grid_dim, answer, answer_dim, masks, max_dist=None, mirrors=7, blank=True, full=False):
    """The best source rectangle of every object of ONE grid under each of the three symmetries, as arcle_mirror_rows reports it
    (include/arcle_hip.h) — the host mirror, straight from the definition: every child grid is built with np.fliplr / np.flipud and
    counted.  grid, answer int8 [H, W]; masks [n, H, W] (truthy = the object's cells; cells outside grid_dim are ignored); max_dist
    None: no limit; mirrors = the mask of the symmetries asked for (bit s = slot s: left-right H, up-down V, point); blank = what
    Paste does (True: the clip's whole rectangle is written; False: its positive cells only).  -> (mirror int32 [n, 3, 4] = dx, dy,
    correct, valid — zeros in the slots not asked for —, base (correct, total) of the grid itself); full=True adds table int32 [n, 3,
    2H - 1, 2W - 1]: correct(s, dx, dy) at [dx + H - 1, dy + W - 1], -1 outside the candidates.  The child of (s, dx, dy): the grid
    with the object's h x w box replaced by pos(flip_s(T)), T = the tile Copy + Paste leave there — the source rectangle R, the box
    moved by (dx, dy), as it is (blank) or its positive cells over the box's own old cells (not blank) —, pos(v) = v if v > 0 else 0:
    what CopyO on R + Paste at the box's corner + Flip of the box leave; R lies inside grid_dim, dx = 0 in slot H, dy = 0 in slot V;
    ties go to the smaller |dx| + |dy|, then the smaller dx, then the smaller dy.  No candidate: (0, 0, 0, 0); an empty object: (0,
    0, base correct, 1)."""
    grid, answer = np.asarray(grid).astype(np.int8), np.asarray(answer).astype(np.int8)
    H, W = grid.shape
    gh, gw = min(int(grid_dim[0]), H), min(int(grid_dim[1]), W)
    ah, aw = min(int(answer_dim[0]), H), min(int(answer_dim[1]), W)
    mh, mw = min(gh, ah), min(gw, aw)
    D = 2 * (H + W) if max_dist is None else int(max_dist)
    total = mh * mw + (abs(ah * aw - gh * gw) if (gh <= ah) == (gw <= aw) else abs(gh - ah) * mw + abs(gw - aw) * mh)
    base = (int((grid[:mh, :mw] == answer[:mh, :mw]).sum()), total)
    masks = np.asarray(masks).reshape(-1, H, W)
    n = masks.shape[0]
    mirror = np.zeros((n, 3, 4), np.int32)
    table = np.full((n, 3, 2 * H - 1, 2 * W - 1), -1, np.int32)
    for k in range(n):
        B = np.zeros((H, W), bool)
        B[:gh, :gw] = masks[k, :gh, :gw] != 0
        bx, by = np.nonzero(B)
        for s in range(3):
            if not (int(mirrors) >> s) & 1:
                continue
            if not len(bx):
                mirror[k, s] = (0, 0, base[0], 1)
                continue
            x0, x1, y0, y1 = int(bx.min()), int(bx.max()), int(by.min()), int(by.max())
            h, w = x1 - x0 + 1, y1 - y0 + 1
            old = grid[x0:x1 + 1, y0:y1 + 1]
            best = None
            for sx in ((x0,) if s == 0 else range(0, gh - h + 1)):
                for sy in ((y0,) if s == 1 else range(0, gw - w + 1)):
                    dx, dy = sx - x0, sy - y0
                    if abs(dx) + abs(dy) > D:
                        continue
                    tile = grid[sx:sx + h, sy:sy + w]
                    if not blank:
                        tile = np.where(tile > 0, tile, old)
                    tile = _flipped(tile, s)
                    child = grid.copy()
                    child[x0:x1 + 1, y0:y1 + 1] = np.where(tile > 0, tile, 0)
                    c = int((child[:mh, :mw] == answer[:mh, :mw]).sum())
                    table[k, s, dx + H - 1, dy + W - 1] = c
                    key = (-c, abs(dx) + abs(dy), dx, dy)
                    if best is None or key < best:
                        best = key
            if best is not None:
                mirror[k, s] = (best[2], best[3], -best[0], 1)
    return (mirror, base, table) if full else (mirror, base)


def mirror_macros(objs, mirrors, copy_op, paste_op, flip_ops, H, W):
    """The best mirror image of every object's box (`ARCVecEnv.mirror` -> Mirrors) as ONE macro per object: {"bits": uint8 [M, C, 4,
    128], "operation": int32 [M, C, 4], "length": int32 [M, C]}.  Step 0 is the source rectangle R — the object's box (objs.box) moved
    by (dx, dy) — with copy_op (CopyO), step 1 the one-bit row of the box's corner (x0, y0) with paste_op, step 2 the box's rectangle
    with FlipH (slots H and POINT) or FlipV (slot V), step 3 (slot POINT only) FlipV on the zero mask, which continues the active
    object (object.py:102-107): lengths 3, 3, 4.  flip_ops = (FlipH index, FlipV index), -1 where the table has none; H, W = the
    plane's size.  Per object the best valid slot that has its ops: more correct, then fewer steps, then the lower slot.  Slots with
    k >= count, no valid slot or correct <= base[0] (the mirror gains nothing) get operation -1 at step 0 and length 1: one
    ARCLE_ST_BAD_OP child, dropped by beam_search.  Built on the device with `pack_bits`: no host synchronisation."""
    dev = objs.box.device
    M, C = int(objs.box.shape[0]), int(objs.box.shape[1])
    fh, fv = int(flip_ops[0]), int(flip_ops[1])
    has = torch.as_tensor([fh >= 0, fv >= 0, fh >= 0 and fv >= 0], device=dev).reshape(1, 1, 3)
    steps = torch.as_tensor([3, 3, 4], dtype=torch.int64, device=dev).reshape(1, 1, 3)
    usable = (mirrors.valid != 0) & has
    score = mirrors.correct.to(torch.int64) * 64 - steps * 8 - torch.arange(3, device=dev).reshape(1, 1, 3)
    score = torch.where(usable, score, torch.full((), -1, dtype=torch.int64, device=dev))
    pick = score.argmax(-1, keepdim=True)
    dx, dy = mirrors.dx.gather(-1, pick).reshape(M, C).to(torch.int64), mirrors.dy.gather(-1, pick).reshape(M, C).to(torch.int64)
    correct = mirrors.correct.gather(-1, pick).reshape(M, C)
    pick = pick.reshape(M, C)
    there = torch.arange(C, device=dev).reshape(1, C) < objs.count.reshape(M, 1)
    ok = there & usable.any(-1) & (correct > mirrors.base[:, 0].reshape(M, 1))
    x0, y0, x1, y1 = (objs.box[..., i].to(torch.int64) for i in range(4))
    last = pick == 2
    corner = _rect_bits(x0, x0, y0, y0, H, W)
    bits = torch.stack([_rect_bits(x0 + dx, x1 + dx, y0 + dy, y1 + dy, H, W), corner, _rect_bits(x0, x1, y0, y1, H, W), torch.zeros_like(corner)], 2)
    bits = torch.where(ok.reshape(M, C, 1, 1), bits, torch.zeros((), dtype=torch.uint8, device=dev))
    minus = torch.full((M, C), -1, dtype=torch.int32, device=dev)
    flip = torch.where(pick == 1, fv, fh).to(torch.int32)
    op = torch.stack([torch.full((M, C), int(copy_op), dtype=torch.int32, device=dev), torch.full((M, C), int(paste_op), dtype=torch.int32, device=dev),
                      flip, torch.where(last, torch.full((), fv, dtype=torch.int32, device=dev), minus)], 2)
    op = torch.where(ok.reshape(M, C, 1), op, minus.reshape(M, C, 1))
    length = torch.where(ok, torch.where(last, 4, 3), 1).to(torch.int32)
    return {"bits": bits.contiguous(), "operation": op.to(torch.int32).contiguous(), "length": length.contiguous()}


def propose_mirrors(copy_op, paste_op, flip_ops, box_ops=(), seed_ops=(), max_dist=None, max_components=16, skip_color=0, any_color=False,
                    diagonal=False, blank=True):
    """A `propose` for beam_search that answers "what belongs here by symmetry?": at every depth the objects of each frontier state's
    grid (`venv.objects` / `venv.components` with their bit rows), first the singles of `object_actions(masks=True)` — box_ops on the
    objects' exact cells, seed_ops on their seeds — as macros of length 1, then for every object ONE macro of three or four steps: copy_op
    (CopyO) on the rectangle whose mirror image fits the object's box best, paste_op at the box's corner, the Flip(s) of the box
    (`venv.mirror`, one launch; `mirror_macros`), K = C * (len(box_ops) + len(seed_ops) + 1), T = 4.  flip_ops = (FlipH index, FlipV
    index), -1 where the table has none: only the symmetries whose ops the table has are asked for.  blank must say what paste_op does
    in the caller's table (True: paste_blank, both default tables).  With skip_color = 0 the holes of a pattern are NOT objects: pass
    skip_color = -1 (and any_color = False) to get the zero-coloured components.  It looks at the answer of each row's env, so it
    carries `wants_src = True` and beam_search calls it with (venv, rows, src_env)."""
    copy_op, paste_op, flip_ops = int(copy_op), int(paste_op), tuple(int(o) for o in flip_ops)
    box_ops, seed_ops = list(box_ops), list(seed_ops)
    assert len(flip_ops) == 2 and any(o >= 0 for o in flip_ops), "flip_ops: (FlipH index, FlipV index), at least one of them >= 0"
    want = (MIRROR_H if flip_ops[0] >= 0 else 0) | (MIRROR_V if flip_ops[1] >= 0 else 0) | (MIRROR_POINT if min(flip_ops) >= 0 else 0)
    T = 4

    def propose(venv, rows, src_env=None):
        if any_color or diagonal:
            objs = venv.objects(rows, max_components=max_components, skip_color=skip_color, any_color=any_color, diagonal=diagonal, bits=True)
        else:
            objs = venv.components(rows, max_components=max_components, skip_color=skip_color, bits=True)
        mm = mirror_macros(objs, venv.mirror(rows, objs, src_env, max_dist, want, blank), copy_op, paste_op, flip_ops, venv.H, venv.W)
        if not box_ops and not seed_ops:
            return mm
        single = object_actions(objs, box_ops, seed_ops, masks=True)
        M, K1 = (int(v) for v in single["operation"].shape)
        dev = single["bits"].device
        b1 = torch.zeros((M, K1, T, int(single["bits"].shape[-1])), dtype=torch.uint8, device=dev)
        b1[:, :, 0] = single["bits"]
        o1 = torch.full((M, K1, T), -1, dtype=torch.int32, device=dev)
        o1[:, :, 0] = single["operation"]
        return {"bits": torch.cat([b1, mm["bits"]], 1).contiguous(), "operation": torch.cat([o1, mm["operation"]], 1).contiguous(),
                "length": torch.cat([torch.ones((M, K1), dtype=torch.int32, device=dev), mm["length"]], 1).contiguous()}
    propose.wants_src = True
    return propose


# ---- the cells around and inside each object ----------------------------------------------------------------------------------------
# the codes of a candidate region (ARCLE_REGION_*)
REGION_NONE, REGION_HALO4, REGION_HALO8, REGION_BOX_REST, REGION_BOX_FRAME, REGION_INSIDE, REGION_BOX, REGION_SELF = range(8)
# the default candidates of `ARCVecEnv.regions` / `propose_regions`
REGION_KINDS = (1, 2, 3, 4, 5, 6, 7)


def region_numpy(grid, grid_dim, answer, answer_dim, masks, kinds=None, free_color=0, through=False, full=False):
    """The regions of every object of ONE grid as arcle_region_rows reports them (include/arcle_hip.h) — the host mirror and the
    normative statement, straight from the definition and deliberately not a bit-board algorithm: neighbourhoods by array slices,
    INSIDE by a cell-by-cell flood from the edge of grid_dim.  grid, answer int8 [H, W]; masks [n, H, W] (truthy = the object's cells;
    cells outside grid_dim are ignored); kinds: region codes (0 none, 1 HALO4, 2 HALO8, 3 BOX_REST, 4 BOX_FRAME, 5 INSIDE, 6 BOX,
    7 SELF; a code above 7 counts as 0; None: REGION_KINDS); free_color: the byte (as int8) a cell outside the object must hold to be
    painted; through=True: every cell may be.  -> (region int32 [n, S, 4] = color, correct, cells, right; best int32 [n, 4] = index,
    color, correct, cells; base (correct, total) of the grid itself); full=True adds cells bool [n, S, H, W]: every candidate's
    selection.  With IN = the cells inside grid_dim, B = the object's cells in IN, box = B's bounding rectangle: HALO4 / HALO8 = the
    cells of IN & ~B with a 4- / 8-neighbour in B; BOX_REST = box & ~B; BOX_FRAME = the rectangle one cell larger than box on every
    side, minus box, clipped to IN; INSIDE = the cells of IN & ~B from which no 4-connected path through IN & ~B leads to a cell on
    the edge of grid_dim (an edge cell is never inside); BOX = box; SELF = B; an empty B gives empty regions.  The candidate's cells
    are R = region & (B | FREE), FREE = the cells of IN whose byte is free_color (through: IN).  color = the c in 0..9 most frequent
    in the answer under R inside the common rectangle (ties: the smaller c), right = that frequency, correct = the correct cells of
    the grid with R painted c.  An empty candidate: (0, base correct, 0, 0).  best: the most correct among the non-empty candidates,
    then the fewest cells, then the lowest index; none: (-1, 0, base correct, 0)."""
    grid, answer = np.asarray(grid).astype(np.int8), np.asarray(answer).astype(np.int8)
    H, W = grid.shape
    gh, gw = min(int(grid_dim[0]), H), min(int(grid_dim[1]), W)
    ah, aw = min(int(answer_dim[0]), H), min(int(answer_dim[1]), W)
    mh, mw = min(gh, ah), min(gw, aw)
    total = mh * mw + (abs(ah * aw - gh * gw) if (gh <= ah) == (gw <= aw) else abs(gh - ah) * mw + abs(gw - aw) * mh)
    base = (int((grid[:mh, :mw] == answer[:mh, :mw]).sum()), total)
    kinds = [int(k) if 0 <= int(k) <= 7 else 0 for k in (REGION_KINDS if kinds is None else kinds)]
    fc = (int(free_color) + 128) % 256 - 128
    masks = np.asarray(masks).reshape(-1, H, W)
    n, S_ = masks.shape[0], len(kinds)
    region, best = np.zeros((n, S_, 4), np.int32), np.zeros((n, 4), np.int32)
    cells = np.zeros((n, S_, H, W), bool)
    IN = np.zeros((H, W), bool)
    IN[:gh, :gw] = True
    FREE = IN & (True if through else grid == fc)

    def grown(X, diagonal):
        out = np.zeros((H + 2, W + 2), bool)
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                if (dx or dy) and (diagonal or not (dx and dy)):
                    out[1 + dx:1 + dx + H, 1 + dy:1 + dy + W] |= X
        return out[1:-1, 1:-1]
    for k in range(n):
        B = np.zeros((H, W), bool)
        B[:gh, :gw] = masks[k, :gh, :gw] != 0
        per = np.zeros((8, H, W), bool)
        if B.any():
            xs, ys = np.nonzero(B)
            x0, x1, y0, y1 = int(xs.min()), int(xs.max()), int(ys.min()), int(ys.max())
            box = np.zeros((H, W), bool)
            box[x0:x1 + 1, y0:y1 + 1] = True
            outer = np.zeros((H, W), bool)
            outer[max(x0 - 1, 0):x1 + 2, max(y0 - 1, 0):y1 + 2] = True
            per[1], per[2] = grown(B, False) & IN & ~B, grown(B, True) & IN & ~B
            per[3], per[4], per[6], per[7] = box & ~B, outer & ~box & IN, box, B
            M = IN & ~B
            out = np.zeros((H, W), bool)
            stack = [(i, j) for i in range(gh) for j in range(gw) if M[i, j] and (i in (0, gh - 1) or j in (0, gw - 1))]
            for i, j in stack:
                out[i, j] = True
            while stack:
                i, j = stack.pop()
                for a, b in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
                    if 0 <= a < gh and 0 <= b < gw and M[a, b] and not out[a, b]:
                        out[a, b] = True
                        stack.append((a, b))
            per[5] = M & ~out
        top = None
        for s, code in enumerate(kinds):
            R = per[code] & (B | FREE)
            cells[k, s] = R
            if not R.any():
                region[k, s] = (0, base[0], 0, 0)
                continue
            under = answer[:mh, :mw][R[:mh, :mw]]
            freq = [int((under == c).sum()) for c in range(10)]
            color = int(np.argmax(freq))  # (the first maximum: the smaller c)
            child = grid.copy()
            child[R] = color
            region[k, s] = (color, int((child[:mh, :mw] == answer[:mh, :mw]).sum()), int(R.sum()), freq[color])
            key = (-int(region[k, s, 1]), int(region[k, s, 2]), s)
            if top is None or key < top:
                top = key
        best[k] = (-1, 0, base[0], 0) if top is None else (top[2], region[k, top[2], 0], -top[0], top[1])
    return (region, best, base, cells) if full else (region, best, base)


def region_actions(objs, regions, color_ops):
    """The best region of every object (`ARCVecEnv.regions` -> Regions, with its bit rows) as ONE single-step candidate per object:
    {"bits": uint8 [M, C, 128] = regions.best_bits, "operation": int32 [M, C] = color_ops[best_color]} — color_ops[c] = the index of
    `Color c` in the caller's op table, c = 0..9.  Slots with k >= count, without a candidate (best_kind < 0) or whose step would not
    gain (best_correct <= base correct) get operation -1 and a zero bit row: an ARCLE_ST_BAD_OP child, dropped by beam_search.  Pure
    indexing on the device: no host synchronisation."""
    assert regions.best_bits is not None, "region_actions needs the candidates' bit rows (regions(bits=True))"
    dev = regions.best_bits.device
    M, C = (int(v) for v in regions.best_kind.shape)
    ops = torch.as_tensor(list(color_ops), dtype=torch.int32, device=dev)
    assert int(ops.numel()) == 10, "color_ops: the ten Color ops, color_ops[c] paints c"
    there = torch.arange(C, device=dev).reshape(1, C) < objs.count.reshape(M, 1)
    ok = there & (regions.best_kind >= 0) & (regions.best_correct > regions.base[:, 0].reshape(M, 1))
    op = torch.where(ok, ops[regions.best_color.clamp(0, 9).to(torch.int64)], torch.full((), -1, dtype=torch.int32, device=dev))
    bits = torch.where(ok.reshape(M, C, 1), regions.best_bits, torch.zeros((), dtype=torch.uint8, device=dev))
    return {"bits": bits.contiguous(), "operation": op.to(torch.int32).contiguous()}


def propose_regions(color_ops, kinds=None, free_color=0, through=False, box_ops=(), seed_ops=(), max_components=16, skip_color=0, any_color=False,
                    diagonal=False):
    """A `propose` for beam_search that answers "which cells around or inside this object should be painted?": at every depth the
    objects of each frontier state's grid (`venv.objects` / `venv.components` with their bit rows), first the singles of
    `object_actions(masks=True)` — box_ops on the objects' exact cells, seed_ops on their seeds — then for every object ONE step:
    `Color c` on the cells of its best region (`venv.regions`, one launch; `region_actions`), K = C * (len(box_ops) + len(seed_ops) +
    1).  color_ops[c] = the index of `Color c` in the env's op table (both default tables: range(10)); kinds, free_color, through as
    for `ARCVecEnv.regions`.  These are single steps: beam_search takes them through `venv.expand` / `venv.transition`.  It looks at
    the answer of each row's env, so it carries `wants_src = True` and beam_search calls it with (venv, rows, src_env)."""
    color_ops, box_ops, seed_ops = [int(o) for o in color_ops], list(box_ops), list(seed_ops)

    def propose(venv, rows, src_env=None):
        if any_color or diagonal:
            objs = venv.objects(rows, max_components=max_components, skip_color=skip_color, any_color=any_color, diagonal=diagonal, bits=True)
        else:
            objs = venv.components(rows, max_components=max_components, skip_color=skip_color, bits=True)
        ra = region_actions(objs, venv.regions(rows, objs, kinds, free_color, through, src_env=src_env), color_ops)
        if not box_ops and not seed_ops:
            return ra
        single = object_actions(objs, box_ops, seed_ops, masks=True)
        return {"bits": torch.cat([single["bits"], ra["bits"]], 1).contiguous(), "operation": torch.cat([single["operation"], ra["operation"]], 1).contiguous()}
    propose.wants_src = True
    return propose


# ---- the grid or the input zoomed, shrunk or tiled onto the answer's canvas ---------------------------------------------------------
SCALE_ZOOM, SCALE_SHRINK, SCALE_TILE = 1, 2, 4  # ARCLE_SCALE_*: bit `mode` of `modes` <-> the candidates of that family
SCALE_CANDS = 132


def scale_candidates():
    """The 132 candidates of arcle_scale_rows in index order -> list of (mode 0 ZOOM | 1 SHRINK | 2 TILE, kx, ky): the factors, for a
    TILE whether the tile rows (kx) / the tile columns (ky) are mirrored in every second tile"""
    return [(m, kx, ky) for m in (0, 1) for kx in range(1, 9) for ky in range(1, 9)] + [(2, t >> 1, t & 1) for t in range(4)]


def _scale_map(mode, k, n_out, n_src):
    """f (or g) of one candidate on 0 .. n_out - 1: the source index each takes its cell from, -1 where that lies outside [0, n_src)"""
    t = np.arange(n_out)
    if mode == 0:
        s = t // k
    elif mode == 1:
        s = t * k
    else:
        q, r = t // n_src, t % n_src
        s = np.where((q & 1) & k, n_src - 1 - r, r)
    return np.where(s < n_src, s, -1)


def scale_numpy(grid, grid_dim, inp, input_dim, answer, answer_dim, sources=3, modes=7, full=False):
    """The best zoom, shrink or tiling of the grid and of the input of ONE state onto the answer's canvas as arcle_scale_rows reports it
    (include/arcle_scale_rows.h) — the host mirror, straight from the definition: every child grid is built and counted.  grid, inp, answer
    int8 [H, W]; sources = ALIGN_GRID | ALIGN_INPUT; modes = SCALE_ZOOM | SCALE_SHRINK | SCALE_TILE.  -> (scale int32 [2, 8] = cand,
    correct, total, colours, sh, sw, ah, aw per source — slot 0 the grid, slot 1 the input; the slot of a source not asked for stays
    zero —, base (correct, total) of the grid itself); full=True adds table int32 [2, 132]: correct of every candidate, -1 for a mode
    not asked for (and everywhere in a slot without a candidate), and children int8 [2, 132, H, W]: the child grid of every candidate
    on the whole plane.  The child of candidate (f, g): G'[i, j] = v(f(i), g(j)) on the canvas [0, ah) x [0, aw), v = the source's
    bytes 1 .. 9 inside its dims, 0 for every other byte and index; ties go to the lowest index.  A dim of 0: cand -1, (0, 0, 0)."""
    grid, inp, answer = (np.asarray(a).astype(np.int8) for a in (grid, inp, answer))
    H, W = grid.shape
    gh, gw = min(int(grid_dim[0]), H), min(int(grid_dim[1]), W)
    ah, aw = min(int(answer_dim[0]), H), min(int(answer_dim[1]), W)
    mh, mw = min(gh, ah), min(gw, aw)
    total = mh * mw + (abs(ah * aw - gh * gw) if (gh <= ah) == (gw <= aw) else abs(gh - ah) * mw + abs(gw - aw) * mh)
    base = (int((grid[:mh, :mw] == answer[:mh, :mw]).sum()), total)
    scale = np.zeros((2, 8), np.int32)
    table = np.full((2, SCALE_CANDS), -1, np.int32)
    children = np.zeros((2, SCALE_CANDS, H, W), np.int8)
    for s, (src, dim) in enumerate(((grid, grid_dim), (inp, input_dim))):
        if not (int(sources) >> s) & 1:
            continue
        sh, sw = max(min(int(dim[0]), H), 0), max(min(int(dim[1]), W), 0)
        scale[s] = (-1, 0, 0, 0, sh, sw, ah, aw)
        if min(sh, sw, ah, aw) < 1:
            continue
        v = np.zeros((sh + 1, sw + 1), np.int8)  # (row / column -1: the zero every index outside the source reads)
        v[:sh, :sw] = np.where((src[:sh, :sw] >= 1) & (src[:sh, :sw] <= 9), src[:sh, :sw], 0)
        best = None
        for c, (mode, kx, ky) in enumerate(scale_candidates()):
            if not (int(modes) >> mode) & 1:
                continue
            child = v[_scale_map(mode, kx, ah, sh)][:, _scale_map(mode, ky, aw, sw)]
            children[s, c, :ah, :aw] = child
            table[s, c] = int((child == answer[:ah, :aw]).sum())
            if best is None or table[s, c] > table[s, best]:
                best = c
        colours = sum(1 << int(k) for k in np.unique(children[s, best]) if k)
        scale[s, :4] = (best, table[s, best], ah * aw, colours)
    return (scale, base, table, children) if full else (scale, base)


def scale_macros(scales, resize_op, color_ops, H, W):
    """The best candidate of every source (`ARCVecEnv.scale` -> Scales, with its bit rows) as ONE macro per source: {"bits": uint8
    [M, 2, 10, 128], "operation": int32 [M, 2, 10], "length": int32 [M, 2]}.  Step 0 is the canvas rectangle (0, 0)..(ah - 1, aw - 1)
    with resize_op (resize_grid), then `Color c` — color_ops[c], c = 0..9 — on the child's cells of colour c for every colour present,
    ascending, packed to the front: length = 1 + popcount(colours); the steps behind it have operation -1 and zero bit rows.  A slot
    with total == 0 (not asked for, or no candidate) or that does not beat the row's own ratio by `align_macros`' rule — correct *
    base_total <= base_correct * total, in integers — gets operation -1 at every step and length 1: one ARCLE_ST_BAD_OP child, dropped
    by beam_search.  Built on the device by sorting and indexing: no host synchronisation."""
    a = scales
    assert a.bits is not None, "scale_macros needs the child's bit rows (scale(bits=True))"
    dev = a.cand.device
    M = int(a.cand.shape[0])
    ops = torch.as_tensor([int(o) for o in color_ops], dtype=torch.int32, device=dev)
    assert int(ops.numel()) == 10, "color_ops: the ten Color ops, color_ops[c] paints c"
    ah, aw = a.ans_dim[..., 0].to(torch.int64), a.ans_dim[..., 1].to(torch.int64)
    zero = torch.zeros_like(ah)
    bc, bt = a.base[:, 0].to(torch.int64).reshape(M, 1), a.base[:, 1].to(torch.int64).reshape(M, 1)
    ok = (a.total > 0) & (a.correct.to(torch.int64) * bt > bc * a.total.to(torch.int64))
    c = torch.arange(1, 10, device=dev, dtype=torch.int64).reshape(1, 1, 9)
    present = ((a.colours.to(torch.int64).reshape(M, 2, 1) >> c) & 1) != 0
    order = torch.argsort(torch.where(present, c, c + 16), dim=2)  # (the colours present first, ascending)
    n = present.sum(2)
    live = (torch.arange(9, device=dev).reshape(1, 1, 9) < n.reshape(M, 2, 1)) & ok.reshape(M, 2, 1)
    cbits = torch.gather(a.bits, 2, order.reshape(M, 2, 9, 1).expand(M, 2, 9, int(a.bits.shape[-1])))
    none8, none32 = torch.zeros((), dtype=torch.uint8, device=dev), torch.full((), -1, dtype=torch.int32, device=dev)
    cbits = torch.where(live.reshape(M, 2, 9, 1), cbits, none8)
    cops = torch.where(live, ops[order + 1], none32)
    rbits = torch.where(ok.reshape(M, 2, 1), _rect_bits(zero, ah - 1, zero, aw - 1, H, W), none8)
    rop = torch.where(ok, torch.full((), int(resize_op), dtype=torch.int32, device=dev), none32)
    length = torch.where(ok, (1 + n).to(torch.int32), torch.ones((), dtype=torch.int32, device=dev))
    return {"bits": torch.cat([rbits.reshape(M, 2, 1, -1), cbits], 2).contiguous(),
            "operation": torch.cat([rop.reshape(M, 2, 1), cops], 2).to(torch.int32).contiguous(), "length": length.to(torch.int32).contiguous()}


def propose_scales(resize_op, color_ops, sources=3, modes=7, box_ops=(), seed_ops=(), max_components=16, skip_color=0, any_color=False,
                   diagonal=False):
    """A `propose` for beam_search that answers "is the answer the grid, or the input, zoomed, shrunk or tiled?" — like
    `propose_alignments` its children have the answer's grid_dim: at every depth, for each frontier state, ONE macro per source asked
    for — resize_op (resize_grid) to the answer's dims, then one `Color c` per colour of the best candidate's child on that colour's
    cells (`venv.scale`, one launch; `scale_macros`): K = 2, T = 10.  color_ops[c] = the index of `Color c` in the env's op table
    (both default tables: range(10)).  With box_ops / seed_ops the singles of `object_actions(masks=True)` on the objects of each
    state's grid come first, as macros of length 1, the way `propose_alignments` puts them: K = C * (len(box_ops) + len(seed_ops)) +
    2.  It looks at the answer of each row's env, so it carries `wants_src = True` and beam_search calls it with (venv, rows, src_env)."""
    resize_op, color_ops = int(resize_op), [int(o) for o in color_ops]
    box_ops, seed_ops = list(box_ops), list(seed_ops)

    def propose(venv, rows, src_env=None):
        sm = scale_macros(venv.scale(rows, src_env, sources, modes), resize_op, color_ops, venv.H, venv.W)
        if not box_ops and not seed_ops:
            return sm
        if any_color or diagonal:
            objs = venv.objects(rows, max_components=max_components, skip_color=skip_color, any_color=any_color, diagonal=diagonal, bits=True)
        else:
            objs = venv.components(rows, max_components=max_components, skip_color=skip_color, bits=True)
        single = object_actions(objs, box_ops, seed_ops, masks=True)
        M, K1 = (int(v) for v in single["operation"].shape)
        dev = single["bits"].device
        b1 = torch.zeros((M, K1, 10, int(single["bits"].shape[-1])), dtype=torch.uint8, device=dev)
        b1[:, :, 0] = single["bits"]
        o1 = torch.full((M, K1, 10), -1, dtype=torch.int32, device=dev)
        o1[:, :, 0] = single["operation"]
        return {"bits": torch.cat([b1, sm["bits"]], 1).contiguous(), "operation": torch.cat([o1, sm["operation"]], 1).contiguous(),
                "length": torch.cat([torch.ones((M, K1), dtype=torch.int32, device=dev), sm["length"]], 1).contiguous()}
    propose.wants_src = True
    return propose
