"""Search over ARCLE action sequences on top of `ARCVecEnv.expand`: the NumPy mirror of the device's state hash, and a plain beam
search.

The hash is defined in include/arcle_hip.h (next to arcle_hash_rows) and computed on the device by arcle_amd/csrc/arcle_search.h;
`hash_rows_numpy` restates it on the host — the same arrangement as arcle_amd/sampling.py for the device RNG — and is what the tests
pin the device against."""
import collections

import numpy as np
import torch

# enum arcle_plane ids of the planes a state row carries, in the row's (FlattenObservation) order, and the record byte every scalar
# field of the row lands in (ARCLE_REC_*)
_PLANE_ID = {"input": 0, "grid": 1, "selected": 2, "clip": 3, "object": 4, "object_sel": 5, "background": 6}
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


def beam_search(venv, rows, actions, width, depth, src_env=None):
    """Beam search over sequences drawn from ONE candidate action set, scored by the dense pair (correct cells / total cells).

    venv: anything with `expand(rows, action, src_env)`, `transition(rows, action, src_env)` and `hash_rows(rows)` as ARCVecEnv has
    them; rows int8 [M0, L] start states; actions = {"bbox": int32 [K,4] | "point": int32 [K,2], "operation": int32 [K]}; src_env
    int32 [M0] = the env whose answer judges row m (default: env m).  Per depth: expand every frontier state by every action; drop
    children with a status bit and children whose state equals their parent's; drop states already seen (in an earlier depth, or
    twice in this one: the lowest child index stays); if a child's grid IS the answer (correct == total: exactly when a Submit
    would pay — with unequal dims the total exceeds the common rectangle — so the candidate set needs no Submit) return the action
    indices that lead to the lowest such child; else keep the `width` best by correct / total, ties to the lower child index, and
    materialise only those with `transition`.  Every tensor lives on rows.device."""
    dev = rows.device
    form = "bbox" if "bbox" in actions else "point"
    pay = actions[form].to(device=dev, dtype=torch.int32).contiguous()
    op = actions["operation"].to(device=dev, dtype=torch.int32).contiguous()
    assert pay.dim() == 2 and op.dim() == 1, "beam_search takes one candidate set for every state"
    K = int(op.shape[0])
    M0 = int(rows.shape[0])
    src = (torch.arange(M0, device=dev) if src_env is None else src_env.to(dev)).to(torch.int32)
    root = torch.arange(M0, device=dev)
    path = torch.empty((M0, 0), dtype=torch.int64, device=dev)
    seen = venv.hash_rows(rows)[:, 0].clone()
    frontier, counts = rows, []
    for _ in range(depth):
        M = int(frontier.shape[0])
        if M == 0:
            break
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
        goal = (c == t) & (t > 0)
        if bool(goal.any()):
            g = int(torch.nonzero(goal)[0])
            counts.append((M * K, int(idx.numel()), 0))
            seq = path[parent[g]].tolist() + [int(k[g])]
            return BeamResult(seq, counts, int(root[parent[g]]))
        # correct / total as an integer key: floor(c * 2^32 / t).  Two different fractions with totals below 2^16 differ by at least
        # 1 / (t1 * t2) > 2^-32, so their keys differ in the same direction; equal fractions give equal keys
        key = (c << 32) // torch.clamp(t, min=1)
        best = torch.argsort(key, descending=True, stable=True)[:width]
        best = torch.sort(best).values  # (kept states stay in child order: the next depth's child indices are deterministic)
        parent, k = parent[best], k[best]
        counts.append((M * K, int(idx.numel()), int(best.numel())))
        if best.numel() == 0:
            break
        src_next = src.index_select(0, parent)
        frontier, _, _ = venv.transition(frontier.index_select(0, parent), {form: pay.index_select(0, k), "operation": op.index_select(0, k)},
                                         src_next)
        path = torch.cat([path.index_select(0, parent), k.reshape(-1, 1)], 1)
        root, src = root.index_select(0, parent), src_next
    return BeamResult(None, counts, None)
