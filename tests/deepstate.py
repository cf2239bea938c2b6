"""State-aware action streams and a census of the situations they reach.  Test infrastructure only.

The random differential traces (backends.random_trace_compare) draw every action without looking at the env: an empty mask meets an
active object in about 1 % of the steps, a second continued op in a row a dozen times per case, a fourth never.  The
generators here read the ORACLE's current state before every step — nothing of the backend under test — and send what that state
makes interesting:

  chain_stream        masks ("mask" / "bits"): while an env's object is active, Move / Rotate / Flip with an EMPTY selection (the
                      continuation branch of init_objsel, object.py:102-107) with probability 0.8, chains of 8 and more, objects walked
                      off the grid and back, int8 wraps of pos + dim and of the Rotate sums on planes with a side >= 64, ROTATE_DOMAIN
                      refusals of continued ops on non-square planes, and on the exotic table the ops without RESET_SEL in between.
  grid_aware_tuples   "bbox" / "bbox5" / "point": boxes drawn relative to the env's current grid_dim / input_dim / clip_dim (inside,
                      touching, == dim, straddling), Copy followed by Paste near the plane's edges, CopyFromInput -> Submit on solved
                      grids, last trials.

The oracle is stepped first; the recorded [S, N, ...] actions are what every backend then receives (`compare`, `rollout_check`,
`rows_check`, `expansion_check`).  `census(pre, action, post)` names the situations of every env's step from the oracle's fields
alone; tests/test_deepstate_host.py asserts floors on those counts for every case the emulator and GPU tests use, so that none of
them can pass vacuously."""
import functools
import random
from collections import Counter, namedtuple

import numpy as np

import backends as B
from oracle import oracle as O

ST_ROTATE_DOMAIN = O.ST_ROTATE_DOMAIN
OBJ_KINDS = {O.OP_MOVE: "Move", O.OP_ROTATE: "Rotate", O.OP_FLIP: "Flip"}
BOX_KINDS = (O.OP_COLOR, O.OP_FLOODFILL, O.OP_RESIZE_GRID, O.OP_CROP_GRID)
FLOOR, FLOOR_CHAIN8 = 20, 100

# One case = one stream.  table "o2arc" | "exotic" (refdriver.variant_table("o2arc_exotic")); stream "chain" | "bbox" | "point".
Case = namedtuple("Case", "stream H W table flags N S")


def table_of(name):
    from oracle import refdriver as RD
    return O.o2arc_ops() if name == "o2arc" else RD.variant_table("o2arc_exotic")[1]


def _i8(x):
    return ((int(x) + 128) & 0xff) - 128


def snapshot(orc):
    """Every field of the oracle's state, copied: what `census` reads and what a one-env re-step starts from."""
    d = {f: orc.get(f) for f in O.PLANES + list(O.REC)}
    d["cnt"] = orc.counters()
    return d


# ---- census -------------------------------------------------------------------------------------------------------------------
def selection_boxes(form, payload, H, W):
    """(non-empty bool [N], xmin, xmax, ymin, ymax int [N]) of the selections the wrappers make of the payload (bbox.py:22-30, :43-49;
    0 / 1 masks as they stand)."""
    pay = np.asarray(payload)
    N = len(pay)
    if form in ("mask",):
        m = pay.reshape(N, H, W) != 0
        r, c = m.any(2), m.any(1)
        any_ = r.any(1)
        return any_, r.argmax(1), H - 1 - r[:, ::-1].argmax(1), c.argmax(1), W - 1 - c[:, ::-1].argmax(1)
    if form == "point":
        x, y = pay[:, 0], pay[:, 1]
        return (x >= 0) & (x < H) & (y >= 0) & (y < W), x, x, y, y
    x0, x1 = np.minimum(pay[:, 0], pay[:, 2]), np.maximum(pay[:, 0], pay[:, 2])
    y0, y1 = np.minimum(pay[:, 1], pay[:, 3]), np.maximum(pay[:, 1], pay[:, 3])
    return (x0 >= 0) & (y0 >= 0) & (x0 < H) & (y0 < W), x0, np.minimum(x1, H - 1), y0, np.minimum(y1, W - 1)


def _rect(f, n):
    """(x, y, h, w, visible) of env n's object as apply_patch sees it (int8 sums, object.py:113-138)."""
    x, y = int(f["object_pos"][n, 0]), int(f["object_pos"][n, 1])
    h, w = int(f["object_dim"][n, 0]), int(f["object_dim"][n, 1])
    gh, gw = int(f["grid_dim"][n, 0]), int(f["grid_dim"][n, 1])
    return x, y, h, w, (_i8(x + h) > 0 and x < gh and _i8(y + w) > 0 and y < gw)


def _restep_status(pre, n, action):
    """The status bits env n's step raises, from a one-env oracle holding its pre-step state (the oracle's status word is per batch)."""
    H, W = action["H"], action["W"]
    one = B.OracleBackend(1, H, W, -1, "o2arc", action["ops"])
    for f in O.PLANES:
        one.env.planes[f][:] = pre[f][n:n + 1]
    one.env.rec[:] = np.concatenate([pre[f][n:n + 1] for f in O.REC], 1)  # (REC is in byte order)
    form = "bbox" if action["form"] == "bbox5" else action["form"]
    one.step(form, np.asarray(action["payload"])[n:n + 1], np.asarray(action["op"])[n:n + 1], action["flags"])
    return one.status()


def census(pre, action, post, track=None):
    """The named situations of one step of N envs -> Counter.  pre / post: `snapshot`s of the oracle around the step, post also with
    "reward" [N]; action: dict(form "mask" | "bbox" | "bbox5" | "point", payload [N, ...] (0 / 1 masks), op [N], flags, ops (the
    descriptor table), H, W).  track: a dict kept by the caller across the steps of one stream — the per-env run of continued steps
    and the previous op live there, and track["names"] is this step's list of names per env."""
    ops, flags, opv, H, W = action["ops"], action["flags"], np.asarray(action["op"]), action["H"], action["W"]
    form = "bbox" if action["form"] == "bbox5" else action["form"]
    N = len(opv)
    any_, bx0, bx1, by0, by1 = selection_boxes(form, action["payload"], H, W)
    track = {} if track is None else track
    chain, prev = track.setdefault("chain", np.zeros(N, np.int64)), track.setdefault("prev", [None] * N)
    names = [[] for _ in range(N)]
    for n in range(N):
        out, cont, this = names[n], False, None
        if (flags & O.STEP_AUTORESET) and pre["terminated"][n, 0]:
            out.append("autoreset:after-terminate")
        elif 0 <= opv[n] < len(ops):
            d = int(ops[opv[n]])
            kind, arg, fl = d & 0xff, (d >> 8) & 0xff, d >> 16
            was_active = bool(pre["active"][n, 0])
            active = was_active and not fl & O.F_RESET_SEL
            stepped = int(post["cnt"][n, 0]) != int(pre["cnt"][n, 0])
            gh, gw = int(pre["grid_dim"][n, 0]), int(pre["grid_dim"][n, 1])
            sel, x0, x1, y0, y1 = bool(any_[n]), int(bx0[n]), int(bx1[n]), int(by0[n]), int(by1[n])
            ran = False
            if kind in OBJ_KINDS:
                px, py, ph, pw, pvis = _rect(pre, n)
                if not sel and not active:
                    out.append("noop:inactive-empty")
                elif not sel:
                    cont = True
                    out.append("cont:" + OBJ_KINDS[kind])
                    if kind == O.OP_ROTATE and arg % 2:
                        out.append("cont-rotate:same-parity" if (ph & 1) == (pw & 1) else f"cont-rotate:odd-even:parity{int(pre['rotation_parity'][n, 0])}")
                        sx, sy = px + _i8(_i8(px + ph) - 1), py + _i8(_i8(py + pw) - 1)
                        if max(H, W) >= 64 and not (-128 <= sx <= 127 and -128 <= sy <= 127):
                            out.append("wrap:rotate-sum>127")
                    if not stepped and kind != O.OP_MOVE and _restep_status(pre, n, action) & ST_ROTATE_DOMAIN:
                        out.append("domain:continued")
                    p = prev[n]
                    if p is not None and p["stepped"]:
                        if p["was_active"] and p["kind"] not in OBJ_KINDS and not p["fl"] & O.F_RESET_SEL:
                            out.append("cont-after-nonreset")
                        if p["ran"] and p["kind"] == O.OP_FLIP and p["arg"] >= 2 and ph != pw:
                            out.append("cont-after-D0D1")
                ran = stepped and (sel or active)
                if ran and post["active"][n, 0]:
                    x, y, h, w, vis = _rect(post, n)
                    g2h, g2w = int(post["grid_dim"][n, 0]), int(post["grid_dim"][n, 1])
                    if vis and (x < 0 or y < 0 or _i8(x + h) > g2h or _i8(y + w) > g2w):
                        out.append("obj:partly-off")
                    if x < 0 or y < 0:
                        out.append("obj:negative-pos")
                    if cont and vis and not pvis:
                        out.append("obj:off->on")
                    if max(H, W) >= 100 and ((x + h > 127 and x < g2h) or (y + w > 127 and y < g2w)):  # (where only the wrap hides the object)
                        out.append("wrap:pos+dim>127")
            elif kind == O.OP_COPY and sel:
                sh, sw = (gh, gw) if arg else (int(pre["input_dim"][n, 0]), int(pre["input_dim"][n, 1]))
                if x1 > sh or y1 > sw:
                    out.append("copy:refused")
                else:
                    out.append("copy:proceeds")
                    if x1 == sh or y1 == sw:
                        out.append("copy:edge==dim")
            elif kind == O.OP_PASTE and sel:
                ch, cw = int(pre["clip_dim"][n, 0]), int(pre["clip_dim"][n, 1])
                if ch and cw:
                    out.append("paste:inside" if x0 + ch <= gh and y0 + cw <= gw else "paste:past-grid_dim")
                    if x0 + ch > H or y0 + cw > W:
                        out.append("paste:clipped-at-plane")
            elif kind in BOX_KINDS and sel and (x0 < gh <= x1 or y0 < gw <= y1):
                out.append("box:straddles-grid_dim")
            elif kind == O.OP_SUBMIT:
                if post["reward"][n] == 1:
                    out.append("submit:reward1")
                if pre["trials_remain"][n, 0] == 1:
                    assert post["terminated"][n, 0] == 1
                    out.append("submit:last-trial")
            this = {"kind": kind, "arg": arg, "fl": fl, "was_active": was_active, "stepped": stepped, "ran": ran}
        chain[n] = chain[n] + 1 if cont else 0
        out += [f"chain>={k}" for k in (2, 4, 8) if chain[n] >= k]
        prev[n] = this
    track["names"] = names
    return Counter(name for out in names for name in out)


def applicable(case):
    """The situations a case must reach (at least FLOOR times, chain>=8 FLOOR_CHAIN8 times)."""
    H, W = case.H, case.W
    if case.stream == "chain":
        need = ["cont:Move", "cont:Rotate", "cont:Flip", "chain>=4", "chain>=8", "cont-rotate:odd-even:parity0", "cont-rotate:odd-even:parity1",
                "cont-rotate:same-parity", "obj:partly-off", "obj:negative-pos", "obj:off->on", "noop:inactive-empty"]
        if H != W:
            need.append("domain:continued")
        if max(H, W) >= 100:
            need.append("wrap:pos+dim>127")
        if max(H, W) >= 64:
            need.append("wrap:rotate-sum>127")
        if case.table == "exotic":
            need += ["cont-after-nonreset", "cont-after-D0D1"]
        return need
    need = ["copy:proceeds", "copy:refused", "copy:edge==dim", "paste:inside", "paste:past-grid_dim", "submit:reward1", "submit:last-trial"]
    if case.stream == "bbox":  # (a point selects one cell: its clip is 1 x 1, which no plane edge clips, and it straddles nothing)
        need += ["paste:clipped-at-plane", "box:straddles-grid_dim"]
    if case.flags & O.STEP_AUTORESET:
        need.append("autoreset:after-terminate")
    return need


# ---- tasks ----------------------------------------------------------------------------------------------------------------------
def make_tasks(seed, N, H, W, full=0.4, same=0.6, lo=None):
    """Padded tasks: a share `full` of the inputs fills the plane, the others have sides in [lo or half the plane's, the plane's]; a
    share `same` of the answers equals the input."""
    rng = np.random.default_rng(seed)
    inp, ans = np.zeros((N, H, W), np.int8), np.zeros((N, H, W), np.int8)
    idim, adim = np.zeros((N, 2), np.int8), np.zeros((N, 2), np.int8)
    for n in range(N):
        ih, iw = (H, W) if rng.random() < full else (rng.integers(lo or (H + 1) // 2, H + 1), rng.integers(lo or (W + 1) // 2, W + 1))
        ih, iw = max(1, min(H, ih)), max(1, min(W, iw))
        g = rng.integers(0, [10, 4][rng.integers(0, 2)], (ih, iw)).astype(np.int8)
        inp[n, :ih, :iw], idim[n] = g, (ih, iw)
        if rng.random() < same:
            ans[n, :ih, :iw], adim[n] = g, (ih, iw)
        else:
            ah, aw = rng.integers(1, H + 1), rng.integers(1, W + 1)
            ans[n, :ah, :aw], adim[n] = rng.integers(0, 10, (ah, aw)), (ah, aw)
    return inp, idim, ans, adim


# ---- the chain policy -----------------------------------------------------------------------------------------------------------
UP, DOWN, RIGHT, LEFT = 20, 21, 22, 23  # O2ARCv2Env table slots (both tables; slot 20 of the exotic table also resets the selection)
OPPOSITE = {DOWN: UP, RIGHT: LEFT}
ROT_ODD = {"o2arc": (24, 25), "exotic": (25,)}  # (exotic slot 24 is Rotate 180)
FLIPS = (26, 27)
NONRESET = (0, 1, 28, 34)  # exotic table: Color 0 (no wrapper), Color 1 (keep_sel), Copy (keep_sel), Submit

# The probabilities of the policy.  0.8 for continuing is the issue's prototype; the others were raised from even odds until every
# situation of `applicable` clears its floor on every case (tests/test_deepstate_host.py prints the counts) — the comment says which
# situation each one feeds, so that a floor that is missed after a change points at the number to move.  Every env has a role:
#   "edge"    (planes with a side >= 64 only) selects at the plane's far edge and walks on past it: wrap:pos+dim>127, wrap:rotate-sum>127
#   "spin"    mostly Rotates objects it can turn: cont-rotate:*, rotation_parity 1
#   "wander"  mostly Moves in its preferred direction: obj:partly-off, obj:negative-pos, obj:off->on
SHARE_EDGE = {True: 0.45, False: 0.4}   # share of "edge" envs, by "a side >= 100" (there the walk past 127 takes 28 Moves of the 48 steps)
SHARE_SPIN_UPTO = {True: 0.8, False: 0.7}  # "spin" envs fill up to this share (by "the plane has edge envs"), "wander" envs the rest
P_CONTINUE = {"edge": 0.99, "spin": 0.8, "wander": 0.8}   # an active object is continued; an "edge" env must not drop its object during the walk
P_WALK_BACK = {"edge": 0.15, "spin": 0.8, "wander": 0.8}  # a wholly off-grid object is moved towards the grid (obj:off->on); "edge" envs stay out
P_EDGE_TURN = 0.35        # "edge", side < 100, Rotate sums past the int8 range: Rotate now (wrap:rotate-sum>127 at 64 x 64)
P_EDGE_STEP_BACK = 0.2    # "edge", pos + dim past 127: one Move back inside (obj:off->on at 127 x 127, where one Move leaves)
EDGE_WALK = (0.93, 0.98)  # "edge" on its way out: preferred Move below the first, odd Rotate below the second, any object op above
EDGE_GONE = (0.45, 0.8)   # ... and once pos + dim is past 127: it stays there and turns (the wrapped sums of object.py:102-107)
SPIN_ROTATE = {True: 0.7, False: 0.5}  # "spin": odd Rotate, by "the object's sides differ in parity" (cont-rotate:odd-even:parity1)
SPIN_FLIP_UPTO, SPIN_PREF_UPTO = 0.8, 0.9  # ... then Flip, then the preferred Move, then any Move
WANDER_PREF, WANDER_MOVE_UPTO = 0.68, 0.8  # "wander": preferred Move, then any Move, then any object op
P_NONRESET_UPTO = 0.93    # exotic table, active, not continuing (u in [0.8, 0.93)): an op without RESET_SEL (cont-after-nonreset)
P_FRESH_UPTO = {True: 0.9, False: 0.6}  # by `active`: a fresh selection with an object op below this ...
P_NOOP_UPTO = 0.9         # ... inactive: an empty mask with an object op below this (noop:inactive-empty), any other op above
P_FRESH_ANY_OP = 0.7      # a fresh selection that fits the plane transposed takes any object op, else a Move / FlipH (it cannot turn)
P_TURNABLE = {"spin": 0.85, "edge": 0.4, "wander": 0.4}  # the box also fits the plane transposed (a Rotate is not refused)
P_ODD_EVEN = 0.5          # "spin": a turnable box of equal parities loses a column (cont-rotate:odd-even)
P_TOO_LONG = 0.3          # non-square planes: a box longer than the short side, refused by a continued Rotate (domain:continued)
P_AT_PREF_EDGE = 0.75     # the box starts at the edge of grid_dim the env prefers to move past (obj:off->on within the stream)
P_FAR_EDGE, P_NEAR_EDGE = 0.2, 0.4  # otherwise: at the far edge of grid_dim below the first, at 0 below the second, anywhere above
P_EDGE_LONG = 0.8         # "edge", side >= 100: long enough that pos + dim passes 127 with the near end still inside grid_dim
P_KEEP_CELL = 0.75        # share of the box's cells kept (non-rectangular selections)


def _roles(rnd, N, H, W):
    """Per env: (role, preferred Move)."""
    roles = []
    for n in range(N):
        r = rnd.random()
        far = [d for d, side in ((DOWN, H), (RIGHT, W)) if side >= 64]
        if far and r < SHARE_EDGE[max(H, W) >= 100]:
            roles.append(("edge", rnd.choice(far)))
        elif r < SHARE_SPIN_UPTO[bool(far)]:
            roles.append(("spin", rnd.choice((UP, DOWN, RIGHT, LEFT))))
        else:
            roles.append(("wander", rnd.choice((UP, DOWN, RIGHT, LEFT))))
    return roles


def _start(rnd, at_pref, span):
    """Where a box starts along one axis with `span` free cells: at the preferred edge (None: the env prefers the other axis), at either
    edge of grid_dim, or anywhere."""
    u = rnd.random()
    if at_pref is not None and u < P_AT_PREF_EDGE:
        return at_pref
    return span if u < P_FAR_EDGE else 0 if u < P_NEAR_EDGE else rnd.randint(0, span)


def _fresh(rnd, nrng, H, W, gh, gw, role, pref):
    """A non-rectangular selection: a box inside grid_dim (an "edge" env: at the plane's far edge) with about a quarter of its cells
    dropped.  -> (mask, fits: the box still fits the plane when transposed)"""
    gh, gw = max(1, min(gh, H)), max(1, min(gw, W))
    bh, bw = rnd.randint(1, min(gh, 6)), rnd.randint(1, min(gw, 6))
    if rnd.random() < P_TURNABLE[role]:
        bh, bw = rnd.randint(1, min(gh, 6, W)), rnd.randint(1, min(gw, 6, H))
        if role == "spin" and not (bh ^ bw) & 1 and bw > 1 and rnd.random() < P_ODD_EVEN:
            bw -= 1
    if W > H and gw > H and rnd.random() < P_TOO_LONG:
        bw = rnd.randint(H + 1, gw)
    elif H > W and gh > W and rnd.random() < P_TOO_LONG:
        bh = rnd.randint(W + 1, gh)
    x = _start(rnd, {DOWN: gh - bh, UP: 0}.get(pref), gh - bh)
    y = _start(rnd, {RIGHT: gw - bw, LEFT: 0}.get(pref), gw - bw)
    if role == "edge" and pref == DOWN:
        bh = rnd.randint(129 - gh, min(H, 137 - gh)) if H >= 100 and 129 - gh <= H and rnd.random() < P_EDGE_LONG else min(bh, 6)
        x = H - bh
    elif role == "edge":
        bw = rnd.randint(129 - gw, min(W, 137 - gw)) if W >= 100 and 129 - gw <= W and rnd.random() < P_EDGE_LONG else min(bw, 6)
        y = W - bw
    m = np.zeros((H, W), np.int8)
    box = (nrng.random((bh, bw)) < P_KEEP_CELL).astype(np.int8)
    box[rnd.randrange(bh), rnd.randrange(bw)] = 1
    m[x:x + bh, y:y + bw] = box
    return m, bw <= H and bh <= W


def _edge_op(rnd, v, pref, pos_dim, turn_sum, small_plane, table, cont_ops):
    """The continued op of an "edge" env: pos_dim = pos + dim and turn_sum = 2 * pos + dim along its preferred axis."""
    gone = pos_dim > 127
    if small_plane and turn_sum > 128 and v < P_EDGE_TURN:
        return rnd.choice(ROT_ODD[table])
    if gone and v < P_EDGE_STEP_BACK:
        return OPPOSITE[pref]
    p_move, p_rotate = EDGE_GONE if gone else EDGE_WALK
    return pref if v < p_move else rnd.choice(ROT_ODD[table]) if v < p_rotate else rnd.choice(cont_ops)


def _spin_op(rnd, v, pref, odd_even, table, moves):
    if v < SPIN_ROTATE[odd_even]:
        return rnd.choice(ROT_ODD[table])
    if v < SPIN_FLIP_UPTO:
        return rnd.choice(FLIPS)
    return pref if v < SPIN_PREF_UPTO and pref in moves else rnd.choice(moves)


def _wander_op(rnd, v, pref, moves, cont_ops):
    if v < WANDER_PREF:
        return pref if pref in moves else rnd.choice(moves)
    return rnd.choice(moves) if v < WANDER_MOVE_UPTO else rnd.choice(cont_ops)


def chain_actions(rnd, nrng, orc, roles, table, hold=False):
    """One step's (masks int8 [N, H, W], op int32 [N]) from the oracle's current state.  hold: never leave the object — continue while
    active, lift a fresh selection with a Move otherwise (the parents of `expansion_check`)."""
    N, H, W = orc.N, orc.H, orc.W
    rec = orc.env.rec
    masks, op = np.zeros((N, H, W), np.int8), np.zeros(N, np.int32)
    ops = table_of(table)
    cont_ops = [k for k in range(20, 28) if not (ops[k] >> 16) & O.F_RESET_SEL]
    moves = [k for k in (UP, DOWN, RIGHT, LEFT) if k in cont_ops]
    for n in range(N):
        role, pref = roles[n]
        gh, gw, active = int(rec[n, 2]), int(rec[n, 3]), bool(rec[n, 12])
        x, y, h, w = int(rec[n, 8]), int(rec[n, 9]), int(rec[n, 6]), int(rec[n, 7])
        u = rnd.random()
        if active and (hold or u < P_CONTINUE[role]):  # continue the object: an empty mask
            back = [k for k, c in ((DOWN, _i8(x + h) <= 0), (UP, x >= gh), (RIGHT, _i8(y + w) <= 0), (LEFT, y >= gw)) if c and k in cont_ops]
            v = rnd.random()
            if back and v < P_WALK_BACK[role]:
                op[n] = rnd.choice(back)
            elif role == "edge":
                pos, dim = (x, h) if pref == DOWN else (y, w)
                op[n] = _edge_op(rnd, v, pref, pos + dim, 2 * pos + dim, max(H, W) < 100, table, cont_ops)
            elif role == "spin":
                op[n] = _spin_op(rnd, v, pref, bool((h ^ w) & 1), table, moves)
            else:
                op[n] = _wander_op(rnd, v, pref, moves, cont_ops)
        elif active and table == "exotic" and u < P_NONRESET_UPTO:  # the object stays active: the next continued op restores the background over this op's write
            op[n] = rnd.choice(NONRESET)
            masks[n, rnd.randrange(max(1, min(gh, H))), rnd.randrange(max(1, min(gw, W)))] = 1
        elif hold or u < P_FRESH_UPTO[active]:
            masks[n], fits = _fresh(rnd, nrng, H, W, gh, gw, role, pref)
            if hold:
                op[n] = rnd.choice(moves)
            else:
                op[n] = rnd.choice(cont_ops) if fits and rnd.random() < P_FRESH_ANY_OP else rnd.choice(moves + [26])
        elif not active and u < P_NOOP_UPTO:
            op[n] = rnd.choice(cont_ops)  # nothing selected, nothing active: the no-op of object.py:110-111
        else:  # anything else: Color, CopyFromInput, ResetGrid, Submit (twice as often: terminations), Copy, Paste
            op[n] = rnd.choice((rnd.randrange(0, 10), 31, 32, 34, 34, 29, 30))
            if rnd.random() < 0.7:
                masks[n] = _fresh(rnd, nrng, H, W, gh, gw, "wander", pref)[0]
    return masks, op


# ---- the tuple policy -----------------------------------------------------------------------------------------------------------
def _rel_span(rnd, dim, side):
    """(lo, hi) of a box along one axis relative to a dimension `dim` on a plane side `side`: inside / touching dim - 1 / ending at
    == dim (the off-by-one of object.py:301) / straddling."""
    dim = max(1, min(dim, side))
    t = rnd.random()
    if t < 0.4 or dim >= side and t >= 0.6:
        lo = rnd.randrange(dim)
        return lo, rnd.randint(lo, dim - 1)
    if t < 0.6:
        return rnd.randrange(dim), dim - 1
    if t < 0.8:
        return rnd.randint(0, dim), dim
    return rnd.randrange(dim), rnd.randint(dim, side - 1)


def tuple_actions(rnd, orc, form):
    """One step's (payload int32 [N, 4 | 2], op int32 [N]) from the oracle's current state."""
    N, H, W = orc.N, orc.H, orc.W
    rec, P = orc.env.rec, orc.env.planes
    pay, op = np.zeros((N, 4), np.int32), np.zeros(N, np.int32)
    gd, ad = rec[:, 2:4].astype(int), rec[:, 14:16].astype(int)
    inside = (np.arange(H)[None, :, None] < gd[:, 0, None, None]) & (np.arange(W)[None, None, :] < gd[:, 1, None, None])
    solved = (gd == ad).all(1) & ~((P["grid"] != P["answer"]) & inside).any((1, 2))
    point = form == "point"
    for n in range(N):
        gh, gw, ch, cw, ih, iw, trials = int(rec[n, 2]), int(rec[n, 3]), int(rec[n, 4]), int(rec[n, 5]), int(rec[n, 0]), int(rec[n, 1]), int(rec[n, 10])
        u = rnd.random()
        box = None
        if (solved[n] and u < 0.35) or u < (0.15 if trials == 1 else 0.05):
            op[n] = 34
        elif ch and cw and u < 0.45:
            op[n] = 30
            t = rnd.random()
            if t < 0.35:    # inside grid_dim
                x, y = rnd.randint(0, max(0, gh - ch)), rnd.randint(0, max(0, gw - cw))
            elif t < 0.7:   # the clip runs past the plane's edge (a 1 x 1 clip: the last row / column)
                x, y = rnd.randint(max(0, H - ch + 1), H - 1) if ch > 1 else H - 1, rnd.randint(0, W - 1)
                if rnd.random() < 0.5:
                    x, y = rnd.randint(0, H - 1), rnd.randint(max(0, W - cw + 1), W - 1) if cw > 1 else W - 1
            else:           # past grid_dim, mostly inside the plane
                x, y = min(H - 1, rnd.randint(max(0, gh - ch + 1), gh)), min(W - 1, rnd.randint(max(0, gw - cw + 1), gw))
            box = (x, min(H - 1, x + rnd.randint(0, 2)), y, min(W - 1, y + rnd.randint(0, 2)))
        elif u < 0.62:
            op[n] = rnd.choice((28, 29))
            sh, sw = (ih, iw) if op[n] == 28 else (gh, gw)
            box = _rel_span(rnd, sh, H) + _rel_span(rnd, sw, W)
        elif u < 0.76:
            op[n] = rnd.randrange(0, 10)
            box = _rel_span(rnd, gh, H) + _rel_span(rnd, gw, W)
        elif u < 0.80:
            op[n] = rnd.randrange(10, 20)
            x, y = rnd.randint(0, min(gh, H - 1)), rnd.randint(0, min(gw, W - 1))  # (a seed at == dim is refused, color.py:96)
            box = (x, x, y, y)
        elif u < 0.83:
            op[n] = 33
            box = _rel_span(rnd, gh, H) + _rel_span(rnd, gw, W)
        elif u < 0.93:
            op[n] = 31
        elif u < 0.95:
            op[n] = 32
        else:
            op[n] = rnd.randrange(20, 28)
            box = _rel_span(rnd, gh, H) + _rel_span(rnd, gw, W)
        if box is not None:
            x0, x1, y0, y1 = box
            if point:
                x1, y1 = (x1, y1) if rnd.random() < 0.5 else (x0, y0)  # a point: one end of the span (the far end is the == dim / outside one)
                pay[n, :2] = (min(x1, H - 1), min(y1, W - 1))
            elif rnd.random() < 0.5:
                pay[n] = (x0, y0, x1, y1)
            else:
                pay[n] = (x1, y1, x0, y0)  # (the wrapper sorts the corners)
    return (np.ascontiguousarray(pay[:, :2]) if point else pay), op


# ---- streams --------------------------------------------------------------------------------------------------------------------
class Stream:
    """The recorded actions of one case with the census of the oracle's run: tasks (padded arrays), payload [S, N, ...], op [S, N],
    names[s][n] (that env-step's situations), counts (Counter over the whole stream), status [S] (the oracle's word per step)."""


def max_trial_of(case):
    return 2 if case.stream != "chain" else 3 if case.flags else -1


@functools.lru_cache(maxsize=6)
def stream_of(case):
    """Generates (once per process: the streams are shared between the tests of a shape) the stream of a Case on the oracle."""
    H, W, N, S = case.H, case.W, case.N, case.S
    seed = (H * 1000 + W) * 8 + case.flags + {"chain": 0, "bbox": 100000, "point": 200000}[case.stream] + (500000 if case.table == "exotic" else 0)
    rnd, nrng = random.Random(seed), np.random.default_rng(seed)
    ops = table_of(case.table)
    st = Stream()
    st.case, st.ops = case, ops
    chain = case.stream == "chain"
    st.tasks = make_tasks(seed, N, H, W) if chain else make_tasks(seed, N, H, W, full=0.15, same=0.6, lo=min(3, H))
    orc = B.OracleBackend(N, H, W, max_trial_of(case), "o2arc", ops)
    orc.set_tasks(*st.tasks)
    orc.reset()
    roles = _roles(rnd, N, H, W) if chain else None
    form = "mask" if chain else case.stream
    pays, opl, st.names, st.status, st.counts, track = [], [], [], [], Counter(), {}
    for s in range(S):
        pay, op = chain_actions(rnd, nrng, orc, roles, case.table) if chain else tuple_actions(rnd, orc, form)
        pre = snapshot(orc)
        r, _ = orc.step(form, pay, op, case.flags)
        post = snapshot(orc)
        post["reward"] = r
        st.status.append(orc.status())
        st.counts += census(pre, {"form": form, "payload": pay, "op": op, "flags": case.flags, "ops": ops, "H": H, "W": W}, post, track)
        st.names.append(track["names"])
        pays.append(pay)
        opl.append(op)
    st.payload, st.op = np.stack(pays), np.stack(opl)
    return st


def chain_stream(H, W, table="o2arc", flags=0, N=64, S=64):
    """The chain stream of a shape: masks [S, N, H, W] (sent as "mask" or packed as "bits") and ops, with its census."""
    return stream_of(Case("chain", H, W, table, flags, N, S))


def grid_aware_tuples(form, H, W, flags=0, N=64, S=64):
    """The tuple stream of a shape in form "bbox" (also sent as "bbox5" records) or "point"."""
    return stream_of(Case("bbox" if form == "bbox5" else form, H, W, "o2arc", flags, N, S))


def check_floors(case, counts=None):
    """-> the list of floors the case's stream misses (empty = none)."""
    counts = stream_of(case).counts if counts is None else counts
    return [f"{case}: {name} occurs {counts[name]} times, floor {FLOOR_CHAIN8 if name == 'chain>=8' else FLOOR}"
            for name in applicable(case) if counts[name] < (FLOOR_CHAIN8 if name == "chain>=8" else FLOOR)]


def table_line(case, counts):
    return f"{case.stream:5s} {case.H:3d}x{case.W:<3d} {case.table:6s} flags {case.flags} N {case.N} S {case.S}: " + ", ".join(
        f"{k} {counts[k]}" for k in sorted(counts))


# ---- comparison -----------------------------------------------------------------------------------------------------------------
FIELDS = [f for f in O.PLANES[:-1]] + [f for f in O.REC if f != "answer_dim"]


def _send(be, form, pay, op, flags):
    if form == "bits":
        return be.step("bits", B.pack_bits(pay, be.bits_stride), op, flags)
    if form == "bbox5":
        return be.step("bbox5", np.concatenate([pay, op[:, None]], 1), None, flags)
    return be.step(form, pay, op, flags)


def _pair(backend_cls, case):
    st = stream_of(case)
    N = case.N
    be = backend_cls(N, case.H, case.W, max_trial_of(case), "o2arc", st.ops)
    orc = B.OracleBackend(N, case.H, case.W, max_trial_of(case), "o2arc", st.ops)
    for b in (be, orc):
        b.set_tasks(*st.tasks)
        b.reset()
    return st, be, orc


def compare(backend_cls, case, form):
    """The recorded stream of `case` through `backend_cls` in ingress form `form` ("mask" | "bits" for a chain stream, "bbox" | "bbox5"
    | "point" for a tuple stream) against the oracle: reward, terminated, counters, status and every field after every step, the shape
    of backends.random_trace_compare.  Every error line names the situations of the failing envs' step."""
    st, be, orc = _pair(backend_cls, case)
    N = be.N
    oform = {"bits": "mask", "bbox5": "bbox"}.get(form, form)
    errs = []
    for s in range(case.S):
        pay, op = st.payload[s][:N], st.op[s][:N]
        r1, t1 = _send(be, form, pay, op, case.flags)
        r2, t2 = orc.step(oform, pay, op, case.flags)
        tag = f"{case.stream} {case.H}x{case.W} {case.table} flags {case.flags} step {s} {form}"

        def where(bad):
            return "; ".join(f"env {n} op {op[n]}: {', '.join(st.names[s][n]) or '-'}" for n in bad[:6])
        if not np.array_equal(r1, r2):
            errs.append(f"{tag}: reward differs: {where(np.nonzero(r1 != r2)[0])}")
        if not np.array_equal(t1, t2):
            errs.append(f"{tag}: terminated differs: {where(np.nonzero(t1 != t2)[0])}")
        c1, c2 = be.counters(), orc.counters()
        if not np.array_equal(c1, c2):
            errs.append(f"{tag}: counters differ: {where(np.nonzero((c1 != c2).any(1))[0])}")
        s1, s2 = be.status(), orc.status()
        if s1 != s2:
            errs.append(f"{tag}: status {s1} vs oracle {s2}")
        for f in FIELDS:
            a, b = be.get(f), orc.get(f)
            if not np.array_equal(a, b):
                errs.append(f"{tag} field {f}: {where(np.nonzero((a != b).reshape(N, -1).any(1))[0])}")
        if len(errs) > 12:
            break
    if hasattr(be, "padding_is_zero") and not be.padding_is_zero():
        errs.append(f"{case}: plane padding bytes (cells >= H * W) are not zero")
    return errs


def rollout_check(backend_cls, case):
    """The whole chain stream as ONE rollout("mask", ..., packed=True) launch: per-step reward / terminated and every step's packed grid
    and grid_dim against the oracle's, then the final state, counters and status."""
    st, be, orc = _pair(backend_cls, case)
    N, H, W = case.N, case.H, case.W
    r1, t1, rows = be.rollout("mask", st.payload, st.op, case.flags, packed=True)
    errs = []
    for s in range(case.S):
        r2, t2 = orc.step("mask", st.payload[s], st.op[s], case.flags)
        g, d, rw, tm = B.unpack_rows(rows[s], H, W)
        for name, got, want in (("reward", r1[s], r2), ("terminated", t1[s], t2), ("packed grid", g, orc.get("grid")), ("packed grid_dim", d, orc.get("grid_dim")),
                                ("packed reward", rw, r2), ("packed terminated", tm, t2)):
            bad = np.nonzero((np.asarray(got).reshape(N, -1) != np.asarray(want).reshape(N, -1)).any(1))[0]
            if len(bad):
                errs.append(f"rollout {H}x{W} step {s}: {name} differs: " + "; ".join(f"env {n} op {st.op[s][n]}: {', '.join(st.names[s][n]) or '-'}" for n in bad[:6]))
        if len(errs) > 12:
            return errs
    for f in FIELDS:
        if not np.array_equal(be.get(f), orc.get(f)):
            errs.append(f"rollout {H}x{W}: final field {f} differs")
    if not np.array_equal(be.counters(), orc.counters()):
        errs.append(f"rollout {H}x{W}: final counters differ")
    s1, s2 = be.status(), orc.status()
    if s1 != s2:
        errs.append(f"rollout {H}x{W}: status {s1} vs oracle {s2}")
    return errs


ROW_STEPS = (8, 24, 40)


def rows_check(backend_cls, case, forms=("mask", "bits")):
    """The oracle's state rows before steps 8, 24 and 40 of a chain stream with those steps' actions through transition_rows, out of
    place and in place, against the oracle's next rows, reward, terminated and status.  At least a third of the rows of every such step
    continue an active object (asserted on the oracle's census).  The handle holds 8 envs more than the stream (the row kernel requests
    1024 bytes from an env's answer plane on, whatever the plane stride: search_bits.flagged_transitions)."""
    st = stream_of(case)
    N, H, W = case.N, case.H, case.W
    tasks = [np.concatenate([a, a[:8]]) for a in st.tasks]
    be = backend_cls(N + 8, H, W, max_trial_of(case), "o2arc", st.ops)
    orc = B.OracleBackend(N, H, W, max_trial_of(case), "o2arc", st.ops)
    be.set_tasks(*tasks)
    orc.set_tasks(*st.tasks)
    be.reset(), orc.reset()
    errs = []
    for s in range(max(ROW_STEPS) + 1):
        rows = B.state_rows(orc)
        r2, t2 = orc.step("mask", st.payload[s], st.op[s], case.flags)
        ost = orc.status()
        if s not in ROW_STEPS:
            continue
        cont = sum(any(nm.startswith("cont:") for nm in st.names[s][n]) for n in range(N))
        assert 3 * cont >= N, f"rows {H}x{W} step {s}: only {cont} of {N} rows continue an active object"
        want, L = B.state_rows(orc), rows.shape[1]
        for form in forms:
            pay = B.pack_bits(st.payload[s]) if form == "bits" else st.payload[s]
            for in_place in (False, True):
                out, r1, t1 = be.transition_rows(rows, form, pay, st.op[s], flags=case.flags, in_place=in_place)
                tag = f"rows {H}x{W} step {s} {form} {'in place' if in_place else 'out of place'}"
                bad = np.nonzero((out[:, :L] != want).any(1))[0]
                if len(bad):
                    errs.append(f"{tag}: rows differ: " + "; ".join(f"row {n} op {st.op[s][n]}: {', '.join(st.names[s][n]) or '-'}" for n in bad[:6]))
                if not (np.array_equal(r1, r2) and np.array_equal(t1, t2)):
                    errs.append(f"{tag}: reward / terminated differ")
                if be.status() != ost:
                    errs.append(f"{tag}: status differs from the oracle's {ost}")
    return errs


def expansion_check(backend_cls, kind, H, W, mt, K=24):
    """expand_rows on parents that are all ACTIVE: search.case_pair envs driven 10 steps down a chain stream (hold: continue, or lift
    a fresh selection with a Move).  Even slots: an all-zero bit row with a Move / Rotate / Flip — the parent's object continued —,
    odd slots: search_bits.mask_mix.  Per-row and shared action sets, compared by search_bits._compare.  Asserted on the oracle's
    children first: every parent is active, at least half of the continued children differ from their parent."""
    import search as SR
    import search_bits as SB
    be, orc, rng, ops = SR.case_pair(backend_cls, kind, H, W, mt)
    N = orc.N
    rnd = random.Random(H * W + mt)
    roles = _roles(rnd, N, H, W)
    for _ in range(10):
        masks, op = chain_actions(rnd, rng, orc, roles, "o2arc", hold=True)
        orc.step("mask", masks, op)
    orc.status()
    rows, answers, adims = B.state_rows(orc), orc.get("answer"), orc.get("answer_dim")
    assert orc.get("active").all(), f"{H}x{W}: parents {np.nonzero(orc.get('active')[:, 0] == 0)[0].tolist()} are not active"
    grids, gdims = SB._grids_of(rows, kind, H, W)
    errs = []
    for per_row in (True, False):
        tag = f"deep expansion {H}x{W} {'per-row' if per_row else 'shared'}"
        if per_row:
            masks, op = SB.mask_mix(rng, grids, gdims, K, H, W), rng.integers(0, len(ops), (N, K)).astype(np.int32)
            masks[:, ::2] = 0
            op[:, ::2] = rng.integers(20, 28, (N, K // 2))
            masks_full, op_full = masks, op
        else:
            masks, op = SB.mask_mix(rng, grids[:1], gdims[:1], K, H, W)[0], rng.integers(0, len(ops), K).astype(np.int32)
            masks[::2] = 0
            op[::2] = rng.integers(20, 28, K // 2)
            masks_full, op_full = np.broadcast_to(masks, (N,) + masks.shape).copy(), np.broadcast_to(op, (N, K)).copy()
        want = SR.oracle_expand(rows, answers, adims, kind, H, W, mt, ops, "mask", masks_full.reshape(N, K, H * W), op_full)
        moved = float((want["rows"][:, ::2] != rows[:, None, :]).any(2).mean())
        print(f"{tag}: {moved:.2f} of the continued children differ from their parent")
        assert moved >= 0.5, f"{tag}: only {moved:.2f} of the continued children differ from their parent"
        got = be.expand_rows(rows, "bits", B.pack_bits(masks.reshape(-1, H, W)).reshape(masks.shape[:-2] + (SB.STRIDE,)), op, dense=True)
        SB._compare(errs, tag, got, want, rows, kind, H, W, op_full)
    return errs


# ---- the cases ------------------------------------------------------------------------------------------------------------------
FLAG_SETS = (0, O.STEP_AUTORESET | B.STEP_ELIDE_SELECTED)
EXOTIC_FLAG_SETS = (0, O.STEP_AUTORESET)  # (the exotic table has keep_sel ops: ARCLE_STEP_ELIDE_SELECTED is not valid for it, backends.can_elide)
STEP_SHAPES = ((30, 30), (32, 32), (12, 20), (7, 12), (2, 100))  # FW_FULL x 2, FW_FAST, FW_GENERIC x 2
EXOTIC_SHAPES = ((30, 30), (17, 20), (9, 32))
BIG_SHAPES = ((40, 40), (64, 64), (127, 127), (33, 100), (100, 12))
STEP_CASES = [Case("chain", H, W, "o2arc", fl, 64, 64) for H, W in STEP_SHAPES for fl in FLAG_SETS]
EXOTIC_CASES = [Case("chain", H, W, "exotic", fl, 64, 64) for H, W in EXOTIC_SHAPES for fl in EXOTIC_FLAG_SETS]
BIG_CASES = [Case("chain", H, W, "o2arc", fl, 32, 48) for H, W in BIG_SHAPES for fl in FLAG_SETS]
ROLLOUT_CASES = [Case("chain", H, W, "o2arc", 0, 64, 48) for H, W in ((30, 30), (7, 12))]
ROWS_CASES = ROLLOUT_CASES + [Case("chain", H, W, "o2arc", 0, 64, 48) for H, W in ((12, 12), (40, 40))]  # (the rows of steps 8 / 24 / 40 of these streams)
TUPLE_CASES = ([Case(f, H, W, "o2arc", fl, 64, 64) for H, W in ((30, 30), (12, 20), (7, 12)) for f in ("bbox", "point") for fl in FLAG_SETS]
               + [Case(f, 40, 40, "o2arc", fl, 32, 48) for f in ("bbox", "point") for fl in FLAG_SETS])
GROUPED_CASE = Case("bbox", 30, 30, "o2arc", 3, 2304, 16)
# The emulators step WHOLE streams of the lists above (every env: what they run is what the floors are asserted on), fewer of them.
EMU_STEP_CASES = [c for c in STEP_CASES if (c.H, c.W) in ((30, 30), (12, 20), (7, 12), (2, 100))]  # (2 x 100: the one-wavefront kernels' int8 wraps)
EMU_EXOTIC_CASES = [c for c in EXOTIC_CASES if (c.H, c.W) != (30, 30)]
EMU_BIG_CASES = [c for c in BIG_CASES if (c.H, c.W) in ((40, 40), (100, 12), (64, 64)) and c.flags]
EMU_TUPLE_CASES = [c for c in TUPLE_CASES if (c.H, c.W) in ((30, 30), (7, 12)) and c.flags]
EMU_127 = Case("chain", 127, 127, "o2arc", 3, 16, 128)  # 16 envs (a 127 x 127 env-step is the emulators' dearest), 128 steps
FLOOR_CASES = list(dict.fromkeys(STEP_CASES + EXOTIC_CASES + BIG_CASES + ROWS_CASES + TUPLE_CASES + [GROUPED_CASE, EMU_127]))
EMU_CASES = EMU_STEP_CASES + EMU_EXOTIC_CASES + EMU_BIG_CASES + EMU_TUPLE_CASES + ROWS_CASES + [EMU_127]
assert set(EMU_CASES) <= set(FLOOR_CASES)


class env_vars:
    """Context manager: environment variables set (None: removed) inside, restored after (the library reads ARCLE_GROUPED & co. when
    a handle is created)."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        import os
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, str(v))

    def __exit__(self, *a):
        import os
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
