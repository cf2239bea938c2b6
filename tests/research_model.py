"""An independent episode model of the research env's step, its action streams and their census.  Test infrastructure only.

The research configuration (ARCVecEnv(autoreset="resample", dense_reward=True, max_episode_steps=..., augment=...): the step flags
ELIDE_SELECTED | TRUNCATE | RESAMPLE | DENSE | FLAT_OBS, with or without ROWS_INCREMENTAL) was compared with itself almost everywhere:
rollouts against single steps of a twin, grouped against plain launches, the emulator against the same body.  `ResearchModel` is the
other side of such a comparison built from parts that are already pinned and from nothing of the code under test: ONE
backends.OracleBackend (the C restatement of the reference, which knows ARCLE_STEP_AUTORESET and nothing else), the documented host
mirror of the device draw (arcle_amd.sampling.draw_task, pinned on the device by features.sampler) and the rules of
include/arcle_hip.h / DESIGN.md §3:

  1. construction == reset_sampled(): env n loads the draw of (seed, env_base + n, episode 0) — entry pair_off[problem] + pair,
     np.rot90(perm[entry], k) zero-padded, a drawn quarter turn that does not fit the H x W plane dropped (k &= 2) —, the oracle's
     init_state, episode 1;
  2. an env that has ENDED (its record says terminated, or with TRUNCATE its step counter is >= step_limit) is re-initialised instead of
     executing the action — with RESAMPLE on the draw of its episode counter, which then advances, with plain AUTORESET on the input it
     has —: reward 0, terminated 0, counters 0.  The model marks those envs terminated and lets the oracle's own AUTORESET do it;
  3. truncated is read AFTER the step: counters[n, 0] >= step_limit;
  4. the dense pair is (0, 0) for a step that executed no action — an ended env, an op index outside the table, a Rotate / Flip the
     oracle refused: told by the oracle's step counter not advancing, never by op number — and (correct, total) of agents/env.py:44-58
     from the oracle's grid / answer otherwise (`dense_pair`);
  5. rows are the model's fields in backends.row_layout order (FilterO2ARC: the nine segments of bigcases.rows_case), the packed row is
     grid | grid_dim | reward | terminated, the status word is the oracle's.

`compare` / `compare_rollout` step a backend and the model side by side on a recorded stream and name, for every mismatch, the env and
what had just happened to it (ended by reward / by trials / by time limit, skipped, executed).  The streams are drawn while reading the
MODEL's state only; `census` names the situations each reaches and tests/test_research_model_host.py holds every stream the emulator
and GPU tests send to the floors."""
import functools
import random
from collections import Counter, namedtuple

import numpy as np

import backends as B
from arcle_amd.sampling import draw_task
from oracle import oracle as O

AUTORESET, ELIDE, TRUNCATE, RESAMPLE, DENSE, FLAT_OBS, PACK_OBS, ROWS_INC = 1, 2, 4, 8, 16, 128, 256, 512
RESEARCH = ELIDE | TRUNCATE | RESAMPLE | DENSE | FLAT_OBS
RESEARCH_INC = RESEARCH | ROWS_INC
AUG_PERMUTE, AUG_ROT90 = 1, 2
FILTERED = ("active", "clip", "clip_dim", "grid", "grid_dim", "object", "object_dim", "object_pos", "trials_remain")  # FilterO2ARC's row
FIELDS = list(O.PLANES) + list(O.REC)
FLOOR = 20


def crop_table():
    """The research env's op table: O2ARCv2Env's with Crop in the place of Resize (agents/env.py:23-28)."""
    ops = O.o2arc_ops()
    ops[33] = O.desc(O.OP_CROP_GRID, 0, O.F_RESET_SEL)
    return ops


def dense_pair(grid, gdim, ans, adim):
    """(correct, total, mixed) of agents/env.py:44-58 for one env: the cells of the grid that equal the answer inside the common
    rectangle, and the size of the union as the reference counts it — through the branch for "one side longer, the other shorter"
    (mixed) or through |A - G|."""
    gh, gw, ah, aw = int(gdim[0]), int(gdim[1]), int(adim[0]), int(adim[1])
    mh, mw = min(gh, ah), min(gw, aw)
    correct = int((grid[:mh, :mw] == ans[:mh, :mw]).sum())
    mixed = (gh <= ah) != (gw <= aw)
    total = mh * mw + (abs(gh - ah) * mw + abs(gw - aw) * mh if mixed else abs(ah * aw - gh * gw))
    return correct, total, mixed


def augmented(a, b, k, perm, H, W):
    """A table entry as a reset loads it: np.rot90(perm[.], k) of input a and answer b, zero-padded to H x W -> (input, input_dim,
    answer, answer_dim, k used).  A quarter turn that does not fit the plane is dropped (square planes always fit)."""
    if k & 1 and (a.shape[1] > H or a.shape[0] > W or b.shape[1] > H or b.shape[0] > W):
        k &= 2
    lut = np.asarray(perm, np.int8)
    out = []
    for g in (a, b):
        t = np.rot90(lut[g], k)
        p = np.zeros((H, W), np.int8)
        p[:t.shape[0], :t.shape[1]] = t
        out += [p, t.shape]
    return out[0], out[1], out[2], out[3], k


class ResearchModel:
    """See the module's docstring.  tasks=(input, input_dim, answer, answer_dim) padded arrays: no table and no draw (ins ... aug_flags
    are ignored), for the flag sets without RESAMPLE on fixed tasks."""

    def __init__(self, N, H, W, max_trial, ops, ins, outs, pair_off, pair_cnt, seed, env_base, aug_flags, step_limit, flags, tasks=None):
        self.N, self.H, self.W, self.kind, self.flags, self.step_limit = N, H, W, "o2arc", flags, step_limit
        self.ins, self.outs, self.pair_off, self.pair_cnt = ins, outs, pair_off, pair_cnt
        self.seed, self.env_base, self.aug_flags = seed, env_base, aug_flags
        self.orc = B.OracleBackend(N, H, W, max_trial, "o2arc", ops)
        self.episode, self.cur_task = np.zeros(N, np.int32), np.full(N, -1, np.int32)
        self.counts = Counter()
        self.last_reward = np.zeros(N, np.int32)
        self.after_reset = np.zeros(N, bool)
        if tasks is not None:
            self.orc.set_tasks(*tasks)
        else:
            for n in range(N):
                self._load(n)
        self.orc.reset()

    # ---- the Backend read interface: the model's fields (state_rows and the tests read them like any backend's) -------------------
    def get(self, f):
        return self.orc.get(f)

    def counters(self):
        return self.orc.counters()

    def _load(self, n):
        """rule 1: the draw of env n's episode counter into the oracle's input / answer planes and dims; -> the quarter turn was dropped"""
        p, s, k, perm = draw_task(self.seed, self.env_base + int(n), int(self.episode[n]), self.pair_cnt, self.aug_flags)
        t = int(self.pair_off[p]) + s
        e = self.orc.env
        e.planes["input"][n], e.field("input_dim")[n], e.planes["answer"][n], e.field("answer_dim")[n], used = augmented(
            self.ins[t], self.outs[t], k, perm, self.H, self.W)
        self.episode[n] += 1
        self.cur_task[n] = t
        return used != k

    def ended(self):
        """rule 2 -> (ended bool [N], why: list of None | "reward" | "trials" | "time limit")"""
        e, c = self.orc.env, self.orc.env.cnt
        term = e.field("terminated")[:, 0] != 0
        late = (c[:, 0] >= self.step_limit) if self.flags & TRUNCATE else np.zeros(self.N, bool)
        if not self.flags & (AUTORESET | RESAMPLE):
            term, late = term & False, late & False
        why = [("reward" if self.last_reward[n] == 1 else "trials") if term[n] else "time limit" if late[n] else None for n in range(self.N)]
        return term | late, why

    def step(self, form, payload, op):
        """One step of every env -> dict(reward, terminated, truncated, dense [N, 2], status, what: per env "ended by reward" | "ended by
        trials" | "ended by time limit" | "skipped" | "executed").  Counts the step's situations into self.counts."""
        e, N = self.orc.env, self.N
        ended, why = self.ended()
        names = Counter()
        pre_grid, pre_gdim, pre_steps = e.planes["grid"].copy(), e.field("grid_dim").copy(), e.cnt[:, 0].copy()
        for n in np.nonzero(ended)[0]:
            names["end:" + why[n]] += 1
            if why[n] == "time limit" and e.field("active")[n, 0] and e.planes["selected"][n].any():
                names["end:time limit, object active and selected != 0"] += 1
            if e.field("clip_dim")[n].all():
                names["end:clip not empty"] += 1
            if tuple(e.field("grid_dim")[n]) != tuple(e.field("input_dim")[n]):
                names["end:grid_dim != input_dim"] += 1
            if self.flags & RESAMPLE:
                old = tuple(e.field("input_dim")[n])
                if self._load(n):
                    names["end:drawn quarter turn dropped"] += 1
                if tuple(e.field("input_dim")[n]) != old:
                    names["end:new task's dims differ"] += 1
            e.field("terminated")[n] = 1  # the oracle's own init_state re-initialises the env (ARCLE_STEP_AUTORESET)
        reward, term = self.orc.step(form, payload, op, AUTORESET if self.flags & (AUTORESET | RESAMPLE) else 0)
        status = self.orc.status()
        steps = e.cnt[:, 0]
        executed = ~ended & (steps != pre_steps)
        opv = np.asarray(payload)[:, 4] if form == "bbox5" else np.asarray(op)
        dense, what = np.zeros((N, 2), np.int32), []
        for n in range(N):
            if ended[n]:
                what.append("ended by " + why[n])
            elif not executed[n]:
                what.append("skipped")
                names["skip:bad op" if not 0 <= opv[n] < len(e.ops) else "skip:refused Rotate / Flip"] += 1
            else:
                what.append("executed")
                c, t, mixed = dense_pair(e.planes["grid"][n], e.field("grid_dim")[n], e.planes["answer"][n], e.field("answer_dim")[n])
                dense[n] = (c, t)
                names["dense:mixed branch"] += int(mixed)
                names["exec:grid unchanged"] += int(np.array_equal(pre_grid[n], e.planes["grid"][n]) and np.array_equal(pre_gdim[n], e.field("grid_dim")[n]))
                names["exec:right after a reset step"] += int(self.after_reset[n])
        self.counts += names
        self.last_reward = np.where(ended, 0, reward).astype(np.int32)
        self.after_reset = ended
        return {"reward": reward, "terminated": term, "truncated": (steps >= self.step_limit).astype(np.uint8), "dense": dense,
                "status": status, "what": what}

    def rows(self, filtered):
        """rule 5: the flattened observation rows, int8 [N, L]"""
        if not filtered:
            return B.state_rows(self)
        return np.ascontiguousarray(np.concatenate([self.get(f).reshape(self.N, -1) for f in FILTERED], 1).astype(np.int8))

    def packed(self, reward, term):
        """rule 5: the packed rows uint8 [N, (P + 7 + 15) & ~15]: grid | grid_dim | reward int32 LE | terminated | zeros"""
        P = self.H * self.W
        out = np.zeros((self.N, (P + 7 + 15) & ~15), np.uint8)
        out[:, :P + 7] = np.concatenate([self.get("grid").reshape(self.N, P).view(np.uint8), self.get("grid_dim").view(np.uint8),
                                         np.ascontiguousarray(reward, "<i4").view(np.uint8).reshape(self.N, 4), np.asarray(term, np.uint8).reshape(self.N, 1)], 1)
        return out


# ---- streams ------------------------------------------------------------------------------------------------------------------------
# One case = one stream.  stream "bbox" (sent as bbox or bbox5) | "mask" (sent as mask or bits) | "point"; mode "resample" (every flag
# set with RESAMPLE) | "autoreset" (AUTORESET | TRUNCATE | DENSE: the env keeps its task) | "vec" (as "resample", on the table ARCVecEnv
# builds from a SyntheticLoader).
Case = namedtuple("Case", "stream H W mode N S")
MAX_TRIAL, STEP_LIMIT, SEED, AUG = 2, 5, 0x5EED0A2C, AUG_PERMUTE | AUG_ROT90
PAIR_OFF, PAIR_CNT = np.array([0, 3, 4, 9], np.int32), np.array([3, 1, 5, 3], np.int32)
MODE_FLAGS = {"resample": RESEARCH, "autoreset": AUTORESET | TRUNCATE | DENSE, "vec": RESEARCH_INC}
VEC_SEED = 7
BAD_OPS = (35, 36, 40, 63, 64, 99, -1)
SUBMIT, COPY_FROM_INPUT, CROP, PASTE, RESET_GRID = 34, 31, 33, 30, 32


@functools.lru_cache(maxsize=None)
def task_table(H, W):
    """12 entries in 4 problems; the answer equals the input in every other entry (a Submit right after a reset, or after
    CopyFromInput, is rewarded there), the other answers have sides of their own."""
    rng = np.random.default_rng(H * 1000 + W)
    ins, outs = [], []
    for j in range(12):
        h, w = rng.integers(min(2, H), H + 1), rng.integers(min(2, W), W + 1)
        if H != W and j % 3 == 1:  # non-square planes: an entry that only fits unturned (a drawn quarter turn is dropped, a Rotate of its width refused)
            h, w = (h, rng.integers(H + 1, W + 1)) if W > H else (rng.integers(W + 1, H + 1), w)
        a = rng.integers(0, 10, (h, w)).astype(np.int8)
        ins.append(a)
        outs.append(a.copy() if j % 2 == 0 else rng.integers(0, 10, (rng.integers(1, H + 1), rng.integers(1, W + 1))).astype(np.int8))
    return ins, outs


@functools.lru_cache(maxsize=None)
def vec_env_table():
    """(loader, ins, outs, pair_off, pair_cnt) of mode "vec": the table ARCVecEnv builds from a loader's data — every demo pair of every
    task, then every test pair — and the sampler's view of it for adaptation=True (the demo pairs), restated from the loader's data."""
    from arcle_amd.loaders import SyntheticLoader
    loader = SyntheticLoader(n_tasks=40, seed=1, max_size=(30, 30))
    ins = [a for t in loader.data for a in t[0]] + [a for t in loader.data for a in t[2]]
    outs = [a for t in loader.data for a in t[1]] + [a for t in loader.data for a in t[3]]
    cnt = np.array([len(t[0]) for t in loader.data], np.int32)
    return loader, ins, outs, (np.cumsum(cnt) - cnt).astype(np.int32), cnt


def sampler_of(case):
    """(ins, outs, pair_off, pair_cnt, seed) of a case"""
    if case.mode == "vec":
        return vec_env_table()[1:] + (VEC_SEED,)
    return task_table(case.H, case.W) + (PAIR_OFF, PAIR_CNT, SEED + case.H * 128 + case.W)


def model_of(case, N=None, env_base=0, flags=None):
    ins, outs, off, cnt, seed = sampler_of(case)
    return ResearchModel(N or case.N, case.H, case.W, MAX_TRIAL, crop_table(), ins, outs, off, cnt, seed, env_base, AUG,
                         STEP_LIMIT, MODE_FLAGS[case.mode] if flags is None else flags)


def _span(rnd, dim, side):
    """(lo, hi) along one axis, relative to a dimension `dim` on a plane side `side`: inside, ending at dim - 1, or running past dim"""
    dim = max(1, min(dim, side))
    t = rnd.random()
    lo = rnd.randrange(dim)
    if t < 0.55:
        return lo, rnd.randint(lo, dim - 1)
    if t < 0.8 or dim >= side:
        return lo, dim - 1
    return lo, rnd.randint(dim, side - 1)


def _actions(rnd, nrng, model, stream):
    """One step's (payload, op) from the MODEL's state.  The weights feed the situations of `applicable` (the comment names which); the
    census of tests/test_research_model_host.py says which number to move when a floor is missed."""
    N, H, W = model.N, model.H, model.W
    rec, P, cnt = model.orc.env.rec, model.orc.env.planes, model.orc.env.cnt
    gd, ad = rec[:, 2:4].astype(int), rec[:, 14:16].astype(int)
    inside = (np.arange(H)[None, :, None] < gd[:, 0, None, None]) & (np.arange(W)[None, None, :] < gd[:, 1, None, None])
    solved = (gd == ad).all(1) & ~((P["grid"] != P["answer"]) & inside).any((1, 2))
    boxes, op = np.zeros((N, 4), np.int64), np.zeros(N, np.int32)
    empty = np.zeros(N, bool)
    for n in range(N):
        gh, gw, trials, active, steps = int(rec[n, 2]), int(rec[n, 3]), int(rec[n, 10]), bool(rec[n, 12]), int(cnt[n, 0])
        clip = bool(rec[n, 4]) and bool(rec[n, 5])
        last = steps >= model.step_limit - 2  # the episode's last two steps: what the env holds now is what the time limit finds
        u = rnd.random()
        x0, x1 = _span(rnd, gh, H)
        y0, y1 = _span(rnd, gw, W)
        if u < 0.05:                                   # skip:bad op
            op[n] = rnd.choice(BAD_OPS)
        elif solved[n] and u < 0.40:                   # end:reward
            op[n] = SUBMIT
        elif u < (0.42 if trials == 1 else 0.19):      # end:trials (two failed Submits inside five steps)
            op[n] = SUBMIT
        elif u < (0.75 if last else 0.50):             # object ops: end:time limit with an active object and selected != 0
            op[n] = rnd.choice((20, 21, 22, 23, 24, 25, 26, 27))
            if stream == "mask" and active and rnd.random() < 0.5:
                empty[n] = True                        # (masks only: the object continued with an empty selection)
            elif stream != "point" and (gw > H or gh > W) and rnd.random() < 0.5:  # skip:refused — a box too long for the plane's short side, turned
                op[n] = rnd.choice((24, 25))
                if gw > H:
                    y0, y1 = 0, rnd.randint(H, gw - 1)
                else:
                    x0, x1 = 0, rnd.randint(W, gh - 1)
            else:
                x1, y1 = min(x1, x0 + 5, max(gh - 1, x0)), min(y1, y0 + 5, max(gw - 1, y0))
        elif u < (0.79 if last else 0.62):             # Copy: end:clip not empty, exec:grid unchanged
            op[n] = rnd.choice((28, 29))
        elif clip and u < 0.70:                        # Paste
            op[n] = PASTE
        elif u < (0.87 if last else 0.78):             # Crop: end:grid_dim != input_dim, dense:mixed branch
            op[n] = CROP
        elif u < 0.86 or last:                         # CopyFromInput: solved grids on the entries whose answer is the input
            op[n] = COPY_FROM_INPUT
        elif u < 0.95:                                 # Color / FloodFill
            op[n] = rnd.randrange(0, 20)
            if op[n] >= 10:
                x1, y1 = x0, y0
        else:
            op[n] = RESET_GRID
        boxes[n] = (x0, y0, x1, y1)
    if stream == "point":
        ends = nrng.random(N) < 0.5
        pay = np.where(ends[:, None], boxes[:, 2:], boxes[:, :2])
        return np.ascontiguousarray(np.minimum(pay, [H - 1, W - 1]).astype(np.int32)), op
    if stream == "bbox":
        swap = nrng.random(N) < 0.5  # (the wrapper sorts the corners)
        return np.ascontiguousarray(np.where(swap[:, None], boxes[:, [2, 3, 0, 1]], boxes).astype(np.int32)), op
    masks = np.zeros((N, H, W), np.int8)
    for n in range(N):
        if not empty[n]:
            x0, y0, x1, y1 = boxes[n]
            box = (nrng.random((x1 - x0 + 1, y1 - y0 + 1)) < 0.8).astype(np.int8)
            box[0, :], box[:, 0], box[-1, -1] = 1, 1, 1  # (the bounding box stays the drawn one)
            masks[n, x0:x1 + 1, y0:y1 + 1] = box
    return masks, op


class Stream:
    """The recorded actions of a case and the census of the model's run: payload [S, N, ...], op [S, N], counts, episodes [N]."""


@functools.lru_cache(maxsize=8)
def stream_of(case):
    seed = (case.H * 1000 + case.W) * 8 + {"bbox": 0, "mask": 1, "point": 2}[case.stream] + {"resample": 0, "autoreset": 4, "vec": 5}[case.mode]
    rnd, nrng = random.Random(seed), np.random.default_rng(seed)
    model = model_of(case)
    st = Stream()
    st.case = case
    pays, opl = [], []
    for s in range(case.S):
        pay, op = _actions(rnd, nrng, model, case.stream)
        model.step(case.stream, pay, op)
        pays.append(pay)
        opl.append(op)
    st.payload, st.op, st.counts, st.episodes = np.stack(pays), np.stack(opl), model.counts, model.episode.copy()
    return st


def applicable(case):
    """The situations a case must reach at least FLOOR times."""
    need = ["end:reward", "end:trials", "end:time limit", "end:time limit, object active and selected != 0", "end:clip not empty",
            "end:grid_dim != input_dim", "skip:bad op", "dense:mixed branch", "exec:grid unchanged", "exec:right after a reset step"]
    if case.mode != "autoreset":
        need.append("end:new task's dims differ")
        if case.H != case.W:
            need.append("end:drawn quarter turn dropped")
    if case.H != case.W and case.stream != "point":  # (a point selects one cell: a 1 x 1 object turns on every plane)
        need.append("skip:refused Rotate / Flip")
    return need


def check_floors(case):
    counts = stream_of(case).counts
    return [f"{case}: {name} occurs {counts[name]} times, floor {FLOOR}" for name in applicable(case) if counts[name] < FLOOR]


def table_line(case):
    st = stream_of(case)
    return (f"{case.stream:5s} {case.H:3d}x{case.W:<3d} {case.mode:9s} N {case.N} S {case.S}, episodes per env {int(st.episodes.min())}-{int(st.episodes.max())}: "
            + ", ".join(f"{k} {st.counts[k]}" for k in sorted(st.counts)))


# ---- comparison ---------------------------------------------------------------------------------------------------------------------
FORMS = {"bbox": ("bbox", "bbox5"), "mask": ("mask", "bits"), "point": ("point",)}


def _send(be, form, pay, op, flags):
    if form == "bits":
        return be.step("bits", B.pack_bits(pay, be.bits_stride), op, flags)
    if form == "bbox5":
        return be.step("bbox5", np.concatenate([pay, op[:, None]], 1), None, flags)
    return be.step(form, pay, op, flags)


def setup(cls, case, flags, rows=None, N=None, env_base=0, step_limit=STEP_LIMIT):
    """A backend in the state the model is constructed in, with the outputs of `flags` installed (rows: "filtered" | "full")."""
    ins, outs, off, cnt, seed = sampler_of(case)
    be = cls(N or case.N, case.H, case.W, MAX_TRIAL, "o2arc", crop_table())
    be.set_task_table(ins, outs)
    be.set_sampler(off, cnt, seed, env_base, AUG)
    if flags & TRUNCATE:
        be.set_truncation(step_limit)
    if flags & DENSE:
        be.set_dense_output()
    be.reset_sampled()
    if flags & FLAT_OBS:
        be.set_flat_output(filtered=rows == "filtered")
    if flags & PACK_OBS:
        be.set_packed_output()
    return be


def _diff(errs, tag, name, got, want, what, op):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        errs.append(f"{tag}: {name} has shape {got.shape}, the model's {want.shape}")
        return
    bad = np.nonzero((got.reshape(len(want), -1) != want.reshape(len(want), -1)).any(1))[0]
    if len(bad):
        errs.append(f"{tag}: {name} differs: " + "; ".join(f"env {n} ({what[n]}, op {op[n]})" for n in bad[:6]))


def _state_diff(errs, tag, parts, model, what, op):
    """every plane and record field (input / answer / their dims included), counters, episode, cur_task"""
    cat = (lambda f: np.concatenate([f(be) for be, _ in parts])) if len(parts) > 1 else (lambda f: f(parts[0][0]))
    for f in FIELDS:
        _diff(errs, tag, f"field {f}", cat(lambda be: be.get(f)), model.get(f), what, op)
    _diff(errs, tag, "counters", cat(lambda be: be.counters()), model.counters(), what, op)
    _diff(errs, tag, "episode", cat(lambda be: np.asarray(be.episode)), model.episode, what, op)
    _diff(errs, tag, "cur_task", cat(lambda be: np.asarray(be.cur_task)), model.cur_task, what, op)


def compare(backend, model, st, flags, rows=None, form=None, steps=None):
    """Steps `backend` — one backend of model.N envs, or a list of (backend, slice of the model's envs) shards — and the model through
    the recorded stream; after every step: reward, terminated, truncated, the dense pair, counters, episode, cur_task, every plane and
    record field, the status word and, where `flags` ask for them, the row (rows "filtered" | "full") and the packed row.  With
    ROWS_INCREMENTAL the first step runs without it: the one full write the flag's contract asks for.  -> mismatch strings."""
    case = st.case
    form = form or case.stream
    parts = backend if isinstance(backend, list) else [(backend, slice(0, model.N))]
    cat = (lambda f: np.concatenate([f(be) for be, _ in parts])) if len(parts) > 1 else (lambda f: f(parts[0][0]))
    errs = []
    for s in range(steps or case.S):
        pay, op = st.payload[s], st.op[s]
        fl = flags & ~ROWS_INC if s == 0 else flags
        want = model.step(case.stream, pay, op)
        got = [_send(be, form, pay[sl], op[sl], fl) for be, sl in parts]
        what = want["what"]
        tag = f"{case.stream} {case.H}x{case.W} {form} flags {flags} step {s}"
        _diff(errs, tag, "reward", np.concatenate([g[0] for g in got]), want["reward"], what, op)
        _diff(errs, tag, "terminated", np.concatenate([g[1] for g in got]), want["terminated"], what, op)
        if flags & TRUNCATE:
            _diff(errs, tag, "truncated", cat(lambda be: np.asarray(be.trunc)), want["truncated"], what, op)
        if flags & DENSE:
            _diff(errs, tag, "dense pair", cat(lambda be: np.asarray(be.dense)), want["dense"], what, op)
        _state_diff(errs, tag, parts, model, what, op)
        if flags & FLAT_OBS:
            _diff(errs, tag, f"{rows} row", cat(lambda be: be.fused_flat()), model.rows(rows == "filtered"), what, op)
        if flags & PACK_OBS:
            _diff(errs, tag, "packed row", cat(lambda be: be.fused_packed()), model.packed(want["reward"], want["terminated"]), what, op)
        status = 0
        for be, _ in parts:
            status |= be.status()
        if status != want["status"]:
            errs.append(f"{tag}: status {status}, the oracle's {want['status']}")
        if len(errs) > 12:
            break
    for be, _ in parts:
        if hasattr(be, "padding_is_zero") and not be.padding_is_zero():
            errs.append(f"{case}: plane padding bytes (cells >= H * W) are not zero")
    return errs


def compare_rollout(be, model, st, flags, rows=None, form=None):
    """The recorded stream as ONE be.rollout_ex launch against the model stepped S times: every step's reward, terminated, truncated,
    dense pair, row and packed row, then the final state, counters, episode, cur_task and the status word (the OR of the steps')."""
    case = st.case
    form = form or case.stream
    pay = np.concatenate([st.payload, st.op[..., None]], 2) if form == "bbox5" else st.payload
    reward, term, out = be.rollout_ex(form, pay, st.op, flags, rows)
    errs, status = [], 0
    for s in range(case.S):
        op = st.op[s]
        want = model.step(case.stream, st.payload[s], op)
        what = want["what"]
        status |= want["status"]
        tag = f"rollout {case.stream} {case.H}x{case.W} {form} flags {flags} step {s}"
        _diff(errs, tag, "reward", reward[s], want["reward"], what, op)
        _diff(errs, tag, "terminated", term[s], want["terminated"], what, op)
        if flags & TRUNCATE:
            _diff(errs, tag, "truncated", out["trunc"][s], want["truncated"], what, op)
        if flags & DENSE:
            _diff(errs, tag, "dense pair", out["dense"][s], want["dense"], what, op)
        if flags & FLAT_OBS:
            w = model.rows(rows == "filtered")
            _diff(errs, tag, f"{rows} row", out["rows"][s][:, :w.shape[1]], w, what, op)
            if out["rows"][s][:, w.shape[1]:].any():
                errs.append(f"{tag}: row padding not zero")
        if flags & PACK_OBS:
            _diff(errs, tag, "packed row", out["packed"][s], model.packed(want["reward"], want["terminated"]), what, op)
        if len(errs) > 12:
            return errs
    _state_diff(errs, f"rollout {case.stream} {case.H}x{case.W} {form} final", [(be, None)], model, what, op)
    if be.status() != status:
        errs.append(f"rollout {case.H}x{case.W} {form}: status differs from the OR of the oracle's {status}")
    return errs


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
SHAPES = ((30, 30), (32, 32), (20, 24), (12, 12), (7, 12))          # FW_FULL x 2, FW_FAST, FW_GENERIC x 2
BIG_SHAPES = ((40, 40), (36, 41), (64, 64), (100, 12))
R = "resample"
GPU_LEAN = [Case(s, 30, 30, R, 64, 48) for s in ("bbox", "mask", "point")]                              # sent in all five forms
GPU_WIDTHS = [Case(s, H, W, R, 64, 48) for H, W in SHAPES[1:] for s in ("bbox", "mask")]
GPU_GROUPED = Case("bbox", 30, 30, R, 512, 12)
GPU_ROLLOUT = GPU_LEAN + [Case("bbox", 10, 10, R, 64, 48)]
GPU_BIG = [Case(s, H, W, R, 32, 48) for H, W in BIG_SHAPES for s in ("bbox", "mask")] + [Case(s, 127, 127, R, 16, 48) for s in ("bbox", "mask")]
GPU_VEC = Case("bbox", 30, 30, "vec", 64, 48)
GPU_SHARDS = [Case("bbox", 30, 30, R, 64, 48), Case("bbox", 40, 40, R, 32, 48)]
# The emulators step whole streams of their own size (an emulated env-step costs milliseconds): 32 envs x 40 steps on the one-wavefront
# body, 24 x 40 on the big-grid bodies — every one of them held to the same floors.
EMU = [Case(s, H, W, R, 32, 40) for H, W in SHAPES for s in ("bbox", "mask", "point")]
EMU_AUTORESET = [Case("bbox", 30, 30, "autoreset", 32, 40), Case("mask", 7, 12, "autoreset", 32, 40)]
EMU_ROLLOUT = [Case(s, H, W, R, 32, 40) for s, H, W in (("bbox", 30, 30), ("point", 30, 30), ("mask", 30, 30), ("bbox", 12, 12), ("mask", 7, 12))]
EMU_BIG = [Case(s, H, W, R, 24, 40) for H, W in BIG_SHAPES for s in ("bbox", "mask")]
EMU_GROUPED = GPU_GROUPED
FLOOR_CASES = list(dict.fromkeys(GPU_LEAN + GPU_WIDTHS + [GPU_GROUPED] + GPU_ROLLOUT + GPU_BIG + GPU_SHARDS + [GPU_VEC] + EMU + EMU_AUTORESET + EMU_ROLLOUT + EMU_BIG))
