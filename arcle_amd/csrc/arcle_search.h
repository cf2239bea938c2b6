// arcle_search.h — search support on flattened state rows: the state hash and the K-actions-per-row expansion.
//
//   wave_hash_row    one wavefront hashes one state row (arcle_hash_rows)
//   wave_expand_row  one wavefront owns one PARENT row and a chunk of its candidate actions (arcle_expand_rows): per action it runs
//                    the very step body of arcle_transition_rows (step_core in resident mode, the planes in registers) and
//                    writes the verdicts — reward, terminated, status, the dense pair, the child's hash — but never the child row
//
// Compiled like arcle_wave.h: by hipcc through arcle_hip.hip and by g++ through tests/emu/search_emu.cpp; it uses only the xl::
// primitives both define and leaves arcle_wave.h as it is.
//
// The hash (restated in include/arcle_hip.h and mirrored in NumPy by arcle_amd/search.py::hash_rows_numpy)
//   fa(x) = murmur3's 32-bit finaliser, fb(x) = the "lowbias32" finaliser: two multiplies and three xor-shifts each
//   a plane dword d at dword index j of plane pl (bytes beyond H*W read as zero, j < ceil(H*W / 4)):   t = (pl + 1) * 256 + j
//       A += fa(d ^ (t * 0x9E3779B1)),   B += fb(d + t * 0x85EBCA77)
//   the record's dwords w[i] (i < 4) restricted to the scalar fields the row of this env kind carries:  t = 0x0F00 + i, same two terms
//   state_hash = A | B << 32 over every plane and the record (sums mod 2^32);  grid_hash = the same over the grid plane and the
//   grid_dim bytes of the record alone (tag 0x0E00)
// Every (dword, plane, position) goes through a nonlinear finaliser BEFORE the sum, so equal deltas at two positions do not cancel
// (what a sum of dword * odd constant does once in 16 pairs); the sum makes the hash decomposable: a child's hash is the parent's
// with the terms of the planes the step stored, and of the record, replaced.
#pragma once
#include "arcle_wave.h"

// How an action gets the parent's planes back.  1 (default): the wave keeps a second register copy of all seven planes (28 VGPRs)
// and restores the working copy from it; 0: on demand — a plane the op reads is requested again from the parent row, which is hot
// in the L2 after the wave's first pass.  Both measured (profiles/expand_bench.txt): the copy wins by 5-20 %.
#ifndef ARCLE_EXPAND_KEEP_PARENT
#define ARCLE_EXPAND_KEEP_PARENT 1
#endif

namespace arcle {

// launch parameters of the two search kernels: the step parameters as arcle_transition_rows sets them up (rows_in = the M parent rows,
// n_envs = M, task_idx = src_env, sel / op = the actions, reward / term / dense = the [M][K] outputs, status = a scratch word), and
// what a StepParams has no field for
struct ExpandParams {
  StepParams p;
  int32_t n_actions;          // K
  int32_t action_row_stride;  // 0: one set of K actions for every row; K: a set per row
  int32_t chunk;              // actions per wavefront
  int32_t n_chunks;           // ceil(K / chunk): wavefronts per parent row
  uint8_t* status_out;        // uint8 [M][K]: ARCLE_ST_* bits child (m, k) raised
  uint64_t* hash;             // uint64 [M][K][2] (state_hash, grid_hash) of every child; arcle_hash_rows: [n_rows][2]
  uint64_t* parent_hash;      // optional uint64 [M][2]
};

ARCLE_DEV uint32_t hash_fa(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  x ^= x >> 16;
  return x;
}
ARCLE_DEV uint32_t hash_fb(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
struct Hash2 {
  uint32_t a, b;
};
ARCLE_DEV void hash_word(Hash2& h, uint32_t d, uint32_t tag) {
  h.a += hash_fa(d ^ (tag * 0x9E3779B1u));
  h.b += hash_fb(d + tag * 0x85EBCA77u);
}
// what a lane's four dwords of ANY plane share: the position part of the two pre-keys (tag * constant splits into a per-plane
// constant + a per-position term, so no multiply per plane), the mask of the cells that exist, and whether the dword exists at all
struct HashKeys {
  uint32_t ka[4], kb[4], keep[4];
};
ARCLE_DEV HashKeys hash_keys(const Wave& w) {
  HashKeys hk;
  const int P = w.p.P;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int b0 = 16 * w.lane + 4 * i;  // first byte of the dword inside the plane
    const uint32_t j = (uint32_t)(4 * w.lane + i);
    hk.ka[i] = j * 0x9E3779B1u;
    hk.kb[i] = j * 0x85EBCA77u;
    hk.keep[i] = b0 >= P ? 0u : P - b0 >= 4 ? 0xffffffffu : (1u << (8 * (P - b0))) - 1u;
  }
  return hk;
}
// this lane's share of plane `pl`'s term: its four dwords (cells beyond H*W masked to zero, dwords beyond the plane skipped)
ARCLE_DEV Hash2 hash_plane_lane(const HashKeys& hk, int pl, const U4& v) {
  Hash2 h = {0u, 0u};
  const uint32_t pa = (uint32_t)(pl + 1) * 256u * 0x9E3779B1u, pb = (uint32_t)(pl + 1) * 256u * 0x85EBCA77u;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const uint32_t d = v[i] & hk.keep[i];
    const uint32_t a = hash_fa(d ^ (pa + hk.ka[i])), b = hash_fb(d + pb + hk.kb[i]);
    h.a += hk.keep[i] ? a : 0u;
    h.b += hk.keep[i] ? b : 0u;
  }
  return h;
}
// the record bytes that are part of a state row of this env kind (answer_dim never is; the rest follows flat_row's layout)
ARCLE_DEV void hash_rec_masks(const StepParams& p, uint32_t m[4]) {
  const bool o2 = p.plane[ARCLE_PL_SELECTED] != nullptr, clip = p.plane[ARCLE_PL_CLIP] != nullptr;
  m[0] = 0xffffffffu;                                  // input_dim, grid_dim
  m[1] = (clip ? 0x0000ffffu : 0u) | (o2 ? 0xffff0000u : 0u);  // clip_dim | object_dim
  m[2] = (o2 ? 0x0000ffffu : 0u) | 0xffff0000u;        // object_pos | trials_remain, terminated
  m[3] = o2 ? 0x0000ffffu : 0u;                        // active, rotation_parity
}
// wave-uniform: the record's term of state_hash, and the grid_dim term of grid_hash
ARCLE_DEV Hash2 hash_rec(const StepParams& p, const Rec& r) {
  uint32_t m[4];
  hash_rec_masks(p, m);
  Hash2 h = {0u, 0u};
#pragma unroll
  for (int i = 0; i < 4; i++) hash_word(h, r.w[i] & m[i], 0x0F00u + (uint32_t)i);
  return h;
}
ARCLE_DEV Hash2 hash_grid_dim(const Rec& r) {
  Hash2 h = {0u, 0u};
  hash_word(h, r.w[0] & 0xffff0000u, 0x0E00u);
  return h;
}
// (state_hash, grid_hash) from the lane-local sums over all planes / over the grid plane: four wave reductions, then the record terms
ARCLE_DEV void hash_finish(const Wave& w, const Rec& r, const Hash2& all, const Hash2& grid, uint64_t* out) {
  const Hash2 hr = hash_rec(w.p, r), hg = hash_grid_dim(r);
  const uint32_t sa = xl::wave_add(all.a) + hr.a, sb = xl::wave_add(all.b) + hr.b;
  const uint32_t ga = xl::wave_add(grid.a) + hg.a, gb = xl::wave_add(grid.b) + hg.b;
  xl::lanes_converged();
  if (w.lane == 0) {
    out[0] = (uint64_t)sa | ((uint64_t)sb << 32);
    out[1] = (uint64_t)ga | ((uint64_t)gb << 32);
  }
}

// arcle_hash_rows: x.hash[row] = hash of row `row` of p.rows_in (any alignment, any stride >= the row length)
ARCLE_DEV void wave_hash_row(const ExpandParams& x, WaveLDS* lds, const U2* lut, int row, int lane) {
  const StepParams& p = x.p;
  Wave w(p, lds, lut, lane, INGRESS_BBOX, FW_GENERIC, false);
  Rec r;
  r.w[0] = r.w[1] = r.w[2] = r.w[3] = 0u;
  Hash2 all = {0u, 0u}, grid = {0u, 0u};
  const HashKeys hk = hash_keys(w);
  read_state_row(w, p.rows_in + (size_t)row * p.rows_in_stride, r, [&](int pl, const U4& v) {
    const Hash2 t = hash_plane_lane(hk, pl, v);
    all.a += t.a;
    all.b += t.b;
    if (pl == ARCLE_PL_GRID) grid = t;
  });
  hash_finish(w, r, all, grid, x.hash + 2 * (size_t)row);
}

// arcle_expand_rows: parent row m, actions [k0, k1) of its set.  Once per wave: the row's scalars, the parent's planes and the
// lane-local hash terms of each (the one pass over the row's 7 planes).  Per action: record, planes and plane bookkeeping back to
// the parent, step_core exactly as wave_transition_row runs it (resident mode: every plane access is a register access), then the
// child's hash from the parent's terms with those of the planes in w.stored recomputed from w.cache.
// (`stored` names every plane a step changed: the invariant the in-place arcle_transition_rows rests on.)
template <int ING, int FW>
ARCLE_DEV void wave_expand_row(const ExpandParams& x, WaveLDS* lds, const U2* lut, int m, int k0, int k1, int lane) {
  const StepParams& p = x.p;
  Wave w(p, lds, lut, lane, ING, FW, false);
  int src = m;
  if (p.task_idx) src = (int)xl::uniform((uint32_t)p.task_idx[m]);
  uint32_t st0 = 0;
  if (src < 0 || src >= p.n_resident) {  // no such env to take the answer from: every child is the parent, with the status bit
    st0 = ARCLE_ST_BAD_TASK;
    src = 0;
  }
  const int8_t* rin = p.rows_in + (size_t)m * p.rows_in_stride;
  w.set_env(src);
  Rec r0 = load_rec(p, src);  // (answer_dim; every state field is overwritten from the row)
  read_state_row(w, rin, r0, [&](int, const U4&) {}, false);
  w.resident = true;
  w.row_src = rin;
  w.answer_env = src;
  // the parent's per-plane terms (lane-local) and their sum
  const HashKeys hk = hash_keys(w);
  Hash2 pt[ARCLE_N_PLANES - 1];
  Hash2 pall = {0u, 0u};
#if ARCLE_EXPAND_KEEP_PARENT
  U4 par[ARCLE_N_PLANES - 1];
  uint32_t par_have = 0;
#endif
#pragma unroll
  for (int pl = 0; pl < ARCLE_N_PLANES - 1; pl++) {
    pt[pl] = Hash2{0u, 0u};
    if (p.plane[pl]) {
      const U4 v = row_plane(w, rin, row_offset(p, pl));
#if ARCLE_EXPAND_KEEP_PARENT
      par[pl] = v;
      par_have |= 1u << pl;
#endif
      pt[pl] = hash_plane_lane(hk, pl, v);
      pall.a += pt[pl].a;
      pall.b += pt[pl].b;
    }
  }
  // The answer plane of env `src`, requested here once per wave and by the lanes that hold bytes of it only.  (Left to Wave::load the
  // request would come from all 64 lanes: with a plane stride below 1024 bytes the lanes past it read behind the env's plane — for the
  // handle's last env behind the allocation, which may be the end of a mapped region.)
  U4 ans = u4_zero();
  if (p.plane[ARCLE_PL_ANSWER] && 16 * lane < p.PS) ans = xl::load16(p.plane[ARCLE_PL_ANSWER], (uint32_t)src * (uint32_t)p.PS + 16u * (uint32_t)lane);
  if (x.parent_hash && k0 == 0) hash_finish(w, r0, pall, pt[ARCLE_PL_GRID], x.parent_hash + 2 * (size_t)m);
  const size_t a0 = (size_t)m * (size_t)x.action_row_stride;  // first action of this row's set
  // the next action's tuple and op are requested under the current op
  U4 pay = load_payload(w, (int)(a0 + (size_t)k0), 0, p.sel);
  int op = (int)xl::uniform((uint32_t)p.op[a0 + (size_t)k0]);
  for (int k = k0; k < k1; k++) {
    const int kn = k + 1 < k1 ? k + 1 : k;
    const U4 pay_next = load_payload(w, (int)(a0 + (size_t)kn), 0, p.sel);
    const int op_next = (int)xl::uniform((uint32_t)p.op[a0 + (size_t)kn]);
    const int c = m * x.n_actions + k;  // child index: every output is [M][K]
    Rec r = r0;
    I2 cnt;
    cnt.x = cnt.y = 0;
#if ARCLE_EXPAND_KEEP_PARENT
#pragma unroll
    for (int pl = 0; pl < ARCLE_N_PLANES - 1; pl++)
      if (p.plane[pl]) w.cache[pl] = par[pl];
    w.have = par_have;
#else
    w.have = 0;
#endif
    w.cache[ARCLE_PL_ANSWER] = ans;
    w.have |= 1u << ARCLE_PL_ANSWER;
    w.dirty = 0;
    w.stored = 0;
    w.env = c;
    StepOut out;
    out.reward = 0;
    out.term = false;
    out.bytes = 0;
    out.status = st0;
    out.grid_loaded = false;
    out.have_grid = false;
    if (!st0) out = step_core<ING, FW, 0, 1>(w, r, cnt, pay, op);
    else if (p.flags & ARCLE_STEP_DENSE) dense_none(w);
    xl::lanes_converged();
    // child terms: the parent's, with every stored plane's share replaced
    Hash2 all = pall, grid = pt[ARCLE_PL_GRID];
#pragma unroll
    for (int pl = 0; pl < ARCLE_N_PLANES - 1; pl++) {
      if (p.plane[pl] && (w.stored & (1u << pl))) {
        const Hash2 t = hash_plane_lane(hk, pl, w.cache[pl]);
        all.a += t.a - pt[pl].a;
        all.b += t.b - pt[pl].b;
        if (pl == ARCLE_PL_GRID) grid = t;
      }
    }
    hash_finish(w, r, all, grid, x.hash + 2 * (size_t)c);
    if (lane == 0) {
      p.reward[c] = out.reward;
      p.term[c] = (uint8_t)out.term;
      x.status_out[c] = (uint8_t)(out.status & 0xffu);
    }
    pay = pay_next;
    op = op_next;
  }
}

// launch parameters of arcle_expand_macros: the expansion's (sel / op are [..][K][T][..], every output still [M][K]) and what a macro
// adds.  A struct of its own: ExpandParams is an argument of the kernels above and stays as it is.
struct MacroParams {
  ExpandParams x;
  int32_t max_len;     // T: steps a macro has room for
  const int32_t* len;  // int32 [..][K]: steps macro (m, k) runs, 1 .. T; NULL: every macro runs T
};

// arcle_expand_macros: parent row m, macros [k0, k1) of its set.  The wave's set-up is wave_expand_row's (restated, not shared: that
// body's code object is pinned, profiles/expand_macros_codeobj.txt).  Per macro: record and planes back to the parent, then len steps of
// step_core on the SAME working copy — step t + 1 sees what step t left in w.cache, as the rollout kernel chains its steps — and one
// set of verdicts: the rewards' sum, the last step's terminated, the OR of the status bits, the dense pair the last step wrote, and
// the hash of the final state.  `stored` and `dirty` are per step (step_core reads `stored` for the dense pair; the in-place
// arcle_transition_rows this kernel stands for starts every call with them clear); the hash needs every plane ANY step stored,
// which `touched` collects.  A macro whose len is outside [1, T] runs no step: ARCLE_ST_BAD_OP, the child is the parent.
template <int ING, int FW>
ARCLE_DEV void wave_expand_macros_row(const MacroParams& y, WaveLDS* lds, const U2* lut, int m, int k0, int k1, int lane) {
  const ExpandParams& x = y.x;
  const StepParams& p = x.p;
  Wave w(p, lds, lut, lane, ING, FW, false);
  int src = m;
  if (p.task_idx) src = (int)xl::uniform((uint32_t)p.task_idx[m]);
  uint32_t st0 = 0;
  if (src < 0 || src >= p.n_resident) {  // no such env to take the answer from: every child is the parent, with the status bit
    st0 = ARCLE_ST_BAD_TASK;
    src = 0;
  }
  const int8_t* rin = p.rows_in + (size_t)m * p.rows_in_stride;
  w.set_env(src);
  Rec r0 = load_rec(p, src);  // (answer_dim; every state field is overwritten from the row)
  read_state_row(w, rin, r0, [&](int, const U4&) {}, false);
  w.resident = true;
  w.row_src = rin;
  w.answer_env = src;
  const HashKeys hk = hash_keys(w);
  Hash2 pt[ARCLE_N_PLANES - 1];
  Hash2 pall = {0u, 0u};
#if ARCLE_EXPAND_KEEP_PARENT
  U4 par[ARCLE_N_PLANES - 1];
  uint32_t par_have = 0;
#endif
#pragma unroll
  for (int pl = 0; pl < ARCLE_N_PLANES - 1; pl++) {
    pt[pl] = Hash2{0u, 0u};
    if (p.plane[pl]) {
      const U4 v = row_plane(w, rin, row_offset(p, pl));
#if ARCLE_EXPAND_KEEP_PARENT
      par[pl] = v;
      par_have |= 1u << pl;
#endif
      pt[pl] = hash_plane_lane(hk, pl, v);
      pall.a += pt[pl].a;
      pall.b += pt[pl].b;
    }
  }
  // (the answer plane through the lanes that own bytes of it: see wave_expand_row)
  U4 ans = u4_zero();
  if (p.plane[ARCLE_PL_ANSWER] && 16 * lane < p.PS) ans = xl::load16(p.plane[ARCLE_PL_ANSWER], (uint32_t)src * (uint32_t)p.PS + 16u * (uint32_t)lane);
  if (x.parent_hash && k0 == 0) hash_finish(w, r0, pall, pt[ARCLE_PL_GRID], x.parent_hash + 2 * (size_t)m);
  const size_t a0 = (size_t)m * (size_t)x.action_row_stride;  // first macro of this row's set
  const int T = y.max_len;
  // step t of macro a is entry a * T + t of sel / op; the next step's tuple and op — of this macro, or the first of the next — are
  // requested under the current op
  U4 pay = load_payload(w, (int)((a0 + (size_t)k0) * (size_t)T), 0, p.sel);
  int op = (int)xl::uniform((uint32_t)p.op[(a0 + (size_t)k0) * (size_t)T]);
  int len = y.len ? (int)xl::uniform((uint32_t)y.len[a0 + (size_t)k0]) : T;
  for (int k = k0; k < k1; k++) {
    const int kn = k + 1 < k1 ? k + 1 : k;
    const size_t first_next = (a0 + (size_t)kn) * (size_t)T;
    const int len_next = y.len ? (int)xl::uniform((uint32_t)y.len[a0 + (size_t)kn]) : T;
    const int c = m * x.n_actions + k;  // child index: every output is [M][K]
    Rec r = r0;
#if ARCLE_EXPAND_KEEP_PARENT
#pragma unroll
    for (int pl = 0; pl < ARCLE_N_PLANES - 1; pl++)
      if (p.plane[pl]) w.cache[pl] = par[pl];
    w.have = par_have;
#else
    w.have = 0;
#endif
    w.cache[ARCLE_PL_ANSWER] = ans;
    w.have |= 1u << ARCLE_PL_ANSWER;
    w.env = c;
    uint32_t status = st0, touched = 0;
    if ((uint32_t)(len - 1) >= (uint32_t)T) status |= ARCLE_ST_BAD_OP;
    const int n = status ? 0 : len;
    int reward = 0;
    bool term = false;
    const size_t first = (a0 + (size_t)k) * (size_t)T;
#pragma nounroll
    for (int t = 0; t < n; t++) {
      const size_t nx = t + 1 < n ? first + (size_t)t + 1 : first_next;
      const U4 pay_next = load_payload(w, (int)nx, 0, p.sel);
      const int op_next = (int)xl::uniform((uint32_t)p.op[nx]);
      I2 cnt;
      cnt.x = cnt.y = 0;
      w.dirty = 0;
      w.stored = 0;
      const StepOut out = step_core<ING, FW, 0, 1>(w, r, cnt, pay, op);
      xl::lanes_converged();
      touched |= w.stored;
      status |= out.status;
      reward += out.reward;
      term = out.term;
      pay = pay_next;
      op = op_next;
    }
    if (n == 0) {  // the child that did not happen: the next macro's first step was not requested under a step
      if (p.flags & ARCLE_STEP_DENSE) dense_none(w);
      pay = load_payload(w, (int)first_next, 0, p.sel);
      op = (int)xl::uniform((uint32_t)p.op[first_next]);
    }
    // child terms: the parent's, with the share of every plane some step stored replaced
    Hash2 all = pall, grid = pt[ARCLE_PL_GRID];
#pragma unroll
    for (int pl = 0; pl < ARCLE_N_PLANES - 1; pl++) {
      if (p.plane[pl] && (touched & (1u << pl))) {
        const Hash2 t = hash_plane_lane(hk, pl, w.cache[pl]);
        all.a += t.a - pt[pl].a;
        all.b += t.b - pt[pl].b;
        if (pl == ARCLE_PL_GRID) grid = t;
      }
    }
    hash_finish(w, r, all, grid, x.hash + 2 * (size_t)c);
    if (lane == 0) {
      p.reward[c] = reward;
      p.term[c] = (uint8_t)term;
      x.status_out[c] = (uint8_t)(status & 0xffu);
    }
    len = len_next;
  }
}

}  // namespace arcle
