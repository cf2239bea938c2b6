// arcle_ray.h — the lines each object of a state row casts toward the answer (arcle_ray_rows): for every object (a bit row, as
// arcle_components_rows / arcle_objects_rows write it) and every set of directions asked for, the cells its rays cover — from the
// object's own cells through free cells up to the first obstacle or the edge of grid_dim — the colour that ONE Color step on those
// cells should paint to leave the most correct cells, and that count; the best set of every object with its cells as a ready-made
// bit-row selection.  The first sibling of arcle_place.h that DRAWS: its child holds cells no object of the row holds.  It takes over
// that file's layout (bit boards, one wavefront per row, AND + popcount against boards of the answer) and changes nothing of it.
//
//   wave_ray_row<FW, FLAT>  one wavefront takes ALL objects of one row: the grid, the answer of env src_env[row], the free board and the ten
//                     boards "answer == c" are built once per row; per object one occluded fill per direction in use, per set an OR
//                     of those and at most four packed wave sums, no step body
//
// Compiled like arcle_place.h: by hipcc through arcle_hip.hip and by g++ through tests/emu/ray_emu.cpp (plain C++ and xl:: only).
//
// With G the grid, B the object's cells inside grid_dim and FREE the cells inside grid_dim that a ray may enter (through = 0: the
// cells whose byte is free_color; through = 1: all of them), F = FREE & ~B, the ray of direction d is the least board with
//     R_d = shift_d(B | R_d) & F
// — it starts next to B's own cells only, runs while the cells are free, and neither B's cells nor anything behind an obstacle belong
// to it.  Candidate s is R_s = the OR of R_d over the directions of sets[s]; Color c on the selection R_s (color.py:70-77) sets exactly
// those cells to c, so with K0 = (grid == answer) and A_c = (answer == c), both inside the common rectangle of grid_dim and answer_dim,
//     correct(s, c) = popc(K0) - popc(R_s & K0) + popc(R_s & A_c)
// and the colour reported is the c in 0..9 with the most popc(R_s & A_c), the smaller c on a tie.
//
// THE FILL is a Kogge-Stone occluded fill on the ROW BOARD (W <= 32 and H <= 64; lane i = row i as a W-bit word):
//     gen = B, pro = F;  for s = 1, 2, 4, .. < n:  gen |= pro & shift_d(gen, s);  pro &= shift_d(pro, s);   R_d = gen & F
// with n = the extent of grid_dim along d (gw for W / E, gh for N / S, the smaller for a diagonal): at most 5 rounds at 30 x 30 where the
// plain loop R <- shift_d(B | R) & F needs one round per cell of the longest ray (up to 29 at 30 x 30, each a cross-lane move, an AND,
// a compare and a wave-uniform branch).  By an ESTIMATE of the instruction count from the source, not a count from the ISA — <= 5
// rounds of 2 shifts (W / E: 2 in-word shifts; N / S: 2 ds_bpermute with a bound check; diagonals: both) + 3 logic ops, roughly 20 to
// 50 instructions per direction, against roughly 29 x 5 for the loop at its longest — the doubling was chosen; the plain loop was not
// built for the row board, so no timing backs the choice.  shift_d by s moves row words by s lanes (0 shifted in beyond lanes 0 / 63) and bits by s columns;
// F is zero in rows >= gh and in bits >= gw, so whatever a shift carries beyond grid_dim meets zeros in `pro` and nothing wraps: no mask
// but F itself.
// On the FLAT BOARD (every other shape of at most 1024 cells; lane j < 32 = cells [32j, 32j + 32)) — the slower path, as in the
// siblings — the fill is the plain loop with flat shifts by 1 (W / E), W (N / S) and W +- 1 (diagonals), ending on a wave-uniform
// "nothing new" after at most max(gh, gw) rounds; a shift that moves a column is ANDed with the board of the columns it may arrive in
// (all but column 0 going east, all but column W - 1 going west), which is what keeps a ray from wrapping into the next row.
//
// THE COUNTS of one candidate — cells, popc(R_s & K0) and the ten popc(R_s & A_c) — are each at most 1023 (a ray never covers B, and B
// is not empty where a ray is not), so three of them share one 32-bit word (10 bits each) and the whole candidate costs FOUR wave sums,
// not twelve; a word whose colours the answer does not hold at all (a wave-uniform mask, built once per row) is skipped.
#pragma once
#include "arcle_place.h"

namespace arcle {

// launch parameters: p = the handle's base parameters with n_envs = the number of rows, n_resident = the handle's envs and rows_in /
// rows_in_stride = the state rows (rows_in NULL: the resident envs 0 .. n_envs-1)
struct RayParams {
  StepParams p;
  int32_t max_comp;        // C: objects per row at most
  int32_t n_sets;          // S: candidates per object, 1 .. RAY_MAX_SETS
  const int32_t* count;    // optional int32 [n_rows][2]: word 0 = the objects of the row (NULL: C)
  const uint8_t* bits;     // uint8 [n_rows][C][ARCLE_BITS_STRIDE], 2-byte aligned
  const int32_t* src_env;  // optional int32 [n_rows]: the env whose answer judges the row (NULL: env = row)
  const uint8_t* sets;     // uint8 [S]: the direction masks (bit 0..7 = N, S, W, E, NW, NE, SW, SE), read by every wave
  int32_t* ray;            // int32 [n_rows][C][S][4] = color, correct, cells, right
  int32_t* best;           // int32 [n_rows][C][4] = set, color, correct, cells
  uint8_t* best_bits;      // optional uint8 [n_rows][C][ARCLE_BITS_STRIDE], 2-byte aligned: the best candidate's cells as a bit row
  int32_t* base;           // optional int32 [n_rows][2]: the dense pair of the row's own grid
  int32_t free_color;      // through = 0: a ray enters the cells whose byte equals this (as int8)
  int32_t through;         // 1: a ray enters every cell of grid_dim outside the object
};

constexpr int RAY_MAX_SETS = 16;
constexpr int RAY_COLORS = 10;  // Color 0 .. 9

ARCLE_DEV void ray_emit(const RayParams& x, int lane, int row, int k, int s, int color, int correct, int cells, int right) {
  if (lane == 0) {
    U4 v;
    v[0] = (uint32_t)color;
    v[1] = (uint32_t)correct;
    v[2] = (uint32_t)cells;
    v[3] = (uint32_t)right;
    xl::store_at(x.ray + ((size_t)row * (size_t)x.max_comp * (size_t)x.n_sets) * 4, (uint32_t)(k * x.n_sets + s) * 16u, v);
  }
}

// the best candidate of object k and (if asked for) its cells: b16 = this lane's 16 cells of the bit row
ARCLE_DEV void ray_emit_best(const RayParams& x, int lane, int row, int k, int set, int color, int correct, int cells, uint32_t b16) {
  if (lane == 0) {
    U4 v;
    v[0] = (uint32_t)set;
    v[1] = (uint32_t)color;
    v[2] = (uint32_t)correct;
    v[3] = (uint32_t)cells;
    xl::store_at(x.best + ((size_t)row * (size_t)x.max_comp) * 4, (uint32_t)k * 16u, v);
  }
  if (x.best_bits) {
    uint8_t* b = x.best_bits + ((size_t)row * (size_t)x.max_comp + (size_t)k) * ARCLE_BITS_STRIDE;
    *reinterpret_cast<uint16_t*>(b + 2 * lane) = (uint16_t)b16;
  }
}

// ROW BOARD: the board moved by s cells along (DX, DY) — the cell (i, j) takes what (i - s DX, j - s DY) held, 0 from beyond the wave
template <int DX, int DY>
ARCLE_DEV uint32_t ray_shift_rows(const Wave& w, uint32_t v, int s) {
  uint32_t u = v;
  if (DX != 0) {
    const int from = w.lane - DX * s;
    u = xl::shfl(v, from & 63);
    if (from < 0 || from > 63) u = 0u;
  }
  if (DY > 0) u <<= (uint32_t)s;
  if (DY < 0) u >>= (uint32_t)s;
  return u;
}

// ROW BOARD: R_d by doubling; n = the extent of grid_dim along the direction (shifts stay below 32: n <= 32 wherever DY != 0)
template <int DX, int DY>
ARCLE_DEV uint32_t ray_fill_rows(const Wave& w, uint32_t B, uint32_t F, int n) {
  uint32_t gen = B, pro = F;
  for (int s = 1; s < n; s <<= 1) {  // (wave-uniform)
    gen |= pro & ray_shift_rows<DX, DY>(w, gen, s);
    if (2 * s < n) pro &= ray_shift_rows<DX, DY>(w, pro, s);
  }
  return gen & F;
}

// FLAT BOARD: R_d by the plain loop; `into` = F AND the columns a step of the direction may arrive in; n = the flat shift of one step
// (DX * W + DY: towards higher cells if positive).  ONE body for all eight directions — the caller loops over them without unrolling:
// eight inlined copies had their shift constants hoisted out of the object loop, more wave-uniform values than there are SGPRs
ARCLE_DEV uint32_t ray_fill_flat(const Wave& w, uint32_t B, uint32_t into, int n, int rounds) {
  uint32_t R = 0u;
  for (int i = 0; i < rounds; i++) {  // (wave-uniform)
    const uint32_t from = B | R;
    uint32_t to = from;
    if (n > 0) to = board_shl(w, from, n);
    else if (n < 0) to = board_shr(w, from, -n);
    to &= into;
    if (!xl::ballot(to != R)) break;  // (R only grows: equal means nothing new)
    R = to;
  }
  return R;
}

// the OR of the rays of the directions in `m`
ARCLE_DEV uint32_t ray_union(const uint32_t (&R)[8], uint32_t m) {
  uint32_t u = 0u;
#pragma unroll
  for (int d = 0; d < 8; d++) u |= ((m >> d) & 1u) ? R[d] : 0u;
  return u;
}

// per-row constants of the evaluation
struct RayBoards {
  uint32_t K0;              // grid == answer inside the common rectangle
  uint32_t A[RAY_COLORS];   // answer == c inside the common rectangle
  uint32_t present;         // bit c: A[c] is not empty anywhere (wave-uniform)
  int base_correct;
};

// all candidates of one object from its eight rays: the ray slots, the best slot and its bit row.  TO16 turns a board into this
// lane's 16 cells of a bit row.
template <typename TO16>
ARCLE_DEV void ray_score(const RayParams& x, const RayBoards& bd, const uint32_t (&R)[8], unsigned long long slo, unsigned long long shi, int lane,
                         int row, int k, TO16 to16f) {
  int bset = -1, bcol = 0, bcor = bd.base_correct, bcells = 0;
  uint32_t bmask = 0u;
  for (int s = 0; s < x.n_sets; s++) {
    const uint32_t m = (uint32_t)((s < 8 ? slo >> (8 * s) : shi >> (8 * (s - 8))) & 0xffull);
    const uint32_t Rs = ray_union(R, m);
    if (!xl::ballot(Rs != 0u)) {  // (wave-uniform)
      ray_emit(x, lane, row, k, s, 0, bd.base_correct, 0, 0);
      continue;
    }
    // three 10-bit counts per word: cells, the correct cells painted over, colour 0 | colours 1-3 | 4-6 | 7-9
    uint32_t cnt[RAY_COLORS];
    const uint32_t t0 = xl::wave_add((uint32_t)__builtin_popcount(Rs) | ((uint32_t)__builtin_popcount(Rs & bd.K0) << 10) |
                                     ((uint32_t)__builtin_popcount(Rs & bd.A[0]) << 20));
    const int cells = (int)(t0 & 1023u), khit = (int)((t0 >> 10) & 1023u);
    cnt[0] = t0 >> 20;
#pragma unroll
    for (int g = 0; g < 3; g++) {
      uint32_t t = 0u;
      if ((bd.present >> (1 + 3 * g)) & 7u)  // (wave-uniform)
        t = xl::wave_add((uint32_t)__builtin_popcount(Rs & bd.A[1 + 3 * g]) | ((uint32_t)__builtin_popcount(Rs & bd.A[2 + 3 * g]) << 10) |
                         ((uint32_t)__builtin_popcount(Rs & bd.A[3 + 3 * g]) << 20));
      cnt[1 + 3 * g] = t & 1023u;
      cnt[2 + 3 * g] = (t >> 10) & 1023u;
      cnt[3 + 3 * g] = t >> 20;
    }
    int color = 0, right = (int)cnt[0];
#pragma unroll
    for (int c = 1; c < RAY_COLORS; c++)
      if ((int)cnt[c] > right) right = (int)cnt[c], color = c;
    const int correct = bd.base_correct - khit + right;
    ray_emit(x, lane, row, k, s, color, correct, cells, right);
    if (bset < 0 || correct > bcor || (correct == bcor && cells < bcells)) bset = s, bcol = color, bcor = correct, bcells = cells, bmask = m;
  }
  ray_emit_best(x, lane, row, k, bset, bcol, bcor, bcells, x.best_bits ? to16f(ray_union(R, bmask)) : 0u);
}

// FLAT = the flat board (W > 32 or H > 64, always with FW_GENERIC): an instantiation of its own, so that no kernel carries both boards'
// per-object loops (together they kept more wave-uniform values alive than there are SGPRs)
template <int FW, bool FLAT>
ARCLE_DEV void wave_ray_row(const RayParams& x, WaveLDS* lds, const U2* lut, int row, int lane) {
  const StepParams& p = x.p;
  Wave w(p, lds, lut, lane, INGRESS_BBOX, FW, false, false, false);
  const int C = x.max_comp, S = x.n_sets;
  int n = C;
  if (x.count) n = imin(imax((int)xl::uniform((uint32_t)x.count[2 * (size_t)row]), 0), C);
  int src = row;
  if (x.src_env) src = (int)xl::uniform((uint32_t)x.src_env[row]);
  if (src < 0 || src >= p.n_resident) {  // no such env to take the answer from
    if (x.base && lane == 0) {
      U2 b;
      b[0] = b[1] = 0u;
      xl::store_at(x.base, (uint32_t)row * 8u, b);
    }
    for (int k = 0; k < n; k++) {
      for (int s = 0; s < S; s++) ray_emit(x, lane, row, k, s, 0, 0, 0, 0);
      ray_emit_best(x, lane, row, k, 0, 0, 0, 0, 0u);
    }
    return;
  }
  // the grid plane and grid_dim, the answer plane and answer_dim: as wave_place_row reads them
  U4 grid = u4_zero(), ans = u4_zero();
  int gh, gw;
  if (p.rows_in) {
    const int8_t* rin = p.rows_in + (size_t)row * p.rows_in_stride;
    const int off = row_offset(p, ARCLE_PL_GRID);
    grid = row_plane(w, rin, off);
    gh = (int)row_byte(rin, off + p.P);
    gw = (int)row_byte(rin, off + p.P + 1);
  } else {
    if (16 * lane < p.PS) grid = xl::load16(p.plane[ARCLE_PL_GRID], (uint32_t)row * (uint32_t)p.PS + 16u * (uint32_t)lane);
    const Rec r = load_rec(p, row);
    gh = r.gh();
    gw = r.gw();
  }
  if (16 * lane < p.PS) ans = xl::load16(p.plane[ARCLE_PL_ANSWER], (uint32_t)src * (uint32_t)p.PS + 16u * (uint32_t)lane);
  const Rec ra = load_rec(p, src);
  gh = imin(gh, p.H);
  gw = imin(gw, p.W);
  const int ah = imin(ra.ah(), p.H), aw = imin(ra.aw(), p.W);
  const int mh = imin(gh, ah), mw = imin(gw, aw);
  const uint32_t inside16 = w.rect16(0, gh - 1, 0, gw - 1), common16 = w.rect16(0, mh - 1, 0, mw - 1);
  const uint32_t K0_16 = (flags16(nzflags(grid[0] ^ ans[0]), nzflags(grid[1] ^ ans[1]), nzflags(grid[2] ^ ans[2]), nzflags(grid[3] ^ ans[3])) ^ 0xffffu) & common16;
  RayBoards bd;
  bd.base_correct = (int)xl::wave_add((uint32_t)__builtin_popcount(K0_16));
  if (x.base && lane == 0) {
    int total = mh * mw;  // (agents/env.py:48-52, as step_core counts it)
    if ((gh <= ah) == (gw <= aw)) total += ah * aw > gh * gw ? ah * aw - gh * gw : gh * gw - ah * aw;
    else total += (gh > ah ? gh - ah : ah - gh) * mw + (gw > aw ? gw - aw : aw - gw) * mh;
    U2 b;
    b[0] = (uint32_t)bd.base_correct;
    b[1] = (uint32_t)total;
    xl::store_at(x.base, (uint32_t)row * 8u, b);
  }
  const uint32_t free16 = x.through ? inside16 : (eq16(grid, (uint32_t)x.free_color) & inside16);
  uint32_t A16[RAY_COLORS], pres = 0u;
#pragma unroll
  for (int c = 0; c < RAY_COLORS; c++) {
    A16[c] = eq16(ans, (uint32_t)c) & common16;
    pres |= A16[c] ? (1u << c) : 0u;
  }
  bd.present = xl::wave_or(pres);
  // the direction sets, eight to a 64-bit scalar, and the directions any of them uses
  unsigned long long slo = 0ull, shi = 0ull;
  uint32_t need = 0u;
  for (int s = 0; s < S; s++) {
    const uint32_t m = xl::uniform((uint32_t)x.sets[s]);
    if (s < 8) slo |= (unsigned long long)m << (8 * s);
    else shi |= (unsigned long long)m << (8 * (s - 8));
    need |= m;
  }
  const uint8_t* brow = x.bits + (size_t)row * (size_t)C * ARCLE_BITS_STRIDE;

  if (!FLAT) {
    // ROW BOARD
    const uint32_t Wb = (uint32_t)p.W;
    const uint32_t FREE = rows_from16(w, free16, Wb);
    bd.K0 = rows_from16(w, K0_16, Wb);
#pragma unroll
    for (int c = 0; c < RAY_COLORS; c++) {
      bd.A[c] = 0u;
      if ((bd.present >> c) & 1u) bd.A[c] = rows_from16(w, A16[c], Wb);
    }
    const int nd = imin(gh, gw);
    for (int k = 0; k < n; k++) {
      const uint32_t b16 = (uint32_t)*reinterpret_cast<const uint16_t*>(brow + (size_t)k * ARCLE_BITS_STRIDE + 2 * lane) & inside16;
      const uint32_t B = rows_from16(w, b16, Wb);
      const uint32_t F = FREE & ~B;
      uint32_t R[8];
#pragma unroll
      for (int d = 0; d < 8; d++) R[d] = 0u;
      if (xl::ballot(B != 0u)) {  // (wave-uniform; an empty object casts nothing)
        if (need & 1u) R[0] = ray_fill_rows<-1, 0>(w, B, F, gh);
        if (need & 2u) R[1] = ray_fill_rows<1, 0>(w, B, F, gh);
        if (need & 4u) R[2] = ray_fill_rows<0, -1>(w, B, F, gw);
        if (need & 8u) R[3] = ray_fill_rows<0, 1>(w, B, F, gw);
        if (need & 16u) R[4] = ray_fill_rows<-1, -1>(w, B, F, nd);
        if (need & 32u) R[5] = ray_fill_rows<-1, 1>(w, B, F, nd);
        if (need & 64u) R[6] = ray_fill_rows<1, -1>(w, B, F, nd);
        if (need & 128u) R[7] = ray_fill_rows<1, 1>(w, B, F, nd);
      }
      ray_score(x, bd, R, slo, shi, lane, row, k, [&](uint32_t v) { return rows_to16(w, v, Wb); });
    }
  } else {
    // FLAT BOARD
    const uint32_t FREE = to32(w, free16);
    bd.K0 = to32(w, K0_16);
#pragma unroll
    for (int c = 0; c < RAY_COLORS; c++) {
      bd.A[c] = 0u;
      if ((bd.present >> c) & 1u) bd.A[c] = to32(w, A16[c]);
    }
    // the columns a step east / west may arrive in: everything else would be a wrap into the next / the previous row
    const uint32_t east = to32(w, w.rect16(0, p.H - 1, 1, p.W - 1)), west = to32(w, w.rect16(0, p.H - 1, 0, p.W - 2));
    const int rounds = imax(gh, gw);
    for (int k = 0; k < n; k++) {
      const uint32_t b16 = (uint32_t)*reinterpret_cast<const uint16_t*>(brow + (size_t)k * ARCLE_BITS_STRIDE + 2 * lane) & inside16;
      const uint32_t B = to32(w, b16);
      const uint32_t F = FREE & ~B;
      uint32_t R[8];
#pragma unroll
      for (int d = 0; d < 8; d++) R[d] = 0u;
      if (xl::ballot(B != 0u)) {  // (wave-uniform)
#pragma unroll 1
        for (int d = 0; d < 8; d++) {  // N, S, W, E, NW, NE, SW, SE
          if (!((need >> d) & 1u)) continue;
          const int dx = d < 4 ? (d == 0 ? -1 : (d == 1 ? 1 : 0)) : (d < 6 ? -1 : 1);
          const int dy = d < 4 ? (d == 2 ? -1 : (d == 3 ? 1 : 0)) : ((d & 1) ? 1 : -1);
          const uint32_t Rd = ray_fill_flat(w, B, dy > 0 ? (F & east) : (dy < 0 ? (F & west) : F), dx * p.W + dy, rounds);
#pragma unroll
          for (int j = 0; j < 8; j++) R[j] = (j == d) ? Rd : R[j];  // (statically indexed: registers)
        }
      }
      ray_score(x, bd, R, slo, shi, lane, row, k, [&](uint32_t v) { return to16(w, v); });
    }
  }
}

}  // namespace arcle
