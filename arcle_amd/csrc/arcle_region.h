// arcle_region.h — the cells AROUND and INSIDE each object of a state row (arcle_region_rows): for every object (a bit row, as
// arcle_components_rows / arcle_objects_rows write it) and every kind of region asked for — its 4- or 8-neighbour halo, the rest of its
// bounding box, the frame round that box, the cells it encloses, the box, the object itself — the colour that ONE Color step on those
// cells should paint to leave the most correct cells, and that count; the best kind of every object with its cells as a ready-made
// bit-row selection.  A sibling of arcle_ray.h, which draws straight lines from an object's cells: its layout (bit boards, one
// wavefront per row, AND + popcount against ten boards of the answer, the outputs and their tie rules) is taken over, and nothing of
// that file or of any other is changed — the closure of op_floodfill is restated here, as arcle_components.h restates it.
//
//   wave_region_row<FW, FLAT>  one wavefront takes ALL objects of one row: the grid, the answer of env src_env[row], the free board and
//                     the ten boards "answer == c" are built once per row; per object the regions of the kinds in use, per candidate
//                     one select and at most six packed wave sums, no step body
//
// Compiled like arcle_ray.h: by hipcc through arcle_hip.hip and by g++ through tests/emu/region_emu.cpp (plain C++ and xl:: only).
//
// With IN the cells inside grid_dim, B the object's cells inside grid_dim, FREE the cells of IN whose byte is free_color (through = 1:
// IN) and box the bounding rectangle of B (computed from B), the region of kind
//     1 HALO4     = the cells of IN & ~B with a 4-neighbour in B          5 INSIDE = the cells of IN & ~B that no 4-connected path
//     2 HALO8     = the same with 8-neighbours                                      through IN & ~B joins to a cell on the edge of grid_dim
//     3 BOX_REST  = box & ~B                                               6 BOX    = box
//     4 BOX_FRAME = (box grown by one cell on every side) & ~box & IN      7 SELF   = B
// and 0 (or a code above 7: `kinds` lives on the device, the host entry point cannot see it) is the empty region.  An empty B has no
// box: all its regions are empty.  The cells scored are R = region & (B | FREE): the free filter spares B's own cells.  Color c on the
// selection R (color.py:70-77) sets exactly those cells to c, so with K0 = (grid == answer) and A_c = (answer == c), both inside the
// common rectangle of grid_dim and answer_dim,
//     correct(s, c) = popc(K0) - popc(R & K0) + popc(R & A_c)
// and the colour reported is the c in 0..9 with the most popc(R & A_c), the smaller c on a tie.
//
// ROW BOARD (W <= 32 and H <= 64; lane i = row i as a W-bit word).  The halos are the word of the lane above and below (xl::lane_prev /
// lane_next, 0 beyond lanes 0 / 63) and the word shifted by one bit either way, ANDed with IN: IN is zero in rows >= gh and bits >= gw,
// so nothing leaks out of grid_dim and nothing wraps.  The box is the ballot of the non-empty row words (rows) and their wave OR
// (columns).  INSIDE is the closure of components' row board — vertical steps of 1, 2, 4 and 8 rows, then the carry-trick fill of every
// row — in M = IN & ~B, started from ALL cells of M on the edge of grid_dim at once; what it does not reach is the answer.  It runs
// ARCLE_FILL_UNROLL (2) passes per convergence ballot like its two models: by an ESTIMATE from the source — a pass is about 45
// instructions, the compare + ballot + branch about 4, and a flood from the whole edge ends after very few passes on most boards, so one
// idle pass more or less decides little either way — the form was kept as it is where it was timed (arcle_wave.h); no other count of
// passes was built or timed here.
// FLAT BOARD (every other shape of at most 1024 cells; lane j < 32 = cells [32j, 32j + 32)) — the slower path, as in the siblings.  The
// halos are flat shifts by W (vertical: they cannot wrap) and by 1 ANDed with the board of the columns such a step may arrive in (all
// but column 0 going up, all but column W - 1 going down); the diagonals are the horizontal step taken from the vertical one, so they
// pass both masks.  The box comes from the cell indices as components' flat path derives it, INSIDE is that path's plain loop to a
// wave-uniform "nothing new".  An instantiation of its own, for the reason arcle_ray.h gives (SGPRs).
//
// THE COUNTS of one candidate — cells, popc(R & K0) and the ten popc(R & A_c) — can reach 1024 here (BOX or SELF of a whole-grid object
// at 32 x 32), which ray's three 10-bit fields to a word cannot hold: TWO counts share a word, 16 bits each, and a candidate costs at
// most SIX wave sums; a word whose two colours the answer does not hold at all (a wave-uniform mask, built once per row) is skipped.
#pragma once
#include "arcle_place.h"

namespace arcle {

// launch parameters: p = the handle's base parameters with n_envs = the number of rows, n_resident = the handle's envs and rows_in /
// rows_in_stride = the state rows (rows_in NULL: the resident envs 0 .. n_envs-1)
struct RegionParams {
  StepParams p;
  int32_t max_comp;        // C: objects per row at most
  int32_t n_kinds;         // S: candidates per object, 1 .. REGION_MAX_KINDS
  const int32_t* count;    // optional int32 [n_rows][2]: word 0 = the objects of the row (NULL: C)
  const uint8_t* bits;     // uint8 [n_rows][C][ARCLE_BITS_STRIDE], 2-byte aligned
  const int32_t* src_env;  // optional int32 [n_rows]: the env whose answer judges the row (NULL: env = row)
  const uint8_t* kinds;    // uint8 [S]: the region codes (ARCLE_REGION_*; above 7: the empty region), read by every wave
  int32_t* region;         // int32 [n_rows][C][S][4] = color, correct, cells, right
  int32_t* best;           // int32 [n_rows][C][4] = index, color, correct, cells
  uint8_t* best_bits;      // optional uint8 [n_rows][C][ARCLE_BITS_STRIDE], 2-byte aligned: the best candidate's cells as a bit row
  int32_t* base;           // optional int32 [n_rows][2]: the dense pair of the row's own grid
  int32_t free_color;      // through = 0: the free filter keeps the cells outside the object whose byte equals this (as int8)
  int32_t through;         // 1: no free filter
};

constexpr int REGION_MAX_KINDS = 16;
constexpr int REGION_CODES = 8;    // 0 none, 1 HALO4, 2 HALO8, 3 BOX_REST, 4 BOX_FRAME, 5 INSIDE, 6 BOX, 7 SELF
constexpr int REGION_COLORS = 10;  // Color 0 .. 9

ARCLE_DEV void region_emit(const RegionParams& x, int lane, int row, int k, int s, int color, int correct, int cells, int right) {
  if (lane == 0) {
    U4 v;
    v[0] = (uint32_t)color;
    v[1] = (uint32_t)correct;
    v[2] = (uint32_t)cells;
    v[3] = (uint32_t)right;
    xl::store_at(x.region + ((size_t)row * (size_t)x.max_comp * (size_t)x.n_kinds) * 4, (uint32_t)(k * x.n_kinds + s) * 16u, v);
  }
}

// the best candidate of object k and (if asked for) its cells: b16 = this lane's 16 cells of the bit row
ARCLE_DEV void region_emit_best(const RegionParams& x, int lane, int row, int k, int idx, int color, int correct, int cells, uint32_t b16) {
  if (lane == 0) {
    U4 v;
    v[0] = (uint32_t)idx;
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

// the region of code `c` among the boards of one object (statically indexed: registers)
ARCLE_DEV uint32_t region_pick(const uint32_t (&R)[REGION_CODES], uint32_t c) {
  uint32_t u = 0u;
#pragma unroll
  for (int d = 1; d < REGION_CODES; d++) u |= (c == (uint32_t)d) ? R[d] : 0u;
  return u;
}

// per-row constants of the evaluation
struct RegionBoards {
  uint32_t K0;                 // grid == answer inside the common rectangle
  uint32_t A[REGION_COLORS];   // answer == c inside the common rectangle
  uint32_t present;            // bit c: A[c] is not empty anywhere (wave-uniform)
  int base_correct;
};

// all candidates of one object from its regions (already ANDed with B | FREE): the region slots, the best slot and its bit row.  `codes`
// holds the S codes, four bits each (above 7 already folded to 0).  TO16 turns a board into this lane's 16 cells of a bit row.
template <typename TO16>
ARCLE_DEV void region_score(const RegionParams& x, const RegionBoards& bd, const uint32_t (&R)[REGION_CODES], unsigned long long codes, int lane,
                            int row, int k, TO16 to16f) {
  int bidx = -1, bcol = 0, bcor = bd.base_correct, bcells = 0;
  uint32_t bcode = 0u;
  for (int s = 0; s < x.n_kinds; s++) {
    const uint32_t c = (uint32_t)((codes >> (4 * s)) & 0xfull);
    const uint32_t Rs = region_pick(R, c);
    if (!xl::ballot(Rs != 0u)) {  // (wave-uniform)
      region_emit(x, lane, row, k, s, 0, bd.base_correct, 0, 0);
      continue;
    }
    // two 16-bit counts per word (each at most 1024): cells | the correct cells painted over, then the colours in pairs
    uint32_t cnt[REGION_COLORS];
    const uint32_t t0 = xl::wave_add((uint32_t)__builtin_popcount(Rs) | ((uint32_t)__builtin_popcount(Rs & bd.K0) << 16));
    const int cells = (int)(t0 & 0xffffu), khit = (int)(t0 >> 16);
#pragma unroll
    for (int g = 0; g < REGION_COLORS / 2; g++) {
      uint32_t t = 0u;
      if ((bd.present >> (2 * g)) & 3u)  // (wave-uniform)
        t = xl::wave_add((uint32_t)__builtin_popcount(Rs & bd.A[2 * g]) | ((uint32_t)__builtin_popcount(Rs & bd.A[2 * g + 1]) << 16));
      cnt[2 * g] = t & 0xffffu;
      cnt[2 * g + 1] = t >> 16;
    }
    int color = 0, right = (int)cnt[0];
#pragma unroll
    for (int cc = 1; cc < REGION_COLORS; cc++)
      if ((int)cnt[cc] > right) right = (int)cnt[cc], color = cc;
    const int correct = bd.base_correct - khit + right;
    region_emit(x, lane, row, k, s, color, correct, cells, right);
    if (bidx < 0 || correct > bcor || (correct == bcor && cells < bcells)) bidx = s, bcol = color, bcor = correct, bcells = cells, bcode = c;
  }
  region_emit_best(x, lane, row, k, bidx, bcol, bcor, bcells, x.best_bits ? to16f(region_pick(R, bcode)) : 0u);
}

// ROW BOARD: the cells of M = IN & ~B that the edge of grid_dim reaches by 4-connected steps through M — the closure of
// wave_components_row's row board (arcle_components.h), restated with a seed of many cells
ARCLE_DEV uint32_t region_outside_rows(const Wave& w, uint32_t M, uint32_t edge) {
  const uint32_t rM = xl::bfrev(M);
  const uint32_t P2d = M & xl::lane_prev(M), P2u = M & xl::lane_next(M);
  const uint32_t P4d = P2d & xl::row_prev<2>(P2d), P4u = P2u & xl::row_next<2>(P2u);
  const uint32_t P8d = P4d & xl::row_prev<4>(P4d), P8u = P4u & xl::row_next<4>(P4u);
  uint32_t F = M & edge;
  for (int it = 0; it < 2 * ARCLE_MAX_CELLS; it++) {
    const uint32_t F0 = F;
#pragma unroll
    for (int u = 0; u < ARCLE_FILL_UNROLL; u++) {
      F |= (xl::lane_prev(F) | xl::lane_next(F)) & M;
      F |= (xl::row_prev<2>(F) & P2d) | (xl::row_next<2>(F) & P2u);
      F |= (xl::row_prev<4>(F) & P4d) | (xl::row_next<4>(F) & P4u);
      F |= (xl::row_prev<8>(F) & P8d) | (xl::row_next<8>(F) & P8u);
      F |= (xl::lane_prev(F) | xl::lane_next(F)) & M;
      const uint32_t rF = xl::bfrev(F);
      F |= ((M ^ (M + F)) & M) | xl::bfrev((rM ^ (rM + rF)) & rM);
    }
    if (!w.any(F != F0)) break;
  }
  return F;
}

// FLAT BOARD: the same by the plain loop of components' flat path
ARCLE_DEV uint32_t region_outside_flat(const Wave& w, uint32_t M, uint32_t edge, uint32_t notfirst, uint32_t notlast) {
  uint32_t F = M & edge;
  for (int it = 0; it < ARCLE_MAX_CELLS; it++) {
    const uint32_t grow = (board_shl(w, F, 1) & notfirst) | (board_shr(w, F, 1) & notlast) | board_shl(w, F, w.p.W) | board_shr(w, F, w.p.W);
    const uint32_t Fn = F | (grow & M);
    const bool changed = w.any(Fn != F);
    F = Fn;
    if (!changed) break;
  }
  return F;
}

// bits lo .. hi of a word, 0 <= lo, hi <= 31 (empty if lo > hi)
ARCLE_DEV uint32_t region_cols(int lo, int hi) { return lo > hi ? 0u : ((0xffffffffu >> (31 - hi)) & (0xffffffffu << lo)); }

// FLAT = the flat board (W > 32 or H > 64, always with FW_GENERIC): an instantiation of its own, so that no kernel carries both boards'
// per-object loops
template <int FW, bool FLAT>
ARCLE_DEV void wave_region_row(const RegionParams& x, WaveLDS* lds, const U2* lut, int row, int lane) {
  const StepParams& p = x.p;
  Wave w(p, lds, lut, lane, INGRESS_BBOX, FW, false, false, false);
  const int C = x.max_comp, S = x.n_kinds;
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
      for (int s = 0; s < S; s++) region_emit(x, lane, row, k, s, 0, 0, 0, 0);
      region_emit_best(x, lane, row, k, 0, 0, 0, 0, 0u);
    }
    return;
  }
  // the grid plane and grid_dim, the answer plane and answer_dim: as wave_ray_row reads them
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
  RegionBoards bd;
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
  uint32_t A16[REGION_COLORS], pres = 0u;
#pragma unroll
  for (int c = 0; c < REGION_COLORS; c++) {
    A16[c] = eq16(ans, (uint32_t)c) & common16;
    pres |= A16[c] ? (1u << c) : 0u;
  }
  bd.present = xl::wave_or(pres);
  // the codes, four bits each in one 64-bit scalar (a code above 7 is the empty region), and the codes any candidate uses
  unsigned long long codes = 0ull;
  uint32_t need = 0u;
  for (int s = 0; s < S; s++) {
    uint32_t c = xl::uniform((uint32_t)x.kinds[s]);
    if (c >= (uint32_t)REGION_CODES) c = 0u;
    codes |= (unsigned long long)c << (4 * s);
    need |= 1u << c;
  }
  const bool need_box = (need & ((1u << 3) | (1u << 4) | (1u << 6))) != 0u;
  const uint8_t* brow = x.bits + (size_t)row * (size_t)C * ARCLE_BITS_STRIDE;

  if (!FLAT) {
    // ROW BOARD
    const uint32_t Wb = (uint32_t)p.W;
    const uint32_t IN = rows_from16(w, inside16, Wb), FREE = rows_from16(w, free16, Wb);
    bd.K0 = rows_from16(w, K0_16, Wb);
#pragma unroll
    for (int c = 0; c < REGION_COLORS; c++) {
      bd.A[c] = 0u;
      if ((bd.present >> c) & 1u) bd.A[c] = rows_from16(w, A16[c], Wb);
    }
    // the cells on the edge of grid_dim: rows 0 and gh - 1 in full, columns 0 and gw - 1 of the others (ANDed with M = IN & ~B below)
    const uint32_t edge = (lane == 0 || lane == gh - 1) ? 0xffffffffu : (1u | (gw > 0 ? 1u << (gw - 1) : 0u));
    for (int k = 0; k < n; k++) {
      const uint32_t b16 = (uint32_t)*reinterpret_cast<const uint16_t*>(brow + (size_t)k * ARCLE_BITS_STRIDE + 2 * lane) & inside16;
      const uint32_t B = rows_from16(w, b16, Wb);
      const uint32_t keep = B | FREE;
      uint32_t R[REGION_CODES];
#pragma unroll
      for (int d = 0; d < REGION_CODES; d++) R[d] = 0u;
      const unsigned long long rowsB = xl::ballot(B != 0u);
      if (rowsB) {  // (wave-uniform; an empty object has no box and nothing around or inside it)
        const uint32_t up = xl::lane_prev(B), dn = xl::lane_next(B);
        if (need & (1u << 1)) R[1] = ((B << 1) | (B >> 1) | up | dn) & IN & ~B & keep;
        if (need & (1u << 2)) {
          const uint32_t V = B | up | dn;
          R[2] = (V | (V << 1) | (V >> 1)) & IN & ~B & keep;
        }
        if (need_box) {
          const uint32_t cols = xl::wave_or(B);
          const int x0 = __builtin_ctzll(rowsB), x1 = 63 - __builtin_clzll(rowsB), y0 = __builtin_ctz(cols), y1 = 31 - __builtin_clz(cols);
          const uint32_t box = (lane >= x0 && lane <= x1) ? region_cols(y0, y1) : 0u;
          R[3] = box & ~B & keep;
          R[6] = box & keep;
          if (need & (1u << 4)) {
            const uint32_t outer = (lane >= x0 - 1 && lane <= x1 + 1) ? region_cols(imax(y0 - 1, 0), imin(y1 + 1, 31)) : 0u;
            R[4] = outer & ~box & IN & keep;
          }
        }
        if (need & (1u << 5)) {
          const uint32_t M = IN & ~B;
          R[5] = M & ~region_outside_rows(w, M, edge) & keep;
        }
        R[7] = B;
      }
      region_score(x, bd, R, codes, lane, row, k, [&](uint32_t v) { return rows_to16(w, v, Wb); });
    }
  } else {
    // FLAT BOARD
    const uint32_t IN = to32(w, inside16), FREE = to32(w, free16);
    bd.K0 = to32(w, K0_16);
#pragma unroll
    for (int c = 0; c < REGION_COLORS; c++) {
      bd.A[c] = 0u;
      if ((bd.present >> c) & 1u) bd.A[c] = to32(w, A16[c]);
    }
    // the columns a step towards higher / lower cells may arrive in: everything else would be a wrap into the next / the previous row
    const uint32_t notfirst = to32(w, w.rect16(0, p.H - 1, 1, p.W - 1)), notlast = to32(w, w.rect16(0, p.H - 1, 0, p.W - 2));
    const uint32_t edge = to32(w, inside16 & ~w.rect16(1, gh - 2, 1, gw - 2));
    // this lane's 32 cells start at column fc
    const int f0 = (32 * lane) & 1023, fc = f0 - cell_row(p, f0) * p.W;
    for (int k = 0; k < n; k++) {
      const uint32_t b16 = (uint32_t)*reinterpret_cast<const uint16_t*>(brow + (size_t)k * ARCLE_BITS_STRIDE + 2 * lane) & inside16;
      const uint32_t B = to32(w, b16);
      const uint32_t keep = B | FREE;
      uint32_t R[REGION_CODES];
#pragma unroll
      for (int d = 0; d < REGION_CODES; d++) R[d] = 0u;
      const unsigned long long lanesB = xl::ballot(B != 0u);
      if (lanesB) {  // (wave-uniform)
        if (need & ((1u << 1) | (1u << 2))) {
          const uint32_t V = B | board_shl(w, B, p.W) | board_shr(w, B, p.W);
          R[1] = (V | (board_shl(w, B, 1) & notfirst) | (board_shr(w, B, 1) & notlast)) & IN & ~B & keep;
          if (need & (1u << 2)) R[2] = (V | (board_shl(w, V, 1) & notfirst) | (board_shr(w, V, 1) & notlast)) & IN & ~B & keep;
        }
        if (need_box) {
          // the box from the cell indices: the first and the last cell's row; the columns per run of this lane's cells inside one grid row
          const int fl = __builtin_ctzll(lanesB), ll = 63 - __builtin_clzll(lanesB);
          const int first = 32 * fl + __builtin_ctz(xl::uniform(xl::readlane(B, fl)));
          const int last = 32 * ll + 31 - __builtin_clz(xl::uniform(xl::readlane(B, ll)));
          const int x0 = cell_row(p, first), x1 = cell_row(p, last);
          int ymin = 4096, ymax = -1;
          if (B) {
            int i = 0, c = fc;
            while (i < 32) {
              const int len = imin(p.W - c, 32 - i);
              const uint32_t seg = (B >> i) & (len >= 32 ? 0xffffffffu : (1u << len) - 1u);
              if (seg) {
                ymin = imin(ymin, c + __builtin_ctz(seg));
                ymax = imax(ymax, c + 31 - __builtin_clz(seg));
              }
              i += len;
              c = 0;
            }
          }
          xl::lanes_converged();
          const int y0 = w.wave_min(ymin), y1 = w.wave_max(ymax);
          const uint32_t box = to32(w, w.rect16(x0, x1, y0, y1));
          R[3] = box & ~B & keep;
          R[6] = box & keep;
          if (need & (1u << 4))
            R[4] = to32(w, w.rect16(imax(x0 - 1, 0), imin(x1 + 1, p.H - 1), imax(y0 - 1, 0), imin(y1 + 1, p.W - 1))) & ~box & IN & keep;
        }
        if (need & (1u << 5)) {
          const uint32_t M = IN & ~B;
          R[5] = M & ~region_outside_flat(w, M, edge, notfirst, notlast) & keep;
        }
        R[7] = B;
      }
      region_score(x, bd, R, codes, lane, row, k, [&](uint32_t v) { return to16(w, v); });
    }
  }
}

}  // namespace arcle
