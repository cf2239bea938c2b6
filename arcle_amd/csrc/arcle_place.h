// arcle_place.h — where each object of a state row best fits the answer (arcle_place_rows): for every object (a bit row, as
// arcle_components_rows / arcle_objects_rows write it) the translation whose Move macro scores the most correct cells, with that count.
//
//   wave_place_row<FW>  one wavefront takes ALL objects of one row: the grid, the answer of env src_env[row] and the boards made of
//                       them are built once per row; per object a handful of AND + popcount per translation, no step body
//
// Compiled like arcle_objects.h: by hipcc through arcle_hip.hip and by g++ through tests/emu/place_emu.cpp; it uses only the xl::
// primitives both define and leaves arcle_wave.h and arcle_components.h as they are (cell_row and the board helpers are used).
//
// After any chain of Moves on a freshly selected object the grid is the background (the grid with the object's cells zeroed) with the
// object's positive cells pasted at the new position (object.py:60-138, 218-243).  With B the object's cells inside grid_dim, F its
// cells whose byte is > 0, K = (background == answer) inside the common rectangle of grid_dim and answer_dim, the child of the
// translation (dx, dy) has
//     correct(dx, dy) = popc(K) - popc(K & shift(F)) + popc(shift(F) & [shifted colour == answer colour] & common rectangle)
// Colours are compared through their BIT PLANES: `used` = the OR of the grid's positive bytes (bits 0-3 for ARC's colours), one board
// per used bit of the grid and of the answer, and AZ = the cells whose answer byte has no bit outside `used`; a shifted cell matches
// where no used plane differs and AZ holds.  The planes are statically indexed (7 unrolled slots under uniform branches): registers.
//
// ROW BOARD (W <= 32 and H <= 64; lane i = row i as a W-bit word): ONE LANE PER TRANSLATION.  The candidate translations of an object
// are the cells of the rectangle [dxmin, dxmax] x [dymin, dymax] (the box stays inside grid_dim, |dx|, |dy| <= max_dist), 64 per pass;
// a lane outside the |dx| + |dy| diamond sits the pass out.  Per row r of the object's box the wave reads F's word and its planes as
// wave-uniform values (readlane), each lane shifts them by ITS dy and fetches the answer rows at r + ITS dx (ds_bpermute): 2 + planes
// cross-lane reads per object row serve 64 translations, and no reduction is needed but the final arg-max of the packed keys
//     correct << 20 | (127 - |dx| - |dy|) << 13 | (63 - dx) << 6 | (31 - dy)
// whose order IS the tie rule (more correct, then nearer, then the smaller dx, then the smaller dy).
// FLAT BOARD (every other shape of at most 1024 cells; lane j < 32 = cells [32j, 32j + 32)): the slower path — a wave-uniform loop
// over the translations, each a flat shift by dx * W + dy of F and its planes (the box stays inside the grid, so no cell changes its
// row by wrapping) and one wave reduction of the count.
#pragma once
#include "arcle_components.h"

namespace arcle {

// launch parameters: p = the handle's base parameters with n_envs = the number of rows, n_resident = the handle's envs and rows_in /
// rows_in_stride = the state rows (rows_in NULL: the resident envs 0 .. n_envs-1)
struct PlaceParams {
  StepParams p;
  int32_t max_comp;        // C: objects per row at most
  int32_t max_dist;        // translations with |dx| + |dy| <= max_dist
  const int32_t* count;    // optional int32 [n_rows][2]: word 0 = the objects of the row (NULL: C)
  const uint8_t* bits;     // uint8 [n_rows][C][ARCLE_BITS_STRIDE], 2-byte aligned
  const int32_t* src_env;  // optional int32 [n_rows]: the env whose answer judges the row (NULL: env = row)
  int32_t* place;          // int32 [n_rows][C][4] = dx, dy, correct(best), correct(0, 0)
  int32_t* base;           // optional int32 [n_rows][2]: the dense pair of the row's own grid
};

// bit b of each of this lane's 16 bytes as a 16-cell mask
ARCLE_DEV uint32_t plane16(const U4& v, int b) {
  return flags16(((v[0] >> b) & 0x01010101u) << 7, ((v[1] >> b) & 0x01010101u) << 7, ((v[2] >> b) & 0x01010101u) << 7, ((v[3] >> b) & 0x01010101u) << 7);
}

ARCLE_DEV void place_emit(const PlaceParams& x, int lane, int row, int k, int dx, int dy, int correct, int stay) {
  if (lane == 0) {
    U4 v;
    v[0] = (uint32_t)dx;
    v[1] = (uint32_t)dy;
    v[2] = (uint32_t)correct;
    v[3] = (uint32_t)stay;
    xl::store_at(x.place + ((size_t)row * (size_t)x.max_comp) * 4, (uint32_t)k * 16u, v);
  }
}

constexpr int PLACE_PLANES = 7;  // bits 0 .. 6 of a positive int8

template <int FW>
ARCLE_DEV void wave_place_row(const PlaceParams& x, WaveLDS* lds, const U2* lut, int row, int lane) {
  const StepParams& p = x.p;
  Wave w(p, lds, lut, lane, INGRESS_BBOX, FW, false, false, false);
  const int C = x.max_comp;
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
    for (int k = 0; k < n; k++) place_emit(x, lane, row, k, 0, 0, 0, 0);
    return;
  }
  // the grid plane and grid_dim, by the lanes that hold bytes of them only (see wave_components_row); the answer plane likewise
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
  const uint32_t Z16 = eq16(ans, 0u) & common16;
  const int base_correct = (int)xl::wave_add((uint32_t)__builtin_popcount(K0_16));
  if (x.base && lane == 0) {
    int total = mh * mw;  // (agents/env.py:48-52, as step_core counts it)
    if ((gh <= ah) == (gw <= aw)) total += ah * aw > gh * gw ? ah * aw - gh * gw : gh * gw - ah * aw;
    else total += (gh > ah ? gh - ah : ah - gh) * mw + (gw > aw ? gw - aw : aw - gw) * mh;
    U2 b;
    b[0] = (uint32_t)base_correct;
    b[1] = (uint32_t)total;
    xl::store_at(x.base, (uint32_t)row * 8u, b);
  }
  // the bits any positive byte of the grid has: the planes a colour comparison needs
  uint32_t ub;
  {
    const U4 pb = posbytes(grid);
    ub = (grid[0] & pb[0]) | (grid[1] & pb[1]) | (grid[2] & pb[2]) | (grid[3] & pb[3]);
    ub |= ub >> 16;
    ub |= ub >> 8;
  }
  const uint32_t used = xl::wave_or(ub & 0x7fu);
  const uint32_t unused4 = (~used & 0xffu) * 0x01010101u;
  const uint32_t AZ16 = (flags16(nzflags(ans[0] & unused4), nzflags(ans[1] & unused4), nzflags(ans[2] & unused4), nzflags(ans[3] & unused4)) ^ 0xffffu) & common16;
  const uint32_t pos16g = pos16(grid) & inside16;
  const int D = x.max_dist;
  const uint8_t* brow = x.bits + (size_t)row * (size_t)C * ARCLE_BITS_STRIDE;

  if (FW != FW_GENERIC || (p.W <= 32 && p.H <= 64)) {
    // ROW BOARD
    const uint32_t Wb = (uint32_t)p.W;
    const uint32_t K0 = rows_from16(w, K0_16, Wb), Z = rows_from16(w, Z16, Wb), AZ = rows_from16(w, AZ16, Wb), GP = rows_from16(w, pos16g, Wb);
    uint32_t Gb[PLACE_PLANES], Ab[PLACE_PLANES];
#pragma unroll
    for (int b = 0; b < PLACE_PLANES; b++) {
      Gb[b] = Ab[b] = 0u;
      if ((used >> b) & 1u) {
        Gb[b] = rows_from16(w, plane16(grid, b), Wb) & GP;
        Ab[b] = rows_from16(w, plane16(ans, b), Wb);
      }
    }
    for (int k = 0; k < n; k++) {
      const uint32_t b16 = (uint32_t)*reinterpret_cast<const uint16_t*>(brow + (size_t)k * ARCLE_BITS_STRIDE + 2 * lane) & inside16;
      const uint32_t B = rows_from16(w, b16, Wb);
      const uint32_t F = B & GP;
      const uint32_t Kobj = (K0 & ~B) | (Z & B);
      // popc(K) and correct(0, 0) = popc(K outside F) + F's cells that are right where they are, in one reduction
      const uint32_t both = xl::wave_add((uint32_t)__builtin_popcount(Kobj) | ((uint32_t)(__builtin_popcount(Kobj & ~F) + __builtin_popcount(F & K0)) << 16));
      const int totalK = (int)(both & 0xffffu), stay = (int)(both >> 16);
      const unsigned long long rowsB = xl::ballot(B != 0u);
      const uint32_t cols = xl::wave_or(B);
      int dx0 = 0, dx1 = 0, dy0 = 0, dy1 = 0, x0 = 0, x1 = -1;
      if (rowsB) {
        x0 = __builtin_ctzll(rowsB);
        x1 = 63 - __builtin_clzll(rowsB);
        const int y0 = __builtin_ctz(cols), y1 = 31 - __builtin_clz(cols);
        dx0 = imax(-x0, -D), dx1 = imin(gh - 1 - x1, D);
        dy0 = imax(-y0, -D), dy1 = imin(gw - 1 - y1, D);
      }
      const int ny = dy1 - dy0 + 1, total = (dx1 - dx0 + 1) * ny;
      const uint32_t magic = 65536u / (uint32_t)ny + 1u;
      int best = 0;
      for (int t0 = 0; t0 < total; t0 += 64) {
        const int t = t0 + lane;
        int i = (int)(((uint32_t)t * magic) >> 16);
        if (i * ny > t) i--;
        const int dx = dx0 + i, dy = dy0 + (t - i * ny);
        const int dist = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
        const bool valid = t < total && dist <= D;
        const uint32_t sl = (uint32_t)imax(dy, 0), sr = (uint32_t)imax(-dy, 0);
        int delta = 0;
        for (int r = x0; r <= x1; r++) {
          const uint32_t f = xl::readlane(F, r);
          if (!f) continue;  // (wave-uniform)
          const int at = (r + dx) & 63;
          const uint32_t fs = (f << sl) >> sr;
          const uint32_t kk = xl::shfl(Kobj, at), az = xl::shfl(AZ, at);
          uint32_t mism = 0;
#pragma unroll
          for (int b = 0; b < PLACE_PLANES; b++) {
            if ((used >> b) & 1u) {
              const uint32_t ob = xl::readlane(Gb[b], r) & f;
              mism |= ((ob << sl) >> sr) ^ xl::shfl(Ab[b], at);
            }
          }
          delta += __builtin_popcount(fs & az & ~mism) - __builtin_popcount(kk & fs);
        }
        const int key = ((totalK + delta) << 20) | ((127 - dist) << 13) | ((63 - dx) << 6) | (31 - dy);
        if (valid) best = imax(best, key);
      }
      xl::lanes_converged();
      best = w.wave_max(best);
      place_emit(x, lane, row, k, 63 - ((best >> 6) & 127), 31 - (best & 63), best >> 20, stay);
    }
  } else {
    // FLAT BOARD
    const uint32_t K0 = to32(w, K0_16), Z = to32(w, Z16), AZ = to32(w, AZ16), GP = to32(w, pos16g);
    uint32_t Gb[PLACE_PLANES], Ab[PLACE_PLANES];
#pragma unroll
    for (int b = 0; b < PLACE_PLANES; b++) {
      Gb[b] = Ab[b] = 0u;
      if ((used >> b) & 1u) {
        Gb[b] = to32(w, plane16(grid, b)) & GP;
        Ab[b] = to32(w, plane16(ans, b));
      }
    }
    const int f0 = (32 * lane) & 1023, fc = f0 - cell_row(p, f0) * p.W;  // this lane's 32 cells start in column fc
    for (int k = 0; k < n; k++) {
      const uint32_t b16 = (uint32_t)*reinterpret_cast<const uint16_t*>(brow + (size_t)k * ARCLE_BITS_STRIDE + 2 * lane) & inside16;
      const uint32_t B = to32(w, b16);
      const uint32_t F = B & GP;
      const uint32_t Kobj = (K0 & ~B) | (Z & B);
      const unsigned long long lanesB = xl::ballot(B != 0u);
      int dx0 = 0, dx1 = 0, dy0 = 0, dy1 = 0;
      // the box from the cell indices, as wave_components_row takes it
      int ymin = 4096, ymax = -1;
      if (B) {
        int kk = 0, c = fc;
        while (kk < 32) {
          const int len = imin(p.W - c, 32 - kk);
          const uint32_t seg = (B >> kk) & (len >= 32 ? 0xffffffffu : (1u << len) - 1u);
          if (seg) {
            ymin = imin(ymin, c + __builtin_ctz(seg));
            ymax = imax(ymax, c + 31 - __builtin_clz(seg));
          }
          kk += len;
          c = 0;
        }
      }
      xl::lanes_converged();
      const int y0 = w.wave_min(ymin), y1 = w.wave_max(ymax);
      if (lanesB) {
        const int lf = __builtin_ctzll(lanesB), ll = 63 - __builtin_clzll(lanesB);
        const int first = 32 * lf + __builtin_ctz(xl::uniform(xl::readlane(B, lf)));
        const int last = 32 * ll + 31 - __builtin_clz(xl::uniform(xl::readlane(B, ll)));
        const int x0 = cell_row(p, first), x1 = cell_row(p, last);
        dx0 = imax(-x0, -D), dx1 = imin(gh - 1 - x1, D);
        dy0 = imax(-y0, -D), dy1 = imin(gw - 1 - y1, D);
      }
      int bc = -1, bd = 0, bdx = 0, bdy = 0, stay = 0;
      for (int dx = dx0; dx <= dx1; dx++) {
        for (int dy = dy0; dy <= dy1; dy++) {
          const int dist = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
          if (dist > D) continue;  // (wave-uniform)
          const int s = dx * p.W + dy;
          uint32_t fs = F, mism = 0;
          if (s > 0) fs = board_shl(w, F, s);
          else if (s < 0) fs = board_shr(w, F, -s);
#pragma unroll
          for (int b = 0; b < PLACE_PLANES; b++) {
            if ((used >> b) & 1u) {
              uint32_t ob = Gb[b] & F;
              if (s > 0) ob = board_shl(w, ob, s);
              else if (s < 0) ob = board_shr(w, ob, -s);
              mism |= ob ^ Ab[b];
            }
          }
          const int c = (int)xl::wave_add((uint32_t)(__builtin_popcount(Kobj & ~fs) + __builtin_popcount(fs & AZ & ~mism)));
          if (s == 0) stay = c;
          if (c > bc || (c == bc && (dist < bd || (dist == bd && (dx < bdx || (dx == bdx && dy < bdy)))))) bc = c, bd = dist, bdx = dx, bdy = dy;
        }
      }
      xl::lanes_converged();
      place_emit(x, lane, row, k, bdx, bdy, bc, stay);
    }
  }
}

}  // namespace arcle
