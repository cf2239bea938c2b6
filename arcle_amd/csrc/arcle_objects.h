// arcle_objects.h — the objects of the grid of every state row under four notions of "object" (arcle_objects_rows): same-colour or
// multi-colour, 4- or 8-connected.
//
//   wave_objects_row<FW, MODE>  one wavefront labels ALL objects of one row's grid, as wave_components_row (arcle_components.h) does
//                               for the one notion of color.py:8-30; MODE = ARCLE_OBJ_ANY_COLOR | ARCLE_OBJ_DIAG at compile time
//
// Compiled like arcle_components.h: by hipcc through arcle_hip.hip and by g++ through tests/emu/objects_emu.cpp; it uses only the xl::
// primitives both define and leaves arcle_wave.h and arcle_components.h as they are (CompParams, comp_emit and cell_row are used, not
// changed; the closure of wave_components_row is restated with the mode's extra steps, so that kernel stays the code it was).
//
// What the modes change, and nothing else does:
//   ANY_COLOR  the membership board M is the same for every object of the row — inside grid_dim and not skip_color, i.e. the initial
//              `todo` — so it and the straight-column jump masks are computed once per row, not once per object
//   DIAG       row board: every pass's single vertical step becomes the three steps into a neighbour row (its word, and its word
//              shifted left and right by one, under M); the straight-column jumps of 2, 4 and 8 rows stay (a straight column is an
//              8-connected path too) and so does the horizontal carry-fill.  Flat board: the shifts by W - 1 and W + 1 in both
//              directions join the four of the 4-connected step; a shift that changes the column by +1 cannot arrive in column 0 and
//              one that changes it by -1 cannot arrive in column W - 1, which is what keeps a diagonal from wrapping from the last
//              column of one row into the first column of the row two rows on.
// `colors` (optional): bit v & 31 for the byte v of every cell of the object — one bit without ANY_COLOR.
#pragma once
#include "arcle_components.h"

namespace arcle {

struct ObjParams {
  CompParams c;      // the rows and the outputs of arcle_components_rows, unchanged
  uint32_t* colors;  // optional uint32 [n_rows][C]: bit (cell byte & 31) for every cell of the object
};

// the colours under the 16-cell window mask m16 of this lane, OR-ed over the wave
ARCLE_DEV uint32_t obj_colors(const U4& grid, uint32_t m16) {
  uint32_t cm = 0;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const uint32_t v = (grid[k >> 2] >> (8 * (k & 3))) & 31u;
    cm |= ((m16 >> k) & 1u) << v;
  }
  return xl::wave_or(cm);
}

ARCLE_DEV void obj_emit_colors(const ObjParams& x, const Wave& w, int row, int n, uint32_t cm) {
  if (w.lane == 0) xl::store_at(x.colors + (size_t)row * (size_t)x.c.max_comp, (uint32_t)n * 4u, cm);
}

template <int FW, int MODE>
ARCLE_DEV void wave_objects_row(const ObjParams& xo, WaveLDS* lds, const U2* lut, int row, int lane) {
  constexpr bool ANY = (MODE & (int)ARCLE_OBJ_ANY_COLOR) != 0, DIAG = (MODE & (int)ARCLE_OBJ_DIAG) != 0;
  const CompParams& x = xo.c;
  const StepParams& p = x.p;
  Wave w(p, lds, lut, lane, INGRESS_BBOX, FW, false, false, false);
  // the grid plane and grid_dim, by the lanes that hold bytes of them only (see wave_components_row)
  U4 grid = u4_zero();
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
  gh = imin(gh, p.H);
  gw = imin(gw, p.W);
  const uint32_t inside = w.rect16(0, gh - 1, 0, gw - 1);
  uint32_t todo16 = inside;
  if (x.skip_color >= 0) todo16 &= ~eq16(grid, (uint32_t)x.skip_color & 0xffu);
  const int C = x.max_comp;
  const bool want16 = x.bits || (ANY && xo.colors);  // the object as 16-cell windows: for the bit row, and to pick its colours
  int n = 0, left;
  if (FW != FW_GENERIC || (p.W <= 32 && p.H <= 64)) {
    // ROW BOARD: lane i holds row i as a W-bit word
    const uint32_t Wb = (uint32_t)p.W;
    uint32_t todo = rows_from16(w, todo16, Wb);
    uint32_t M = todo, rM = xl::bfrev(M);  // ANY: the one membership board of the row
    uint32_t P2d = M & xl::lane_prev(M), P2u = M & xl::lane_next(M);
    uint32_t P4d = P2d & xl::row_prev<2>(P2d), P4u = P2u & xl::row_next<2>(P2u);
    uint32_t P8d = P4d & xl::row_prev<4>(P4d), P8u = P4u & xl::row_next<4>(P4u);
    for (;;) {
      const unsigned long long live = xl::ballot(todo != 0u);
      if (!live || n >= C) break;
      const int sx = __builtin_ctzll(live);
      const int sy = __builtin_ctz(xl::uniform(xl::readlane(todo, sx)));
      const int seed = sx * p.W + sy;
      const uint32_t col = xl::uniform(xl::readlane(u4_byte(grid, seed & 15), seed >> 4));
      if (!ANY) {
        M = rows_from16(w, eq16(grid, col) & inside, Wb);
        rM = xl::bfrev(M);
        P2d = M & xl::lane_prev(M), P2u = M & xl::lane_next(M);
        P4d = P2d & xl::row_prev<2>(P2d), P4u = P2u & xl::row_next<2>(P2u);
        P8d = P4d & xl::row_prev<4>(P4d), P8u = P4u & xl::row_next<4>(P4u);
      }
      uint32_t F = (lane == sx) ? (1u << sy) : 0u;
      for (int it = 0; it < 2 * ARCLE_MAX_CELLS; it++) {
        const uint32_t F0 = F;
#pragma unroll
        for (int u = 0; u < ARCLE_FILL_UNROLL; u++) {
          // one row up and down: straight, and with DIAG one column to either side (bits shifted past column W - 1 are outside M)
          uint32_t V = xl::lane_prev(F) | xl::lane_next(F);
          if (DIAG) V |= (V << 1) | (V >> 1);
          F |= V & M;
          F |= (xl::row_prev<2>(F) & P2d) | (xl::row_next<2>(F) & P2u);
          F |= (xl::row_prev<4>(F) & P4d) | (xl::row_next<4>(F) & P4u);
          F |= (xl::row_prev<8>(F) & P8d) | (xl::row_next<8>(F) & P8u);
          V = xl::lane_prev(F) | xl::lane_next(F);
          if (DIAG) V |= (V << 1) | (V >> 1);
          F |= V & M;
          const uint32_t rF = xl::bfrev(F);
          F |= ((M ^ (M + F)) & M) | xl::bfrev((rM ^ (rM + rF)) & rM);
        }
        if (!w.any(F != F0)) break;
      }
      todo &= ~F;
      const unsigned long long rowsF = xl::ballot(F != 0u);
      const uint32_t cols = xl::wave_or(F);
      const int x1 = 63 - __builtin_clzll(rowsF), y0 = __builtin_ctz(cols), y1 = 31 - __builtin_clz(cols);
      const int cells = (int)xl::wave_add((uint32_t)__builtin_popcount(F));
      uint32_t b16 = 0;
      if (want16) b16 = rows_to16(w, F, Wb);
      xl::lanes_converged();
      comp_emit(x, w, row, n, sx, y0, x1, y1, sx, sy, (int)(int8_t)col, cells, b16);
      if (xo.colors) {
        const uint32_t cm = ANY ? obj_colors(grid, b16) : 1u << (col & 31u);
        xl::lanes_converged();
        obj_emit_colors(xo, w, row, n, cm);
      }
      n++;
    }
    left = (int)xl::wave_add((uint32_t)__builtin_popcount(todo));
  } else {
    // FLAT BOARD: lane j < 32 holds cells [32j, 32j + 32)
    uint32_t todo = to32(w, todo16);
    const uint32_t notfirst = to32(w, w.rect16(0, p.H - 1, 1, p.W - 1));
    const uint32_t notlast = to32(w, w.rect16(0, p.H - 1, 0, p.W - 2));
    const int f0 = (32 * lane) & 1023, fc = f0 - cell_row(p, f0) * p.W;
    uint32_t Mb = todo;  // ANY: the one membership board of the row
    for (;;) {
      const unsigned long long live = xl::ballot(todo != 0u);
      if (!live || n >= C) break;
      const int sl = __builtin_ctzll(live);
      const int seed = 32 * sl + __builtin_ctz(xl::uniform(xl::readlane(todo, sl)));
      const int sx = cell_row(p, seed), sy = seed - sx * p.W;
      const uint32_t col = xl::uniform(xl::readlane(u4_byte(grid, seed & 15), seed >> 4));
      if (!ANY) Mb = to32(w, eq16(grid, col) & inside);
      uint32_t F = (lane == sl) ? (1u << (seed & 31)) : 0u;
      for (int it = 0; it < ARCLE_MAX_CELLS; it++) {
        uint32_t grow = (board_shl(w, F, 1) & notfirst) | (board_shr(w, F, 1) & notlast) | board_shl(w, F, p.W) | board_shr(w, F, p.W);
        if (DIAG) {
          // (r + 1, c + 1) and (r - 1, c + 1) arrive in a column > 0, (r + 1, c - 1) and (r - 1, c - 1) in a column < W - 1
          grow |= ((board_shl(w, F, p.W + 1) | board_shr(w, F, p.W - 1)) & notfirst) |
                  ((board_shl(w, F, p.W - 1) | board_shr(w, F, p.W + 1)) & notlast);
        }
        const uint32_t Fn = F | (grow & Mb);
        const bool changed = w.any(Fn != F);
        F = Fn;
        if (!changed) break;
      }
      todo &= ~F;
      const unsigned long long lanesF = xl::ballot(F != 0u);
      const int ll = 63 - __builtin_clzll(lanesF);
      const int last = 32 * ll + 31 - __builtin_clz(xl::uniform(xl::readlane(F, ll)));
      int x1 = cell_row(p, last);
      int ymin = 4096, ymax = -1;
      if (F) {
        int k = 0, c = fc;
        while (k < 32) {
          const int len = imin(p.W - c, 32 - k);
          const uint32_t seg = (F >> k) & (len >= 32 ? 0xffffffffu : (1u << len) - 1u);
          if (seg) {
            ymin = imin(ymin, c + __builtin_ctz(seg));
            ymax = imax(ymax, c + 31 - __builtin_clz(seg));
          }
          k += len;
          c = 0;
        }
      }
      xl::lanes_converged();
      const int y0 = w.wave_min(ymin), y1 = w.wave_max(ymax);
      const int cells = (int)xl::wave_add((uint32_t)__builtin_popcount(F));
      uint32_t b16 = 0;
      if (want16) b16 = to16(w, F);
      xl::lanes_converged();
      comp_emit(x, w, row, n, sx, y0, x1, y1, sx, sy, (int)(int8_t)col, cells, b16);
      if (xo.colors) {
        const uint32_t cm = ANY ? obj_colors(grid, b16) : 1u << (col & 31u);
        xl::lanes_converged();
        obj_emit_colors(xo, w, row, n, cm);
      }
      n++;
    }
    left = (int)xl::wave_add((uint32_t)__builtin_popcount(todo));
  }
  xl::lanes_converged();
  if (lane == 0) {
    U2 c;
    c[0] = (uint32_t)n;
    c[1] = (uint32_t)left;
    xl::store_at(x.count, (uint32_t)row * 8u, c);
  }
}

}  // namespace arcle
