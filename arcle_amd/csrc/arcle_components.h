// arcle_components.h — the connected components of the grid of every state row (arcle_components_rows): the objects a search
// proposes its actions from.
//
//   wave_components_row  one wavefront labels ALL components of one row's grid: color.py:8-30 (`dfs`) — 4-connected cells of the same
//                        colour inside grid_dim — from every not-yet-covered cell in row-major order
//
// Compiled like arcle_search.h: by hipcc through arcle_hip.hip and by g++ through tests/emu/components_emu.cpp; it uses only the xl::
// primitives both define and leaves arcle_wave.h as it is.  The closure of a seed is the very sequence of passes of op_floodfill
// (arcle_wave.h), restated here rather than factored out of it, so that every kernel built from that header stays the code it was.
//
// Per row: the grid plane (4 VGPRs) and grid_dim are loaded ONCE; `todo` = the cells inside grid_dim whose colour is not skip_color,
// as a bit board; while it is non-empty and fewer than max_comp components are written: seed = its first cell, M = the cells of the
// seed's colour, F = the closure of the seed in M, todo &= ~F, and F's box / seed / colour / size (and, asked for, its bit mask)
// go out.  The seed is the component's first cell in row-major order: every component lies wholly inside or wholly outside `todo`.
// The board is the row board of op_floodfill (lane i = row i as a W-bit word) for W <= 32 and H <= 64, the flat 1024-bit board
// (lane j < 32 = cells [32j, 32j + 32)) otherwise.
#pragma once
#include "arcle_wave.h"

namespace arcle {

// launch parameters: p = the handle's base parameters with n_envs = the number of rows and rows_in / rows_in_stride = the state
// rows (rows_in NULL: the resident envs 0 .. n_envs-1, grid plane + record)
struct CompParams {
  StepParams p;
  int32_t max_comp;    // C: descriptors per row at most
  int32_t skip_color;  // -1: none; else cells of this colour belong to no component
  int32_t* count;      // int32 [n_rows][2] = (written, left)
  int32_t* comp;       // int32 [n_rows][C][8] = x0, y0, x1, y1, sx, sy, colour, cells
  uint8_t* bits;       // optional uint8 [n_rows][C][ARCLE_BITS_STRIDE]: bit f & 7 of byte f >> 3, f = row * W + col
};

// lane 0's 32-byte descriptor as two 16-byte stores, and every lane's 2 bytes of the bit mask
ARCLE_DEV void comp_emit(const CompParams& x, const Wave& w, int row, int n, int x0, int y0, int x1, int y1, int sx, int sy, int col, int cells,
                         uint32_t bits16) {
  if (w.lane == 0) {
    int32_t* d = x.comp + ((size_t)row * (size_t)x.max_comp) * 8;
    U4 a, b;
    a[0] = (uint32_t)x0;
    a[1] = (uint32_t)y0;
    a[2] = (uint32_t)x1;
    a[3] = (uint32_t)y1;
    b[0] = (uint32_t)sx;
    b[1] = (uint32_t)sy;
    b[2] = (uint32_t)col;
    b[3] = (uint32_t)cells;
    xl::store_at(d, (uint32_t)n * 32u, a);
    xl::store_at(d, (uint32_t)n * 32u + 16u, b);
  }
  if (x.bits) {
    uint8_t* b = x.bits + ((size_t)row * (size_t)x.max_comp + (size_t)n) * ARCLE_BITS_STRIDE;
    *reinterpret_cast<uint16_t*>(b + 2 * w.lane) = (uint16_t)bits16;
  }
}

// f / W for a cell index f < 1024: the reciprocal multiply of StepParams::div_magic (65536 / W + 1) overshoots by one where f's
// remainder is close to W (W = 127: cell 1015 = (7, 126) would land in row 8), so the quotient is checked against f.  (arcle_create
// refuses the widths where the multiply alone is inexact, so on a handle of the library the check never fires: it keeps this header
// right for any W the emulator is given.)
ARCLE_DEV int cell_row(const StepParams& p, int f) {
  const int q = (int)(((uint32_t)f * p.div_magic) >> 16);
  return q * p.W > f ? q - 1 : q;
}

template <int FW>
ARCLE_DEV void wave_components_row(const CompParams& x, WaveLDS* lds, const U2* lut, int row, int lane) {
  const StepParams& p = x.p;
  Wave w(p, lds, lut, lane, INGRESS_BBOX, FW, false, false, false);
  // the grid plane and grid_dim, nothing else of the state; bytes are requested by the lanes that hold bytes of the plane / of the
  // row's grid segment only (a 64-lane request of a plane stride below 1024 bytes reads behind the env's plane — for the last env
  // behind the allocation; row_plane never reads past the segment)
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
  gh = imin(gh, p.H);  // (a row from outside may say anything: the boards hold H x W cells)
  gw = imin(gw, p.W);
  const uint32_t inside = w.rect16(0, gh - 1, 0, gw - 1);
  uint32_t todo16 = inside;
  if (x.skip_color >= 0) todo16 &= ~eq16(grid, (uint32_t)x.skip_color & 0xffu);
  const int C = x.max_comp;
  int n = 0, left;
  if (FW != FW_GENERIC || (p.W <= 32 && p.H <= 64)) {
    // ROW BOARD: lane i holds row i as a W-bit word (op_floodfill's, with its closure: vertical steps of 1, 2, 4 and 8 rows through
    // DPP shifts, then the carry-trick horizontal fill of every row, ARCLE_FILL_UNROLL passes per convergence ballot)
    const uint32_t Wb = (uint32_t)p.W;
    uint32_t todo = rows_from16(w, todo16, Wb);
    for (;;) {
      const unsigned long long live = xl::ballot(todo != 0u);
      if (!live || n >= C) break;
      const int sx = __builtin_ctzll(live);
      const int sy = __builtin_ctz(xl::uniform(xl::readlane(todo, sx)));
      const int seed = sx * p.W + sy;
      const uint32_t col = xl::uniform(xl::readlane(u4_byte(grid, seed & 15), seed >> 4));
      const uint32_t M = rows_from16(w, eq16(grid, col) & inside, Wb), rM = xl::bfrev(M);
      const uint32_t P2d = M & xl::lane_prev(M), P2u = M & xl::lane_next(M);
      const uint32_t P4d = P2d & xl::row_prev<2>(P2d), P4u = P2u & xl::row_next<2>(P2u);
      const uint32_t P8d = P4d & xl::row_prev<4>(P4d), P8u = P4u & xl::row_next<4>(P4u);
      uint32_t F = (lane == sx) ? (1u << sy) : 0u;
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
      todo &= ~F;
      // the box: rows from the ballot of the non-empty row words, columns from their OR; the seed's row is the first row
      const unsigned long long rowsF = xl::ballot(F != 0u);
      const uint32_t cols = xl::wave_or(F);
      const int x1 = 63 - __builtin_clzll(rowsF), y0 = __builtin_ctz(cols), y1 = 31 - __builtin_clz(cols);
      const int cells = (int)xl::wave_add((uint32_t)__builtin_popcount(F));
      uint32_t b16 = 0;
      if (x.bits) b16 = rows_to16(w, F, Wb);
      xl::lanes_converged();
      comp_emit(x, w, row, n, sx, y0, x1, y1, sx, sy, (int)(int8_t)col, cells, b16);
      n++;
    }
    left = (int)xl::wave_add((uint32_t)__builtin_popcount(todo));
  } else {
    // FLAT BOARD: lane j < 32 holds cells [32j, 32j + 32); the four shifts of op_floodfill with its first- / last-column masks
    uint32_t todo = to32(w, todo16);
    const uint32_t notfirst = to32(w, w.rect16(0, p.H - 1, 1, p.W - 1));
    const uint32_t notlast = to32(w, w.rect16(0, p.H - 1, 0, p.W - 2));
    // this lane's 32 cells start at (fr, fc)
    const int f0 = (32 * lane) & 1023, fc = f0 - cell_row(p, f0) * p.W;
    for (;;) {
      const unsigned long long live = xl::ballot(todo != 0u);
      if (!live || n >= C) break;
      const int sl = __builtin_ctzll(live);
      const int seed = 32 * sl + __builtin_ctz(xl::uniform(xl::readlane(todo, sl)));
      const int sx = cell_row(p, seed), sy = seed - sx * p.W;
      const uint32_t col = xl::uniform(xl::readlane(u4_byte(grid, seed & 15), seed >> 4));
      const uint32_t Mb = to32(w, eq16(grid, col) & inside);
      uint32_t F = (lane == sl) ? (1u << (seed & 31)) : 0u;
      for (int it = 0; it < ARCLE_MAX_CELLS; it++) {
        const uint32_t grow = (board_shl(w, F, 1) & notfirst) | (board_shr(w, F, 1) & notlast) | board_shl(w, F, p.W) | board_shr(w, F, p.W);
        const uint32_t Fn = F | (grow & Mb);
        const bool changed = w.any(Fn != F);
        F = Fn;
        if (!changed) break;
      }
      todo &= ~F;
      // the box from the cell indices: the last cell's row; the columns per run of this lane's cells inside one grid row
      const unsigned long long lanesF = xl::ballot(F != 0u);
      const int ll = 63 - __builtin_clzll(lanesF);
      const int last = 32 * ll + 31 - __builtin_clz(xl::uniform(xl::readlane(F, ll)));
      const int x1 = cell_row(p, last);
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
      if (x.bits) b16 = to16(w, F);
      xl::lanes_converged();
      comp_emit(x, w, row, n, sx, y0, x1, y1, sx, sy, (int)(int8_t)col, cells, b16);
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
