// arcle_stamp.h — where a COPY of each object of a state row best fits the answer (arcle_stamp_rows): for every object (a bit row, as
// arcle_components_rows / arcle_objects_rows write it) the cell (px, py) at which CopyO + Paste — copy the object, paste the clip with
// its top-left corner there — leaves the most correct cells, with that count.  The sibling of arcle_place.h, whose layout it takes over
// (bit boards, colours through bit planes, one lane per candidate, AND + popcount) and whose helpers (plane16) it uses; nothing of
// arcle_place.h is changed.
//
//   wave_stamp_row<FW>  one wavefront takes ALL objects of one row: the grid, the answer of env src_env[row] and the boards made of
//                       them are built once per row; per object a handful of AND + popcount per paste position, no step body
//
// Compiled like arcle_place.h: by hipcc through arcle_hip.hip and by g++ through tests/emu/stamp_emu.cpp.
//
// CopyO clips the object's box out of the grid, the box's cells outside the object as 0 (object.py:291-312); Paste writes the clip at
// the selected cell, cut at the PLANE's H x W (object.py:340-341) — the whole h x w rectangle where the table's Paste has paste_blank
// (blank = 1; both default tables), only the clip's positive cells otherwise (blank = 0).  Nothing else of the grid changes, so with B
// the object's cells inside grid_dim, K0 = (grid == answer) inside the common rectangle of grid_dim and answer_dim, Ws the write mask
// (blank = 1: B's box as a rectangle; blank = 0: B's cells whose byte is > 0) shifted to (px, py) and cut at H x W,
//     correct(px, py) = popc(K0) - popc(K0 & Ws) + popc(Ws & AZ & ~mism)
// mism = the OR over the used bit planes of (shifted clip plane XOR answer plane), the clip planes = the grid's planes AND B (AND the
// positive cells for blank = 0): a rectangle cell outside B carries colour 0 and matches exactly where the answer is 0.  `used` = the OR
// of the bytes a paste can write (blank = 1: every byte, negative ones are pasted too, so bit 7 is a plane: EIGHT statically indexed
// slots where arcle_place.h has seven; blank = 0: the positive bytes); AZ = the cells of the common rectangle whose answer byte has no
// bit outside `used`.  K0 and AZ are zero outside the common rectangle: write-mask bits shifted past column W - 1 of a row word, or
// past cell H * W of the flat board, meet zeros there and count nothing.
//
// ROW BOARD (W <= 32 and H <= 64; lane i = row i as a W-bit word): ONE LANE PER PASTE POSITION, 64 per pass over the rectangle of the
// positions within max_dist of (x0, y0) inside grid_dim; a lane outside the |dx| + |dy| diamond sits the pass out.  Per row r of the
// box the wave reads the write mask's word and the clip planes' as wave-uniform values (readlane), each lane shifts them by ITS dy and
// fetches the answer rows at r + ITS dx (ds_bpermute).  A stamp may hang over the bottom edge: a box row that lands at r + dx >= H
// contributes NOTHING (the lane index of the fetch wraps modulo 64, so the lane zeroes its write mask instead).  The arg-max is that of
// arcle_place.h: the packed keys  correct << 20 | (127 - |dx| - |dy|) << 13 | (63 - dx) << 6 | (31 - dy),  (dx, dy) = (px - x0, py - y0).
// FLAT BOARD (every other shape of at most 1024 cells; lane j < 32 = cells [32j, 32j + 32)): a wave-uniform loop over the positions,
// each a flat shift by dx * W + dy.  A stamp may hang over the right edge: the box columns that reach W are masked off BEFORE the shift
// (they would be carried into the next row); rows that reach H land at cells >= H * W, where K0 and AZ are zero.
#pragma once
#include "arcle_place.h"

namespace arcle {

// launch parameters: p = the handle's base parameters with n_envs = the number of rows, n_resident = the handle's envs and rows_in /
// rows_in_stride = the state rows (rows_in NULL: the resident envs 0 .. n_envs-1)
struct StampParams {
  StepParams p;
  int32_t max_comp;        // C: objects per row at most
  int32_t max_dist;        // positions with |px - x0| + |py - y0| <= max_dist
  const int32_t* count;    // optional int32 [n_rows][2]: word 0 = the objects of the row (NULL: C)
  const uint8_t* bits;     // uint8 [n_rows][C][ARCLE_BITS_STRIDE], 2-byte aligned
  const int32_t* src_env;  // optional int32 [n_rows]: the env whose answer judges the row (NULL: env = row)
  int32_t* stamp;          // int32 [n_rows][C][4] = px, py, correct(px, py), cells of B
  int32_t* base;           // optional int32 [n_rows][2]: the dense pair of the row's own grid
  int32_t blank;           // 1: Paste writes the clip's whole rectangle (paste_blank); 0: its positive cells only
  int32_t pad_;
};

ARCLE_DEV void stamp_emit(const StampParams& x, int lane, int row, int k, int px, int py, int correct, int cells) {
  if (lane == 0) {
    U4 v;
    v[0] = (uint32_t)px;
    v[1] = (uint32_t)py;
    v[2] = (uint32_t)correct;
    v[3] = (uint32_t)cells;
    xl::store_at(x.stamp + ((size_t)row * (size_t)x.max_comp) * 4, (uint32_t)k * 16u, v);
  }
}

constexpr int STAMP_PLANES = 8;  // bits 0 .. 7: with blank = 1 a negative byte is pasted like any other

template <int FW>
ARCLE_DEV void wave_stamp_row(const StampParams& x, WaveLDS* lds, const U2* lut, int row, int lane) {
  const StepParams& p = x.p;
  Wave w(p, lds, lut, lane, INGRESS_BBOX, FW, false, false, false);
  const int C = x.max_comp;
  const bool blank = x.blank != 0;
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
    for (int k = 0; k < n; k++) stamp_emit(x, lane, row, k, 0, 0, 0, 0);
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
  // the bits of the bytes a paste can write: the planes a colour comparison needs
  uint32_t ub;
  if (blank) {
    ub = grid[0] | grid[1] | grid[2] | grid[3];
  } else {
    const U4 pb = posbytes(grid);
    ub = (grid[0] & pb[0]) | (grid[1] & pb[1]) | (grid[2] & pb[2]) | (grid[3] & pb[3]);
  }
  ub |= ub >> 16;
  ub |= ub >> 8;
  const uint32_t used = xl::wave_or(ub & (blank ? 0xffu : 0x7fu));
  const uint32_t unused4 = (~used & 0xffu) * 0x01010101u;
  // (inside the common rectangle, like K0: bits of a write mask shifted out of the rectangle count nothing)
  const uint32_t AZ16 = (flags16(nzflags(ans[0] & unused4), nzflags(ans[1] & unused4), nzflags(ans[2] & unused4), nzflags(ans[3] & unused4)) ^ 0xffffu) & common16;
  const uint32_t pos16g = pos16(grid) & inside16;
  const int D = x.max_dist;
  const uint8_t* brow = x.bits + (size_t)row * (size_t)C * ARCLE_BITS_STRIDE;

  if (FW != FW_GENERIC || (p.W <= 32 && p.H <= 64)) {
    // ROW BOARD
    const uint32_t Wb = (uint32_t)p.W;
    const uint32_t K0 = rows_from16(w, K0_16, Wb), AZ = rows_from16(w, AZ16, Wb), GP = rows_from16(w, pos16g, Wb);
    uint32_t Gb[STAMP_PLANES], Ab[STAMP_PLANES];
#pragma unroll
    for (int b = 0; b < STAMP_PLANES; b++) {
      Gb[b] = Ab[b] = 0u;
      if ((used >> b) & 1u) {
        Gb[b] = rows_from16(w, plane16(grid, b), Wb);
        Ab[b] = rows_from16(w, plane16(ans, b), Wb);
      }
    }
    for (int k = 0; k < n; k++) {
      const uint32_t b16 = (uint32_t)*reinterpret_cast<const uint16_t*>(brow + (size_t)k * ARCLE_BITS_STRIDE + 2 * lane) & inside16;
      const uint32_t B = rows_from16(w, b16, Wb);
      const uint32_t S = blank ? B : (B & GP);  // the cells whose colour the clip carries
      const int cells = (int)xl::wave_add((uint32_t)__builtin_popcount(B));
      const unsigned long long rowsB = xl::ballot(B != 0u);
      if (!rowsB) {  // (wave-uniform)
        stamp_emit(x, lane, row, k, 0, 0, base_correct, 0);
        continue;
      }
      const uint32_t cols = xl::wave_or(B);
      const int x0 = __builtin_ctzll(rowsB), x1 = 63 - __builtin_clzll(rowsB);
      const int y0 = __builtin_ctz(cols), y1 = 31 - __builtin_clz(cols);
      const uint32_t rect = (2u << y1) - (1u << y0);  // one row of the box
      const int px0 = imax(x0 - D, 0), px1 = imin(x0 + D, gh - 1);
      const int py0 = imax(y0 - D, 0), py1 = imin(y0 + D, gw - 1);
      const int ny = py1 - py0 + 1, total = (px1 - px0 + 1) * ny;
      const uint32_t magic = 65536u / (uint32_t)ny + 1u;
      int best = 0;
      for (int t0 = 0; t0 < total; t0 += 64) {
        const int t = t0 + lane;
        int i = (int)(((uint32_t)t * magic) >> 16);
        if (i * ny > t) i--;
        const int dx = px0 + i - x0, dy = py0 + (t - i * ny) - y0;
        const int dist = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
        const bool valid = t < total && dist <= D;
        const uint32_t sl = (uint32_t)imax(dy, 0) & 31u, sr = (uint32_t)imax(-dy, 0) & 31u;
        int delta = 0;
        for (int r = x0; r <= x1; r++) {
          const uint32_t s = xl::readlane(S, r);
          const uint32_t wm = blank ? rect : s;
          if (!wm) continue;  // (wave-uniform)
          const int at = r + dx;
          // a box row that hangs over the bottom edge writes nothing (and `at & 63` would name a real row)
          const uint32_t ws = (at >= 0 && at < p.H) ? ((wm << sl) >> sr) : 0u;
          const uint32_t kk = xl::shfl(K0, at & 63), az = xl::shfl(AZ, at & 63);
          uint32_t mism = 0;
#pragma unroll
          for (int b = 0; b < STAMP_PLANES; b++) {
            if ((used >> b) & 1u) {
              const uint32_t ob = xl::readlane(Gb[b], r) & s;
              mism |= ((ob << sl) >> sr) ^ xl::shfl(Ab[b], at & 63);
            }
          }
          delta += __builtin_popcount(ws & az & ~mism) - __builtin_popcount(kk & ws);
        }
        const int key = ((base_correct + delta) << 20) | ((127 - dist) << 13) | ((63 - dx) << 6) | (31 - dy);
        if (valid) best = imax(best, key);
      }
      xl::lanes_converged();
      best = w.wave_max(best);
      stamp_emit(x, lane, row, k, x0 + 63 - ((best >> 6) & 127), y0 + 31 - (best & 63), best >> 20, cells);
    }
  } else {
    // FLAT BOARD
    const uint32_t K0 = to32(w, K0_16), AZ = to32(w, AZ16), GP = to32(w, pos16g);
    uint32_t Gb[STAMP_PLANES], Ab[STAMP_PLANES];
#pragma unroll
    for (int b = 0; b < STAMP_PLANES; b++) {
      Gb[b] = Ab[b] = 0u;
      if ((used >> b) & 1u) {
        Gb[b] = to32(w, plane16(grid, b));
        Ab[b] = to32(w, plane16(ans, b));
      }
    }
    const int f0 = (32 * lane) & 1023, fc = f0 - cell_row(p, f0) * p.W;  // this lane's 32 cells start in column fc
    for (int k = 0; k < n; k++) {
      const uint32_t b16 = (uint32_t)*reinterpret_cast<const uint16_t*>(brow + (size_t)k * ARCLE_BITS_STRIDE + 2 * lane) & inside16;
      const uint32_t B = to32(w, b16);
      const uint32_t S = blank ? B : (B & GP);
      const int cells = (int)xl::wave_add((uint32_t)__builtin_popcount(B));
      const unsigned long long lanesB = xl::ballot(B != 0u);
      // the box from the cell indices, as wave_place_row takes it
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
      if (!lanesB) {  // (wave-uniform)
        stamp_emit(x, lane, row, k, 0, 0, base_correct, 0);
        continue;
      }
      const int lf = __builtin_ctzll(lanesB), ll = 63 - __builtin_clzll(lanesB);
      const int first = 32 * lf + __builtin_ctz(xl::uniform(xl::readlane(B, lf)));
      const int last = 32 * ll + 31 - __builtin_clz(xl::uniform(xl::readlane(B, ll)));
      const int x0 = cell_row(p, first), x1 = cell_row(p, last);
      const int px0 = imax(x0 - D, 0), px1 = imin(x0 + D, gh - 1);
      const int py0 = imax(y0 - D, 0), py1 = imin(y0 + D, gw - 1);
      int bc = -1, bd = 0, bdx = 0, bdy = 0;
      for (int py = py0; py <= py1; py++) {
        const int dy = py - y0;
        // the box columns that stay below W at this py: the others are cut BEFORE the shift, which would carry them into the next row
        const uint32_t keep = to32(w, w.rect16(x0, x1, y0, imin(y1, p.W - 1 - dy)));
        const uint32_t wm = blank ? keep : (S & keep), sc = S & keep;
        for (int px = px0; px <= px1; px++) {
          const int dx = px - x0;
          const int dist = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
          if (dist > D) continue;  // (wave-uniform)
          const int s = dx * p.W + dy;
          uint32_t ws = wm, mism = 0;
          if (s > 0) ws = board_shl(w, wm, s);
          else if (s < 0) ws = board_shr(w, wm, -s);
#pragma unroll
          for (int b = 0; b < STAMP_PLANES; b++) {
            if ((used >> b) & 1u) {
              uint32_t ob = Gb[b] & sc;
              if (s > 0) ob = board_shl(w, ob, s);
              else if (s < 0) ob = board_shr(w, ob, -s);
              mism |= ob ^ Ab[b];
            }
          }
          // (the difference may be negative: the sum wraps modulo 2^32 and comes back as an int)
          const int c = base_correct + (int)xl::wave_add((uint32_t)(__builtin_popcount(ws & AZ & ~mism) - __builtin_popcount(K0 & ws)));
          if (c > bc || (c == bc && (dist < bd || (dist == bd && (dx < bdx || (dx == bdx && dy < bdy)))))) bc = c, bd = dist, bdx = dx, bdy = dy;
        }
      }
      xl::lanes_converged();
      stamp_emit(x, lane, row, k, x0 + bdx, y0 + bdy, bc, cells);
    }
  }
}

}  // namespace arcle
