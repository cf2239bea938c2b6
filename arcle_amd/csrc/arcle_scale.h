// arcle_scale.h — the grid or the input of a state row ZOOMED, SHRUNK or TILED onto the ANSWER'S CANVAS (arcle_scale_rows): for each
// source asked for (the row's grid, the row's input) the best of 132 separable cell maps — every cell a kx x ky block, the top-left cell
// of every kx x ky block, the source repeated with or without mirrored tile columns / rows — with its correct cells, the colours of its
// child and that child's cells colour by colour as ready-made bit-row selections.  A sibling of arcle_align.h, the other proposer whose
// child has the answer's grid_dim: its reading of the row, its dims and its `base` are taken over, its helpers (plane16 of arcle_place.h,
// the boards of arcle_wave.h) are used, and nothing of the sibling headers is changed.
//
//   wave_scale_row<FW, FLAT>  one wavefront takes one row: the answer of env src_env[row], its four bit planes and the canvas mask are built
//                       once per row, per source its planes; per candidate one cross-lane fetch and one XOR per plane, one popcount and
//                       one wave sum, no step body
//
// Compiled like arcle_align.h: by hipcc through arcle_hip.hip and by g++ through tests/emu/scale_emu.cpp (plain C++ and xl:: only).
//
// With S the source plane, (sh, sw) its dims and (ah, aw) the answer's, the source value is v(x, y) = S[x, y] if (x, y) lies inside
// (sh, sw) and 1 <= S[x, y] <= 9, else 0, and the child of candidate (f, g) on the canvas [0, ah) x [0, aw) is G'[i, j] = v(f(i), g(j)):
//     ZOOM(kx, ky)     index (kx - 1) * 8 + (ky - 1)        f(i) = i div kx,  g(j) = j div ky
//     SHRINK(kx, ky)   index 64 + (kx - 1) * 8 + (ky - 1)   f(i) = i * kx,    g(j) = j * ky
//     TILE(t)          index 128 + t                        g(j) = j mod sw, mirrored (sw - 1 - j mod sw) in the odd tile columns when
//                                                           bit 0 of t is set; f likewise with sh and bit 1
// An f(i) or g(j) outside the source's dims reads 0.  Colours 0 .. 9 fit FOUR bit planes; the source's planes are masked to (sh, sw) and
// to the bytes 1 .. 9 before anything else, the answer's to the canvas cells whose byte is 0 .. 9 (CZ: no other byte ever matches), so
//     correct = popc(CZ & ~mism),  mism = the OR over the planes of (child plane XOR answer plane).
// A plane the source has no bit in is all zero in every child: its answer plane is taken out of CZ once per source, and the candidates
// XOR the planes in use only (wave-uniform branches, statically indexed plane slots: registers).
//
// Both maps work on whole rows and whole columns, so a candidate is a column map applied to every row word and a row map that moves
// row words.  The column map has 8 + 8 + 2 variants only; each is built once and serves the 8 (TILE: 2) row maps.  The running best is
// the packed key  correct << 8 | (255 - index): more correct, then the lower index.  The winner's child is built once more for its
// colours and its nine bit rows.
//
// ROW BOARD (W <= 32 and H <= 64; lane i = row i as a W-bit word).  The column map is bit work inside the lane's own word: bit j takes
// bit g(j), j wave-uniform.  The row map is one cross-lane fetch per plane: lane i takes the word of lane f(i) — and zeroes it when f(i)
// is outside [0, sh): the lane index of the fetch wraps modulo 64 and would name a real row (the trap arcle_stamp.h documents; i * kx
// reaches 504).
// FLAT BOARD (every other shape of at most 1024 cells; lane j < 32 = cells [32j, 32j + 32)): the column map gathers every cell's bit
// from the word that holds cell (x, g(y)), one fetch per cell and plane; the row map takes, for every run of the lane's cells inside one
// canvas row i, the 32 cells that start (f(i) - i) * W cells further on (two fetches per plane, the offset differs per lane) under the
// run's mask.  The loops run to wave-uniform bounds, lanes without work fetch and drop.  The slow path: checked for its answers.
#pragma once
#include "arcle_align.h"

namespace arcle {

// launch parameters: p = the handle's base parameters with n_envs = the number of rows, n_resident = the handle's envs and rows_in /
// rows_in_stride = the state rows (rows_in NULL: the resident envs 0 .. n_envs-1)
struct ScaleParams {
  StepParams p;
  uint32_t sources;        // ARCLE_ALIGN_GRID | ARCLE_ALIGN_INPUT
  uint32_t modes;          // ARCLE_SCALE_ZOOM | ARCLE_SCALE_SHRINK | ARCLE_SCALE_TILE
  const int32_t* src_env;  // optional int32 [n_rows]: the env whose answer judges the row (NULL: env = row)
  int32_t* scale;          // int32 [n_rows][2][8] = cand, correct, total, colours, sh, sw, ah, aw; slot 0 the grid, slot 1 the input
  int32_t* table;          // optional int32 [n_rows][2][SCALE_CANDS]: correct of every candidate, -1 for a mode not asked for
  uint8_t* bits;           // optional uint8 [n_rows][2][9][ARCLE_BITS_STRIDE], 2-byte aligned: the best child's cells of colour 1 .. 9
  int32_t* base;           // optional int32 [n_rows][2]: the dense pair of the row's own grid
};

constexpr int SCALE_PLANES = 4;   // colours 0 .. 9
constexpr int SCALE_CANDS = 132;  // 64 zooms, 64 shrinks, 4 tiles
constexpr int SCALE_COLORS = 9;   // the bit rows: colours 1 .. 9

// the source index a map takes index t from — mode 0: zoom by k, 1: shrink by k, 2: tile of period n, mirrored in the odd tiles when
// k != 0 — or -1 where it lies outside [0, n); 1 <= n, 0 <= t
ARCLE_DEV int scale_map(int mode, int k, int t, int n) {
  int s;
  if (mode == 0) {
    s = (int)((uint32_t)t / (uint32_t)k);
  } else if (mode == 1) {
    s = t * k;
  } else {
    const uint32_t q = (uint32_t)t / (uint32_t)n, r = (uint32_t)t - q * (uint32_t)n;
    s = (k && (q & 1u)) ? n - 1 - (int)r : (int)r;
  }
  return s < n ? s : -1;
}

// candidate index -> (mode, row parameter, column parameter) as scale_map takes them
ARCLE_DEV void scale_decode(int cand, int& mode, int& kx, int& ky) {
  if (cand < 128) {
    mode = cand >> 6;
    kx = ((cand >> 3) & 7) + 1;
    ky = (cand & 7) + 1;
  } else {
    mode = 2;
    kx = (cand >> 1) & 1;
    ky = cand & 1;
  }
}

// the cells whose byte is 0 .. 9: no bit in the high nibble, and not 10 .. 15 (bit 3 with bit 2 or bit 1)
ARCLE_DEV uint32_t scale_ok16(const U4& v) {
  const uint32_t hi = flags16(nzflags(v[0] & 0xf0f0f0f0u), nzflags(v[1] & 0xf0f0f0f0u), nzflags(v[2] & 0xf0f0f0f0u), nzflags(v[3] & 0xf0f0f0f0u));
  return (hi ^ 0xffffu) & ~(plane16(v, 3) & (plane16(v, 2) | plane16(v, 1))) & 0xffffu;
}

ARCLE_DEV void scale_emit(const ScaleParams& x, int lane, int row, int slot, int cand, int correct, int total, uint32_t colours, const AlignDims& d) {
  if (lane == 0) {
    U4 a, b;
    a[0] = (uint32_t)cand;
    a[1] = (uint32_t)correct;
    a[2] = (uint32_t)total;
    a[3] = colours;
    b[0] = (uint32_t)d.sh;
    b[1] = (uint32_t)d.sw;
    b[2] = (uint32_t)d.ah;
    b[3] = (uint32_t)d.aw;
    xl::store_at(x.scale + (size_t)row * 16, (uint32_t)slot * 32u, a);
    xl::store_at(x.scale + (size_t)row * 16, (uint32_t)slot * 32u + 16u, b);
  }
}

// lane l holds the table's words l, 64 + l and 128 + l
ARCLE_DEV void scale_emit_table(const ScaleParams& x, int lane, int row, int slot, int t0, int t1, int t2) {
  if (!x.table) return;
  int32_t* t = x.table + ((size_t)row * 2 + (size_t)slot) * SCALE_CANDS;
  t[lane] = t0;
  t[64 + lane] = t1;
  if (lane < SCALE_CANDS - 128) t[128 + lane] = t2;
}

// this lane's 16 cells of the bit row of colour c (1 .. 9)
ARCLE_DEV void scale_emit_bits(const ScaleParams& x, int lane, int row, int slot, int c, uint32_t b16) {
  uint8_t* b = x.bits + (((size_t)row * 2 + (size_t)slot) * SCALE_COLORS + (size_t)(c - 1)) * ARCLE_BITS_STRIDE;
  *reinterpret_cast<uint16_t*>(b + 2 * lane) = (uint16_t)b16;
}

// a slot with no candidate
ARCLE_DEV void scale_emit_none(const ScaleParams& x, int lane, int row, int slot, const AlignDims& d) {
  scale_emit(x, lane, row, slot, -1, 0, 0, 0u, d);
  scale_emit_table(x, lane, row, slot, -1, -1, -1);
  if (x.bits) {
#pragma unroll 1
    for (int c = 1; c <= SCALE_COLORS; c++) scale_emit_bits(x, lane, row, slot, c, 0u);
  }
}

// ROW BOARD: the source's planes as row words, the column map inside the word, the row map by a cross-lane fetch
struct ScaleRowBoard {
  const Wave& w;
  int lane;
  AlignDims d;
  uint32_t used;                 // the planes the source has a bit in
  uint32_t CZ;                   // the canvas cells that can match: answer byte 0 .. 9, no bit in a plane the source does not use
  uint32_t Sb[SCALE_PLANES];     // the source, masked
  uint32_t Ab[SCALE_PLANES];     // the answer
  uint32_t Cm[SCALE_PLANES];     // the source under the current column map
  uint32_t Ch[SCALE_PLANES];     // the current child

  ARCLE_DEV void colmap(int mode, int k) {
    if (mode < 2 && k == 1) {  // g(j) = j (wave-uniform)
      const uint32_t cols = d.aw >= 32 ? 0xffffffffu : (1u << d.aw) - 1u;
#pragma unroll
      for (int b = 0; b < SCALE_PLANES; b++) Cm[b] = Sb[b] & cols;
      return;
    }
#pragma unroll
    for (int b = 0; b < SCALE_PLANES; b++) Cm[b] = 0u;
    // g(j) by counting, j = q * period + r (wave-uniform; a scalar division costs registers the candidates' loop needs): the period
    // is k for a zoom and sw for a tiling; scale_map says the same of one index
    const int period = mode == 0 ? k : d.sw;
    int q = 0, r = 0;
#pragma unroll 1
    for (int j = 0; j < d.aw; j++) {
      const int s = mode == 0 ? q : mode == 1 ? j * k : ((k && (q & 1)) ? d.sw - 1 - r : r);
      if (++r == period) r = 0, q++;
      if (s >= d.sw) continue;
#pragma unroll
      for (int b = 0; b < SCALE_PLANES; b++)
        if ((used >> b) & 1u) Cm[b] |= ((Sb[b] >> (uint32_t)s) & 1u) << (uint32_t)j;
    }
  }
  ARCLE_DEV void child(int mode, int k) {
    const int s = lane < d.ah ? scale_map(mode, k, lane, d.sh) : -1;
#pragma unroll
    for (int b = 0; b < SCALE_PLANES; b++) {
      Ch[b] = 0u;
      if ((used >> b) & 1u) {
        // a row outside the source is no row (and `s & 63` would name a real one)
        const uint32_t v = xl::shfl(Cm[b], s & 63);
        Ch[b] = s >= 0 ? v : 0u;
      }
    }
  }
  ARCLE_DEV uint32_t to16(uint32_t v) const { return rows_to16(w, v, (uint32_t)w.p.W); }
};

// FLAT BOARD: the same on 32-cell words
struct ScaleFlatBoard {
  const Wave& w;
  int lane;
  AlignDims d;
  uint32_t used;
  uint32_t CZ;
  uint32_t Sb[SCALE_PLANES];
  uint32_t Ab[SCALE_PLANES];
  uint32_t Cm[SCALE_PLANES];
  uint32_t Ch[SCALE_PLANES];
  int r0, c0, nseg;  // the lane's first cell; the rows 32 cells can touch (wave-uniform)

  ARCLE_DEV void colmap(int mode, int k) {
    if (mode < 2 && k == 1) {
#pragma unroll
      for (int b = 0; b < SCALE_PLANES; b++) Cm[b] = Sb[b];
      return;
    }
#pragma unroll
    for (int b = 0; b < SCALE_PLANES; b++) Cm[b] = 0u;
    const int W = w.p.W;
    int i = r0, j = c0;
#pragma unroll 1
    for (int t = 0; t < 32; t++) {
      // cell (i, j) takes cell (i, g(j)); a lane beyond the board, a column beyond the canvas: fetch and drop
      const int s = (lane < 32 && j < d.aw) ? scale_map(mode, k, j, d.sw) : -1;
      const int from = i * W + (s < 0 ? 0 : s);
#pragma unroll
      for (int b = 0; b < SCALE_PLANES; b++)
        if ((used >> b) & 1u) {
          const uint32_t v = xl::shfl(Sb[b], (from >> 5) & 63);
          Cm[b] |= s >= 0 ? ((v >> ((uint32_t)from & 31u)) & 1u) << (uint32_t)t : 0u;
        }
      if (++j == W) j = 0, i++;
    }
  }
  ARCLE_DEV void child(int mode, int k) {
#pragma unroll
    for (int b = 0; b < SCALE_PLANES; b++) Ch[b] = 0u;
    const int W = w.p.W;
    int i = r0, c = c0, at = 0;
#pragma unroll 1
    for (int sg = 0; sg < nseg; sg++) {
      // the run of this lane's cells inside canvas row i: bits [at, at + len)
      const int len = imin(W - c, 32 - at);
      const bool run = lane < 32 && len > 0 && i < d.ah;
      const int s = run ? scale_map(mode, k, i, d.sh) : -1;
      const uint32_t m = (run && s >= 0) ? ((len >= 32 ? 0xffffffffu : (1u << len) - 1u) << (uint32_t)at) : 0u;
      // the 32 cells that start (s - i) * W cells further on
      const int q = 32 * lane + (s < 0 ? 0 : (s - i) * W);
      const int l0 = q >> 5, l1 = l0 + 1;
      const uint32_t sh = (uint32_t)q & 31u;
#pragma unroll
      for (int b = 0; b < SCALE_PLANES; b++)
        if ((used >> b) & 1u) {
          uint32_t w0 = xl::shfl(Cm[b], l0 & 63), w1 = xl::shfl(Cm[b], l1 & 63);
          if (l0 < 0 || l0 > 31) w0 = 0u;
          if (l1 < 0 || l1 > 31) w1 = 0u;
          Ch[b] |= (sh ? ((w0 >> sh) | (w1 << (32u - sh))) : w0) & m;
        }
      if (len > 0) at += len, c = 0, i++;
    }
  }
  ARCLE_DEV uint32_t to16(uint32_t v) const { return arcle::to16(w, v); }
};

// the cells of the current child whose colour is c
template <typename BOARD>
ARCLE_DEV uint32_t scale_cells(const BOARD& bd, uint32_t canvas, int c) {
  uint32_t m = canvas;
#pragma unroll
  for (int b = 0; b < SCALE_PLANES; b++) m &= ((c >> b) & 1) ? bd.Ch[b] : ~bd.Ch[b];
  return m;
}

// one source on either board: bd holds the source's and the answer's planes; canvas = the canvas as a board
template <typename BOARD>
ARCLE_DEV void scale_source(const ScaleParams& x, int lane, int row, int slot, BOARD& bd, uint32_t canvas) {
  const AlignDims& d = bd.d;
  int best = -1, t0 = -1, t1 = -1, t2 = -1;
  // (rolled loops: the 132 candidates are one body, not 132 copies of it)
#pragma unroll 1
  for (int mode = 0; mode < 3; mode++) {
    if (!((x.modes >> mode) & 1u)) continue;  // (wave-uniform)
    const int nk = mode == 2 ? 2 : 8, k0 = mode == 2 ? 0 : 1;
#pragma unroll 1
    for (int yi = 0; yi < nk; yi++) {
      bd.colmap(mode, k0 + yi);
#pragma unroll 1
      for (int xi = 0; xi < nk; xi++) {
        const int cand = mode == 2 ? 128 + 2 * xi + yi : 64 * mode + 8 * xi + yi;
        bd.child(mode, k0 + xi);
        uint32_t mism = 0u;
#pragma unroll
        for (int b = 0; b < SCALE_PLANES; b++)
          if ((bd.used >> b) & 1u) mism |= bd.Ch[b] ^ bd.Ab[b];
        const int c = (int)xl::wave_add((uint32_t)__builtin_popcount(bd.CZ & ~mism));
        best = imax(best, (c << 8) | (255 - cand));
        if ((cand & 63) == lane) {
          if (cand < 64) t0 = c;
          else if (cand < 128) t1 = c;
          else t2 = c;
        }
      }
    }
  }
  xl::lanes_converged();
  const int cand = 255 - (best & 255);
  int mode, kx, ky;
  scale_decode(cand, mode, kx, ky);
  bd.colmap(mode, ky);
  bd.child(mode, kx);
  uint32_t colours = 0u;
#pragma unroll 1
  for (int c = 1; c <= SCALE_COLORS; c++) {
    const uint32_t cells = scale_cells(bd, canvas, c);
    if (xl::ballot(cells != 0u)) colours |= 1u << c;
    if (x.bits) scale_emit_bits(x, lane, row, slot, c, bd.to16(cells));
  }
  scale_emit(x, lane, row, slot, cand, best >> 8, d.ah * d.aw, colours, d);
  scale_emit_table(x, lane, row, slot, t0, t1, t2);
}

// FLAT = the flat board (W > 32 or H > 64, always with FW_GENERIC): an instantiation of its own, as in arcle_region.h, so that no kernel
// carries both boards' loops (scalar registers)
template <int FW, bool FLAT>
ARCLE_DEV void wave_scale_row(const ScaleParams& x, WaveLDS* lds, const U2* lut, int row, int lane) {
  const StepParams& p = x.p;
  Wave w(p, lds, lut, lane, INGRESS_BBOX, FW, false, false, false);
  const bool want_g = (x.sources & 1u) != 0u, want_i = (x.sources & 2u) != 0u;
  int src = row;
  if (x.src_env) src = (int)xl::uniform((uint32_t)x.src_env[row]);
  if (src < 0 || src >= p.n_resident) {  // no such env to take the answer from
    if (x.base && lane == 0) {
      U2 b;
      b[0] = b[1] = 0u;
      xl::store_at(x.base, (uint32_t)row * 8u, b);
    }
    AlignDims z;
    z.sh = z.sw = z.ah = z.aw = 0;
    if (want_g) scale_emit_none(x, lane, row, 0, z);
    if (want_i) scale_emit_none(x, lane, row, 1, z);
    return;
  }
  // the grid plane and grid_dim (always: `base` is the grid's), the input plane and input_dim when asked for, the answer plane and
  // answer_dim: as wave_align_row reads them
  U4 grid = u4_zero(), inp = u4_zero(), ans = u4_zero();
  int gh, gw, ih = 0, iw = 0;
  if (p.rows_in) {
    const int8_t* rin = p.rows_in + (size_t)row * p.rows_in_stride;
    const int off = row_offset(p, ARCLE_PL_GRID);
    grid = row_plane(w, rin, off);
    gh = (int)row_byte(rin, off + p.P);
    gw = (int)row_byte(rin, off + p.P + 1);
    if (want_i) {
      const int offi = row_offset(p, ARCLE_PL_INPUT);
      inp = row_plane(w, rin, offi);
      ih = (int)row_byte(rin, offi + p.P);
      iw = (int)row_byte(rin, offi + p.P + 1);
    }
  } else {
    if (16 * lane < p.PS) grid = xl::load16(p.plane[ARCLE_PL_GRID], (uint32_t)row * (uint32_t)p.PS + 16u * (uint32_t)lane);
    const Rec r = load_rec(p, row);
    gh = r.gh();
    gw = r.gw();
    if (want_i) {
      if (16 * lane < p.PS) inp = xl::load16(p.plane[ARCLE_PL_INPUT], (uint32_t)row * (uint32_t)p.PS + 16u * (uint32_t)lane);
      ih = r.in_h();
      iw = r.in_w();
    }
  }
  if (16 * lane < p.PS) ans = xl::load16(p.plane[ARCLE_PL_ANSWER], (uint32_t)src * (uint32_t)p.PS + 16u * (uint32_t)lane);
  const Rec ra = load_rec(p, src);
  AlignDims dg, di;
  dg.sh = align_dim(gh, p.H);
  dg.sw = align_dim(gw, p.W);
  di.sh = align_dim(ih, p.H);
  di.sw = align_dim(iw, p.W);
  dg.ah = di.ah = imin(ra.ah(), p.H);
  dg.aw = di.aw = imin(ra.aw(), p.W);
  if (x.base) {  // the dense pair of the row's own grid, as the siblings write it
    gh = imin(gh, p.H);
    gw = imin(gw, p.W);
    const int ah = dg.ah, aw = dg.aw;
    const int mh = imin(gh, ah), mw = imin(gw, aw);
    const uint32_t common16 = w.rect16(0, mh - 1, 0, mw - 1);
    const uint32_t K0_16 = (flags16(nzflags(grid[0] ^ ans[0]), nzflags(grid[1] ^ ans[1]), nzflags(grid[2] ^ ans[2]), nzflags(grid[3] ^ ans[3])) ^ 0xffffu) & common16;
    const int base_correct = (int)xl::wave_add((uint32_t)__builtin_popcount(K0_16));
    if (lane == 0) {
      int total = mh * mw;  // (agents/env.py:48-52, as step_core counts it)
      if ((gh <= ah) == (gw <= aw)) total += ah * aw > gh * gw ? ah * aw - gh * gw : gh * gw - ah * aw;
      else total += (gh > ah ? gh - ah : ah - gh) * mw + (gw > aw ? gw - aw : aw - gw) * mh;
      U2 b;
      b[0] = (uint32_t)base_correct;
      b[1] = (uint32_t)total;
      xl::store_at(x.base, (uint32_t)row * 8u, b);
    }
  }
  // the canvas, and its cells whose answer byte is a colour
  const uint32_t canvas16 = w.rect16(0, dg.ah - 1, 0, dg.aw - 1);
  const uint32_t az16 = canvas16 & scale_ok16(ans);
#pragma unroll 1
  for (int slot = 0; slot < 2; slot++) {
    if (!((x.sources >> slot) & 1u)) continue;  // (wave-uniform)
    // (by value: a reference picked at run time would put both planes into memory)
    U4 S;
    AlignDims d;
#pragma unroll
    for (int q = 0; q < 4; q++) S[q] = slot ? inp[q] : grid[q];
    d.sh = slot ? di.sh : dg.sh;
    d.sw = slot ? di.sw : dg.sw;
    d.ah = dg.ah;
    d.aw = dg.aw;
    if (d.sh < 1 || d.sw < 1 || d.ah < 1 || d.aw < 1) {  // no candidate (wave-uniform)
      scale_emit_none(x, lane, row, slot, d);
      continue;
    }
    // the source's cells that carry a colour 1 .. 9 inside its dims; a zero byte has no bit in any plane
    const uint32_t m16 = w.rect16(0, d.sh - 1, 0, d.sw - 1) & scale_ok16(S);
    uint32_t s16[SCALE_PLANES], a16[SCALE_PLANES], ub = 0u;
#pragma unroll
    for (int b = 0; b < SCALE_PLANES; b++) {
      s16[b] = plane16(S, b) & m16;
      a16[b] = plane16(ans, b) & az16;
      ub |= s16[b] ? (1u << b) : 0u;
    }
    const uint32_t used = xl::wave_or(ub);
    uint32_t cz16 = az16;
#pragma unroll
    for (int b = 0; b < SCALE_PLANES; b++)
      if (!((used >> b) & 1u)) cz16 &= ~a16[b];
    if (!FLAT) {
      const uint32_t Wb = (uint32_t)p.W;
      ScaleRowBoard bd = {w, lane, d, used, rows_from16(w, cz16, Wb), {}, {}, {}, {}};
#pragma unroll
      for (int b = 0; b < SCALE_PLANES; b++) {
        bd.Sb[b] = bd.Ab[b] = 0u;
        if ((used >> b) & 1u) bd.Sb[b] = rows_from16(w, s16[b], Wb), bd.Ab[b] = rows_from16(w, a16[b], Wb);
      }
      scale_source(x, lane, row, slot, bd, rows_from16(w, canvas16, Wb));
    } else {
      const int f0 = (32 * lane) & 1023, fr = cell_row(p, f0);
      ScaleFlatBoard bd = {w, lane, d, used, to32(w, cz16), {}, {}, {}, {}, fr, f0 - fr * p.W, p.W >= 32 ? 2 : (31 + p.W - 1) / p.W + 1};
#pragma unroll
      for (int b = 0; b < SCALE_PLANES; b++) {
        bd.Sb[b] = bd.Ab[b] = 0u;
        if ((used >> b) & 1u) bd.Sb[b] = to32(w, s16[b]), bd.Ab[b] = to32(w, a16[b]);
      }
      scale_source(x, lane, row, slot, bd, to32(w, canvas16));
    }
  }
}

}  // namespace arcle
