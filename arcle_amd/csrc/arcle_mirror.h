// arcle_mirror.h — each object's box filled from its MIRROR IMAGE (arcle_mirror_rows): for every object (a bit row, as
// arcle_components_rows / arcle_objects_rows write it) and each of the three symmetries — left-right (H), up-down (V), point — the source
// rectangle R whose flipped copy, written over the object's box, leaves the most correct cells, with that count: what CopyO on R + Paste
// at the box's corner + Flip of the box leave.  The fifth sibling; it takes the boards, the bit planes and the packed-key arg-max of
// arcle_place.h and the 64-lanes-per-pass scan of arcle_stamp.h with the roles INVERTED: the destination (the box) is fixed and the source
// moves.  None of those files is changed.
//
//   wave_mirror_row<FW>  one wavefront takes ALL objects of one row: the grid, the answer of env src_env[row] and the boards made of
//                        them are built once per row; per (object, symmetry) a handful of AND + popcount per candidate, no step body
//
// Compiled like arcle_turn.h: by hipcc through arcle_hip.hip and by g++ through tests/emu/mirror_emu.cpp.
//
// With B the object's cells inside grid_dim and (x0, y0, x1, y1) its box of h x w cells, a candidate of slot s is the h x w rectangle R
// with its corner at (sx, sy) = (x0 + dx, y0 + dy) inside grid_dim, |dx| + |dy| <= max_dist, dx = 0 in slot H and dy = 0 in slot V (R may
// overlap the box; dx = dy = 0 flips the box where it stands).  The child is the grid with box cell (r, c) replaced by pos(T') —
//     T' = G[sx + r - x0][sy + y1 - c]  (H),   G[sx + x1 - r][sy + c - y0]  (V),   G[sx + x1 - r][sy + y1 - c]  (POINT)
// under blank = 1; under blank = 0 a source byte <= 0 is not pasted, and the box's OWN old cell at the same mirrored place (the candidate
// dx = dy = 0) shows through — and pos(v) = v for v > 0, else 0: the Flip lifts the rectangle and writes back its positive cells only
// (object.py:60-138, 265-276, 291-348).  Nothing outside the box changes, so
//     correct(s, dx, dy) = popc(K0) - popc(K0 & box) + popc(box & AZ & ~mism)
// K0 = (grid == answer) inside the common rectangle, mism = the OR over the used bit planes of (new colour plane XOR answer plane), the new
// colour's planes = the grid's POSITIVE planes read through the mirror (a cell whose source is not positive carries colour 0 and matches
// exactly where the answer is 0), `used` and AZ as in arcle_place.h.  The arg-max is that of arcle_place.h: the packed keys
// correct << 20 | (127 - |dx| - |dy|) << 13 | (63 - dx) << 6 | (31 - dy);  dx = dy = 0 is always a candidate, so a valid key exists.
//
// ROW BOARD (W <= 32 and H <= 64; lane i = row i as a W-bit word): ONE LANE PER CANDIDATE, 64 per pass over the rectangle of corners
// within max_dist (slot POINT has up to 64 x 32 of them); a lane outside the |dx| + |dy| diamond sits the pass out.  Per box row r the
// answer planes' words and AZ are wave-uniform (readlane); each lane fetches the grid planes' words of ITS source row (ds_bpermute: sx +
// r - x0, or sx + x1 - r when rows are mirrored), bit-reverses them when columns are mirrored (v_bfrev_b32) and shifts them by ITS amount
// so that the source column lands on box column c: 31 - y1 - sy after the reversal (in [-31, 31]), dy without it.
// FLAT BOARD (every other shape of at most 1024 cells): the slow path — a wave-uniform loop over the candidates, one lane per box cell, 64
// per pass; each lane gathers the bytes of its source cell, its box cell and the answer cell across the wave (lane l holds the bytes of
// cells [16l, 16l + 16)) and compares them as bytes; one wave reduction per candidate.
#pragma once
#include "arcle_turn.h"

namespace arcle {

constexpr int MIRROR_SLOTS = 3;   // slot s <-> bit s of `mirrors`: H, V, POINT
constexpr int MIRROR_PLANES = 7;  // bits 0 .. 6 of a positive int8

// launch parameters: p = the handle's base parameters with n_envs = the number of rows, n_resident = the handle's envs and rows_in /
// rows_in_stride = the state rows (rows_in NULL: the resident envs 0 .. n_envs-1)
struct MirrorParams {
  StepParams p;
  int32_t max_comp;        // C: objects per row at most
  int32_t max_dist;        // candidates with |dx| + |dy| <= max_dist
  const int32_t* count;    // optional int32 [n_rows][2]: word 0 = the objects of the row (NULL: C)
  const uint8_t* bits;     // uint8 [n_rows][C][ARCLE_BITS_STRIDE], 2-byte aligned
  const int32_t* src_env;  // optional int32 [n_rows]: the env whose answer judges the row (NULL: env = row)
  int32_t* mirror;         // int32 [n_rows][C][3][4] = dx, dy, correct, valid; slots of symmetries not asked for are not written
  int32_t* base;           // optional int32 [n_rows][2]: the dense pair of the row's own grid
  uint32_t mirrors;        // the symmetries asked for (ARCLE_MIRROR_*)
  int32_t blank;           // 1: Paste writes the clip's whole rectangle (paste_blank); 0: its positive cells only
};

ARCLE_DEV void mirror_emit(const MirrorParams& x, int lane, int row, int k, int s, int dx, int dy, int correct, int valid) {
  if (lane == 0) {
    U4 v;
    v[0] = (uint32_t)dx;
    v[1] = (uint32_t)dy;
    v[2] = (uint32_t)correct;
    v[3] = (uint32_t)valid;
    xl::store_at(x.mirror + ((size_t)row * (size_t)x.max_comp) * (4 * MIRROR_SLOTS), (uint32_t)(k * MIRROR_SLOTS + s) * 16u, v);
  }
}

// the byte of cell `cell` (< 1024) of a plane held 16 bytes per lane, fetched across the wave
ARCLE_DEV int mirror_byte(const U4& v, int cell) {
  const int l = (cell >> 4) & 63;
  U4 f;
  f[0] = xl::shfl(v[0], l);
  f[1] = xl::shfl(v[1], l);
  f[2] = xl::shfl(v[2], l);
  f[3] = xl::shfl(v[3], l);
  return (int)(int8_t)u4_byte(f, cell & 15);
}

template <int FW>
ARCLE_DEV void wave_mirror_row(const MirrorParams& x, WaveLDS* lds, const U2* lut, int row, int lane) {
  const StepParams& p = x.p;
  Wave w(p, lds, lut, lane, INGRESS_BBOX, FW, false, false, false);
  const int C = x.max_comp;
  const uint32_t mirrors = x.mirrors;
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
    for (int k = 0; k < n; k++)
      for (int s = 0; s < MIRROR_SLOTS; s++)
        if ((mirrors >> s) & 1u) mirror_emit(x, lane, row, k, s, 0, 0, 0, 0);
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
  const int D = x.max_dist;
  const uint8_t* brow = x.bits + (size_t)row * (size_t)C * ARCLE_BITS_STRIDE;

  if (FW != FW_GENERIC || (p.W <= 32 && p.H <= 64)) {
    // ROW BOARD
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
    const uint32_t Wb = (uint32_t)p.W;
    const uint32_t K0 = rows_from16(w, K0_16, Wb), AZ = rows_from16(w, AZ16, Wb), GP = rows_from16(w, pos16g, Wb);
    uint32_t Gb[MIRROR_PLANES], Ab[MIRROR_PLANES];
#pragma unroll
    for (int b = 0; b < MIRROR_PLANES; b++) {
      Gb[b] = Ab[b] = 0u;
      if ((used >> b) & 1u) {
        Gb[b] = rows_from16(w, plane16(grid, b), Wb) & GP;
        Ab[b] = rows_from16(w, plane16(ans, b), Wb);
      }
    }
    for (int k = 0; k < n; k++) {
      const uint32_t b16 = (uint32_t)*reinterpret_cast<const uint16_t*>(brow + (size_t)k * ARCLE_BITS_STRIDE + 2 * lane) & inside16;
      const uint32_t B = rows_from16(w, b16, Wb);
      const unsigned long long rowsB = xl::ballot(B != 0u);
      const uint32_t cols = xl::wave_or(B);
      if (!rowsB) {  // (wave-uniform) B empty: nothing is copied, the grid scores what it scores
        for (int s = 0; s < MIRROR_SLOTS; s++)
          if ((mirrors >> s) & 1u) mirror_emit(x, lane, row, k, s, 0, 0, base_correct, 1);
        continue;
      }
      const int x0 = __builtin_ctzll(rowsB), x1 = 63 - __builtin_clzll(rowsB);
      const int y0 = __builtin_ctz(cols), y1 = 31 - __builtin_clz(cols);
      const int h = x1 - x0 + 1, wd = y1 - y0 + 1;
      const uint32_t rect = (2u << y1) - (1u << y0);  // one row of the box
      // what the box holds right now that is right: every candidate loses it
      const int keep = base_correct - (int)xl::wave_add((lane >= x0 && lane <= x1) ? (uint32_t)__builtin_popcount(K0 & rect) : 0u);
      for (int s = 0; s < MIRROR_SLOTS; s++) {
        if (!((mirrors >> s) & 1u)) continue;  // (wave-uniform)
        const bool fh = s != 1, fv = s != 0;   // columns mirrored, rows mirrored
        const int sx0 = s == 0 ? x0 : imax(x0 - D, 0), sx1 = s == 0 ? x0 : imin(x0 + D, gh - h);
        const int sy0 = s == 1 ? y0 : imax(y0 - D, 0), sy1 = s == 1 ? y0 : imin(y0 + D, gw - wd);
        const int npy = sy1 - sy0 + 1, total = (sx1 - sx0 + 1) * npy;
        const uint32_t magic = 65536u / (uint32_t)npy + 1u;
        // (blank = 0) the box read through the mirror where it stands: what shows through where the source is not positive
        const int sh0 = 31 - y1 - y0;
        const uint32_t sr0 = (uint32_t)imax(fh ? sh0 : 0, 0), sl0 = (uint32_t)imax(fh ? -sh0 : 0, 0);
        int best = 0;
        for (int t0 = 0; t0 < total; t0 += 64) {
          const int c = t0 + lane;
          int i = (int)(((uint32_t)c * magic) >> 16);
          if (i * npy > c) i--;
          const bool in = c < total;
          const int sx = in ? sx0 + i : sx0, sy = in ? sy0 + (c - i * npy) : sy0;
          const int dx = sx - x0, dy = sy - y0;
          const int dist = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
          const bool valid = in && dist <= D;
          const int sh = fh ? 31 - y1 - sy : dy;  // in [-31, 31]
          const uint32_t sr = (uint32_t)imax(sh, 0), sl = (uint32_t)imax(-sh, 0);
          int cnt = 0;
          for (int r = x0; r <= x1; r++) {
            const uint32_t az = xl::readlane(AZ, r) & rect;
            if (!az) continue;  // (wave-uniform) no cell of this box row can come out right
            const int at = (fv ? sx + x1 - r : sx + r - x0) & 63;  // (a row of R: < gh)
            const int at0 = fv ? x0 + x1 - r : r;
            uint32_t open = 0u;  // (blank = 0) the cells whose source is not positive
            if (!blank) {
              uint32_t sp = xl::shfl(GP, at);
              if (fh) sp = xl::bfrev(sp);
              open = ~((sp >> sr) << sl);
            }
            uint32_t mism = 0;
#pragma unroll
            for (int b = 0; b < MIRROR_PLANES; b++) {
              if ((used >> b) & 1u) {
                uint32_t g = xl::shfl(Gb[b], at);
                if (fh) g = xl::bfrev(g);
                g = (g >> sr) << sl;
                if (!blank) {
                  uint32_t o = xl::readlane(Gb[b], at0);
                  if (fh) o = xl::bfrev(o);
                  g |= ((o >> sr0) << sl0) & open;
                }
                mism |= g ^ xl::readlane(Ab[b], r);
              }
            }
            cnt += __builtin_popcount(az & ~mism);
          }
          const int key = ((keep + cnt) << 20) | ((127 - dist) << 13) | ((63 - dx) << 6) | (31 - dy);
          if (valid) best = imax(best, key);
        }
        xl::lanes_converged();
        best = w.wave_max(best);
        if (best) mirror_emit(x, lane, row, k, s, 63 - ((best >> 6) & 127), 31 - (best & 63), best >> 20, 1);
        else mirror_emit(x, lane, row, k, s, 0, 0, 0, 0);
      }
    }
  } else {
    // FLAT BOARD
    const int f0 = (32 * lane) & 1023, fc = f0 - cell_row(p, f0) * p.W;  // this lane's 32 cells start in column fc
    for (int k = 0; k < n; k++) {
      const uint32_t b16 = (uint32_t)*reinterpret_cast<const uint16_t*>(brow + (size_t)k * ARCLE_BITS_STRIDE + 2 * lane) & inside16;
      const uint32_t B = to32(w, b16);
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
        for (int s = 0; s < MIRROR_SLOTS; s++)
          if ((mirrors >> s) & 1u) mirror_emit(x, lane, row, k, s, 0, 0, base_correct, 1);
        continue;
      }
      const int lf = __builtin_ctzll(lanesB), ll = 63 - __builtin_clzll(lanesB);
      const int first = 32 * lf + __builtin_ctz(xl::uniform(xl::readlane(B, lf)));
      const int last = 32 * ll + 31 - __builtin_clz(xl::uniform(xl::readlane(B, ll)));
      const int x0 = cell_row(p, first), h = cell_row(p, last) - x0 + 1;
      const int wd = y1 - y0 + 1, cells = h * wd;
      const uint32_t magic = 65536u / (uint32_t)wd + 1u;
      for (int s = 0; s < MIRROR_SLOTS; s++) {
        if (!((mirrors >> s) & 1u)) continue;  // (wave-uniform)
        const bool fh = s != 1, fv = s != 0;
        const int sx0 = s == 0 ? x0 : imax(x0 - D, 0), sx1 = s == 0 ? x0 : imin(x0 + D, gh - h);
        const int sy0 = s == 1 ? y0 : imax(y0 - D, 0), sy1 = s == 1 ? y0 : imin(y0 + D, gw - wd);
        int bc = -1, bd = 0, bdx = 0, bdy = 0;
        for (int sx = sx0; sx <= sx1; sx++) {
          for (int sy = sy0; sy <= sy1; sy++) {
            const int dx = sx - x0, dy = sy - y0;
            const int dist = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
            if (dist > D) continue;  // (wave-uniform)
            int diff = 0;
            for (int q0 = 0; q0 < cells; q0 += 64) {
              const int q = q0 + lane;
              const bool in = q < cells;
              int i = (int)(((uint32_t)q * magic) >> 16);
              if (i * wd > q) i--;
              const int j = q - i * wd;
              const int mi = fv ? h - 1 - i : i, mj = fh ? wd - 1 - j : j;  // the tile cell the mirror reads
              const int dcell = in ? (x0 + i) * p.W + y0 + j : 0;           // (cells of grid_dim: < H * W)
              const int scell = in ? (sx + mi) * p.W + sy + mj : 0;
              int nv = mirror_byte(grid, scell);
              if (!blank) {
                const int ov = mirror_byte(grid, in ? (x0 + mi) * p.W + y0 + mj : 0);
                if (nv <= 0) nv = ov;
              }
              nv = imax(nv, 0);
              const int av = mirror_byte(ans, dcell), gv = mirror_byte(grid, dcell);
              if (in && x0 + i < mh && y0 + j < mw) diff += (nv == av ? 1 : 0) - (gv == av ? 1 : 0);
            }
            xl::lanes_converged();
            // (the difference may be negative: the sum wraps modulo 2^32 and comes back as an int)
            const int c = base_correct + (int)xl::wave_add((uint32_t)diff);
            if (c > bc || (c == bc && (dist < bd || (dist == bd && (dx < bdx || (dx == bdx && dy < bdy)))))) bc = c, bd = dist, bdx = dx, bdy = dy;
          }
        }
        if (bc >= 0) mirror_emit(x, lane, row, k, s, bdx, bdy, bc, 1);
        else mirror_emit(x, lane, row, k, s, 0, 0, 0, 0);
      }
    }
  }
}

}  // namespace arcle
