// arcle_turn.h — where each object of a state row best fits the answer AFTER A TURN (arcle_turn_rows): for every object (a bit row, as
// arcle_components_rows / arcle_objects_rows write it) and each of the five turns — Rotate 90 / 180 / 270, Flip H / V — the translation
// at which select + turn + Moves leave the most correct cells, with that count.  The third sibling: the background and `delta`
// arithmetic of arcle_place.h (the object's cells are zeroed, only positive bytes are written: seven colour planes), the scan of
// arcle_stamp.h with blank = 0 (one lane per candidate position of the tile's corner); neither file is changed.
//
//   wave_turn_row<FW>  one wavefront takes ALL objects of one row: the grid, the answer of env src_env[row] and the boards made of
//                      them are built once per row; per (object, turn) the turned tile is built on the wavefront, then a handful of
//                      AND + popcount per candidate, no step body
//
// Compiled like arcle_stamp.h: by hipcc through arcle_hip.hip and by g++ through tests/emu/turn_emu.cpp.
//
// With B the object's cells inside grid_dim, (x0, y0, x1, y1) its box of h x w cells, O the box's tile (0 outside B) and O_t the turned
// tile of h' x w' cells, the turn leaves a freshly selected object with its corner at (nx, ny): (x0, y0) for Rotate 180 and the flips,
// ((2 x0 + h - w) >> 1, (2 y0 + w - h) >> 1) for the quarter turns (object.py:186-207; the shift is the floor).  A candidate is a corner
// (px, py) = (nx + dx, ny + dy) that keeps the tile inside grid_dim, |dx| + |dy| <= max_dist.  With Kobj = (background == answer)
// inside the common rectangle — (K0 & ~B) | (Z & B), Z the answer's zero cells — and Ft the positive cells of O_t at (px, py),
//     correct(t, dx, dy) = popc(Kobj) - popc(Kobj & Ft) + popc(Ft & AZ & ~mism)
// (mism, AZ and `used` as in arcle_place.h).  The arg-max packs  correct << 20 | (127 - |dx| - |dy|) << 13 | (63 - px) << 6 | (31 - py):
// nx is fixed per (object, turn), so the order of px IS the order of dx; |dx| + |dy| <= 94 on a 64 x 32 board, and a valid key is > 0.
//
// ROW BOARD (W <= 32 and H <= 64; lane i = row i as a W-bit word).  The tile is made TILE-LOCAL first (lane i = tile row i, bit j = tile
// column j: one fetch from lane x0 + i, a shift by y0), turned in registers —
//     Flip H       bit-reverse the word, shift right by 32 - w
//     Flip V       one cross-lane fetch from lane h - 1 - i
//     Rotate 180   both
//     Rotate 90    a bit transpose: one ballot per tile column c, kept by lane w - 1 - c
//     Rotate 270   Flip V, then the transpose with column c kept by lane c
// (a quarter turn has candidates only when h <= gw <= 32: a ballot's low word holds the column) — and scanned as wave_stamp_row scans
// with blank = 0: per tile row r the wave reads the write mask's word and the planes' as wave-uniform values, each lane shifts them by
// ITS py and fetches the answer rows at ITS px + r (< gh: the tile stays inside grid_dim, so nothing wraps and nothing is cut).
// FLAT BOARD (every other shape of at most 1024 cells; lane j < 32 = cells [32j, 32j + 32)): the slow path.  The turned tile is gathered
// BYTE BY BYTE to the origin of a plane — lane l builds the bytes of cells [16l, 16l + 16): for each the source cell under the turn, its
// lane's four dwords fetched across the wave — read as boards with plane16 / to32 and shifted by px * W + py >= 0 in a wave-uniform
// loop over the candidates (the tile stays inside grid_dim: no cell changes its row by wrapping), one wave reduction per candidate.
#pragma once
#include "arcle_stamp.h"

namespace arcle {

constexpr int TURN_SLOTS = 5;  // slot t <-> bit t of `turns`: rot90, rot180, rot270, flip H, flip V
constexpr int TURN_PLANES = 7;  // bits 0 .. 6 of a positive int8

// launch parameters: p = the handle's base parameters with n_envs = the number of rows, n_resident = the handle's envs and rows_in /
// rows_in_stride = the state rows (rows_in NULL: the resident envs 0 .. n_envs-1)
struct TurnParams {
  StepParams p;
  int32_t max_comp;        // C: objects per row at most
  int32_t max_dist;        // candidates with |dx| + |dy| <= max_dist
  const int32_t* count;    // optional int32 [n_rows][2]: word 0 = the objects of the row (NULL: C)
  const uint8_t* bits;     // uint8 [n_rows][C][ARCLE_BITS_STRIDE], 2-byte aligned
  const int32_t* src_env;  // optional int32 [n_rows]: the env whose answer judges the row (NULL: env = row)
  int32_t* turn;           // int32 [n_rows][C][5][4] = dx, dy, correct, valid; slots of turns not asked for are not written
  int32_t* base;           // optional int32 [n_rows][2]: the dense pair of the row's own grid
  uint32_t turns;          // the turns asked for (ARCLE_TURN_*)
  int32_t pad_;
};

ARCLE_DEV void turn_emit(const TurnParams& x, int lane, int row, int k, int t, int dx, int dy, int correct, int valid) {
  if (lane == 0) {
    U4 v;
    v[0] = (uint32_t)dx;
    v[1] = (uint32_t)dy;
    v[2] = (uint32_t)correct;
    v[3] = (uint32_t)valid;
    xl::store_at(x.turn + ((size_t)row * (size_t)x.max_comp) * (4 * TURN_SLOTS), (uint32_t)(k * TURN_SLOTS + t) * 16u, v);
  }
}

// a board of the row board as the turned tile: lane i = row i of O_t, bit j = its column j.  X is zero outside the box.
ARCLE_DEV uint32_t turn_tile(uint32_t X, int t, int x0, int y0, int h, int w, int lane) {
  uint32_t T = xl::shfl(X, (x0 + lane) & 63) >> y0;
  if (lane >= h) T = 0u;
  if (t == 1 || t == 2 || t == 4) {  // rows upside down
    const uint32_t v = xl::shfl(T, (h - 1 - lane) & 63);
    T = lane < h ? v : 0u;
  }
  if (t == 1 || t == 3) T = xl::bfrev(T) >> (32 - w);  // columns mirrored (1 <= w <= 32)
  if (t == 0 || t == 2) {  // the transpose; h <= 32: the ballot's low word is the whole column
    uint32_t out = 0u;
    for (int c = 0; c < w; c++) {
      const uint32_t col = (uint32_t)xl::ballot(((T >> c) & 1u) != 0u);
      if (lane == (t == 0 ? w - 1 - c : c)) out = col;
    }
    T = out;
  }
  return T;
}

// the 0xff-per-byte mask of a 4-bit mask
ARCLE_DEV uint32_t bytes_of4(uint32_t m4) { return (((m4 & 15u) * 0x00204081u) & 0x01010101u) * 0xffu; }

template <int FW>
ARCLE_DEV void wave_turn_row(const TurnParams& x, WaveLDS* lds, const U2* lut, int row, int lane) {
  const StepParams& p = x.p;
  Wave w(p, lds, lut, lane, INGRESS_BBOX, FW, false, false, false);
  const int C = x.max_comp;
  const uint32_t turns = x.turns;
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
      for (int t = 0; t < TURN_SLOTS; t++)
        if ((turns >> t) & 1u) turn_emit(x, lane, row, k, t, 0, 0, 0, 0);
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
    uint32_t Gb[TURN_PLANES], Ab[TURN_PLANES];
#pragma unroll
    for (int b = 0; b < TURN_PLANES; b++) {
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
      const int totalK = (int)xl::wave_add((uint32_t)__builtin_popcount(Kobj));
      const unsigned long long rowsB = xl::ballot(B != 0u);
      const uint32_t cols = xl::wave_or(B);
      int x0 = 0, y0 = 0, h = 0, wd = 0;
      if (rowsB) {
        x0 = __builtin_ctzll(rowsB);
        y0 = __builtin_ctz(cols);
        h = 64 - __builtin_clzll(rowsB) - x0;
        wd = 32 - __builtin_clz(cols) - y0;
      }
      for (int t = 0; t < TURN_SLOTS; t++) {
        if (!((turns >> t) & 1u)) continue;  // (wave-uniform)
        if (!rowsB) {                        // B empty: nothing turns, the grid scores what it scores
          turn_emit(x, lane, row, k, t, 0, 0, base_correct, 1);
          continue;
        }
        const bool quarter = t == 0 || t == 2;
        const int th = quarter ? wd : h, tw = quarter ? h : wd;
        const int nx = quarter ? (2 * x0 + h - wd) >> 1 : x0, ny = quarter ? (2 * y0 + wd - h) >> 1 : y0;
        const int px0 = imax(nx - D, 0), px1 = imin(nx + D, gh - th);
        const int py0 = imax(ny - D, 0), py1 = imin(ny + D, gw - tw);
        if (px0 > px1 || py0 > py1) {  // the turned tile fits nowhere within max_dist
          turn_emit(x, lane, row, k, t, 0, 0, 0, 0);
          continue;
        }
        const uint32_t Ft = turn_tile(F, t, x0, y0, h, wd, lane);
        uint32_t Pt[TURN_PLANES];
#pragma unroll
        for (int b = 0; b < TURN_PLANES; b++) {
          Pt[b] = 0u;
          if ((used >> b) & 1u) Pt[b] = turn_tile(Gb[b] & F, t, x0, y0, h, wd, lane);
        }
        const int npy = py1 - py0 + 1, total = (px1 - px0 + 1) * npy;
        const uint32_t magic = 65536u / (uint32_t)npy + 1u;
        int best = 0;
        for (int t0 = 0; t0 < total; t0 += 64) {
          const int c = t0 + lane;
          int i = (int)(((uint32_t)c * magic) >> 16);
          if (i * npy > c) i--;
          const bool in = c < total;
          const int px = in ? px0 + i : px0, py = in ? py0 + (c - i * npy) : py0;
          const int dx = px - nx, dy = py - ny;
          const int dist = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
          const bool valid = in && dist <= D;
          int delta = 0;
          for (int r = 0; r < th; r++) {
            const uint32_t f = xl::readlane(Ft, r);
            if (!f) continue;  // (wave-uniform)
            const int at = (px + r) & 63;
            const uint32_t fs = f << py;
            const uint32_t kk = xl::shfl(Kobj, at), az = xl::shfl(AZ, at);
            uint32_t mism = 0;
#pragma unroll
            for (int b = 0; b < TURN_PLANES; b++) {
              if ((used >> b) & 1u) mism |= (xl::readlane(Pt[b], r) << py) ^ xl::shfl(Ab[b], at);
            }
            delta += __builtin_popcount(fs & az & ~mism) - __builtin_popcount(kk & fs);
          }
          const int key = ((totalK + delta) << 20) | ((127 - dist) << 13) | ((63 - px) << 6) | (31 - py);
          if (valid) best = imax(best, key);
        }
        xl::lanes_converged();
        best = w.wave_max(best);
        if (best) turn_emit(x, lane, row, k, t, 63 - ((best >> 6) & 127) - nx, 31 - (best & 63) - ny, best >> 20, 1);
        else turn_emit(x, lane, row, k, t, 0, 0, 0, 0);  // (the rectangle's corner nearest to (nx, ny) is still too far)
      }
    }
  } else {
    // FLAT BOARD
    const uint32_t K0 = to32(w, K0_16), Z = to32(w, Z16), AZ = to32(w, AZ16);
    uint32_t Ab[TURN_PLANES];
#pragma unroll
    for (int b = 0; b < TURN_PLANES; b++) {
      Ab[b] = 0u;
      if ((used >> b) & 1u) Ab[b] = to32(w, plane16(ans, b));
    }
    const int f0 = (32 * lane) & 1023, fc = f0 - cell_row(p, f0) * p.W;  // this lane's 32 cells start in column fc
    const int g0 = 16 * lane, gr = cell_row(p, g0), gc = g0 - gr * p.W;  // this lane's 16 bytes start at (gr, gc)
    for (int k = 0; k < n; k++) {
      const uint32_t b16 = (uint32_t)*reinterpret_cast<const uint16_t*>(brow + (size_t)k * ARCLE_BITS_STRIDE + 2 * lane) & inside16;
      const uint32_t B = to32(w, b16);
      const uint32_t Kobj = (K0 & ~B) | (Z & B);
      const int totalK = (int)xl::wave_add((uint32_t)__builtin_popcount(Kobj));
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
      int x0 = 0, h = 0;
      if (lanesB) {
        const int lf = __builtin_ctzll(lanesB), ll = 63 - __builtin_clzll(lanesB);
        const int first = 32 * lf + __builtin_ctz(xl::uniform(xl::readlane(B, lf)));
        const int last = 32 * ll + 31 - __builtin_clz(xl::uniform(xl::readlane(B, ll)));
        x0 = cell_row(p, first);
        h = cell_row(p, last) - x0 + 1;
      }
      const int wd = y1 - y0 + 1;
      // the object's positive bytes, everything else 0: what a turn carries
      const uint32_t f16 = b16 & pos16g;
      U4 ob;
#pragma unroll
      for (int q = 0; q < 4; q++) ob[q] = grid[q] & bytes_of4(f16 >> (4 * q));
      for (int t = 0; t < TURN_SLOTS; t++) {
        if (!((turns >> t) & 1u)) continue;  // (wave-uniform)
        if (!lanesB) {
          turn_emit(x, lane, row, k, t, 0, 0, base_correct, 1);
          continue;
        }
        const bool quarter = t == 0 || t == 2;
        const int th = quarter ? wd : h, tw = quarter ? h : wd;
        const int nx = quarter ? (2 * x0 + h - wd) >> 1 : x0, ny = quarter ? (2 * y0 + wd - h) >> 1 : y0;
        const int px0 = imax(nx - D, 0), px1 = imin(nx + D, gh - th);
        const int py0 = imax(ny - D, 0), py1 = imin(ny + D, gw - tw);
        if (px0 > px1 || py0 > py1) {
          turn_emit(x, lane, row, k, t, 0, 0, 0, 0);
          continue;
        }
        // the turned tile at the plane's origin, byte by byte: cell (i, j) of O_t takes O's cell (si, sj)
        U4 tile = u4_zero();
        {
          int i = gr, j = gc;
          // (one dword of the tile per trip, not unrolled: sixteen gathers in flight would cost a hundred registers)
#pragma unroll 1
          for (int qd = 0; qd < 4; qd++) {
            uint32_t d = 0u;
#pragma unroll
            for (int qb = 0; qb < 4; qb++) {
              const bool in = i < th && j < tw;
              int si = i, sj = j;
              if (t == 0) si = j, sj = wd - 1 - i;
              else if (t == 1) si = h - 1 - i, sj = wd - 1 - j;
              else if (t == 2) si = h - 1 - j, sj = i;
              else if (t == 3) sj = wd - 1 - j;
              else si = h - 1 - i;
              const int s = in ? (x0 + si) * p.W + y0 + sj : 0;  // (a cell of the box: < H * W)
              U4 v;
              v[0] = xl::shfl(ob[0], (s >> 4) & 63);
              v[1] = xl::shfl(ob[1], (s >> 4) & 63);
              v[2] = xl::shfl(ob[2], (s >> 4) & 63);
              v[3] = xl::shfl(ob[3], (s >> 4) & 63);
              if (in) d |= u4_byte(v, s & 15) << (8 * qb);
              if (++j == p.W) j = 0, i++;
            }
            tile[0] = qd == 0 ? d : tile[0];
            tile[1] = qd == 1 ? d : tile[1];
            tile[2] = qd == 2 ? d : tile[2];
            tile[3] = qd == 3 ? d : tile[3];
          }
        }
        const uint32_t Ft = to32(w, pos16(tile));
        uint32_t Pt[TURN_PLANES];
#pragma unroll
        for (int b = 0; b < TURN_PLANES; b++) {
          Pt[b] = 0u;
          if ((used >> b) & 1u) Pt[b] = to32(w, plane16(tile, b));
        }
        int bc = -1, bd = 0, bdx = 0, bdy = 0;
        for (int px = px0; px <= px1; px++) {
          for (int py = py0; py <= py1; py++) {
            const int dx = px - nx, dy = py - ny;
            const int dist = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
            if (dist > D) continue;  // (wave-uniform)
            const int s = px * p.W + py;
            uint32_t fs = Ft, mism = 0;
            if (s > 0) fs = board_shl(w, Ft, s);
#pragma unroll
            for (int b = 0; b < TURN_PLANES; b++) {
              if ((used >> b) & 1u) {
                uint32_t o = Pt[b];
                if (s > 0) o = board_shl(w, o, s);
                mism |= o ^ Ab[b];
              }
            }
            // (the difference may be negative: the sum wraps modulo 2^32 and comes back as an int)
            const int c = totalK + (int)xl::wave_add((uint32_t)(__builtin_popcount(fs & AZ & ~mism) - __builtin_popcount(Kobj & fs)));
            if (c > bc || (c == bc && (dist < bd || (dist == bd && (dx < bdx || (dx == bdx && dy < bdy)))))) bc = c, bd = dist, bdx = dx, bdy = dy;
          }
        }
        xl::lanes_converged();
        if (bc >= 0) turn_emit(x, lane, row, k, t, bdx, bdy, bc, 1);
        else turn_emit(x, lane, row, k, t, 0, 0, 0, 0);
      }
    }
  }
}

}  // namespace arcle
