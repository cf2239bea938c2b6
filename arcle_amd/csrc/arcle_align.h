// arcle_align.h — the offset at which the grid or the input of a state row best fits the ANSWER'S CANVAS (arcle_align_rows): for each
// source asked for (the row's grid: Copy_O; the row's input: Copy_I) the offset (ox, oy) at which Copy + resize_grid to answer_dim +
// Paste — copy the source's rectangle that the canvas covers at that offset, resize the grid to the answer's dims, paste the clip — leaves
// the most correct cells, with that count.  The only sibling that changes grid_dim: the child's dims ARE the answer's, so its dense
// pair is (correct, ah * aw).  It takes over the layout of arcle_stamp.h (bit boards, colours through eight bit planes, one lane per
// candidate, AND + popcount) and uses its helpers (plane16 of arcle_place.h); nothing of the sibling headers is changed.
//
//   wave_align_row<FW>  one wavefront takes one row: the answer of env src_env[row], its bit planes and the canvas mask are built once
//                       per row, per source its planes; per offset and canvas row one XOR per plane and one popcount, no step body
//
// Compiled like arcle_stamp.h: by hipcc through arcle_hip.hip and by g++ through tests/emu/align_emu.cpp.
//
// With S the source plane, (sh, sw) its dims and (ah, aw) the answer's, Copy clips S's rectangle R = [max(ox, 0), min(sh, ah + ox)) x
// [max(oy, 0), min(sw, aw + oy)) (object.py:291-312; Copy_I: critical.py:39-46), resize_grid leaves an all-zero ah x aw grid, and Paste
// at P = (max(-ox, 0), max(-oy, 0)) writes the clip there, cut at the plane (object.py:340-348) — its whole rectangle (blank = 1) or its
// positive cells only (blank = 0).  The child on the canvas [0, ah) x [0, aw) is therefore
//     G'[i, j] = S[i + ox, j + oy]  where (i + ox, j + oy) lies inside (sh, sw) (blank = 0: and that byte is > 0), else 0
// and correct(ox, oy) = popc(canvas & AZ & ~mism), mism = the OR over the used bit planes of (source plane shifted by (-ox, -oy) XOR
// answer plane).  The source planes are masked to (sh, sw) (blank = 0: and to the positive cells) BEFORE any shift: bytes outside the
// source's dims are never read as anything but 0, and a canvas cell no source cell lands on carries 0 in every plane, so it matches
// exactly where the answer is 0.  `used` = the OR of the bytes of the sources asked for (blank = 1: every byte, negative ones are
// pasted too, bit 7 is a plane; blank = 0: the positive bytes) — ONE set for both sources: a plane one source has no bit in is all zero
// for it, and XOR against the answer's plane then says what AZ would have said.  AZ = the canvas cells whose answer byte has no bit
// outside `used`.  Eight statically indexed plane slots under wave-uniform branches: registers.
//
// ROW BOARD (W <= 32 and H <= 64; lane i = row i as a W-bit word): ONE LANE PER OFFSET, 64 per pass over the rectangle (-ah, sh) x
// (-aw, sw) cut to the max_dist box; a lane outside the |ox| + |oy| diamond sits the pass out.  Per canvas row i (wave-uniform) the
// canvas & AZ word and the answer planes' words come by readlane; each lane fetches source row i + ITS ox (ds_bpermute) and zeroes it
// when i + ox is outside [0, H): the lane index of the fetch wraps modulo 64 and would name a real row (the trap arcle_stamp.h
// documents).  It then shifts by ITS oy — right for oy > 0, left otherwise — so bits pushed past column aw - 1 meet the canvas mask and
// bits pushed past bit 31 are gone.  The arg-max packs
//     correct << 20 | (127 - |ox| - |oy|) << 13 | (63 - ox) << 6 | (31 - oy)
// — correct <= 1024 in bits 20-30, |ox| + |oy| <= 63 + 31 in seven bits, 63 - ox in [0, 126] in seven bits (ox spans -63 .. 63),
// 31 - oy in [0, 62] in six bits (oy spans -31 .. 31): 31 bits, a positive int whose order IS the tie rule (more correct, then nearer,
// then the smaller ox, then the smaller oy).  The fields of arcle_place.h's key are wide enough for these ranges; only the decoding
// differs (no box corner is added).
// FLAT BOARD (every other shape of at most 1024 cells; lane j < 32 = cells [32j, 32j + 32)): a wave-uniform loop over the offsets, each
// a flat shift by ox * W + oy towards the lower cells.  The source is cut to R BEFORE the shift: a column outside [max(oy, 0), aw + oy)
// would cross a row end and land in the neighbouring canvas row.  The slow path: checked for its answers.
#pragma once
#include "arcle_stamp.h"

namespace arcle {

// launch parameters: p = the handle's base parameters with n_envs = the number of rows, n_resident = the handle's envs and rows_in /
// rows_in_stride = the state rows (rows_in NULL: the resident envs 0 .. n_envs-1)
struct AlignParams {
  StepParams p;
  int32_t max_dist;        // offsets with |ox| + |oy| <= max_dist
  uint32_t sources;        // ARCLE_ALIGN_GRID | ARCLE_ALIGN_INPUT
  const int32_t* src_env;  // optional int32 [n_rows]: the env whose answer judges the row (NULL: env = row)
  int32_t* align;          // int32 [n_rows][2][8] = ox, oy, correct, total, sh, sw, ah, aw; slot 0 the grid, slot 1 the input
  int32_t* base;           // optional int32 [n_rows][2]: the dense pair of the row's own grid
  int32_t blank;           // 1: Paste writes the clip's whole rectangle (paste_blank); 0: its positive cells only
  int32_t pad_;
};

constexpr int ALIGN_PLANES = 8;  // bits 0 .. 7: with blank = 1 a negative byte is pasted like any other

struct AlignDims {
  int sh, sw, ah, aw;
};

ARCLE_DEV void align_emit(const AlignParams& x, int lane, int row, int slot, int ox, int oy, int correct, int total, const AlignDims& d) {
  if (lane == 0) {
    U4 a, b;
    a[0] = (uint32_t)ox;
    a[1] = (uint32_t)oy;
    a[2] = (uint32_t)correct;
    a[3] = (uint32_t)total;
    b[0] = (uint32_t)d.sh;
    b[1] = (uint32_t)d.sw;
    b[2] = (uint32_t)d.ah;
    b[3] = (uint32_t)d.aw;
    xl::store_at(x.align + (size_t)row * 16, (uint32_t)slot * 32u, a);
    xl::store_at(x.align + (size_t)row * 16, (uint32_t)slot * 32u + 16u, b);
  }
}

// a dim byte as the reference holds it (int8), never below 0
ARCLE_DEV int align_dim(int v, int cap) { return imin(imax((int)(int8_t)(uint8_t)v, 0), cap); }

// the source's cells that a paste can carry: inside its dims, and (blank = 0) positive
ARCLE_DEV uint32_t align_cells16(const Wave& w, const U4& S, const AlignDims& d, bool blank) {
  const uint32_t in16 = w.rect16(0, d.sh - 1, 0, d.sw - 1);
  return blank ? in16 : (in16 & pos16(S));
}

// ROW BOARD, one source: CZ = canvas & AZ, Ab = the answer's planes, all as row words
ARCLE_DEV void align_rows_source(const AlignParams& x, const Wave& w, int lane, int row, int slot, const U4& S, const AlignDims& d, uint32_t used,
                                 uint32_t CZ, const uint32_t (&Ab)[ALIGN_PLANES], bool blank) {
  const StepParams& p = x.p;
  if (d.sh < 1 || d.sw < 1 || d.ah < 1 || d.aw < 1) {  // no candidate (wave-uniform)
    align_emit(x, lane, row, slot, 0, 0, 0, 0, d);
    return;
  }
  const uint32_t Wb = (uint32_t)p.W;
  const uint32_t m16 = align_cells16(w, S, d, blank);
  uint32_t Sb[ALIGN_PLANES];
#pragma unroll
  for (int b = 0; b < ALIGN_PLANES; b++) {
    Sb[b] = 0u;
    if ((used >> b) & 1u) Sb[b] = rows_from16(w, plane16(S, b) & m16, Wb);
  }
  const int D = x.max_dist;
  const int ox0 = imax(1 - d.ah, -D), ox1 = imin(d.sh - 1, D);
  const int oy0 = imax(1 - d.aw, -D), oy1 = imin(d.sw - 1, D);
  const int ny = oy1 - oy0 + 1, total = (ox1 - ox0 + 1) * ny;
  const uint32_t magic = 65536u / (uint32_t)ny + 1u;  // (t < 127 * 63: the quotient is off by one at most, corrected below)
  int best = 0;
  for (int t0 = 0; t0 < total; t0 += 64) {
    const int t = t0 + lane;
    int i = (int)(((uint32_t)t * magic) >> 16);
    if (i * ny > t) i--;
    const int ox = ox0 + i, oy = oy0 + (t - i * ny);
    const int dist = (ox < 0 ? -ox : ox) + (oy < 0 ? -oy : oy);
    const bool valid = t < total && dist <= D;
    const uint32_t sr = (uint32_t)imax(oy, 0) & 31u, sl = (uint32_t)imax(-oy, 0) & 31u;
    int cnt = 0;
    for (int r = 0; r < d.ah; r++) {
      const uint32_t cz = xl::readlane(CZ, r);
      if (!cz) continue;  // (wave-uniform)
      const int at = r + ox;
      // a source row outside the plane is no row (and `at & 63` would name a real one)
      const bool there = at >= 0 && at < p.H;
      uint32_t mism = 0;
#pragma unroll
      for (int b = 0; b < ALIGN_PLANES; b++) {
        if ((used >> b) & 1u) {
          uint32_t sv = xl::shfl(Sb[b], at & 63);
          sv = there ? sv : 0u;
          mism |= ((sv >> sr) << sl) ^ xl::readlane(Ab[b], r);
        }
      }
      cnt += __builtin_popcount(cz & ~mism);
    }
    const int key = (cnt << 20) | ((127 - dist) << 13) | ((63 - ox) << 6) | (31 - oy);
    if (valid) best = imax(best, key);
  }
  xl::lanes_converged();
  best = w.wave_max(best);
  align_emit(x, lane, row, slot, 63 - ((best >> 6) & 127), 31 - (best & 63), best >> 20, d.ah * d.aw, d);
}

// FLAT BOARD, one source: CZ and Ab as 32-cell words
ARCLE_DEV void align_flat_source(const AlignParams& x, const Wave& w, int lane, int row, int slot, const U4& S, const AlignDims& d, uint32_t used,
                                 uint32_t CZ, const uint32_t (&Ab)[ALIGN_PLANES], bool blank) {
  const StepParams& p = x.p;
  if (d.sh < 1 || d.sw < 1 || d.ah < 1 || d.aw < 1) {  // no candidate (wave-uniform)
    align_emit(x, lane, row, slot, 0, 0, 0, 0, d);
    return;
  }
  const uint32_t m16 = align_cells16(w, S, d, blank);
  uint32_t Sb[ALIGN_PLANES];
#pragma unroll
  for (int b = 0; b < ALIGN_PLANES; b++) {
    Sb[b] = 0u;
    if ((used >> b) & 1u) Sb[b] = to32(w, plane16(S, b) & m16);
  }
  const int D = x.max_dist;
  const int ox0 = imax(1 - d.ah, -D), ox1 = imin(d.sh - 1, D);
  const int oy0 = imax(1 - d.aw, -D), oy1 = imin(d.sw - 1, D);
  int bc = -1, bd = 0, box = 0, boy = 0;
  for (int oy = oy0; oy <= oy1; oy++) {
    for (int ox = ox0; ox <= ox1; ox++) {
      const int dist = (ox < 0 ? -ox : ox) + (oy < 0 ? -oy : oy);
      if (dist > D) continue;  // (wave-uniform)
      // R: the source cells the canvas covers at this offset — cut BEFORE the shift, which would carry the other columns into the
      // neighbouring canvas row
      const uint32_t keep = to32(w, w.rect16(imax(ox, 0), imin(d.sh, d.ah + ox) - 1, imax(oy, 0), imin(d.sw, d.aw + oy) - 1));
      const int s = ox * p.W + oy;
      uint32_t mism = 0;
#pragma unroll
      for (int b = 0; b < ALIGN_PLANES; b++) {
        if ((used >> b) & 1u) {
          uint32_t sv = Sb[b] & keep;
          if (s > 0) sv = board_shr(w, sv, s);
          else if (s < 0) sv = board_shl(w, sv, -s);
          mism |= sv ^ Ab[b];
        }
      }
      const int c = (int)xl::wave_add((uint32_t)__builtin_popcount(CZ & ~mism));
      if (c > bc || (c == bc && (dist < bd || (dist == bd && (ox < box || (ox == box && oy < boy)))))) bc = c, bd = dist, box = ox, boy = oy;
    }
  }
  xl::lanes_converged();
  align_emit(x, lane, row, slot, box, boy, bc, d.ah * d.aw, d);
}

template <int FW>
ARCLE_DEV void wave_align_row(const AlignParams& x, WaveLDS* lds, const U2* lut, int row, int lane) {
  const StepParams& p = x.p;
  Wave w(p, lds, lut, lane, INGRESS_BBOX, FW, false, false, false);
  const bool blank = x.blank != 0;
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
    if (want_g) align_emit(x, lane, row, 0, 0, 0, 0, 0, z);
    if (want_i) align_emit(x, lane, row, 1, 0, 0, 0, 0, z);
    return;
  }
  // the grid plane and grid_dim (always: `base` is the grid's), the input plane and input_dim when asked for, the answer plane and
  // answer_dim: as wave_place_row reads them
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
  // the bits of the bytes a paste can write, of both sources asked for: the planes a colour comparison needs
  uint32_t ub = 0;
  if (blank) {
    if (want_g) ub |= grid[0] | grid[1] | grid[2] | grid[3];
    if (want_i) ub |= inp[0] | inp[1] | inp[2] | inp[3];
  } else {
    if (want_g) {
      const U4 pb = posbytes(grid);
      ub |= (grid[0] & pb[0]) | (grid[1] & pb[1]) | (grid[2] & pb[2]) | (grid[3] & pb[3]);
    }
    if (want_i) {
      const U4 pb = posbytes(inp);
      ub |= (inp[0] & pb[0]) | (inp[1] & pb[1]) | (inp[2] & pb[2]) | (inp[3] & pb[3]);
    }
  }
  ub |= ub >> 16;
  ub |= ub >> 8;
  const uint32_t used = xl::wave_or(ub & (blank ? 0xffu : 0x7fu));
  const uint32_t unused4 = (~used & 0xffu) * 0x01010101u;
  // canvas & AZ: the canvas cells whose answer byte has no bit outside `used`
  const uint32_t CZ16 = (flags16(nzflags(ans[0] & unused4), nzflags(ans[1] & unused4), nzflags(ans[2] & unused4), nzflags(ans[3] & unused4)) ^ 0xffffu) &
                        w.rect16(0, dg.ah - 1, 0, dg.aw - 1);
  uint32_t Ab[ALIGN_PLANES];
  if (FW != FW_GENERIC || (p.W <= 32 && p.H <= 64)) {
    // ROW BOARD
    const uint32_t Wb = (uint32_t)p.W;
    const uint32_t CZ = rows_from16(w, CZ16, Wb);
#pragma unroll
    for (int b = 0; b < ALIGN_PLANES; b++) {
      Ab[b] = 0u;
      if ((used >> b) & 1u) Ab[b] = rows_from16(w, plane16(ans, b), Wb);
    }
    if (want_g) align_rows_source(x, w, lane, row, 0, grid, dg, used, CZ, Ab, blank);
    if (want_i) align_rows_source(x, w, lane, row, 1, inp, di, used, CZ, Ab, blank);
  } else {
    // FLAT BOARD
    const uint32_t CZ = to32(w, CZ16);
#pragma unroll
    for (int b = 0; b < ALIGN_PLANES; b++) {
      Ab[b] = 0u;
      if ((used >> b) & 1u) Ab[b] = to32(w, plane16(ans, b));
    }
    if (want_g) align_flat_source(x, w, lane, row, 0, grid, dg, used, CZ, Ab, blank);
    if (want_i) align_flat_source(x, w, lane, row, 1, inp, di, used, CZ, Ab, blank);
  }
}

}  // namespace arcle
