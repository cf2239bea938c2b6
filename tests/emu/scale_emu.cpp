// scale_emu.cpp — the body of arcle_scale_kernel (arcle_amd/csrc/arcle_scale.h: wave_scale_row<FW, FLAT>) on the lock-step CPU emulation of
// one 64-lane wavefront.
//
// TEST INFRASTRUCTURE ONLY, like stamp_emu.cpp, whose harness (namespace xl: every cross-lane primitive is a rendezvous of 64 ucontext
// fibers; the scheduler asserts wave-uniform control flow at each) is repeated here: that file's lane_main is hard-wired to its own kernel.
//
// Built two ways: as libscale_emu.so (scale_emu_run, driven through ctypes by tests/scale.py), and with -DSCALE_EMU_MAIN as a standalone
// program that reads one dumped case from a file, runs it on buffers exactly as long as the data and prints the outputs (the sanitized
// build of tests/test_scale_emu.py).
#include <ucontext.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#define ARCLE_DEV inline
#define ARCLE_HD inline

namespace xl {
static int cur_lane;
static uint32_t exch[64];
static int sync_tag[64];
static long sync_seq[64];
static bool finished[64];
static ucontext_t sched_ctx, lane_ctx[64];
static int error_flag;

static void yield(int tag) {
  int me = cur_lane;
  sync_tag[me] = tag;
  sync_seq[me]++;
  swapcontext(&lane_ctx[me], &sched_ctx);
  cur_lane = me;
}
ARCLE_DEV uint32_t shfl(uint32_t v, int src_lane) {
  exch[cur_lane] = v;
  yield(1);
  uint32_t r = exch[src_lane & 63];
  yield(2);
  return r;
}
ARCLE_DEV unsigned long long ballot(bool b) {
  exch[cur_lane] = b ? 1u : 0u;
  yield(3);
  unsigned long long m = 0;
  for (int i = 0; i < 64; i++) m |= (unsigned long long)(exch[i] & 1u) << i;
  yield(4);
  return m;
}
ARCLE_DEV uint32_t uniform(uint32_t v) {
  exch[cur_lane] = v;
  yield(5);
  for (int i = 0; i < 64; i++)
    if (exch[i] != v) {
      if (!error_flag) fprintf(stderr, "scale_emu: xl::uniform() value differs across lanes (%u vs %u)\n", exch[i], v);
      error_flag |= 2;
    }
  yield(6);
  return v;
}
ARCLE_DEV uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) {
  return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * (sh & 3u)));
}
ARCLE_DEV void lds_fence() { yield(7); }
ARCLE_DEV void atomic_or(uint32_t* p, uint32_t v) { *p |= v; }
ARCLE_DEV int lds_idx(int i, int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }  // host memory: stay inside the tile
ARCLE_DEV uint64_t clock() { return 0; }
ARCLE_DEV uint32_t lane_prev(uint32_t v) {
  int me = cur_lane;
  uint32_t r = shfl(v, (me + 63) & 63);
  return me == 0 ? 0u : r;
}
ARCLE_DEV uint32_t lane_next(uint32_t v) {
  int me = cur_lane;
  uint32_t r = shfl(v, (me + 1) & 63);
  return me == 63 ? 0u : r;
}
template <int K>
ARCLE_DEV uint32_t row_prev(uint32_t v) {  // row_shr:K — lane j-K of the same 16-lane row, else 0
  int me = cur_lane;
  uint32_t r = shfl(v, (me - K) & 63);
  return (me & 15) < K ? 0u : r;
}
template <int K>
ARCLE_DEV uint32_t row_next(uint32_t v) {  // row_shl:K
  int me = cur_lane;
  uint32_t r = shfl(v, (me + K) & 63);
  return (me & 15) + K > 15 ? 0u : r;
}
ARCLE_DEV uint32_t readlane(uint32_t v, int lane) { return shfl(v, lane); }
ARCLE_DEV uint32_t wave_or(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v |= shfl(v, cur_lane ^ o);
  return v;
}
ARCLE_DEV uint32_t wave_add(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += shfl(v, cur_lane ^ o);
  return v;
}
ARCLE_DEV uint32_t dot4(uint32_t a, uint32_t b, uint32_t c) {
  for (int k = 0; k < 4; k++) c += ((a >> (8 * k)) & 0xffu) * ((b >> (8 * k)) & 0xffu);
  return c;
}
typedef uint32_t U4 __attribute__((vector_size(16)));
typedef uint32_t U2 __attribute__((vector_size(8)));
ARCLE_DEV U4 load16u(const int8_t* p) { U4 v; memcpy(&v, p, 16); return v; }
// wave-uniform scalar loads: every lane reads the same address
ARCLE_DEV uint32_t uload1(const void* p) { uint32_t v; memcpy(&v, p, 4); return v; }
ARCLE_DEV U2 uload2(const void* p) { U2 v; memcpy(&v, p, 8); return v; }
ARCLE_DEV U4 uload4(const void* p) { U4 v; memcpy(&v, p, 16); return v; }
ARCLE_DEV U4 load16(const int8_t* base, uint32_t off) { U4 v; memcpy(&v, base + off, 16); return v; }
ARCLE_DEV void store16(int8_t* base, uint32_t off, const U4& v) { memcpy(base + off, &v, 16); }
ARCLE_DEV void store16_nt(int8_t* base, uint32_t off, const U4& v) { store16(base, off, v); }
ARCLE_DEV void release_store_system(uint32_t* p, uint32_t v) { *p = v; }
ARCLE_DEV void wg_barrier() { yield(8); }
ARCLE_DEV void lanes_converged() { yield(9); }
ARCLE_DEV uint32_t mul24(uint32_t a, uint32_t b) { return (a & 0xffffffu) * (b & 0xffffffu); }
ARCLE_DEV uint32_t opaque(uint32_t v) { return v; }
ARCLE_DEV int rare_s(int v) { return v; }
ARCLE_DEV int rare_v(int v) { return v; }
ARCLE_DEV uint32_t tov(uint32_t x) { return x; }
ARCLE_DEV uint32_t perm_bytes(uint32_t hi, uint32_t lo, uint32_t sel) {  // v_perm_b32 for selector bytes 0..7
  const uint64_t t = ((uint64_t)hi << 32) | lo;
  uint32_t r = 0;
  for (int k = 0; k < 4; k++) r |= (uint32_t)((t >> (8 * ((sel >> (8 * k)) & 7u))) & 0xffu) << (8 * k);
  return r;
}
template <typename T>
ARCLE_DEV void store_at(void* base, uint32_t off, const T& v) { memcpy((char*)base + off, &v, sizeof(T)); }
ARCLE_DEV uint32_t bfrev(uint32_t v) {
  uint32_t r = 0;
  for (int i = 0; i < 32; i++) r |= ((v >> i) & 1u) << (31 - i);
  return r;
}
#define ARCLE_STOP_AT 0
ARCLE_DEV void sink_s(uint32_t) {}
ARCLE_DEV void own_stores_visible() {}
ARCLE_DEV void sink_v(uint32_t) {}
ARCLE_DEV void arrived(U4&, U2&, uint32_t&, U4&) {}
ARCLE_DEV void arrived3(U4&, U2&, uint32_t&) {}
}  // namespace xl

#include "../../arcle_amd/csrc/arcle_scale.h"

namespace {
const arcle::ScaleParams* g_x;
int g_row, g_fw;
char* g_stacks;
const size_t STACK = 256 * 1024;

void lane_main(int lane) {
  xl::cur_lane = lane;
  // (no LDS: the kernel neither stages a plane nor expands a mask)
  // (the three instantiations the library launches: the row board under both width classes, the flat board)
  if (g_fw) arcle::wave_scale_row<arcle::FW_FAST, false>(*g_x, nullptr, nullptr, g_row, lane);
  else if (g_x->p.W <= 32 && g_x->p.H <= 64) arcle::wave_scale_row<arcle::FW_GENERIC, false>(*g_x, nullptr, nullptr, g_row, lane);
  else arcle::wave_scale_row<arcle::FW_GENERIC, true>(*g_x, nullptr, nullptr, g_row, lane);
  xl::finished[lane] = true;
  // returning resumes uc_link (the scheduler)
}

void run_wave() {
  for (int l = 0; l < 64; l++) {
    xl::finished[l] = false;
    xl::sync_seq[l] = 0;
    xl::sync_tag[l] = 0;
    getcontext(&xl::lane_ctx[l]);
    xl::lane_ctx[l].uc_stack.ss_sp = g_stacks + (size_t)l * STACK;
    xl::lane_ctx[l].uc_stack.ss_size = STACK;
    xl::lane_ctx[l].uc_link = &xl::sched_ctx;
    makecontext(&xl::lane_ctx[l], (void (*)())lane_main, 1, l);
  }
  for (;;) {
    int alive = 0;
    for (int l = 0; l < 64; l++) {
      if (xl::finished[l]) continue;
      xl::cur_lane = l;
      swapcontext(&xl::sched_ctx, &xl::lane_ctx[l]);
      if (!xl::finished[l]) alive++;
    }
    if (!alive) break;
    // all lanes that are still running must wait at the same primitive, and none may have finished
    int tag = -1;
    long seq = -1;
    for (int l = 0; l < 64; l++) {
      if (xl::finished[l]) {
        if (!(xl::error_flag & 1)) fprintf(stderr, "scale_emu: lane %d returned while others wait at a cross-lane op (env %d)\n", l, g_row);
        xl::error_flag |= 1;
        continue;
      }
      if (tag < 0) {
        tag = xl::sync_tag[l];
        seq = xl::sync_seq[l];
      } else if (tag != xl::sync_tag[l] || seq != xl::sync_seq[l]) {
        if (!(xl::error_flag & 1)) fprintf(stderr, "scale_emu: divergent cross-lane op (lane %d tag %d vs %d, env %d)\n", l, xl::sync_tag[l], tag, g_row);
        xl::error_flag |= 1;
      }
    }
    if (xl::error_flag & 1) {  // cannot continue a diverged wave safely
      return;
    }
  }
}
}  // namespace

// fw: -1 = the instantiation the library launches (FW_FAST for 16 <= W <= 32, FW_GENERIC otherwise), 0 = FW_GENERIC at any width.
// p.n_envs = the rows, p.n_resident = the envs.  Fills the derived fields (P, PS, div_magic, nseg) like arcle_create does.
extern "C" int scale_emu_run(arcle::ScaleParams* x, int fw) {
  arcle::StepParams* p = &x->p;
  p->P = p->H * p->W;
  if (p->PS == 0) p->PS = ARCLE_DEFAULT_PLANE_STRIDE(p->P);
  p->div_magic = 65536u / (uint32_t)p->W + 1u;
  p->nseg = (p->W >= 16) ? 2 : 1 + (15 + p->W - 1) / p->W;
  if (p->P > ARCLE_MAX_CELLS || x->sources == 0u || x->sources > 3u || x->modes == 0u || x->modes > 7u) return -1;
  if (!g_stacks) g_stacks = (char*)malloc(64 * STACK);
  g_x = x;
  g_fw = fw < 0 ? (p->W >= 16 && p->W <= 32) : 0;
  xl::error_flag = 0;
  for (int row = 0; row < p->n_envs; row++) {
    g_row = row;
    run_wave();
    if (xl::error_flag & 1) return -100 - xl::error_flag;
  }
  return xl::error_flag ? -100 - xl::error_flag : 0;
}
extern "C" int scale_emu_params_size() { return (int)sizeof(arcle::ScaleParams); }

#ifdef SCALE_EMU_MAIN
// scale_emu <case file>: one case as tests/scale.py::dump_case writes it —
//   int32 hdr[14] = magic 0x5343414c, H, W, plane mask, N, M, row stride, modes, resident, byte offset of row 0, has_src, has_base,
//                   sources, outputs (bit 0: table, bit 1: bits)
//   int8 answer[N][PS] | int8 rec[N][16] | resident: int8 grid[N][PS] | int8 input[N][PS] (M <= N rows = envs 0 .. M-1)
//                                        | rows:     int8 buf[offset + (M - 1) * stride + L] (the last row ends with the buffer)
//   (has_src) int32 src[M]
// — and prints per row: (has_base) the base pair, then per source slot: its eight words, (table) its 132 table words, (bits) its nine bit
// rows in hex, one line each (77s in a slot not asked for)
#include <vector>
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t h[14];
  if (fread(h, 4, 14, f) != 14 || h[0] != 0x5343414c) return 3;
  const int H = h[1], W = h[2], N = h[4], M = h[5], stride = h[6], resident = h[8], offset = h[9];
  const int P = H * W, PS = ARCLE_DEFAULT_PLANE_STRIDE(P);
  arcle::ScaleParams x;
  memset(&x, 0, sizeof x);
  int8_t dummy = 0;
  for (int i = 0; i < ARCLE_N_PLANES - 1; i++) x.p.plane[i] = (h[3] >> i) & 1 ? &dummy : nullptr;  // (row mode tests presence only)
  x.p.H = H; x.p.W = W; x.p.n_resident = N; x.p.n_envs = M;
  // (buffers of exactly the bytes the kernel may touch: the sanitizer sees every access past a plane or a row)
  std::vector<int8_t> answer((size_t)N * PS), rec((size_t)N * 16), grid, input, buf;
  bool ok = fread(answer.data(), 1, answer.size(), f) == answer.size() && fread(rec.data(), 1, rec.size(), f) == rec.size();
  x.p.plane[ARCLE_PL_ANSWER] = answer.data();
  x.p.rec = rec.data();
  if (resident) {
    grid.resize((size_t)N * PS);
    input.resize((size_t)N * PS);
    ok = ok && fread(grid.data(), 1, grid.size(), f) == grid.size() && fread(input.data(), 1, input.size(), f) == input.size();
    x.p.plane[ARCLE_PL_GRID] = grid.data();
    x.p.plane[ARCLE_PL_INPUT] = input.data();
  } else {
    const bool clip = (h[3] >> ARCLE_PL_CLIP) & 1, o2 = (h[3] >> ARCLE_PL_SELECTED) & 1;
    const int L = 2 * P + 6 + (clip ? P + 2 : 0) + (o2 ? 4 * P + 6 : 0);
    buf.resize((size_t)offset + (size_t)(M - 1) * stride + L);
    ok = ok && fread(buf.data(), 1, buf.size(), f) == buf.size();
    x.p.rows_in = buf.data() + offset;
    x.p.rows_in_stride = stride;
  }
  std::vector<int32_t> src(h[10] ? (size_t)M : 0);
  ok = ok && fread(src.data(), 4, src.size(), f) == src.size();
  fclose(f);
  if (!ok) return 3;
  const bool has_table = h[13] & 1, has_bits = h[13] & 2;
  std::vector<int32_t> scale((size_t)M * 16, 77), base(h[11] ? 2 * (size_t)M : 0, 77), table(has_table ? (size_t)M * 2 * arcle::SCALE_CANDS : 0, 77);
  std::vector<uint16_t> bits(has_bits ? (size_t)M * 2 * 9 * (ARCLE_BITS_STRIDE / 2) : 0, 0x4d4d);  // (2-byte aligned)
  x.modes = (uint32_t)h[7]; x.sources = (uint32_t)h[12];
  x.src_env = h[10] ? src.data() : nullptr;
  x.scale = scale.data(); x.base = h[11] ? base.data() : nullptr;
  x.table = has_table ? table.data() : nullptr;
  x.bits = has_bits ? reinterpret_cast<uint8_t*>(bits.data()) : nullptr;
  const int rc = scale_emu_run(&x, -1);
  if (rc) {
    fprintf(stderr, "scale_emu: error %d\n", rc);
    return 1;
  }
  for (int m = 0; m < M; m++) {
    if (h[11]) printf("%d %d\n", base[2 * m], base[2 * m + 1]);
    for (int s = 0; s < 2; s++) {
      const int32_t* d = &scale[((size_t)m * 2 + s) * 8];
      printf("%d %d %d %d %d %d %d %d\n", d[0], d[1], d[2], d[3], d[4], d[5], d[6], d[7]);
      if (has_table) {
        for (int c = 0; c < arcle::SCALE_CANDS; c++) printf("%d ", table[((size_t)m * 2 + s) * arcle::SCALE_CANDS + c]);
        printf("\n");
      }
      if (has_bits)
        for (int c = 0; c < 9; c++) {
          const uint8_t* b = x.bits + (((size_t)m * 2 + s) * 9 + c) * ARCLE_BITS_STRIDE;
          for (int k = 0; k < ARCLE_BITS_STRIDE; k++) printf("%02x", b[k]);
          printf("\n");
        }
    }
  }
  free(g_stacks);
  return 0;
}
#endif
