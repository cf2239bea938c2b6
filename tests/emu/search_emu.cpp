// search_emu.cpp — the search kernels' bodies (arcle_amd/csrc/arcle_search.h: wave_expand_row, wave_hash_row) on the lock-step CPU
// emulation of one 64-lane wavefront.
//
// TEST INFRASTRUCTURE ONLY, like wave_emu.cpp, whose harness (namespace xl: every cross-lane primitive is a rendezvous of 64 ucontext
// fibers; the scheduler asserts wave-uniform control flow at each) is repeated here: that file's lane_main is hard-wired to its own
// kernels.  A shared header is a later clean-up.
//
// Built two ways: as libsearch_emu.so (search_emu_run, driven through ctypes by tests/search.py), and with -DSEARCH_EMU_MAIN as a
// standalone program that reads one dumped expansion case from a file, runs it and prints the outputs (the sanitized build of
// tests/test_search_emu.py).
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
      if (!error_flag) fprintf(stderr, "search_emu: xl::uniform() value differs across lanes (%u vs %u)\n", exch[i], v);
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

#include "../../arcle_amd/csrc/arcle_search.h"

namespace {
const arcle::ExpandParams* g_x;
arcle::BlockLDS<1> g_lds;
int g_row, g_k0, g_k1, g_kind;
char* g_stacks;
const size_t STACK = 256 * 1024;

#define RUN_EXPAND(I, F) arcle::wave_expand_row<I, F>(*g_x, &g_lds.wave[0], g_lds.lut, g_row, g_k0, g_k1, lane)

void lane_main(int lane) {
  xl::cur_lane = lane;
  const arcle::StepParams& p = g_x->p;
  arcle::lut_init(g_lds.lut, lane, 64);
  xl::wg_barrier();
  if (g_kind == 1) {
    arcle::wave_hash_row(*g_x, &g_lds.wave[0], g_lds.lut, g_row, lane);
  } else {
    const int f = (p.W >= 16 && p.W <= 32) ? 1 : 0;  // (as the library: FW_FAST code for FW_FULL)
    switch (p.ingress * 2 + f) {
      case 2: RUN_EXPAND(1, 0); break;
      case 3: RUN_EXPAND(1, 1); break;
      case 4: RUN_EXPAND(2, 0); break;
      default: RUN_EXPAND(2, 1); break;
    }
  }
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
        if (!(xl::error_flag & 1)) fprintf(stderr, "search_emu: lane %d returned while others wait at a cross-lane op (env %d)\n", l, g_row);
        xl::error_flag |= 1;
        continue;
      }
      if (tag < 0) {
        tag = xl::sync_tag[l];
        seq = xl::sync_seq[l];
      } else if (tag != xl::sync_tag[l] || seq != xl::sync_seq[l]) {
        if (!(xl::error_flag & 1)) fprintf(stderr, "search_emu: divergent cross-lane op (lane %d tag %d vs %d, env %d)\n", l, xl::sync_tag[l], tag, g_row);
        xl::error_flag |= 1;
      }
    }
    if (xl::error_flag & 1) {  // cannot continue a diverged wave safely
      return;
    }
  }
}
}  // namespace

// kind 0: expand (one emulated wave per (row, chunk) exactly as the kernel splits a row's K actions: x->chunk, x->n_chunks from the
// caller), 1: hash rows.  Fills the derived fields (P, PS, div_magic, nseg) like arcle_create does.
extern "C" int search_emu_run(int kind, arcle::ExpandParams* x) {
  arcle::StepParams* p = &x->p;
  p->P = p->H * p->W;
  if (p->PS == 0) p->PS = ARCLE_DEFAULT_PLANE_STRIDE(p->P);
  p->div_magic = 65536u / (uint32_t)p->W + 1u;
  p->nseg = (p->W >= 16) ? 2 : 1 + (15 + p->W - 1) / p->W;
  if (kind == 0 && (p->ingress != arcle::INGRESS_BBOX && p->ingress != arcle::INGRESS_POINT)) return -1;
  if (kind == 0 && (x->chunk <= 0 || x->n_chunks != (x->n_actions + x->chunk - 1) / x->chunk)) return -2;
  if (!g_stacks) g_stacks = (char*)malloc(64 * STACK);
  g_x = x;
  g_kind = kind;
  xl::error_flag = 0;
  for (int row = 0; row < p->n_envs; row++) {
    for (int j = 0; j < (kind == 0 ? x->n_chunks : 1); j++) {
      g_row = row;
      g_k0 = j * x->chunk;
      g_k1 = g_k0 + x->chunk < x->n_actions ? g_k0 + x->chunk : x->n_actions;
      memset(&g_lds, 0xA5, sizeof g_lds);  // stale LDS must never matter
      run_wave();
      if (xl::error_flag & 1) return -100 - xl::error_flag;
    }
  }
  return xl::error_flag ? -100 - xl::error_flag : 0;
}
extern "C" int search_emu_params_size() { return (int)sizeof(arcle::ExpandParams); }

#ifdef SEARCH_EMU_MAIN
// search_emu <case file>: one expansion case as tests/search.py::dump_case writes it —
//   int32 hdr[16] = magic 0x53454152, H, W, plane mask, n_ops, max_trial, N, M, K, ingress, action_row_stride, flags, row stride,
//                   has_src, has_dense, chunk
//   uint32 ops[65] | int8 answer[N][PS] | int8 rec[N][16] | int8 rows[M][stride] | int32 sel[A][4 | 2] | int32 op[A] | int32 src[M] (has_src)
// (A = K or M * K) — and prints per child: reward term status state_hash grid_hash correct total
#include <vector>
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t h[16];
  if (fread(h, 4, 16, f) != 16 || h[0] != 0x53454152) return 3;
  const int H = h[1], W = h[2], N = h[6], M = h[7], K = h[8], ing = h[9], ars = h[10], stride = h[12];
  const int P = H * W, PS = ARCLE_DEFAULT_PLANE_STRIDE(P), A = ars ? M * K : K, tw = ing == arcle::INGRESS_BBOX ? 4 : 2;
  std::vector<uint32_t> ops(65);
  // (buffers of exactly the bytes the kernel may touch: the sanitizer sees every access past a plane, a row or an action array)
  std::vector<int8_t> answer((size_t)N * PS), rec((size_t)N * 16), rows((size_t)M * stride), dummy((size_t)PS);
  std::vector<int32_t> sel((size_t)A * tw), op(A), src(M);
  bool ok = fread(ops.data(), 4, 65, f) == 65 && fread(answer.data(), 1, (size_t)N * PS, f) == (size_t)N * PS &&
            fread(rec.data(), 1, rec.size(), f) == rec.size() && fread(rows.data(), 1, rows.size(), f) == rows.size() &&
            fread(sel.data(), 4, sel.size(), f) == sel.size() && fread(op.data(), 4, op.size(), f) == op.size();
  if (ok && h[13]) ok = fread(src.data(), 4, src.size(), f) == src.size();
  fclose(f);
  if (!ok) return 3;
  const size_t C = (size_t)M * K;
  std::vector<int32_t> reward(C), dense(2 * C);
  std::vector<uint8_t> term(C), status(C);
  std::vector<uint64_t> hash(2 * C), phash(2 * (size_t)M);
  uint32_t scratch = 0;
  arcle::ExpandParams x;
  memset(&x, 0, sizeof x);
  // (the kernels only test the state planes' pointers for presence and read the answer plane: the rows carry the state)
  for (int i = 0; i < ARCLE_N_PLANES - 1; i++) x.p.plane[i] = (h[3] >> i) & 1 ? dummy.data() : nullptr;
  x.p.plane[ARCLE_PL_ANSWER] = answer.data();
  x.p.rec = rec.data();
  x.p.H = H; x.p.W = W; x.p.n_ops = h[4]; x.p.max_trial = h[5];
  x.p.n_resident = N; x.p.n_envs = M; x.p.ingress = ing; x.p.flags = (uint32_t)h[11];
  x.p.d_ops = ops.data();
  x.p.rows_in = rows.data(); x.p.rows_in_stride = stride;
  x.p.sel = sel.data(); x.p.op = op.data();
  x.p.task_idx = h[13] ? src.data() : nullptr;
  x.p.reward = reward.data(); x.p.term = term.data();
  x.p.dense = h[14] ? dense.data() : nullptr;
  x.p.status = &scratch;
  x.n_actions = K; x.action_row_stride = ars; x.chunk = h[15]; x.n_chunks = (K + h[15] - 1) / h[15];
  x.status_out = status.data(); x.hash = hash.data(); x.parent_hash = phash.data();
  const int rc = search_emu_run(0, &x);
  if (rc) {
    fprintf(stderr, "search_emu: error %d\n", rc);
    return 1;
  }
  for (size_t c = 0; c < C; c++)
    printf("%d %d %d %llu %llu %d %d\n", reward[c], term[c], status[c], (unsigned long long)hash[2 * c], (unsigned long long)hash[2 * c + 1],
           dense[2 * c], dense[2 * c + 1]);
  free(g_stacks);
  return 0;
}
#endif
