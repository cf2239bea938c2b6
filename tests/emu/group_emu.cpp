// group_emu.cpp — the deal of a self-ordering step launch (arcle_amd/csrc/arcle_group.h: arcle::group_slot, group_position, deal_group) and
// whole launches (deal + arcle::wave_step of arcle_wave.h) on the lock-step CPU emulation of one 64-lane wavefront.
//
// TEST INFRASTRUCTURE ONLY, like wave_emu.cpp, search_emu.cpp and components_emu.cpp, whose harness (namespace xl: every cross-lane
// primitive is a rendezvous of 64 ucontext fibers; the scheduler asserts wave-uniform control flow at each) is repeated here: those files'
// lane_main are hard-wired to their own kernels.
//
// What the GPU decides and a test cannot — in which order the slots of a launch run — is an ARGUMENT here: group_emu_launch runs the slots
// in a given order, each wave (deal + step) to completion before the next starts, on the launch's shared in-place buffers.  That is the
// extreme of what the hardware may do (a group's slots are chosen to start one after the other), and any interleaving in between is
// covered by the invariant it checks: the env a slot steps does not depend on what the waves before it stored.
//
// Entry points (driven through ctypes by tests/grouping.py):
//   group_emu_slots   the slot geometry of a whole launch, no lanes needed (arcle::group_slot is scalar arithmetic)
//   group_emu_trade   the trade inside one group for every position (arcle::group_position), in replay mode (see namespace xl)
//   group_emu_deal    every slot's env and extracted inputs (arcle::deal_group), no step
//   group_emu_launch  a whole step launch: slots in a given order, or the plain twin (slot i steps env i, arcle::load_inputs)
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
// ---- replay mode (group_emu_trade): straight-line code with a handful of cross-lane primitives is run lane after lane, pass after pass.
// A pass knows the 64 contributions to primitives 0 .. rp_known-1 (recorded by earlier passes) and records primitive rp_known's; a lane that
// meets a primitive not yet known gets a placeholder and its result is discarded.  The pass in which no lane met one is the wave's execution.
// Contributions recorded for OTHER arguments may be kept (the trade of one group is evaluated for 32 positions): every lane's contribution
// to a known primitive is compared with the record, and the first one that differs makes everything from there on unknown again.
static bool replay, rp_poison;
static int rp_idx, rp_known, rp_stale;
static uint32_t rp_val[16][64];
static unsigned long long rp_mask[16];
static bool rp_mask_ok[16];
static bool rp_exchange(uint32_t v, int* k) {  // true: primitive *k is known
  *k = rp_idx++;
  if (*k >= 16) { error_flag |= 4; rp_poison = true; return false; }
  if (*k < rp_known && !rp_poison) {
    if (rp_val[*k][cur_lane] == v) return true;
    if (*k < rp_stale) rp_stale = *k;
  } else if (*k == rp_known && !rp_poison) rp_val[*k][cur_lane] = v;
  rp_poison = true;
  return false;
}
// one wave-uniform evaluation of f(lane) in replay mode, keeping the first `keep` recorded primitives of the previous evaluation as candidates
template <class F>
static int rp_run(int keep, F&& f) {
  int result[64];
  rp_known = keep < rp_known ? keep : rp_known;
  for (int pass = 0; pass < 64; pass++) {
    bool poisoned = false;
    rp_stale = 16;
    for (int k = rp_known; k < 16; k++) rp_mask_ok[k] = false;
    for (int lane = 0; lane < 64; lane++) {
      cur_lane = lane;
      rp_idx = 0;
      rp_poison = false;
      result[lane] = f(lane);
      poisoned = poisoned || rp_poison;
    }
    if (!poisoned) break;
    if (error_flag) return -1;
    rp_known = rp_stale < rp_known ? rp_stale : rp_known + 1;
  }
  for (int lane = 1; lane < 64; lane++)
    if (result[lane] != result[0]) error_flag |= 2;
  return result[0];
}
ARCLE_DEV uint32_t shfl(uint32_t v, int src_lane) {
  if (replay) {
    int k;
    return rp_exchange(v, &k) ? rp_val[k][src_lane & 63] : 0u;
  }
  exch[cur_lane] = v;
  yield(1);
  uint32_t r = exch[src_lane & 63];
  yield(2);
  return r;
}
ARCLE_DEV unsigned long long ballot(bool b) {
  if (replay) {
    int k;
    if (!rp_exchange(b ? 1u : 0u, &k)) return ~0ull;
    if (!rp_mask_ok[k]) {
      rp_mask[k] = 0;
      for (int i = 0; i < 64; i++) rp_mask[k] |= (unsigned long long)(rp_val[k][i] & 1u) << i;
      rp_mask_ok[k] = true;
    }
    return rp_mask[k];
  }
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
      if (!error_flag) fprintf(stderr, "group_emu: xl::uniform() value differs across lanes (%u vs %u)\n", exch[i], v);
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
// ---- what arcle::deal_group (arcle_group.h) needs beyond the above ----
ARCLE_DEV U2 load8(const void* base, uint32_t off) { U2 v; memcpy(&v, (const char*)base + off, 8); return v; }
ARCLE_DEV uint32_t load32(const void* base, uint32_t off) { uint32_t v; memcpy(&v, (const char*)base + off, 4); return v; }
ARCLE_DEV U4 load16u_at(const void* base, uint32_t off) { U4 v; memcpy(&v, (const char*)base + off, 16); return v; }
ARCLE_DEV uint32_t quad_bcast_odd(uint32_t v) {  // DPP quad_perm [1, 1, 3, 3]: lanes 0-1 of a quad take lane 1's value, lanes 2-3 lane 3's
  int me = cur_lane;
  return shfl(v, me | 1);
}
ARCLE_DEV uint32_t umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
ARCLE_DEV uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
// v_mbcnt_lo_u32_b32: base + the mask's bits below this lane, counting lanes 0-31 only (lanes 32-63 see all 32 bits)
ARCLE_DEV uint32_t mbcnt_lo(uint32_t mask, uint32_t base) {
  return base + (uint32_t)__builtin_popcount(cur_lane < 32 ? mask & ((1u << cur_lane) - 1u) : mask);
}
ARCLE_DEV bool inverse_ballot(uint64_t mask) { return (mask >> cur_lane) & 1ull; }
ARCLE_DEV int mul24s(uint32_t s, int v) {  // v_mul_i32_i24: both operands' low 24 bits as signed numbers, low 32 bits of the product
  const int64_t a = (int32_t)(s << 8) >> 8, b = (int32_t)((uint32_t)v << 8) >> 8;
  return (int)(uint32_t)(uint64_t)(a * b);
}
ARCLE_DEV void touch_args(const void*, const void*) {}
}  // namespace xl

#include "../../arcle_amd/csrc/arcle_group.h"

namespace {
// the flag sets of the LEAN table of arcle_hip.hip that have a self-ordering twin, as compile-time constants
constexpr int HOT_FLAGS = ARCLE_STEP_AUTORESET | ARCLE_STEP_ELIDE_SELECTED;
constexpr int HOT_PACK_FLAGS = HOT_FLAGS | ARCLE_STEP_PACK_OBS;
constexpr int RESEARCH_INC_FL = ARCLE_STEP_ELIDE_SELECTED | ARCLE_STEP_TRUNCATE | ARCLE_STEP_RESAMPLE | ARCLE_STEP_DENSE | ARCLE_STEP_FLAT_OBS |
                                ARCLE_STEPX_FLAT_FILTERED | ARCLE_STEP_ROWS_INCREMENTAL;

arcle::StepParams g_p;  // the launch's parameters as the kernel sees them (its register-promoted copy with the compile-time fields set)
arcle::BlockLDS<1> g_lds;
int g_kind;             // 0: deal only, 1: deal + step, 2: plain step (slot = env)
int g_row;              // LEAN row: 0 HOT_FLAGS, 1 ELIDE_SELECTED, 2 HOT_PACK_FLAGS, 3 RESEARCH_INC_FL
uint32_t g_block, g_wave;
int g_env_out;
int32_t g_in_out[11];   // rec[4], cnt[2], op, payload[4]
char* g_stacks;
const size_t STACK = 256 * 1024;

template <int ING, int FEAT, int FL>
void run_slot(int lane) {
  // as arcle_step_kernel<ING, FW_FULL, 0, FEAT, FL | ARCLE_STEPX_GROUPED, 30>: no accounting, no expansion table
  arcle::Wave w(g_p, &g_lds.wave[0], nullptr, lane, ING, arcle::FW_FULL, false, false, false);
  arcle::StepInputs in;
  int env;
  if (g_kind == 2) {
    env = (int)(g_block * (uint32_t)g_p.wpw + g_wave);
    in = arcle::load_inputs<ING>(w, env, g_p.rec, g_p.cnt, g_p.op, g_p.sel);
  } else {
    const uint32_t tid = 64u * g_wave + (uint32_t)lane;
    const arcle::GroupSlot slot = arcle::group_slot_of_wave(g_block, tid, g_p.group_magic, (uint32_t)g_p.n_envs >> 3, (uint32_t)__builtin_ctz((unsigned)g_p.wpw));
    env = arcle::deal_group<ING>(w, slot, tid, g_p.long_mask, g_p.rec, g_p.cnt, g_p.op, g_p.sel, g_p.plane[ARCLE_PL_GRID], g_p.d_ops, in);
    if (lane == 0) {
      g_env_out = env;
      for (int k = 0; k < 4; k++) g_in_out[k] = (int32_t)in.rec[k], g_in_out[7 + k] = (int32_t)in.payload[k];
      g_in_out[4] = (int32_t)in.cnt[0], g_in_out[5] = (int32_t)in.cnt[1], g_in_out[6] = (int32_t)in.op;
    }
    if (g_kind == 0) return;
  }
  arcle::wave_step<ING, arcle::FW_FULL, 0, FEAT, FL>(w, env, in);
}

// the cells of the LEAN table's "grouped" column
template <int ING>
bool run_form(int lane) {
  constexpr bool t5 = ING == arcle::INGRESS_BBOX || ING == arcle::INGRESS_BBOX5;
  switch (g_row) {
    case 0: run_slot<ING, 0, HOT_FLAGS>(lane); return true;
    case 1: if constexpr (t5 || ING == arcle::INGRESS_POINT) return run_slot<ING, 0, (int)ARCLE_STEP_ELIDE_SELECTED>(lane), true; else return false;
    case 2: if constexpr (t5) return run_slot<ING, 0, HOT_PACK_FLAGS>(lane), true; else return false;
    case 3: if constexpr (t5) return run_slot<ING, 1, RESEARCH_INC_FL>(lane), true; else return false;
  }
  return false;
}

void lane_main(int lane) {
  xl::cur_lane = lane;
  bool ok = false;
  switch (g_p.ingress) {
    case arcle::INGRESS_MASK: ok = run_form<arcle::INGRESS_MASK>(lane); break;
    case arcle::INGRESS_BBOX: ok = run_form<arcle::INGRESS_BBOX>(lane); break;
    case arcle::INGRESS_POINT: ok = run_form<arcle::INGRESS_POINT>(lane); break;
    case arcle::INGRESS_BBOX5: ok = run_form<arcle::INGRESS_BBOX5>(lane); break;
    case arcle::INGRESS_BITS: ok = run_form<arcle::INGRESS_BITS>(lane); break;
  }
  if (!ok) xl::error_flag |= 8;  // (a cell the table does not have)
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
        if (!(xl::error_flag & 1)) fprintf(stderr, "group_emu: lane %d returned while others wait at a cross-lane op (slot %u.%u)\n", l, g_block, g_wave);
        xl::error_flag |= 1;
        continue;
      }
      if (tag < 0) {
        tag = xl::sync_tag[l];
        seq = xl::sync_seq[l];
      } else if (tag != xl::sync_tag[l] || seq != xl::sync_seq[l]) {
        if (!(xl::error_flag & 1)) fprintf(stderr, "group_emu: divergent cross-lane op (lane %d tag %d vs %d, slot %u.%u)\n", l, xl::sync_tag[l], tag, g_block, g_wave);
        xl::error_flag |= 1;
      }
    }
    if (xl::error_flag & 1) {  // cannot continue a diverged wave safely
      return;
    }
  }
}

// what a self-ordering launch needs of the batch (grouped_applies of arcle_hip.hip: whole groups on every XCD, at least two per XCD; the
// slot is rebuilt from log2 of the workgroup's waves)
bool launch_shape_ok(int n_envs, int wpw) {
  return n_envs > 0 && n_envs % (8 * ARCLE_GROUP_SIZE) == 0 && n_envs >= 16 * ARCLE_GROUP_SIZE && wpw > 0 && wpw <= 16 && !(wpw & (wpw - 1));
}
}  // namespace

// Slot geometry of a launch of n_envs envs in workgroups of wpw waves with the reciprocal `magic`: for every slot s = block * wpw + wave
// (block < n_envs / wpw) its stratum j[s] and its group's first env gfirst[s].
extern "C" int group_emu_slots(int n_envs, int wpw, uint32_t magic, uint32_t* j, uint32_t* gfirst) {
  if (!launch_shape_ok(n_envs, wpw)) return -1;
  const uint32_t lg = (uint32_t)__builtin_ctz((unsigned)wpw), nb = (uint32_t)(n_envs / wpw);
  for (uint32_t b = 0; b < nb; b++)
    for (uint32_t wv = 0; wv < (uint32_t)wpw; wv++)
      arcle::group_slot(b, 64u * wv, magic, (uint32_t)n_envs >> 3, lg, j[b * (uint32_t)wpw + wv], gfirst[b * (uint32_t)wpw + wv]);
  return 0;
}

// The trade inside n_groups groups: ops int32 [n_groups][32] -> pos int32 [n_groups][32], pos[g][js] = the position whose env position js steps.
extern "C" int group_emu_trade(int n_groups, const int32_t* ops, uint64_t long_mask, int32_t* pos) {
  xl::error_flag = 0;
  xl::replay = true;
  for (int g = 0; g < n_groups; g++)
    for (uint32_t js = 0; js < 32; js++)  // (a new group: nothing kept; a new position of the same group: all but the last primitive are candidates)
      pos[32 * g + (int)js] = xl::rp_run(js ? xl::rp_known - 1 : 0, [&](int lane) {
        return arcle::group_position((uint32_t)ops[32 * g + (lane & 31)], (uint32_t)lane, long_mask, js);  // (wave-uniform: the kernel adds it to a scalar)
      });
  xl::replay = false;
  return xl::error_flag ? -100 - xl::error_flag : 0;
}

static void kernel_params(const arcle::StepParams* p, int row) {
  // as arcle_step_kernel<..., FL, 30>: the standard grid and the flag set (with the shape of the fused rows) are compile-time constants
  static const int FLS[4] = {HOT_FLAGS, (int)ARCLE_STEP_ELIDE_SELECTED, HOT_PACK_FLAGS, RESEARCH_INC_FL};
  g_p = *p;
  g_p.H = g_p.W = 30;
  g_p.P = 900;
  g_p.PS = ARCLE_MAX_CELLS;
  g_p.div_magic = 65536u / 30u + 1u;
  g_p.nseg = 2;
  g_p.flags = (uint32_t)FLS[row] & 0xffffu;
  if (FLS[row] & ARCLE_STEP_FLAT_OBS) {
    g_p.flat_filter = 1;
    g_p.flat_tail = 0;
    g_p.flat_stride = ARCLE_ROW30_FILTERED_STRIDE;
  }
  g_row = row;
}

// mode 0: deal only (env_of_slot[s] and inputs[s][11] = rec[4], cnt[2], op, payload[4] for every slot of `order`), 1: deal + step,
// 2: the plain twin (slot s steps env s; env_of_slot / inputs untouched).  order: n_order slots s = block * wpw + wave, run one after the
// other, each wave to completion.  p: 30 x 30, plane stride 1024; wpw, group_magic and long_mask as launch_step sets them.
extern "C" int group_emu_launch(const arcle::StepParams* p, int row, int mode, const int32_t* order, int n_order, int32_t* env_of_slot, int32_t* inputs) {
  if (row < 0 || row > 3 || mode < 0 || mode > 2 || p->H != 30 || p->W != 30 || p->PS != ARCLE_MAX_CELLS) return -1;
  if (!launch_shape_ok(p->n_envs, p->wpw) || (mode != 2 && !p->group_magic)) return -1;
  if (!g_stacks) g_stacks = (char*)malloc(64 * STACK);
  kernel_params(p, row);
  g_kind = mode;
  xl::error_flag = 0;
  for (int i = 0; i < n_order; i++) {
    const int s = order[i];
    if (s < 0 || s >= p->n_envs) return -2;
    g_block = (uint32_t)s / (uint32_t)p->wpw;
    g_wave = (uint32_t)s % (uint32_t)p->wpw;
    memset(&g_lds, 0xA5, sizeof g_lds);  // stale LDS must never matter
    run_wave();
    if (xl::error_flag & 1) return -100 - xl::error_flag;
    if (mode != 2) {
      env_of_slot[s] = g_env_out;
      if (inputs) memcpy(inputs + 11 * (size_t)s, g_in_out, sizeof g_in_out);
    }
  }
  return xl::error_flag ? -100 - xl::error_flag : 0;
}
extern "C" int group_emu_params_size() { return (int)sizeof(arcle::StepParams); }
