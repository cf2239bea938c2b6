// macro_emu.cpp — the macro expansion's wave body (arcle_search.h wave_expand_macros_row<ING, FW>, every form arcle_expand_macros
// serves: bbox, point, bit rows; both width classes) on the lock-step CPU emulation of one 64-lane wavefront.
//
// TEST INFRASTRUCTURE ONLY.  The harness (namespace xl) is the one of search_emu.cpp, included as it stands, and through it the
// headers as they are; that file's lane_main is hard-wired to its own kernels, so — as in search_bits_emu.cpp — the dispatch and the
// scheduler loop that calls it are restated here and have to be kept in step with search_emu.cpp's divergence check.
//
// Built two ways: as libmacro_emu.so (macro_emu_run, driven through ctypes by tests/macros.py), and with -DMACRO_EMU_MAIN as a standalone
// program that reads one dumped case from a file, runs it and prints the outputs (the sanitized build of tests/test_macros_emu.py).
#include "search_emu.cpp"

namespace macro_emu {
const arcle::MacroParams* m_y;
arcle::BlockLDS<1> m_lds;
int m_row, m_k0, m_k1;
char* m_stacks;
const size_t M_STACK = 256 * 1024;

#define RUN_MACROS(I, F) arcle::wave_expand_macros_row<I, F>(*m_y, &m_lds.wave[0], m_lds.lut, m_row, m_k0, m_k1, lane)

void lane_main(int lane) {
  xl::cur_lane = lane;
  const arcle::StepParams& p = m_y->x.p;
  arcle::lut_init(m_lds.lut, lane, 64);
  xl::wg_barrier();
  const int f = (p.W >= 16 && p.W <= 32) ? 1 : 0;  // (as the library: FW_FAST code for FW_FULL)
  switch (p.ingress * 2 + f) {
    case 2: RUN_MACROS(arcle::INGRESS_BBOX, arcle::FW_GENERIC); break;
    case 3: RUN_MACROS(arcle::INGRESS_BBOX, arcle::FW_FAST); break;
    case 4: RUN_MACROS(arcle::INGRESS_POINT, arcle::FW_GENERIC); break;
    case 5: RUN_MACROS(arcle::INGRESS_POINT, arcle::FW_FAST); break;
    case 8: RUN_MACROS(arcle::INGRESS_BITS, arcle::FW_GENERIC); break;
    default: RUN_MACROS(arcle::INGRESS_BITS, arcle::FW_FAST); break;
  }
  xl::finished[lane] = true;
}

void run_wave() {
  for (int l = 0; l < 64; l++) {
    xl::finished[l] = false;
    xl::sync_seq[l] = 0;
    xl::sync_tag[l] = 0;
    getcontext(&xl::lane_ctx[l]);
    xl::lane_ctx[l].uc_stack.ss_sp = m_stacks + (size_t)l * M_STACK;
    xl::lane_ctx[l].uc_stack.ss_size = M_STACK;
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
      if (xl::finished[l] || (tag >= 0 && (tag != xl::sync_tag[l] || seq != xl::sync_seq[l]))) {
        if (!(xl::error_flag & 1)) fprintf(stderr, "macro_emu: divergent cross-lane op (lane %d, row %d)\n", l, m_row);
        xl::error_flag |= 1;
      } else if (tag < 0) {
        tag = xl::sync_tag[l];
        seq = xl::sync_seq[l];
      }
    }
    if (xl::error_flag & 1) return;  // cannot continue a diverged wave safely
  }
}
}  // namespace macro_emu

// One emulated wave per (row, chunk), as the kernel splits a row's K macros (y->x.chunk, y->x.n_chunks from the caller).  Fills the
// derived fields (P, PS, div_magic, nseg) like arcle_create does.
extern "C" int macro_emu_run(arcle::MacroParams* y) {
  using namespace macro_emu;
  arcle::ExpandParams* x = &y->x;
  arcle::StepParams* p = &x->p;
  p->P = p->H * p->W;
  if (p->PS == 0) p->PS = ARCLE_DEFAULT_PLANE_STRIDE(p->P);
  p->div_magic = 65536u / (uint32_t)p->W + 1u;
  p->nseg = (p->W >= 16) ? 2 : 1 + (15 + p->W - 1) / p->W;
  if (p->ingress != arcle::INGRESS_BBOX && p->ingress != arcle::INGRESS_POINT && p->ingress != arcle::INGRESS_BITS) return -1;
  if (x->chunk <= 0 || x->n_chunks != (x->n_actions + x->chunk - 1) / x->chunk || y->max_len < 1) return -2;
  if (!m_stacks) m_stacks = (char*)malloc(64 * M_STACK);
  m_y = y;
  xl::error_flag = 0;
  for (int row = 0; row < p->n_envs; row++) {
    for (int j = 0; j < x->n_chunks; j++) {
      m_row = row;
      m_k0 = j * x->chunk;
      m_k1 = m_k0 + x->chunk < x->n_actions ? m_k0 + x->chunk : x->n_actions;
      memset(&m_lds, 0xA5, sizeof m_lds);  // stale LDS must never matter
      macro_emu::run_wave();
      if (xl::error_flag & 1) return -100 - xl::error_flag;
    }
  }
  return xl::error_flag ? -100 - xl::error_flag : 0;
}
extern "C" int macro_emu_params_size() { return (int)sizeof(arcle::MacroParams); }

#ifdef MACRO_EMU_MAIN
// macro_emu <case file>: one case as tests/macros.py::dump_case writes it — search_emu.cpp's format with the macro fields:
//   int32 hdr[20] = magic 0x4D414352, H, W, plane mask, n_ops, max_trial, N, M, K, ingress, action_row_stride, flags, row stride,
//                   has_src, has_dense, chunk, T, has_len, 0, 0
//   uint32 ops[65] | int8 answer[N][PS] | int8 rec[N][16] | int8 rows[M][stride] | sel[A][T][w bytes] | int32 op[A][T] |
//   int32 len[A] (has_len) | int32 src[M] (has_src)
// (A = K or M * K; w = 16, 8 or 128 bytes) — and prints per child: reward term status state_hash grid_hash correct total
#include <vector>
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t h[20];
  if (fread(h, 4, 20, f) != 20 || h[0] != 0x4D414352) return 3;
  const int H = h[1], W = h[2], N = h[6], M = h[7], K = h[8], ing = h[9], ars = h[10], stride = h[12], T = h[16];
  const int P = H * W, PS = ARCLE_DEFAULT_PLANE_STRIDE(P), A = ars ? M * K : K;
  const size_t w = ing == arcle::INGRESS_BBOX ? 16 : ing == arcle::INGRESS_POINT ? 8 : ARCLE_BITS_STRIDE;
  std::vector<uint32_t> ops(65);
  // (buffers of exactly the bytes the kernel may touch: the sanitizer sees every access past a plane, a row, a macro's steps or lengths)
  std::vector<int8_t> answer((size_t)N * PS), rec((size_t)N * 16), rows((size_t)M * stride), dummy((size_t)PS);
  std::vector<uint8_t> sel((size_t)A * T * w);
  std::vector<int32_t> op((size_t)A * T), len(A), src(M);
  bool ok = fread(ops.data(), 4, 65, f) == 65 && fread(answer.data(), 1, answer.size(), f) == answer.size() &&
            fread(rec.data(), 1, rec.size(), f) == rec.size() && fread(rows.data(), 1, rows.size(), f) == rows.size() &&
            fread(sel.data(), 1, sel.size(), f) == sel.size() && fread(op.data(), 4, op.size(), f) == op.size();
  if (ok && h[17]) ok = fread(len.data(), 4, len.size(), f) == len.size();
  if (ok && h[13]) ok = fread(src.data(), 4, src.size(), f) == src.size();
  fclose(f);
  if (!ok) return 3;
  const size_t C = (size_t)M * K;
  std::vector<int32_t> reward(C), dense(2 * C);
  std::vector<uint8_t> term(C), status(C);
  std::vector<uint64_t> hash(2 * C), phash(2 * (size_t)M);
  uint32_t scratch = 0;
  arcle::MacroParams y;
  memset(&y, 0, sizeof y);
  arcle::ExpandParams& x = y.x;
  // (the kernel only tests the state planes' pointers for presence and reads the answer plane: the rows carry the state)
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
  y.max_len = T; y.len = h[17] ? len.data() : nullptr;
  const int rc = macro_emu_run(&y);
  if (rc) {
    fprintf(stderr, "macro_emu: error %d\n", rc);
    return 1;
  }
  for (size_t c = 0; c < C; c++)
    printf("%d %d %d %llu %llu %d %d\n", reward[c], term[c], status[c], (unsigned long long)hash[2 * c], (unsigned long long)hash[2 * c + 1],
           dense[2 * c], dense[2 * c + 1]);
  free(macro_emu::m_stacks);
  return 0;
}
#endif
