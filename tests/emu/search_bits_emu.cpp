// search_bits_emu.cpp — the search kernels' bodies with bit-packed selection masks (INGRESS_BITS: arcle_search.h wave_expand_row<4, FW>,
// arcle_wave.h wave_transition_row<4, FW>) on the lock-step CPU emulation of one 64-lane wavefront.
//
// TEST INFRASTRUCTURE ONLY.  The harness (namespace xl: every cross-lane primitive a rendezvous of 64 ucontext fibers) is the one of
// search_emu.cpp, included as it stands; that file's lane_main is hard-wired to the tuple forms, so the dispatch and the scheduler
// loop that calls it are restated here for the bit rows.  run_wave below is a second copy of that file's divergence check and has to be kept
// in step with it; when search_emu.cpp is next touched, its lane_main should take the dispatch as a parameter and this copy go.
//
// Built two ways: as libsearch_bits_emu.so (search_bits_emu_run, driven through ctypes by tests/search_bits.py), and with
// -DSEARCH_BITS_EMU_MAIN as a standalone program that reads one dumped expansion case from a file, runs it and prints the outputs
// (the sanitized build of tests/test_search_bits_emu.py).
#include "search_emu.cpp"

namespace bits_emu {
const arcle::ExpandParams* b_x;
arcle::BlockLDS<1> b_lds;
int b_row, b_k0, b_k1, b_kind;
char* b_stacks;
const size_t B_STACK = 256 * 1024;

void lane_main(int lane) {
  xl::cur_lane = lane;
  const arcle::StepParams& p = b_x->p;
  arcle::lut_init(b_lds.lut, lane, 64);
  xl::wg_barrier();
  const bool fast = p.W >= 16 && p.W <= 32;  // (as the library: FW_FAST code for FW_FULL)
  if (b_kind == 0) {
    if (fast) arcle::wave_expand_row<arcle::INGRESS_BITS, arcle::FW_FAST>(*b_x, &b_lds.wave[0], b_lds.lut, b_row, b_k0, b_k1, lane);
    else arcle::wave_expand_row<arcle::INGRESS_BITS, arcle::FW_GENERIC>(*b_x, &b_lds.wave[0], b_lds.lut, b_row, b_k0, b_k1, lane);
  } else {
    if (fast) arcle::wave_transition_row<arcle::INGRESS_BITS, arcle::FW_FAST>(p, &b_lds.wave[0], b_lds.lut, b_row, lane);
    else arcle::wave_transition_row<arcle::INGRESS_BITS, arcle::FW_GENERIC>(p, &b_lds.wave[0], b_lds.lut, b_row, lane);
  }
  xl::finished[lane] = true;
}

void run_wave() {
  for (int l = 0; l < 64; l++) {
    xl::finished[l] = false;
    xl::sync_seq[l] = 0;
    xl::sync_tag[l] = 0;
    getcontext(&xl::lane_ctx[l]);
    xl::lane_ctx[l].uc_stack.ss_sp = b_stacks + (size_t)l * B_STACK;
    xl::lane_ctx[l].uc_stack.ss_size = B_STACK;
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
        if (!(xl::error_flag & 1)) fprintf(stderr, "search_bits_emu: divergent cross-lane op (lane %d, row %d)\n", l, b_row);
        xl::error_flag |= 1;
      } else if (tag < 0) {
        tag = xl::sync_tag[l];
        seq = xl::sync_seq[l];
      }
    }
    if (xl::error_flag & 1) return;  // cannot continue a diverged wave safely
  }
}
}  // namespace bits_emu

// kind 0: expand (one emulated wave per (row, chunk), as the kernel splits a row's K actions), 2: arcle_transition_rows over x->p (one
// wave per row).  p.ingress must be INGRESS_BITS.  Fills the derived fields (P, PS, div_magic, nseg) like arcle_create does.
extern "C" int search_bits_emu_run(int kind, arcle::ExpandParams* x) {
  using namespace bits_emu;
  arcle::StepParams* p = &x->p;
  p->P = p->H * p->W;
  if (p->PS == 0) p->PS = ARCLE_DEFAULT_PLANE_STRIDE(p->P);
  p->div_magic = 65536u / (uint32_t)p->W + 1u;
  p->nseg = (p->W >= 16) ? 2 : 1 + (15 + p->W - 1) / p->W;
  if ((kind != 0 && kind != 2) || p->ingress != arcle::INGRESS_BITS) return -1;
  if (kind == 0 && (x->chunk <= 0 || x->n_chunks != (x->n_actions + x->chunk - 1) / x->chunk)) return -2;
  if (!b_stacks) b_stacks = (char*)malloc(64 * B_STACK);
  b_x = x;
  b_kind = kind;
  xl::error_flag = 0;
  for (int row = 0; row < p->n_envs; row++) {
    for (int j = 0; j < (kind == 0 ? x->n_chunks : 1); j++) {
      b_row = row;
      b_k0 = j * x->chunk;
      b_k1 = b_k0 + x->chunk < x->n_actions ? b_k0 + x->chunk : x->n_actions;
      memset(&b_lds, 0xA5, sizeof b_lds);  // stale LDS must never matter
      bits_emu::run_wave();
      if (xl::error_flag & 1) return -100 - xl::error_flag;
    }
  }
  return xl::error_flag ? -100 - xl::error_flag : 0;
}
extern "C" int search_bits_emu_params_size() { return (int)sizeof(arcle::ExpandParams); }

#ifdef SEARCH_BITS_EMU_MAIN
// search_bits_emu <case file>: one expansion case as tests/search_bits.py::dump_case writes it — search_emu.cpp's format with the
// selection as bit rows:
//   int32 hdr[16] = magic 0x53454152, H, W, plane mask, n_ops, max_trial, N, M, K, ingress (4), action_row_stride, flags, row stride,
//                   has_src, has_dense, chunk
//   uint32 ops[65] | int8 answer[N][PS] | int8 rec[N][16] | int8 rows[M][stride] | uint8 sel[A][128] | int32 op[A] | int32 src[M] (has_src)
// (A = K or M * K) — and prints per child: reward term status state_hash grid_hash correct total
#include <vector>
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t h[16];
  if (fread(h, 4, 16, f) != 16 || h[0] != 0x53454152 || h[9] != arcle::INGRESS_BITS) return 3;
  const int H = h[1], W = h[2], N = h[6], M = h[7], K = h[8], ars = h[10], stride = h[12];
  const int P = H * W, PS = ARCLE_DEFAULT_PLANE_STRIDE(P), A = ars ? M * K : K;
  std::vector<uint32_t> ops(65);
  // (buffers of exactly the bytes the kernel may touch: the sanitizer sees every access past a plane, a row or the A * 128 mask bytes)
  std::vector<int8_t> answer((size_t)N * PS), rec((size_t)N * 16), rows((size_t)M * stride), dummy((size_t)PS);
  std::vector<uint8_t> sel((size_t)A * ARCLE_BITS_STRIDE);
  std::vector<int32_t> op(A), src(M);
  bool ok = fread(ops.data(), 4, 65, f) == 65 && fread(answer.data(), 1, (size_t)N * PS, f) == (size_t)N * PS &&
            fread(rec.data(), 1, rec.size(), f) == rec.size() && fread(rows.data(), 1, rows.size(), f) == rows.size() &&
            fread(sel.data(), 1, sel.size(), f) == sel.size() && fread(op.data(), 4, op.size(), f) == op.size();
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
  x.p.n_resident = N; x.p.n_envs = M; x.p.ingress = arcle::INGRESS_BITS; x.p.flags = (uint32_t)h[11];
  x.p.d_ops = ops.data();
  x.p.rows_in = rows.data(); x.p.rows_in_stride = stride;
  x.p.sel = sel.data(); x.p.op = op.data();
  x.p.task_idx = h[13] ? src.data() : nullptr;
  x.p.reward = reward.data(); x.p.term = term.data();
  x.p.dense = h[14] ? dense.data() : nullptr;
  x.p.status = &scratch;
  x.n_actions = K; x.action_row_stride = ars; x.chunk = h[15]; x.n_chunks = (K + h[15] - 1) / h[15];
  x.status_out = status.data(); x.hash = hash.data(); x.parent_hash = phash.data();
  const int rc = search_bits_emu_run(0, &x);
  if (rc) {
    fprintf(stderr, "search_bits_emu: error %d\n", rc);
    return 1;
  }
  for (size_t c = 0; c < C; c++)
    printf("%d %d %d %llu %llu %d %d\n", reward[c], term[c], status[c], (unsigned long long)hash[2 * c], (unsigned long long)hash[2 * c + 1],
           dense[2 * c], dense[2 * c + 1]);
  free(bits_emu::b_stacks);
  return 0;
}
#endif
