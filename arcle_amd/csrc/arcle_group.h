// arcle_group.h — the deal of a launch that orders itself (ARCLE_STEPX_GROUPED instantiations of arcle_step_kernel): from a wave's slot
// coordinates to the env it steps and that env's inputs.
//
// Compiled by hipcc for gfx950 (arcle_hip.hip) and by g++ against the lock-step wavefront emulation of tests/emu/group_emu.cpp, which runs
// the slots of a launch in any order on the CPU: everything the deal needs from the machine is an xl:: primitive.
//
// An XCD starts the workgroups of its slot range in index order, so the range falls into GS = 32 strata of G = rs / 32 consecutive slots
// that start one after the other.  Group g of the XCD = the 32 slots {g + j G, j = 0..31} (one per stratum) and the 32 CONTIGUOUS envs
// xbase + 32 g .. + 31.  Every wave of the group loads the inputs of ALL 32 envs — records, counters, tuples, op indices: one request of
// the whole wave per array, 1.4 KB — ballots which ops are object operations (m, L = popc(m)) and applies one rule inside
// the group: by default position j steps env j; the k-th object op found in a position >= L trades places with the k-th other op found
// in a position < L.
//
// INVARIANT: the permutation is computed from launch-constant inputs only — the group's 32 op indices and the op table's object-op mask,
// memory that no wave of the launch writes.  All 32 waves of a group therefore compute the same permutation whenever they start, and every
// env is stepped exactly once whatever the ops are.  (The waves DO write the records and counters they load here, in place, in wave_step's
// epilogue, and a group's slots are chosen to start one after the other: a late wave sees the other envs' post-step records and counters.
// It may only ever USE those of the env it was dealt, which nobody else touches; a classification that reads them — say, an env about to
// be re-initialised counted as long — gives late waves another permutation than early ones: one env stepped twice, another not at all, no
// fault.  tests/test_group_emu.py runs the launches slot by slot, in ascending, descending and shuffled order.)
// The slot's env is then picked out of the lanes with v_readlane: no table, no hint, no second round trip, no barrier.
// Measured (profiles/round5_experiments.txt): 8192 envs 5.37 -> 4.90 us per launch (the table form with hints: 4.93; ops dealt in the
// ideal order: 4.72); groups of 16: 5.00, of 64: 4.92; a group of 16 whose traded slots re-request their inputs (scalar loads): 5.25.
#pragma once
#include "arcle_wave.h"

#ifndef ARCLE_GROUP_SIZE
#define ARCLE_GROUP_SIZE 32  // envs (= dispatch strata) per group of a self-ordering launch
#endif

namespace arcle {

// The slot's place: its stratum j (= its position in the group) and the first env of its group.  block: the slot's workgroup of the launch;
// tid: the thread's index in the workgroup (wave tid >> 6 — a host passes 64 * wave); magic: the reciprocal of G (floor(2^32 / G) + 1; every
// slot holds an env: n_envs % 256 == 0, checked by the launcher); rs: the slots per XCD; wpw_log2: log2 of the waves per workgroup.
// (The kernel hands blockIdx.x / threadIdx.x over as they are and the shifts happen here, where they always stood: the instruction order of
// the self-ordering kernels is the one they were tuned with — profiles/group_header_codeobj.txt.)
ARCLE_DEV void group_slot(uint32_t block, uint32_t tid, uint32_t magic, uint32_t rs, uint32_t wpw_log2, uint32_t& j, uint32_t& gfirst) {
  constexpr uint32_t GS = ARCLE_GROUP_SIZE;
  static_assert(GS == 32, "the lane layout below is written for groups of 32");
  // (wave-uniform arithmetic on the vector ALUs — xl::tov — the CU's scalar unit is the short resource)
  const uint32_t vb = xl::tov(block);
  const uint32_t s_local = ((vb >> 3) << wpw_log2) + (tid >> 6);
  j = xl::umulhi(s_local, magic);  // stratum of this slot = its position in the group
  // first env of the group: xcd rs + GS (s_local - j G), G = rs / GS
  gfirst = (uint32_t)xl::mul24s(rs, (int)(vb & 7u) - (int)j) + (s_local << 5);
}
// ... of a running wave: the same, with the two values the deal indexes lanes and forms the env index with declared wave-uniform
struct GroupSlot {
  uint32_t js, gfirst, gfirst_s;  // position in the group; first env of the group, per lane and as a scalar
};
ARCLE_DEV GroupSlot group_slot_of_wave(uint32_t block, uint32_t tid, uint32_t magic, uint32_t rs, uint32_t wpw_log2) {
  uint32_t j, gfirst;
  group_slot(block, tid, magic, rs, wpw_log2, j, gfirst);
  GroupSlot s;
  s.js = xl::uniform(j), s.gfirst_s = xl::uniform(gfirst);
  s.gfirst = gfirst;
  return s;
}

// The trade: which position's env does position js step?  vop: lane e (and e + 32) holds env e's op index; long_mask: the op table's 64-bit
// object-op mask.  (The classification reads NOTHING but the op indices: see INVARIANT above.)
ARCLE_DEV int group_position(uint32_t vop, uint32_t lane, uint64_t long_mask, uint32_t js) {
  const bool lg = ((long_mask >> xl::umin(vop, 63u)) & 1ull) != 0ull;
  const uint64_t m = xl::ballot(lg) & 0xffffffffull;
  const uint64_t hi = xl::ballot(lane >= (uint32_t)__builtin_popcountll(m));  // positions >= L, as a lane compare
  const uint64_t late_long = m & hi, early_other = ~(m | hi);                 // the two sides of the trade, k-th with k-th
  const uint32_t ra = xl::mbcnt_lo((uint32_t)late_long, 0u), rb = xl::mbcnt_lo((uint32_t)early_other, 0u);
  // code: what a position is (0x40 | rank: a late object op, 0x80 | rank: an early other op, 0x100 | lane: it keeps its env); want: the code of
  // the position whose env it steps (the k-th of the other side, or itself) — found with ONE ballot, no branch
  uint32_t code = 0x100u | lane;
  code = xl::inverse_ballot(late_long) ? (0x40u | ra) : code;
  code = xl::inverse_ballot(early_other) ? (0x80u | rb) : code;
  const uint32_t want = (code & 0x100u) ? code : (code ^ 0xc0u);
  return __builtin_ctzll(xl::ballot(code == xl::readlane(want, (int)js)));
}

// The deal of one slot: the env it steps (returned) and that env's inputs (`in`).  w: the wave (mask forms fetch the env's payload through
// it); s: the slot's place; tid: the thread's index in the workgroup (lane tid & 63); long_mask: the op table's object-op mask; rec, cnt, op,
// sel: the launch's input arrays; hint_a, hint_b: argument-block fields whose fetch is issued beside the group's loads.
template <int ING>
ARCLE_DEV int deal_group(const Wave& w, const GroupSlot& s, uint32_t tid, uint64_t long_mask, const int8_t* rec, const int32_t* cnt, const int32_t* op,
                         const void* sel, const void* hint_a, const void* hint_b, StepInputs& in) {
  const uint32_t js = s.js, gfirst = s.gfirst, gfirst_s = s.gfirst_s;
  static_assert(ING != INGRESS_BBOX5_PF, "grouped launches: tuples, 5-tuple records, masks — not the record-prefetching form");
  constexpr bool REC5 = ING == INGRESS_BBOX5, CELLS = is_cells(ING);  // (masks / bit-packed masks: the payload is per cell — fetched for the slot's env once it is known)
  // the group's inputs: lanes 0-31 read the 32 op indices (the upper half repeats them); records (16 B per env), bbox tuples (16 B), point
  // tuples and counters (8 B) as ONE contiguous block per array spread over the 64 lanes — env e's item in lanes 2 e, 2 e + 1
  const uint32_t lane = tid & 63u, e = lane & 31u;
  const uint32_t vop = REC5 ? xl::load32(sel, 20u * (gfirst + e) + 16u) : xl::load32(op, (gfirst + e) << 2);
  const xl::U2 vrec = xl::load8(rec, (gfirst << 4) + (lane << 3));
  xl::U4 vsel = {0u, 0u, 0u, 0u};
  if constexpr (CELLS) {
  } else if constexpr (REC5) vsel = xl::load16u_at(sel, 20u * (gfirst + e));  // (records are only dword aligned; per lane e)
  else if constexpr (ING == INGRESS_BBOX) {
    const xl::U2 t = xl::load8(sel, (gfirst << 4) + (lane << 3));
    vsel[0] = t[0], vsel[1] = t[1];
  } else vsel[0] = xl::load32(sel, (gfirst << 3) + (lane << 2));
  xl::U2 vcnt = {0u, 0u};
  vcnt[0] = xl::load32(cnt, (gfirst << 3) + (lane << 2));
  // (the fetch of the argument block — plane bases, op table — is issued HERE, beside the loads above, not behind the wait for the group's ops)
  xl::touch_args(hint_a, hint_b);
  const int pos = group_position(vop, lane, long_mask, js);
  const int my_env = (int)gfirst_s + pos;
  // the env's scalars out of the lanes that hold them; an item that spans two lanes has its upper words moved to the even lane first (DPP),
  // so that ONE lane index serves every v_readlane of the array (no scalar index arithmetic)
  const int h = pos << 1;
  in.rec[0] = xl::readlane(vrec[0], h);
  in.rec[1] = xl::readlane(vrec[1], h);
  in.rec[2] = xl::readlane(xl::quad_bcast_odd(vrec[0]), h);
  in.rec[3] = xl::readlane(xl::quad_bcast_odd(vrec[1]), h);
  if constexpr (CELLS) {
    in.payload = load_payload(w, my_env, 0, sel);
  } else if constexpr (REC5) {
#pragma unroll
    for (int k = 0; k < 4; k++) in.payload[k] = xl::readlane(vsel[k], pos);
  } else if constexpr (ING == INGRESS_BBOX) {
    in.payload[0] = xl::readlane(vsel[0], h);
    in.payload[1] = xl::readlane(vsel[1], h);
    in.payload[2] = xl::readlane(xl::quad_bcast_odd(vsel[0]), h);
    in.payload[3] = xl::readlane(xl::quad_bcast_odd(vsel[1]), h);
  } else {
    in.payload = u4_zero();
    in.payload[0] = xl::readlane(vsel[0], h);
    in.payload[1] = xl::readlane(xl::quad_bcast_odd(vsel[0]), h);
  }
  in.cnt[0] = xl::readlane(vcnt[0], h);
  in.cnt[1] = xl::readlane(xl::quad_bcast_odd(vcnt[0]), h);
  in.op = xl::readlane(vop, pos);
  return my_env;
}

}  // namespace arcle
