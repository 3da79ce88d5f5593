// c4_session.hip -- GPU-resident batched MCTS self-play for Connect Four on MI355X (gfx950),
// behind the C ABI of include/c4a0_hip.h.
//
// Replaces the reference's CPU loop (rust/src/self_play.rs + mcts.rs + c4r.rs): G games stay
// resident in HBM and advance in lock-step, one MCTS simulation per game per `c4_session_step`
// (plus a second one in the same launch when the leaf just selected is terminal and so needs no
// evaluator).
//
// Mapping to the hardware
//   * one game  <-> one 8-lane group of a wave64 (lanes 0..6 = the 7 children of a node,
//     lane 7 = bookkeeping); 8 games per wavefront, one wavefront per workgroup so that a
//     launch of G games spreads over G/8 workgroups (G = 4096 -> 512 workgroups on 256 CUs).
//   * tree node storage = "children blocks": the 7 children of an expanded node live in ONE
//     128-byte, 128-byte-aligned block {n, q_penalty, q_no_penalty, prior} x 7 + seven 16-bit
//     child links, so one select level is one cache line read by one 16-byte load per lane, the
//     child link needed for the next level arrives with it, and a backup touches one sector.
//   * no parent links: select records the root->leaf path in the slot state and the next
//     step's backup walks that list with independent loads (no pointer chase).
//   * positions are not stored in nodes: select replays make_move from the root position.
//   * arenas are bump-allocated per slot and never compacted: 288 GB of HBM holds the worst
//     case (43 * n_mcts_iterations blocks per game) for thousands of games.
//
// Bit-exactness: f32 arithmetic follows the reference operation by operation; this file is
// compiled with -ffp-contract=off (see build.py) and uses the glibc expf/logf ports.
//
// This file: the step kernel family (everything step_body calls, bar the layout and the lane-group primitives of c4_tree.hpp) and
// the session itself -- create / destroy, games, bindings, settings, start, the step launches, counters, progress.  Beside it:
// c4_session_maint.hip (tail compaction, arena reclaim), c4_session_callback.hip (unique leaves for an evaluator outside the
// device), c4_session_readout.hip (records, root statistics, hold snapshot) and c4_elementwise.hip (the parity kernels).
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/c4a0_hip.h"
#include "c4_device.hpp"
#include "c4_head_out.hpp"
#include "c4_host.hpp"
#include "c4_session_impl.hpp"
#include "c4_timeline.hpp"
#include "c4_tree.hpp"

#pragma clang fp contract(off)

namespace {

constexpr uint32_t kWavesPerTimingHelper = 1024;   // stamps one timing helper workgroup reduces

// Diagnostic build only (-DC4_PHASE_STAMPS, tools/phase_profile.py): per-wavefront device-clock
// stamps at the phase boundaries of the step kernel.  `force` makes the stamp wait for the values
// the phase produced.  Never compiled into libc4a0_hip.so.
#ifdef C4_PHASE_STAMPS
#define C4_STAMP(i, force)                                                                          \
  do {                                                                                              \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                       \
    if (lane == 0) p.phase[(size_t)wave_index * 16 + (i)] = __builtin_amdgcn_s_memrealtime() + ((force) & 0);  \
  } while (0)
// stamp by whichever lane is active first (second trip of the simulation loop: lane 0's game may have left it)
#define C4_STAMP_ANY(i)                                                                             \
  do {                                                                                              \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                                       \
    if (lane == (uint32_t)(__ffsll((long long)__ballot(1)) - 1)) p.phase[(size_t)wave_index * 16 + (i)] = __builtin_amdgcn_s_memrealtime();  \
  } while (0)
#else
#define C4_STAMP(i, force) do { } while (0)
#define C4_STAMP_ANY(i) do { } while (0)
#endif

// ------------------------------------------------------------------------------------------
// Evaluation cache (extension, off by default): evaluator outputs keyed by position.
// Entry = 16 dwords: [0..1] mask, [2..3] value, [4..10] the 7 policy outputs, [11..12] the 2 values,
// [13] seal, [14..15] 0.  Lane `sub` of a game's group owns dwords 2 sub, 2 sub + 1, so an entry is
// read and written by ONE 8-byte-per-lane instruction.  The seal makes the XOR of all 16 dwords a
// constant: an empty (zeroed) or torn entry never validates.  Direct-mapped, always overwritten.
// ------------------------------------------------------------------------------------------
constexpr uint32_t kCacheMagic = 0xC4A0C4A0u;
C4_DEV uint32_t cache_index(uint64_t mask, uint64_t value, uint32_t cache_mask) {
  const uint64_t h = (mask * 0x9E3779B97F4A7C15ull) ^ (value * 0xC2B2AE3D27D4EB4Full);
  return (uint32_t)(h >> 24) & cache_mask;
}

// Evaluation cache, lane-group side (entry layout at kCacheMagic).  `logit` = policy output `sub` on
// lanes 0..6; q_pen / q_nopen group-uniform.
C4_DEV void cache_store(uint2* cache, uint32_t cache_mask, uint64_t mask, uint64_t value, float logit, float q_pen,
                        float q_nopen, uint32_t sub, int gbase) {
  const uint32_t lb = __float_as_uint(logit);
  const int s2 = 2 * ((int)sub - 2);
  uint32_t a = shfl_u32(lb, gbase + (s2 < 0 ? 0 : (s2 > 6 ? 6 : s2)));
  uint32_t b = shfl_u32(lb, gbase + (s2 + 1 < 0 ? 0 : (s2 + 1 > 6 ? 6 : s2 + 1)));
  if (sub == 0) { a = (uint32_t)mask; b = (uint32_t)(mask >> 32); }
  if (sub == 1) { a = (uint32_t)value; b = (uint32_t)(value >> 32); }
  if (sub == 5) b = __float_as_uint(q_pen);
  if (sub == 6) { a = __float_as_uint(q_nopen); b = 0u; }
  if (sub == 7) { a = 0u; b = 0u; }
  uint32_t x = a ^ b;
  x ^= grp_xchg<0>(x); x ^= grp_xchg<1>(x); x ^= grp_xchg<2>(x);
  if (sub == 6) b = x ^ kCacheMagic;                               // the 16 dwords now XOR to the constant
  cache[(size_t)cache_index(mask, value, cache_mask) * 8 + sub] = make_uint2(a, b);
}
// true (for the whole group) when a valid entry for (mask, value) is present; then the outputs are set
C4_DEV bool cache_lookup(const uint2* cache, uint32_t cache_mask, uint64_t mask, uint64_t value, float& logit, float& q_pen,
                         float& q_nopen, uint32_t sub, int gbase) {
  const uint2 w = cache[(size_t)cache_index(mask, value, cache_mask) * 8 + sub];
  uint32_t x = w.x ^ w.y;
  x ^= grp_xchg<0>(x); x ^= grp_xchg<1>(x); x ^= grp_xchg<2>(x);
  const uint64_t key = ((uint64_t)w.y << 32) | w.x;
  const bool kok = sub == 0 ? key == mask : (sub == 1 ? key == value : true);
  const bool hit = x == kCacheMagic && ((__ballot(kok) >> gbase) & 0xFFull) == 0xFFull;
  if (hit) {
    const int src = gbase + (int)((4 + sub) >> 1);                   // dword 4 + sub lives in lane (4 + sub) / 2
    const uint32_t ux = shfl_u32(w.x, src), uy = shfl_u32(w.y, src);
    logit = __uint_as_float(((4 + sub) & 1u) ? uy : ux);
    q_pen = __uint_as_float(shfl_u32(w.y, gbase + 5));
    q_nopen = __uint_as_float(shfl_u32(w.x, gbase + 6));
  }
  return hit;
}

// Level `level` of the path a game's lanes hold (pv of lane 4 + j = levels j, j + 4, j + 8, j + 12),
// for every lane of the group; levels beyond the hot line come from the slot's second line.
C4_DEV uint32_t path_level(const uint4& pv, const Slot* st, uint32_t level, int gbase) {
  const uint32_t c = (level >> 2) & 3u;
  const uint32_t mine = c == 0 ? pv.x : (c == 1 ? pv.y : (c == 2 ? pv.z : pv.w));
  const uint32_t hotv = shfl_u32(mine, gbase + 4 + (int)(level & 3u));
  return level < kHotPath ? hotv : st->path_deep[level - kHotPath];
}

// ln(visit count) of uct_value (mcts.rs:379): visit counts are small integers, so the glibc logf port's
// result is read from a table filled by that same port at session creation (L1-resident: 4 bytes per
// count); counts beyond the table (reference KATs with tens of thousands of iterations) compute it.
C4_DEV float ln_visits(const Params& p, uint32_t n) {
  return n < p.n_ln ? p.ln_tab[n] : c4::c4_logf((float)n);
}

// select_new_leaf (mcts.rs:160-183) for one game on its 8 lanes: from the root down to the first
// unexpanded node, replaying make_move, recording the path (entry refs) in the lanes as the slot's
// hot line keeps it: lane 4 + j holds levels j, j + 4, j + 8, j + 12 in pv[0..3] (deeper levels go
// straight to the slot's second line).  Returns 0 or C4_ERR_NAN_IN_TREE.
C4_DEV uint32_t select_leaf(const Params& p, const Block* blocks, Slot* st, uint64_t rmask, uint64_t rvalue, uint32_t root_block,
                            uint32_t root_ref, uint32_t root_n, float c_exploration, uint32_t sub, int gbase,
                            uint64_t& leaf_mask, uint64_t& leaf_value, uint32_t& depth, uint32_t& leaf_ref,
                            uint4& pv, uint32_t& levels) {
  uint64_t m = rmask, v = rvalue;
  uint32_t blk = root_block, d = 0, last_ref = root_ref;
  float ln_np = ln_visits(p, root_n);                     // ln(parent visits) of the level being scored
  uint32_t nan_seen = 0;
  pv.x = (sub == 4) ? root_ref : pv.x;                    // level 0 of the path = the root's own entry
  while (blk != 0 && d + 1 < kMaxPath) {
    const uint4 ce = load_block_lane(blocks, blk, sub);   // {n, q_pen, q_nopen, prior} | tail
    // off the dependent chain: ln of THIS lane's child's visit count -- the parent term of the next
    // level if that child wins (lane 7 holds the tail, not an entry)
    const float my_ln = ln_visits(p, sub < 7 ? ce.x : 0u);
    const uint32_t legal = c4::legal_mask(m);
    const bool ok = sub < 7 && ((legal >> sub) & 1u);
    // uct_value (mcts.rs:359-388), computed on every lane without a branch (a lane without a legal
    // move computes on whatever it loaded and its score is never looked at); ln(1) == 0 makes every
    // first-level score -0+0
    const float nf = (float)ce.x + 1.0f;
    const float qv = __uint_as_float(ce.y) / nf;
    float ex = ln_np / nf;
    ex = __builtin_sqrtf(ex);
    ex = ex * (__uint_as_float(ce.w) + 1e-8f);
    const float cx = c_exploration * ex;
    const float score = -qv + cx;
    // max_by_key keeps the LAST maximum (mcts.rs:165-173); a NaN among two or more candidates panics
    // (utils.rs:12).  The walk finishes the level either way and reports after the loop: an errored
    // game's state is never used again.
    nan_seen |= (ok && (score != score)) ? (uint32_t)(__popc(legal) >= 2) : 0u;
    // Argmax as the maximum of a 64-bit key: high word = the score mapped monotonically onto
    // unsigned integers (-0 first folded into +0: the two compare equal as floats), low word =
    // column + 1, so equal scores go to the LAST column and a lane without a legal move (key 0)
    // never wins.  Three DPP exchanges, one 64-bit compare each.
    const uint32_t sbits = __float_as_uint(score + 0.0f);
    const uint32_t ord = sbits ^ ((uint32_t)((int32_t)sbits >> 31) | 0x80000000u);
    unsigned long long key = ok ? (((unsigned long long)ord << 32) | (sub + 1u)) : 0ull;
#define C4_KEYMAX_STEP(K)                                                                                          \
    {                                                                                                          \
      const unsigned long long o = ((unsigned long long)grp_xchg<K>((uint32_t)(key >> 32)) << 32) | grp_xchg<K>((uint32_t)key); \
      key = o > key ? o : key;                                                                                 \
    }
    C4_KEYMAX_STEP(0) C4_KEYMAX_STEP(1) C4_KEYMAX_STEP(2)
#undef C4_KEYMAX_STEP
    const uint32_t best = (uint32_t)key - 1u;
    // the winner's ln (next level's parent term) and its child link (out of the tail, lane 7)
    ln_np = shfl_f32(my_ln, gbase + (int)best);
    const uint32_t w = best >> 1;
    const uint32_t tw = w == 0 ? ce.x : (w == 1 ? ce.y : (w == 2 ? ce.z : ce.w));
    const uint32_t next_blk = (shfl_u32(tw, gbase + 7) >> (16u * (best & 1u))) & 0xFFFFu;
    c4::make_move(m, v, best);
    d += 1;
    last_ref = (blk << 3) | best;
    {                                                      // the lanes keep the path: level d on lane 4 + (d & 3)
      const bool mine = sub == 4u + (d & 3u);
      const uint32_t comp = d >> 2;
      pv.x = (mine && comp == 0) ? last_ref : pv.x;
      pv.y = (mine && comp == 1) ? last_ref : pv.y;
      pv.z = (mine && comp == 2) ? last_ref : pv.z;
      pv.w = (mine && comp == 3) ? last_ref : pv.w;
    }
    if (d >= kHotPath && sub == 0) st->path_deep[d - kHotPath] = last_ref;   // rare: beyond what the lanes hold
    blk = next_blk;
    levels += 1;
  }
  leaf_mask = m; leaf_value = v; depth = d; leaf_ref = last_ref;
  return ((__ballot(nan_seen != 0) >> gbase) & 0xFFull) ? (uint32_t)C4_ERR_NAN_IN_TREE : 0u;
}

// A game's leaf as the evaluator's input row (c4r.rs:378-392): 84 elements, plane 0 = the bits of
// `value`, plane 1 = the opponent's pieces, in bit order.  bf16: the 84-bit string value | opp << 42 is
// cut into bytes, lane `sub` expands byte `sub` (and, lanes 0..2, the bits 64..83) into eight bf16 0/1
// and writes them with one 16-byte store -- two store instructions per game instead of eleven.
template <typename PlaneT>
C4_DEV void encode_leaf(void* planes, uint32_t g, uint64_t mask, uint64_t value, uint32_t sub);
template <>
C4_DEV void encode_leaf<float>(void* planes, uint32_t g, uint64_t mask, uint64_t value, uint32_t sub) {
  for (uint32_t e = sub; e < C4_PLANES_LEN; e += 8) store_plane<float>(planes, (size_t)g * C4_PLANES_LEN + e, c4::plane_bit(mask, value, e));
}
C4_DEV uint4 bf16_bits8(uint32_t byte) {   // bit j of `byte` -> bf16 1.0 / 0.0 in element j
  uint4 r;
  r.x = ((byte >> 0) & 1u) * 0x3F80u + ((byte >> 1) & 1u) * 0x3F800000u;
  r.y = ((byte >> 2) & 1u) * 0x3F80u + ((byte >> 3) & 1u) * 0x3F800000u;
  r.z = ((byte >> 4) & 1u) * 0x3F80u + ((byte >> 5) & 1u) * 0x3F800000u;
  r.w = ((byte >> 6) & 1u) * 0x3F80u + ((byte >> 7) & 1u) * 0x3F800000u;
  return r;
}
template <>
C4_DEV void encode_leaf<uint16_t>(void* planes, uint32_t g, uint64_t mask, uint64_t value, uint32_t sub) {
  const uint64_t opp = mask & ~value;
  const uint64_t lo = value | (opp << 42);          // elements 0..63
  const uint32_t hi = (uint32_t)(opp >> 22);        // elements 64..83
  uint16_t* row = (uint16_t*)planes + (size_t)g * C4_PLANES_LEN;
  const uint4 a = bf16_bits8((uint32_t)(lo >> (8u * sub)) & 0xFFu);
  // rows are 168 bytes apart: 8-byte aligned, so the 16 bytes go out as two 8-byte stores
  reinterpret_cast<uint2*>(row + 8 * sub)[0] = make_uint2(a.x, a.y);
  reinterpret_cast<uint2*>(row + 8 * sub)[1] = make_uint2(a.z, a.w);
  if (sub < 3) {
    const uint4 b = bf16_bits8((hi >> (8u * sub)) & 0xFFu);
    reinterpret_cast<uint2*>(row + 64 + 8 * sub)[0] = make_uint2(b.x, b.y);
    if (sub < 2) reinterpret_cast<uint2*>(row + 64 + 8 * sub)[1] = make_uint2(b.z, b.w);
  }
}

// MctsGame::leaf_model_id_to_play (mcts.rs:70-76): player 0's model on even plies, player 1's on odd.
C4_DEV void publish_leaf_model(const Params& p, uint32_t g, unsigned long long ordinal, uint64_t leaf_mask) {
  if (p.leaf_models) {
    const c4_game_metadata md = p.reqs[ordinal];
    p.leaf_models[g] = (__popcll(leaf_mask) & 1) ? md.player1_id : md.player0_id;
  }
}

// Put game `ordinal` on a slot: MctsGame::new_from_pos (mcts.rs:48-56).  Called by all 8 lanes.
C4_DEV void reset_slot(const Params& p, Slot* st, Block* blocks, uint32_t sub, unsigned long long ordinal) {
  const uint64_t m = p.start_mask ? p.start_mask[ordinal] : 0ull;
  const uint64_t v = p.start_value ? p.start_value[ordinal] : 0ull;
  // block 0 holds only the root's own entry (prior 1.0, mcts.rs:49) in column 0
  reinterpret_cast<uint4*>(blocks)[sub] = make_uint4(0, 0, 0, sub == 0 ? __float_as_uint(1.0f) : 0u);
  if (sub == 0) {
    st->root_mask = m; st->root_value = v;
    st->leaf_mask = m; st->leaf_value = v;
    st->game_id = p.reqs[ordinal].game_id;
    st->ordinal = (uint32_t)ordinal;
    st->root_n = 0;
    // the start position may be anything, terminal included: full terminal_state
    st->state = slot_state(kActive, 0, 0, c4::terminal_state(m, v), 0);
    st->arena = 1;            // n_blocks = 1, root not expanded
    st->root_ref = 0;
    st->path[0] = 0;
  }
}

// ------------------------------------------------------------------------------------------
// K0: start -- the state after self_play.rs:55-58 (every slot holds a fresh game whose leaf is
// its start position) with the first leaves written to the evaluator's input tensor.
// ------------------------------------------------------------------------------------------
template <typename PlaneT>
__global__ __launch_bounds__(64) void c4_start_kernel(Params p) {
  const uint32_t sub = threadIdx.x & 7;
  const uint32_t g = blockIdx.x * (blockDim.x >> 3) + (threadIdx.x >> 3);
  if (g >= p.n_slots) return;
  Slot* st = p.slots + g;
  Block* blocks = p.blocks + (size_t)g * p.blocks_per_slot;
  uint64_t m = 0, v = 0;
  if (g < p.n_games) {
    reset_slot(p, st, blocks, sub, g);
    m = p.start_mask ? p.start_mask[g] : 0ull;
    v = p.start_value ? p.start_value[g] : 0ull;
    if (sub == 0) publish_leaf_model(p, g, g, m);
  } else if (sub == 0) {
    st->state = kIdle;
    st->ordinal = 0xFFFFFFFFu;
  }
  for (uint32_t e = sub; e < C4_PLANES_LEN; e += 8) store_plane<PlaneT>(p.planes, (size_t)g * C4_PLANES_LEN + e, c4::plane_bit(m, v, e));
}

// ------------------------------------------------------------------------------------------
// K2-K5 fused: one MCTS simulation for every resident game.
//   expand (mcts.rs:114-132, softmax mcts.rs:416-434)  ->  backup (mcts.rs:137-155)
//   -> gate / move / finish / refill (self_play.rs:283-308, mcts.rs:187-222, 271-313)
//   -> select (mcts.rs:160-183)  ->  encode the new leaf (c4r.rs:378-392)
// ------------------------------------------------------------------------------------------
// The extra workgroups a timed launch carries (they own no games; one per kWavesPerTimingHelper
// wavefronts): duration of the PREVIOUS launch = last wavefront end - first wavefront start (its stamps are
// complete: kernel boundary).  Each helper reduces its chunk, the last one to finish adds the launch to the
// totals.  No game's critical path carries any of this.
C4_DEV void timing_helper(const Params& p, uint32_t lane) {
  if (p.seq <= 1) return;
  const uint32_t h = blockIdx.x - p.n_waves, n_helpers = gridDim.x - p.n_waves;
  const unsigned long long* prev = p.stamps + (size_t)((p.seq - 1) & 1) * p.n_waves * 2;
  const uint32_t w_end = (h + 1) * kWavesPerTimingHelper < p.n_waves ? (h + 1) * kWavesPerTimingHelper : p.n_waves;
  unsigned long long lo = ~0ull, hi = 0ull;
#pragma unroll 8
  for (uint32_t w = h * kWavesPerTimingHelper + lane; w < w_end; w += 64) {
    const ulonglong2 ab = reinterpret_cast<const ulonglong2*>(prev)[w];
    lo = ab.x < lo ? ab.x : lo;
    hi = ab.y > hi ? ab.y : hi;
  }
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned long long ol = ((unsigned long long)shfl_u32((uint32_t)(lo >> 32), (int)(lane ^ off)) << 32) | shfl_u32((uint32_t)lo, (int)(lane ^ off));
    const unsigned long long oh = ((unsigned long long)shfl_u32((uint32_t)(hi >> 32), (int)(lane ^ off)) << 32) | shfl_u32((uint32_t)hi, (int)(lane ^ off));
    lo = ol < lo ? ol : lo;
    hi = oh > hi ? oh : hi;
  }
  if (lane == 0) {
    unsigned long long* tmp = p.clock_acc + 2;   // [2] running min start, [3] running max end, [4] helpers done
    atomicMin(&tmp[0], lo);
    atomicMax(&tmp[1], hi);
    __threadfence();
    if (atomicAdd(&tmp[2], 1ull) == n_helpers - 1) {
      __threadfence();
      const unsigned long long first = atomicExch(&tmp[0], ~0ull), last = atomicExch(&tmp[1], 0ull);
      atomicExch(&tmp[2], 0ull);
      if (last > first) { p.clock_acc[0] += last - first; p.clock_acc[1] += 1; }
    }
  }
}

// Wavefronts per SIMD the default instantiation is compiled for.  Measured (tools/tree_roofline.py, 65 536 /
// 131 072 games per launch): 3 (137 registers) 37.7 / 71.4 us, 4 (127 registers, no spill) 35.1 / 64.4 us,
// 5 (96 registers, spills) 46.2 / 93.6 us; at 2 048 games all three take 10.3 us.  The extension
// instantiations keep what they need.
#ifndef C4_STEP_WAVES
#define C4_STEP_WAVES 4
#endif
// The step of the 8 games of ONE wavefront (the body of c4_step_kernel, and of the fused output + step kernel below).
// `wave_index` = the wavefront's row in the per-wavefront arrays (games 8 wave_index .. + 7), `hot` = this lane's 16 bytes of its
// game's state line, `nn_logit` / `nn_q` = the evaluator's outputs for the game (lane sub < 7: logit sub; q_penalty / q_no_penalty
// on even / odd lanes), `t_start` = the wavefront's start stamp (timed launches).
// SEARCH (C4_FLAG_SEARCH, an instantiation of its own like NOISE / CACHE: the default carries none of it): a game is ONE search of its
// start position (mcts.rs:48-56 new_from_pos + the run_mcts helper, mcts.rs:469-485; interactive_play.rs:33, 57).  A terminal root is
// searched like any other, the gate writes one record -- root policy and root q -- instead of moving, and the slot takes the next
// request; no temperature, no move RNG.
// HOLD (C4_FLAG_HOLD, an instantiation of its own too): every slot keeps ONE game whose tree persists across moves
// (interactive_play.rs: InteractivePlay around one MctsGame).  The gate follows State::bg_thread_should_stop
// (interactive_play.rs:188-191): a game whose root has n_iter visits after expand + backup is PARKED -- status kParked, no select,
// no planes, no move, no record -- and skipped by every later step; nothing is ever refilled.
// RESUME (with HOLD; k_hold_resume, the one place where a game becomes active): the first trip has no evaluator answer to consume.
// It starts at the gate, with an optional move from outside (InteractivePlay::make_move / make_random_move,
// interactive_play.rs:70-85, 169-185: the self-play gate's own record / re-root / finish code, the column and the temperature given
// per slot, a refusal instead of a panic), parks or selects, and goes on as any trip does.
template <typename PlaneT, bool NOISE, bool CACHE, bool SEARCH = false, bool HOLD = false, bool RESUME = false>
C4_DEV void step_body(const Params& p, const uint32_t wave_index, const uint32_t lane, const uint32_t n_slots, Slot* st, const uint4 hot,
                      const float nn_logit, const float nn_q, const unsigned long long t_start, const uint32_t g) {
  // g = this lane group's game (>= n_slots: none).  The stand-alone kernels give a wavefront the 8 games 8 wave_index .. + 7; the fused
  // output + step kernel may give it fewer (c4_session_set_step_shape), its other lane groups idle.
  const uint32_t sub = lane & 7;
  const int gbase = (int)(lane & ~7u);
  uint32_t c_sims = 0, c_S = 0, c_K = 0, c_E = 0, c_moves = 0, c_done = 0, c_skipped = 0, c_samples = 0;   // this launch only
  uint32_t c_probes = 0, c_hits = 0;
  // header words to every lane of the group (lane 3: state, arena, root ref, rng word)
  const uint32_t state0 = shfl_u32(hot.x, gbase + 3);
  bool active = (g < n_slots) && (slot_status(state0) == kActive);
  // hold sessions: was the slot active when the launch began (a slot c4_session_start has just reset counts as new), is it parked
  // by this launch, does a refused move / a search already under way leave it exactly as it is; the move asked of it from outside
  const bool was_active = HOLD && active && !(RESUME && p.hold_fresh);
  bool park = false, untouched = false;
  int32_t mv = C4_HOLD_MOVE_NONE;
  float mv_temp = 1.0f;
  if (RESUME) {
    active = (g < n_slots) && (slot_status(state0) == kActive || slot_status(state0) == kParked);
    if (g < n_slots && p.hold_cols) {
      mv = p.hold_cols[g];
      mv_temp = p.hold_temps ? p.hold_temps[g] : 1.0f;
      // (a slot without a live game -- never given one, or ended by a device error -- has nothing to move)
      if (sub == 0 && p.hold_results) p.hold_results[g] = (mv != C4_HOLD_MOVE_NONE && !active) ? C4_HOLD_NO_GAME : C4_HOLD_OK;
    }
  }
  uint4 line = hot;          // what goes back to the slot at the end
  bool store_line = false;
  // move RNG precompute (see the end of the kernel): what this game will need at its next move
  bool pre_need = false;
  uint32_t pre_n_moves = 0;
  unsigned long long pre_game_id = 0;

  if (active) {
    Block* blocks = p.blocks + (size_t)g * p.blocks_per_slot;

#define C4_BCAST64(lo, hi, src) (((uint64_t)shfl_u32(hi, gbase + (src)) << 32) | shfl_u32(lo, gbase + (src)))
    uint64_t rmask = C4_BCAST64(hot.x, hot.y, 0), rvalue = C4_BCAST64(hot.z, hot.w, 0);
    uint64_t leaf_mask = C4_BCAST64(hot.x, hot.y, 1), leaf_value = C4_BCAST64(hot.z, hot.w, 1);
    unsigned long long game_id = C4_BCAST64(hot.x, hot.y, 2);
#undef C4_BCAST64
    uint32_t ordinal = shfl_u32(hot.z, gbase + 2);
    const uint32_t arena0 = shfl_u32(hot.y, gbase + 3);
    uint32_t root_ref = shfl_u32(hot.z, gbase + 3);
    uint32_t rng_word = shfl_u32(hot.w, gbase + 3);
    uint32_t depth = (state0 >> 8) & 0xFFu;
    uint32_t n_moves = (state0 >> 16) & 0xFFu;
    uint32_t term = (state0 >> 24) & 3u;          // terminal_state of the waiting leaf, computed when it was selected
    uint32_t rng_for = state0 >> 26;
    uint32_t n_blocks = arena0 & 0xFFFFu;
    uint32_t root_block = arena0 >> 16;
    // the recorded path as the line keeps it: lane 4 + j holds levels j, j + 4, j + 8, j + 12
    uint4 pv = hot;
    uint32_t leaf_ref = path_level(pv, st, depth, gbase);   // the waiting leaf's own entry
    bool fresh = false;                  // the slot took a new game in this launch
    uint32_t err = 0;
    uint32_t root_n = RESUME ? shfl_u32(hot.w, gbase + 2) : 0u;   // (a resumed game: the slot's mirror of the root's visit count)
    // One simulation per game per launch, plus a second one when the leaf just selected is terminal:
    // such a leaf needs no evaluator row (mcts.rs:92-98 ignores the network for it), so its value is
    // backed up here and now instead of idling through an evaluator pass.  The order of a game's
    // simulations and every value in them is unchanged; C4_FLAG_NO_MOVES / C4_FLAG_ONE_SIM_PER_STEP
    // keep exactly one.
    // (p.max_sims: 1 under those flags, else 2 -- measured: a third trip costs more launch time than
    // it saves rows -- or more with the evaluation cache, whose hits need no evaluator either.)
    const uint32_t max_sims = p.max_sims;
    // this trip's evaluator outputs: the network's for the first trip, a cached entry's after a hit
    float cur_logit = nn_logit;
    float cur_qp = shfl_f32(nn_q, gbase), cur_qn = shfl_f32(nn_q, gbase + 1);

    C4_STAMP(1, depth + n_blocks + pv.x + (uint32_t)leaf_mask);
#define C4_STAMP_TRIP1(i, force) do { if (sim == 0) C4_STAMP(i, force); } while (0)
#pragma clang loop unroll(disable)
    for (uint32_t sim = 0; sim < max_sims; sim++) {
      // A terminal leaf at depth 0 is a terminal START position (a move into a terminal position closes the game in the launch that
      // makes it).  The reference gives such a root its n simulations, none of which can change the game's one sample
      // (self_play.rs:283-308, mcts.rs:271-313): as after a move into a terminal position, the game is closed now and the
      // simulations are counted as skipped.  (C4_FLAG_NO_MOVES, the reference's run_mcts, keeps searching such a root.)
      // (A search keeps searching it too: its root q is q_sum / (n + 1), not the terminal value.)
      // (A hold session never searches a terminal root: it is parked from the start, or from the move that made it terminal.)
      const bool term_start = !SEARCH && !HOLD && term != 0 && depth == 0 && !(p.flags & C4_FLAG_NO_MOVES);
      float v_pen, v_nopen;
      if (!(RESUME && sim == 0)) {   // (a resumed game's first trip has no answer to consume: it starts at the gate)
        // ---------------- on_received_policy: terminal value or expansion -------------------
        if (term) {
          c4::terminal_value(term, leaf_mask, p.c_ply_penalty, v_pen, v_nopen);  // NN output ignored (mcts.rs:92-98)
        } else {
          // first simulation: the network's outputs; a later one gets here only on an evaluation-cache hit
          const uint32_t legal = c4::legal_mask(leaf_mask);
          const bool is_legal = sub < 7 && ((legal >> sub) & 1u);
          float logit = __uint_as_float(0xff800000u);                             // mask_policy, c4r.rs:272-286
          if (is_legal) logit = cur_logit;
          float mx = logit;                                                       // f32::max fold (NaN-ignoring)
          mx = c4::rust_max(mx, grp_xchg<0>(mx));
          mx = c4::rust_max(mx, grp_xchg<1>(mx));
          mx = c4::rust_max(mx, grp_xchg<2>(mx));
          if (__builtin_isinf(mx)) err = C4_ERR_DEGENERATE_POLICY;                // mcts.rs:421-425
          const float ex = c4::c4_expf(logit - mx);
          float sum = 0.0f;                                                       // left-to-right, mcts.rs:432
          for (int i = 0; i < 7; i++) sum = sum + shfl_f32(ex, gbase + i);
          float prior = ex / sum;
          if (NOISE && p.dir_eps > 0.0f && depth == 0) {
            // extension: the root is expanded only now -> its children start with noisy priors
            float eta[7];
            c4::dirichlet_noise(game_id, n_moves, legal, p.dir_alpha, eta);
            float mine = eta[0];
            for (int c = 1; c < 7; c++) mine = (sub == (uint32_t)c) ? eta[c] : mine;
            if (is_legal) {
              const float keep = (1.0f - p.dir_eps) * prior;
              const float add = p.dir_eps * mine;
              prior = keep + add;
            }
          }
          const uint32_t nb = n_blocks;
          // (a reclaimed arena is two halves: the bump pointer of the lower one stops at the boundary; half_blocks == 0 otherwise, never a block number)
          if (nb >= p.blocks_per_slot || nb == p.half_blocks) err = err ? err : C4_ERR_ARENA_OVERFLOW;
          if (!err) {
            // Node::new (mcts.rs:345-355) for the 7 children; lane 7 writes the tail (no links yet)
            reinterpret_cast<uint4*>(blocks + nb)[sub] =
                sub < 7 ? make_uint4(0u, 0u, 0u, __float_as_uint(prior)) : make_uint4(0u, 0u, 0u, legal << 16);
            if (sub == 0) blocks[leaf_ref >> 3].t.child[leaf_ref & 7] = (uint16_t)nb;   // leaf.children = Some(..)
            if (depth == 0) root_block = nb;
            n_blocks = nb + 1;
            c_E += 1;
          }
          v_pen = cur_qp;
          v_nopen = cur_qn;
          if (CACHE && sim == 0)     // extension: remember what the evaluator said about this position
            cache_store(p.cache, p.cache_mask, leaf_mask, leaf_value, nn_logit, cur_qp, cur_qn, sub, gbase);
        }
        if (err) break;

        C4_STAMP_TRIP1(2, n_blocks);
        // ---------------- backpropagate_value: leaf -> root along the recorded path ----------
        root_n = 0;
        if (sub >= 4) {   // level d on lane 4 + (d & 3): the first four levels update in parallel
          for (uint32_t d = sub - 4; d <= depth; d += 4) {
            const uint32_t c = d >> 2;
            const uint32_t ref = c == 0 ? pv.x : (c == 1 ? pv.y : (c == 2 ? pv.z : (c == 3 ? pv.w : st->path_deep[d - kHotPath])));
            Entry* e = &blocks[ref >> 3].e[ref & 7];
            const bool odd = ((depth - d) & 1u) != 0;                             // value negated per step up
            const uint32_t n1 = e->n + 1;
            const float q1 = e->q_pen + (odd ? -v_pen : v_pen);
            const float q2 = e->q_nopen + (odd ? -v_nopen : v_nopen);
            e->n = n1;
            e->q_pen = q1;
            e->q_nopen = q2;
            if (d == 0) root_n = n1;
          }
        }
        root_n = shfl_u32(root_n, gbase + 4);
        c_sims += term_start ? 0u : 1u;
        // (a search's simulations of a terminal root are not counted in K, as the oracle counts backup_nodes)
        c_K += (term_start || (SEARCH && term != 0 && depth == 0)) ? 0u : depth + 1;
        // The stores above are read back below through other lanes of THIS wavefront.  A wavefront's
        // vector-memory instructions reach the cache in program order, so a later load of the same
        // address returns the stored bytes without waiting for the store's acknowledgement: only the
        // compiler must not reorder them (a wavefront-scope fence emits no instruction).
        C4_STAMP_TRIP1(3, root_n);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        C4_STAMP_TRIP1(4, root_n);
      }

      // ---------------- gate: self_play.rs:283-308 ------------------------------------------
      bool finished = false;
      if (SEARCH && root_n >= p.n_iter) {
        // The search is over: ONE record at the head of the request's 43, and the slot is free for the next request.
        // root_policy (mcts.rs:396-412): child visit counts / their left-to-right sum; 1/7 each without children or visits
        const uint4 re = load_block_lane(blocks, root_block, sub);          // (root_block == 0: the root's own block, not counted)
        const float cnt = (sub < 7 && root_block != 0) ? (float)re.x : 0.0f;
        float w[7];
        float csum = 0.0f;
        for (int i = 0; i < 7; i++) { w[i] = shfl_f32(cnt, gbase + i); csum = csum + w[i]; }
        float pol[7];
        for (int i = 0; i < 7; i++) pol[i] = (csum == 0.0f) ? (1.0f / 7.0f) : (w[i] / csum);
        // root_q_with_penalty / root_q_no_penalty (mcts.rs:359-367): q_sum / (visit_count as f32 + 1.0), as c4_session_root_stats
        const Entry* re0 = &blocks[root_ref >> 3].e[root_ref & 7];
        const float nf = (float)re0->n + 1.0f;
        const float rq_pen = re0->q_pen / nf, rq_nopen = re0->q_nopen / nf;
        c4_sample_rec* rec = p.samples + (size_t)ordinal * C4_MAX_SAMPLES_PER_GAME;
        if (sub < 7) rec->policy[sub] = pol[sub];
        if (sub == 7) {
          rec->game_id = game_id; rec->mask = rmask; rec->value = rvalue;
          rec->q_penalty = rq_pen; rec->q_no_penalty = rq_nopen; rec->meta = 0u | (2u << 16);
          p.sample_counts[ordinal] = 1;
        }
        c_done += 1;
        c_samples += 1;
        finished = true;
      }
      // A hold session moves only when asked to from outside, in k_hold_resume's first trip: a given column, or a sampled one at
      // the slot's temperature.  What the reference answers with `false` or a panic is a REFUSAL here (C4_HOLD_REFUSED_*): a
      // terminal root (interactive_play.rs:171, 180), a column outside 0-6 or full (:171), a root without children yet
      // (mcts.rs:196 panics) and a sampled column that is not legal (mcts.rs:196-200); the slot then stays exactly as it is.
      uint32_t refused = 0;
      uint32_t root_term = 0;                                // hold: terminal state of the root, before and after the move
      if (RESUME && sim == 0) {
        root_term = c4::terminal_state(rmask, rvalue);        // (any start position: the full test)
        if (mv != C4_HOLD_MOVE_NONE) {
          if (root_term) refused = C4_HOLD_REFUSED_TERMINAL;
          else if (mv != C4_HOLD_MOVE_SAMPLE && (mv < 0 || mv > 6 || !((c4::legal_mask(rmask) >> mv) & 1u))) refused = C4_HOLD_REFUSED_COLUMN;
          else if (root_block == 0) refused = C4_HOLD_REFUSED_UNSEARCHED;
        }
      }
      // (A terminal START position is a finished game as it stands: c4_session_start's launch closes it with its one sample.)
      if (!SEARCH && (HOLD ? (RESUME && sim == 0 && ((mv != C4_HOLD_MOVE_NONE && !refused) || (p.hold_fresh && root_term != 0)))
                           : ((root_n >= p.n_iter && !(p.flags & C4_FLAG_NO_MOVES)) || term_start))) {
        const size_t rec0 = (size_t)ordinal * C4_MAX_SAMPLES_PER_GAME;
        uint32_t rterm = HOLD ? root_term : (term_start ? term : 0u);   // a root is terminal only as a terminal START position
        uint32_t retained = term_start ? 0u : p.n_iter;
        if (!rterm) {
          // root_policy (mcts.rs:396-412): child visit counts / their sum
          const uint4 re = load_block_lane(blocks, root_block, sub);
          const float cnt = (sub < 7) ? (float)re.x : 0.0f;
          float w[7];
          float csum = 0.0f;
          for (int i = 0; i < 7; i++) { w[i] = shfl_f32(cnt, gbase + i); csum = csum + w[i]; }
          float pol[7];
          for (int i = 0; i < 7; i++) pol[i] = (csum == 0.0f) ? (1.0f / 7.0f) : (w[i] / csum);
          // make_random_move (mcts.rs:214-222); the 7 columns' logf/expf and the 4 ChaCha columns
          // run on the game's own lanes instead of 8 redundant copies
          const float temperature = HOLD ? mv_temp : c4::temperature_for_ply((uint32_t)__popcll(rmask));
          C4_STAMP_TRIP1(9, (uint32_t)pol[0]);
          float tp[7];
          c4::apply_temperature_group(pol, temperature, tp, sub, gbase);
          C4_STAMP_TRIP1(10, (uint32_t)tp[0]);
          const uint64_t seed = game_id * (uint64_t)(42 + n_moves);
          // the word was normally computed in an earlier, uncontended step (end of this kernel)
          // (a hold session keeps no precomputed word: its moves come from outside, one launch each)
          const uint32_t u32 = (!HOLD && !fresh && rng_for == n_moves + 1) ? rng_word : c4::rng_first_u32_group(seed, sub, gbase);
          const int col = (HOLD && mv >= 0) ? (int)mv : c4::weighted_index(tp, u32);
          C4_STAMP_TRIP1(11, (uint32_t)col);
          if (col < 0) {
            err = C4_ERR_DEGENERATE_POLICY;
          } else if (!((c4::legal_mask(rmask) >> col) & 1u)) {
            if (HOLD) refused = C4_HOLD_REFUSED_SAMPLE; else err = C4_ERR_ILLEGAL_MOVE;   // mcts.rs:196-200 expect()
          } else {
            // make_move (mcts.rs:187-206): record (root position, untempered policy), re-root
            c4_sample_rec* rec = p.samples + rec0 + n_moves;
            if (sub < 7) rec->policy[sub] = pol[sub];
            if (sub == 7) {
              rec->game_id = game_id; rec->mask = rmask; rec->value = rvalue; rec->meta = n_moves;
            }
            retained = shfl_u32(re.x, gbase + col);
            const uint32_t child_blk = child_link(re, (uint32_t)col, gbase);
            root_ref = (root_block << 3) | (uint32_t)col;
            root_block = child_blk;
            root_n = retained;
            c4::make_move(rmask, rvalue, (uint32_t)col);
            n_moves += 1;
            c_moves += 1;
            rterm = c4::terminal_after_move(rmask, rvalue);   // the position moved from was not terminal
            if (NOISE && p.dir_eps > 0.0f && !rterm && root_block != 0) {
              // extension: the new root keeps its subtree; fresh noise goes into its children's priors
              const uint32_t nlegal = c4::legal_mask(rmask);
              float eta[7];
              c4::dirichlet_noise(game_id, n_moves, nlegal, p.dir_alpha, eta);
              float mine = eta[0];
              for (int c = 1; c < 7; c++) mine = (sub == (uint32_t)c) ? eta[c] : mine;
              if (sub < 7 && ((nlegal >> sub) & 1u)) {
                Entry* ce = &blocks[root_block].e[sub];
                const float keep = (1.0f - p.dir_eps) * ce->prior;
                const float add = p.dir_eps * mine;
                ce->prior = keep + add;
              }
              __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            }
          }
        }
        if (!err && rterm) {
          // Game over (self_play.rs:302-308).  After a move INTO a terminal position the
          // reference keeps evaluating that root until it has n visits (self_play.rs:283-301);
          // those sims cannot change the samples (mcts.rs:271-313), so the game is closed now
          // and the skipped sims are counted.
          if (!HOLD) c_skipped += (p.n_iter > retained) ? (p.n_iter - retained) : 0;   // (the reference's InteractivePlay stops at a terminal root too)
          float tq_pen, tq_nopen;
          c4::terminal_value(rterm, rmask, p.c_ply_penalty, tq_pen, tq_nopen);
          // to_result (mcts.rs:271-313): sample i gets +q iff (M - i) is even
          for (uint32_t i = sub; i < n_moves; i += 8) {
            const bool neg = ((n_moves - i) & 1u) != 0;
            p.samples[rec0 + i].q_penalty = neg ? -tq_pen : tq_pen;
            p.samples[rec0 + i].q_no_penalty = neg ? -tq_nopen : tq_nopen;
          }
          c4_sample_rec* tr = p.samples + rec0 + n_moves;
          if (sub < 7) tr->policy[sub] = 1.0f / 7.0f;                         // UNIFORM_POLICY, mcts.rs:45
          if (sub == 7) {
            tr->game_id = game_id; tr->mask = rmask; tr->value = rvalue;
            tr->q_penalty = tq_pen; tr->q_no_penalty = tq_nopen; tr->meta = n_moves | (1u << 16);
            p.sample_counts[ordinal] = n_moves + 1;
          }
          c_done += 1;
          c_samples += n_moves + 1;
          finished = true;
        }
        if (HOLD) root_term = rterm;
      }
      // Did any game of this wavefront move in this launch?  Asked here, where every game that entered the
      // trip is still in it (a wavefront's 8 games run in lock-step: one game's extra work is everybody's).
      const bool wave_moved = (SEARCH || HOLD) ? false : (__ballot(c_moves != 0) != 0ull);   // (a search never moves; a hold session not in a step)
      if (err) break;
      if (HOLD) {
        // The hold gate (State::bg_thread_should_stop, interactive_play.rs:188-191), inside the trip loop: a root never gets a
        // visit beyond its target.  A refused move, and a resume that finds a search under way with visits still to go, leave
        // the slot as it is, pending leaf and all.
        if (RESUME && sim == 0 && refused) {
          if (sub == 0 && p.hold_results) p.hold_results[g] = (int32_t)refused;
          untouched = true;
        } else if (finished || root_term != 0 || root_n >= p.n_iter) {
          if (finished && sub == 0) atomicAdd(&p.glob->games_done, 1ull);
          park = true;
          leaf_mask = rmask; leaf_value = rvalue; depth = 0; term = root_term;
          pv.x = (sub == 4) ? root_ref : pv.x;
        } else if (RESUME && sim == 0 && was_active && c_moves == 0) {
          untouched = true;
        }
        if (park || untouched) break;
      }

      C4_STAMP_TRIP1(12, root_n);
      if (!HOLD && finished) {
        // replace the finished game by the next one of the request list (keeps the batch full)
        unsigned long long next = 0;
        if (sub == 0) {
          atomicAdd(&p.glob->games_done, 1ull);
          next = atomicAdd(&p.glob->queue_head, 1ull);
        }
        next = ((unsigned long long)shfl_u32((uint32_t)(next >> 32), gbase) << 32) | shfl_u32((uint32_t)next, gbase);
        if (next < p.n_games) {
          reset_slot(p, st, blocks, sub, next);
          __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
          rmask = p.start_mask ? p.start_mask[next] : 0ull;
          rvalue = p.start_value ? p.start_value[next] : 0ull;
          root_ref = 0; root_block = 0; root_n = 0; n_blocks = 1; n_moves = 0;
          ordinal = (uint32_t)next;
          game_id = p.reqs[next].game_id;
          fresh = true;
        } else {
          active = false;
          if (sub == 0) { st->state = kIdle; st->ordinal = 0xFFFFFFFFu; }
          break;
        }
      }
      C4_STAMP_TRIP1(5, root_n);
      // ---------------- select_new_leaf (mcts.rs:160-183) -------------------------------
      err = select_leaf(p, blocks, st, rmask, rvalue, root_block, root_ref, root_n, p.c_exploration, sub, gbase,
                        leaf_mask, leaf_value, depth, leaf_ref, pv, c_S);
      if (err) break;
      C4_STAMP_TRIP1(6, depth);
      if (sim == 1) C4_STAMP_ANY(13);
      // terminal_state of the new leaf (kept for the simulation that consumes it): below the root it was
      // reached by a move from a non-terminal node; the root itself may be an arbitrary start position
      term = depth == 0 ? c4::terminal_state(leaf_mask, leaf_value) : c4::terminal_after_move(leaf_mask, leaf_value);
      // a terminal leaf needs no evaluator, nor does one whose evaluation is in the cache: run that
      // simulation now, while trips remain
      if (sim + 1 < max_sims) {
        // A launch lasts as long as its slowest wavefront.  A wavefront with a MOVING game has already
        // paid the longest path of the step (root policy, temperature, sampling, sample record, re-root:
        // +1.7-2.7 us), and a second, terminal-leaf simulation costs +2.0 us more: such a wavefront leaves
        // its terminal leaves to the next launch (an evaluator row is then wasted on them, as the reference
        // wastes one on every terminal leaf, mcts.rs:92-98; samples are identical either way).  Measured:
        // 10.36 -> 9.61 us per 2 048-game launch alone, 11.5 -> 10.6 beside the evaluator
        // (profiles/r03_step_second_trip_ab.txt).  The evaluation-cache build keeps all its trips.
        bool again = term != 0 && (CACHE || !wave_moved);
        if (CACHE && !again) {
          c_probes += 1;
          again = cache_lookup(p.cache, p.cache_mask, leaf_mask, leaf_value, cur_logit, cur_qp, cur_qn, sub, gbase);
          c_hits += again ? 1 : 0;
        }
        if (again) {
          if (depth >= kHotPath) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // deeper levels are re-read from the slot's second line
          continue;
        }
      }
      break;
    }

#undef C4_STAMP_TRIP1
    if (err) {
      if (sub == 0) raise_error(p, st, g, err);
    } else if (HOLD && untouched) {
      // nothing: the slot stays byte for byte what it was
    } else if (active) {
      const bool waits = !(HOLD && park);   // (a parked game waits for no evaluator row)
      if (waits && sub == 0) publish_leaf_model(p, g, ordinal, leaf_mask);
      pre_need = fresh || (rng_for != n_moves + 1);   // after a move / refill the stored word is stale
      pre_n_moves = n_moves;
      pre_game_id = game_id;
      // ---------------- leaf -> evaluator input (c4r.rs:378-392) ----------------------
      if (waits) encode_leaf<PlaneT>(p.planes, g, leaf_mask, leaf_value, sub);
      // ---------------- the game's state goes back as one line: lane k owns dwords 4k..4k+3 ----
      line = pv;                                                    // lanes 4..7: the recorded path
      if (sub == 0) line = make_uint4((uint32_t)rmask, (uint32_t)(rmask >> 32), (uint32_t)rvalue, (uint32_t)(rvalue >> 32));
      if (sub == 1) line = make_uint4((uint32_t)leaf_mask, (uint32_t)(leaf_mask >> 32), (uint32_t)leaf_value, (uint32_t)(leaf_value >> 32));
      if (sub == 2) line = make_uint4((uint32_t)game_id, (uint32_t)(game_id >> 32), ordinal, root_n);
      if (sub == 3) line = make_uint4(slot_state((HOLD && park) ? kParked : kActive, depth, n_moves, term, fresh ? 0u : rng_for), n_blocks | (root_block << 16), root_ref, rng_word);
      store_line = true;
    }
  }
  if (HOLD) {
    // the session's count of active slots (c4_session_hold_poll), and how far the farthest root is from its target
    const bool now_active = untouched ? was_active : (store_line && !park);
    if (sub == 0 && g < n_slots && now_active != was_active) atomicAdd(&p.glob->hold_active, now_active ? 1u : 0xFFFFFFFFu);
    const uint32_t have = shfl_u32(line.w, gbase + 2);   // the root's visit count as the slot's line holds it
    if (RESUME && sub == 0 && g < n_slots && now_active) {
      atomicMax(&p.glob->hold_need, p.n_iter > have ? p.n_iter - have : 0u);
    }
  }

  C4_STAMP(7, 0);
  // ---------------- per-wavefront counters (one row per wavefront: no contention) ----------
  // lane `sub` of each game adds that game's counter number `sub` to the wavefront's row: one
  // no-return atomic instruction for the whole wave (nobody waits for it; rows have one writer wave)
  {
    uint32_t add = c_sims;
    add = sub == CTR_S ? c_S : add;
    add = sub == CTR_K ? c_K : add;
    add = sub == CTR_E ? c_E : add;
    add = sub == CTR_MOVES ? c_moves : add;
    add = sub == CTR_DONE ? c_done : add;
    add = sub == CTR_SKIPPED ? c_skipped : add;
    add = sub == CTR_SAMPLES ? c_samples : add;
    if (add) atomicAdd(&p.wave_ctr[(size_t)wave_index * CTR_N + sub], (unsigned long long)add);
    const uint32_t add2 = sub == 0 ? c_probes : (sub == 1 ? c_hits : 0u);
    if (CACHE && add2) atomicAdd(&p.wave_ctr[(size_t)wave_index * CTR_N + CTR_PROBES + sub], (unsigned long long)add2);
  }
  // ---------------- move RNG, off the critical path ------------------------------------------
  // The launch lasts as long as its slowest wavefront, and that is one with a MOVING game.  The
  // ChaCha12 word a game will need at its next move depends only on (game_id, moves played), so it
  // is computed here, in a step where no game of this wavefront moved, and kept in the slot.
  if (!SEARCH && !HOLD && __ballot(c_moves != 0) == 0ull && pre_need) {
    const uint32_t w = c4::rng_first_u32_group(pre_game_id * (uint64_t)(42 + pre_n_moves), sub, gbase);
    if (sub == 3) { line.w = w; line.x = (line.x & 0x03FFFFFFu) | ((pre_n_moves + 1u) << 26); }
  }
  if (store_line) reinterpret_cast<uint4*>(st)[sub] = line;
  C4_STAMP(8, 0);
  if (lane == 0 && p.seq) {
    unsigned long long* my = p.stamps + ((size_t)(p.seq & 1) * p.n_waves + wave_index) * 2;
    my[0] = t_start;
    my[1] = __builtin_amdgcn_s_memrealtime();
  }
}

template <typename PlaneT, bool NOISE, bool CACHE, bool SEARCH = false, bool HOLD = false>
__global__ __launch_bounds__(64, (NOISE || CACHE) ? 1 : C4_STEP_WAVES) void c4_step_kernel(
    // What the head of every wavefront's dependent chain needs, as leading SCALAR arguments (copies of p's fields): with
    // -mllvm -amdgpu-kernarg-preload-count (build.py) they are in SGPRs when the wavefront starts, so the state line and
    // the evaluator's outputs are requested at once instead of behind a scalar-load round trip to the kernarg segment.
    Slot* __restrict__ a_slots, const float* __restrict__ a_logprobs, const float* __restrict__ a_q, uint32_t a_n_waves, uint32_t a_n_slots,
    Params p) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t sub = lane & 7;
  const uint32_t wave_index = blockIdx.x;
  const uint32_t g = wave_index * 8 + (lane >> 3);
  const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();   // 100 MHz device clock
  C4_STAMP(0, 0);
#ifdef C4_PHASE_STAMPS
  if (lane == 0) for (int i = 9; i < 16; i++) p.phase[(size_t)wave_index * 16 + i] = 0;
#endif
  if (blockIdx.x >= a_n_waves) { timing_helper(p, lane); return; }

  const uint32_t gs = g < a_n_slots ? g : 0;
  Slot* st = a_slots + gs;
  // The game's state: ONE 128-byte line, 16 bytes per lane in one instruction; the evaluator's
  // outputs for this game travel in the same round trip.
  const uint4 hot = reinterpret_cast<const uint4*>(st)[sub];
  const float nn_logit = a_logprobs[(size_t)gs * 7 + (sub < 7 ? sub : 6)];
  const float nn_q = a_q[(size_t)gs * 2 + (sub & 1)];
  // ... and they must LEAVE together: without this fence hipcc sinks the two evaluator loads into the
  // `if (active)` below, i.e. behind the wait for the state line -- a second, serial memory round trip (plus the
  // scalar loads of the two pointers) at the head of every wavefront's chain (round 3, found in the ISA).
  __builtin_amdgcn_sched_barrier(0);
  step_body<PlaneT, NOISE, CACHE, SEARCH, HOLD>(p, wave_index, lane, a_n_slots, st, hot, nn_logit, nn_q, t_start, g);
}

// ------------------------------------------------------------------------------------------
// Hold sessions (C4_FLAG_HOLD): the single place where a game becomes active (c4_session_start, c4_session_hold_resume).  For every
// slot with a game, 8 lanes per game like the step: an optional move from outside, then park -- the root is terminal or has its
// n_iter visits -- or select the next leaf from the tree as it stands, encode it and publish the state line as active.  All of it is
// the tail of step_body (its RESUME form: gate -> select -> encode -> write-back), so the select, the path write-back and the deep
// path are the step's own code.  c4_session_start's launch (p.hold_fresh) first puts request g on slot g (MctsGame::new_from_pos).
// ------------------------------------------------------------------------------------------
template <typename PlaneT>
__global__ __launch_bounds__(64) void k_hold_resume(Params p) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t sub = lane & 7;
  const uint32_t wave_index = blockIdx.x;
  const uint32_t g = wave_index * 8 + (lane >> 3);
  const uint32_t gs = g < p.n_slots ? g : 0;
  Slot* st = p.slots + gs;
  if (p.hold_fresh && g < p.n_slots) {
    if (g < p.n_games) {
      reset_slot(p, st, p.blocks + (size_t)g * p.blocks_per_slot, sub, g);
    } else if (sub == 0) {
      st->state = kIdle;
      st->ordinal = 0xFFFFFFFFu;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");   // read back below by the other lanes of this wavefront
  }
  const uint4 hot = reinterpret_cast<const uint4*>(st)[sub];
  step_body<PlaneT, false, false, false, true, true>(p, wave_index, lane, p.n_slots, st, hot, 0.0f, 0.0f, 0ull, g);
}

// c4_session_scatter_outputs + c4_session_step as ONE launch (callback mode, c4_session_step_gather): a game takes its evaluator
// outputs from row inverse[g] of the callback's answers (7 log-probabilities, q_penalty, q_no_penalty per row; pinned host memory
// or device memory) instead of from the bound tensors -- one launch and one boundary less per callback round trip.  The bound
// logprobs / q tensors are NOT updated by this form (callers that watch them use the two entry points).
template <typename PlaneT, bool NOISE, bool CACHE>
__global__ __launch_bounds__(64, (NOISE || CACHE) ? 1 : C4_STEP_WAVES) void c4_step_gather_kernel(
    Slot* __restrict__ a_slots, const float* __restrict__ a_answers, const uint32_t* __restrict__ a_inverse, uint32_t a_n_unique, uint32_t a_n_waves,
    uint32_t a_n_slots, Params p) {
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t sub = lane & 7;
  const uint32_t wave_index = blockIdx.x;
  const uint32_t g = wave_index * 8 + (lane >> 3);
  const unsigned long long t_start = __builtin_amdgcn_s_memrealtime();
  C4_STAMP(0, 0);
  if (blockIdx.x >= a_n_waves) { timing_helper(p, lane); return; }
  const uint32_t gs = g < a_n_slots ? g : 0;
  Slot* st = a_slots + gs;
  const uint4 hot = reinterpret_cast<const uint4*>(st)[sub];
  const uint32_t row = a_inverse[gs];
  float nn_logit = 0.f, nn_q = 0.f;
  if (row < a_n_unique) {                                           // (idle slots have no row: their values are never used)
    nn_logit = a_answers[(size_t)row * 9 + (sub < 7 ? sub : 6)];
    nn_q = a_answers[(size_t)row * 9 + 7 + (sub & 1)];
  }
  step_body<PlaneT, NOISE, CACHE>(p, wave_index, lane, a_n_slots, st, hot, nn_logit, nn_q, t_start, g);
}

// ------------------------------------------------------------------------------------------
// The heads' output layers AND the step in one launch (c4_session_step_head_out).  A workgroup of the output kernel owns
// 16 boards -- the games of exactly two step wavefronts -- so nothing crosses a workgroup: wavefronts 0 and 1 request
// their games' state lines at the very start (the round trip is over long before the outputs exist), all six compute the
// outputs (c4_head_out.hpp: the same code as the stand-alone kernel, the same bits; the outputs still go to the bound
// logprobs / q tensors for whoever watches them), and wavefronts 0 and 1 go on as the step of their 8 games each, taking
// the logits from LDS.  One launch boundary, the step kernel's argument fetch and both of its head-of-chain round trips
// leave a session's per-round chain.  Default configuration only (no Dirichlet noise, no evaluation cache, no per-launch
// timing): everything else keeps the two launches.
// ------------------------------------------------------------------------------------------
// (151 registers: two of this kernel's wavefronts on a SIMD take 304 of its 512, and the launch shares a compute unit with a
// 4-wavefront hidden-layer GEMM workgroup of the OTHER session -- 208 registers per SIMD, 120 KB + 15 KB of LDS -- instead of
// queueing for a free one; not with the 8-wavefront form's 2 x 112.)
#ifdef C4_OUT_STEP_WAVES_PER_EU   // diagnostic (build_variant.py ... -DC4_OUT_STEP_WAVES_PER_EU=4): 128 registers, fits beside any GEMM workgroup; spills 116 bytes per lane
#define C4_OUT_STEP_ATTR __attribute__((amdgpu_waves_per_eu(C4_OUT_STEP_WAVES_PER_EU, C4_OUT_STEP_WAVES_PER_EU)))
#else
#define C4_OUT_STEP_ATTR
#endif
// kGpw: games per stepping wavefront -- 8 (wavefronts 0 and 1 step the workgroup's 16 games) or 4 (wavefronts 0-3 step four games
// each, their other four lane groups idle; c4_session_set_step_shape).  A wavefront runs the UNION of its games' control flow (the
// deepest descent, a mover's temperature + sampling, a second simulation behind a terminal leaf, one after the other), and the
// workgroup's six wavefronts are there anyway.  Measured (profiles/r05_out_step_gpw.txt): beside a second session's kernels
// (BASELINE config 2, the paired graph) 4 is +0.5 % (six of six alternating pairs), for a session alone (the reference's default job)
// -0.4 %: the paired driver asks for 4, everybody else gets 8.  Which wavefront steps a game changes nothing the game records.
// (Counter rows: two wavefronts add to one row, by atomics as before.)
// SEARCH: the step of a search session (C4_FLAG_SEARCH, see step_body); the output layers are the same code.
// HOLD: the step of a hold session (C4_FLAG_HOLD), likewise.
template <typename PlaneT, uint32_t kGpw, bool SEARCH = false, bool HOLD = false>
__global__ __launch_bounds__(64 * c4ho::kHeadWaves, 1) C4_OUT_STEP_ATTR void c4_out_step_kernel(
    const uint4* __restrict__ hp, const uint4* __restrict__ hv, const uint4* __restrict__ wp, const uint4* __restrict__ wv,
    const float* __restrict__ bp, const float* __restrict__ bv, Slot* __restrict__ a_slots, uint32_t a_n_slots, uint32_t f8, uint32_t sp8, uint32_t sv8,
    Params p) {
  __shared__ c4ho::Shared sh;
  C4_TL_BEGIN();
  constexpr uint32_t kStepWaves = 16 / kGpw;
  static_assert(kGpw == 8 || kGpw == 4, "16 games per workgroup on two or four stepping wavefronts");
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & 7, grp = lane >> 3;
  const uint32_t b = wave * kGpw + grp;                                 // the lane group's board among the workgroup's 16
  const bool mine = wave < kStepWaves && grp < kGpw;
  const uint32_t g = mine ? blockIdx.x * 16 + b : a_n_slots;            // (>= n_slots: this lane group steps nothing)
  const uint32_t wave_index = blockIdx.x * 2 + wave / (kStepWaves / 2);  // the counters' row: as many rows as the stand-alone kernel has wavefronts
  const uint32_t gs = g < a_n_slots ? g : 0;
  Slot* st = a_slots + gs;
  uint4 hot = make_uint4(0, 0, 0, 0);
  if (wave < kStepWaves) hot = reinterpret_cast<const uint4*>(st)[sub]; // in flight under the output layers
  c4ho::head_out_block<16>(sh, hp, hv, wp, wv, bp, bv, a_n_slots, f8, sp8, sv8, const_cast<float*>(p.logprobs), const_cast<float*>(p.q), blockIdx.x);
  __syncthreads();
  if (wave >= kStepWaves || wave_index >= p.n_waves) return;
  const float nn_logit = sh.res[b & 15][sub < 7 ? sub : 6];
  const float nn_q = sh.res[b & 15][7 + (sub & 1)];
  step_body<PlaneT, false, false, SEARCH, HOLD>(p, wave_index, lane, a_n_slots, st, hot, nn_logit, nn_q, 0ull, g);
  C4_TL_END(3, a_slots);
}

// The element-wise Dirichlet kernel (c4_dirichlet; its siblings are c4_elementwise.hip) stays in THIS file on purpose:
// c4::dirichlet_noise is an out-of-line function the NOISE step kernels call, and hipcc specialises its body to the arguments of the
// callers it sees.  This kernel passes an arbitrary `legal`; without it in the translation unit the function loses three instructions
// (the 7-bit mask before the popcount) -- equivalent for the step kernels, but not the code that was measured.
__global__ void k_dirichlet(const uint64_t* game_id, const uint32_t* n_moves, const uint32_t* legal, float alpha, uint64_t n, float* eta) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float e[7];
  c4::dirichlet_noise(game_id[i], n_moves[i], legal[i], alpha, e);
  for (int c = 0; c < 7; c++) eta[7 * i + c] = e[c];
}

// ln_tab[k] = c4_logf((float)k): the same port the kernel would otherwise run per tree level
__global__ void k_ln_table(float* tab, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) tab[i] = c4::c4_logf((float)i);
}

// ------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------
thread_local std::string g_last_error;
using c4host::fail;
using c4host::grid_for;
using c4host::with_flag;
using c4host::with_planes;

// The tree arena is by far a session's largest allocation (13 GB for the reference's default job: 1 700 slots x
// (43 x 1 400 + 8) blocks) and the driver scrubs freed device memory before it hands it out again: a session created
// right after one of that size was destroyed waited 0.6 s in hipMalloc (tools/whole_job_phases.py).  One freed arena
// per process is therefore kept for the next session on the same device that fits it (no more than twice as big as
// needed); nothing in it is ever read before it is written (blocks are bump-allocated per slot, c4_start_kernel
// writes each slot's root).  c4_trim_cached_memory() gives it back; C4_ARENA_CACHE=0 switches the cache off.
struct ArenaCache { void* ptr = nullptr; size_t bytes = 0; int device = -1; };
ArenaCache g_arena_cache;
std::mutex g_arena_mutex;
bool arena_cache_enabled() {
  static const bool on = [] { const char* e = getenv("C4_ARENA_CACHE"); return !(e && e[0] == '0'); }();
  return on;
}
// Gives the kept arena back to its device (the caller holds no lock).  Returns true if there was one.
bool arena_drop_cached() {
  ArenaCache old;
  {
    std::lock_guard<std::mutex> lock(g_arena_mutex);
    old = g_arena_cache;
    g_arena_cache = ArenaCache{};
  }
  if (!old.ptr) return false;
  c4host::DeviceGuard guard(old.device);
  (void)hipFree(old.ptr);
  return true;
}
hipError_t arena_acquire(int device, size_t bytes, void** out) {
  {
    std::lock_guard<std::mutex> lock(g_arena_mutex);
    ArenaCache& c = g_arena_cache;
    if (c.ptr && c.device == device && c.bytes >= bytes && c.bytes / 2 <= bytes) {
      *out = c.ptr;
      c = ArenaCache{};
      return hipSuccess;
    }
  }
  hipError_t e = hipMalloc(out, bytes);
  if (e == hipErrorOutOfMemory && arena_drop_cached()) {   // a kept arena that does not fit this request must not cause its failure
    (void)hipGetLastError();
    e = hipMalloc(out, bytes);
  }
  return e;
}
void arena_release(int device, void* ptr, size_t bytes) {
  if (!ptr) return;
  void* drop = ptr;
  if (arena_cache_enabled()) {
    std::lock_guard<std::mutex> lock(g_arena_mutex);
    ArenaCache& c = g_arena_cache;
    if (!c.ptr || c.bytes < bytes) {       // keep the bigger one
      drop = c.ptr;
      if (drop && c.device != device) { c4host::DeviceGuard guard(c.device); (void)hipFree(drop); drop = nullptr; }
      c = ArenaCache{ptr, bytes, device};
    }
  }
  if (drop) (void)hipFree(drop);
}

static hipError_t reset_clock_acc(unsigned long long* acc_dev) {
  const unsigned long long init[5] = {0ull, 0ull, ~0ull, 0ull, 0ull};   // totals; running min start, max end, helpers done
  return hipMemcpy(acc_dev, init, sizeof init, hipMemcpyHostToDevice);
}

static int session_create_on_device(const c4_config* cfg, c4_session* s) {
  uint64_t bps = cfg->blocks_per_slot;
  const bool reclaim = reclaim_mode(cfg);
  if (reclaim) {
    s->reclaim_period = cfg->reclaim_period ? cfg->reclaim_period : kReclaimPeriod;
    if (bps == 0) {
      // automatic: 1.5 n blocks beyond the minimum, i.e. a compaction every second or third move of a game
      // (1 700 slots at n = 1 400: 1.8 GB where the never-reclaimed arena took 13 GB)
      uint64_t half = reclaim_half_min(cfg->n_mcts_iterations, s->reclaim_period, 2) + 3ull * cfg->n_mcts_iterations / 2;
      bps = 2 * (half > kMaxBlocksPerSlot / 2 ? kMaxBlocksPerSlot / 2 : half);
    }
    s->p.half_blocks = (uint32_t)(bps / 2);
    bps = 2ull * s->p.half_blocks;
  } else {
    // a search expands at most once per simulation and never re-roots: the root's own block + n, + slack
    if (bps == 0 && (cfg->flags & C4_FLAG_SEARCH)) bps = (uint64_t)cfg->n_mcts_iterations + 8;
    if (bps == 0) bps = 43ull * (cfg->n_mcts_iterations ? cfg->n_mcts_iterations : 1) + 8;
    if (bps < 2) bps = 2;
  }
  s->cfg.blocks_per_slot = (uint32_t)bps;
  const size_t n = cfg->n_slots;
  s->n_waves = s->n_waves_cap = (uint32_t)((n + kGamesPerWave - 1) / kGamesPerWave);
  Params& p = s->p;
  p.n_slots = cfg->n_slots;
  p.blocks_per_slot = (uint32_t)bps;
  p.n_iter = cfg->n_mcts_iterations;
  p.c_exploration = cfg->c_exploration;
  p.c_ply_penalty = cfg->c_ply_penalty;
  p.flags = cfg->flags;
  p.max_sims = (cfg->flags & (C4_FLAG_NO_MOVES | C4_FLAG_ONE_SIM_PER_STEP)) ? 1u : 2u;
  // visit counts stay below n_mcts_iterations + 1 in self-play (the gate); the table covers them with
  // room to spare, larger counts (C4_FLAG_NO_MOVES runs) take the computed path
  uint32_t n_ln = cfg->n_mcts_iterations + 64u;
  n_ln = n_ln < 1024u ? 1024u : (n_ln > 65536u ? 65536u : n_ln);
  hipError_t e;
  // one row of phase stamps per wavefront plus one per timing-helper workgroup (one helper per kWavesPerTimingHelper wavefronts)
  const size_t phase_rows = (size_t)s->n_waves_cap + (s->n_waves_cap + kWavesPerTimingHelper - 1) / kWavesPerTimingHelper + 1;
  if ((e = hipMalloc(&p.slots, n * sizeof(Slot))) != hipSuccess ||
      (e = arena_acquire(cfg->device, s->arena_bytes = n * bps * sizeof(Block), (void**)&p.blocks)) != hipSuccess ||
      (e = hipMalloc(&p.wave_ctr, (size_t)s->n_waves_cap * CTR_N * sizeof(unsigned long long))) != hipSuccess ||
      (e = hipMalloc(&p.glob, sizeof(Globals))) != hipSuccess ||
      (e = hipMalloc(&p.stamps, (size_t)s->n_waves_cap * 4 * sizeof(unsigned long long))) != hipSuccess ||
      (e = hipMalloc(&p.clock_acc, 5 * sizeof(unsigned long long))) != hipSuccess ||
      (e = hipMalloc(&p.phase, phase_rows * 16 * sizeof(unsigned long long))) != hipSuccess ||   // + the timing helper workgroups (diagnostic builds stamp them too)
      (e = hipMalloc(&s->ln_tab_dev, (size_t)n_ln * sizeof(float))) != hipSuccess ||
      (e = hipMalloc(&p.reclaim_ctr, 2 * sizeof(unsigned long long))) != hipSuccess ||
      (e = hipHostMalloc(&s->probe_host, sizeof(Globals))) != hipSuccess ||
      (e = hipEventCreateWithFlags(&s->probe_event, hipEventDisableTiming)) != hipSuccess)
    return fail(C4_ERR_HIP, std::string("allocating session (") + std::to_string((n * bps * sizeof(Block)) >> 20) +
                                " MiB of tree arena): " + hipGetErrorString(e));
  p.n_waves = s->n_waves;
  p.ln_tab = s->ln_tab_dev;
  p.n_ln = n_ln;
  hipLaunchKernelGGL(k_ln_table, dim3((n_ln + 255) / 256), dim3(256), 0, nullptr, s->ln_tab_dev, n_ln);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemset(p.stamps, 0, (size_t)s->n_waves_cap * 4 * sizeof(unsigned long long)));
  HIP_TRY(reset_clock_acc(p.clock_acc));
  HIP_TRY(hipMemset(p.phase, 0, phase_rows * 16 * sizeof(unsigned long long)));
  HIP_TRY(hipMemset(p.slots, 0, n * sizeof(Slot)));
  HIP_TRY(hipMemset(p.glob, 0, sizeof(Globals)));
  HIP_TRY(hipMemset(p.reclaim_ctr, 0, 2 * sizeof(unsigned long long)));
  HIP_TRY(hipMemset(p.wave_ctr, 0, (size_t)s->n_waves_cap * CTR_N * sizeof(unsigned long long)));
  memset(s->probe_host, 0, sizeof(Globals));
  return C4_OK;
}

// k_hold_resume on the session's stream: the arrays are device views (or null); fresh = c4_session_start's launch
static int hold_launch_resume(c4_session* s, const int32_t* cols, const float* temps, int32_t* results, bool fresh) {
  Params q = s->p;
  q.seq = 0;
  q.hold_cols = cols; q.hold_temps = temps; q.hold_results = results; q.hold_fresh = fresh ? 1u : 0u;
  s->hold_epoch++;   // what a probe enqueued before this point saw is history
  s->hold_probe_valid = false;
  HIP_TRY(hipMemsetAsync(&s->p.glob->hold_need, 0, sizeof(uint32_t), s->stream));
  if (fresh) HIP_TRY(hipMemsetAsync(&s->p.glob->hold_active, 0, sizeof(uint32_t), s->stream));   // every slot is counted anew
  with_planes(s->cfg.planes_dtype, [&](auto planes) {
    hipLaunchKernelGGL(k_hold_resume<decltype(planes)>, dim3((s->p.n_slots + 7) / 8), dim3(64), 0, s->stream, q);
  });
  HIP_TRY(hipGetLastError());
  return C4_OK;
}

static int launch_step(c4_session* s, const uint32_t* inverse, const float* answers, uint32_t n_unique) {
  if (!s) return fail(C4_ERR_BAD_ARG, "null session");
  if (!s->bound || !s->have_games) return fail(C4_ERR_NOT_BOUND, "bind_io and set_games must precede step");
  C4_ON_DEVICE(s->cfg.device);
  // launch sequence number for the device-clock stamps; frozen at 0 (= no per-launch timing) when
  // timing is off, which is what a launch captured into a HIP graph needs (arguments are baked in)
  s->p.seq = s->timing ? ++s->seq : 0;
  // the Dirichlet-noise and evaluation-cache extensions are separate instantiations: the default
  // kernel carries none of their registers or scratch
  const bool noise = s->p.dir_eps > 0.0f, cache = s->p.cache != nullptr;
#ifdef C4_DIAG_VARIANTS
  // C4_STEP_LDS_BYTES (diagnostic build only, tools/occupancy_probe.sh): unused dynamic LDS per workgroup caps the
  // wavefronts a CU holds (160 KB / bytes) without touching the code: how the launch time scales with occupancy
  static const unsigned lds_pad = [] { const char* e = getenv("C4_STEP_LDS_BYTES"); return e ? (unsigned)atoi(e) : 0u; }();
#else
  constexpr unsigned lds_pad = 0;
#endif
  // a timed launch (seq != 0) carries extra workgroups that fold the previous launch's stamps
  const uint32_t helpers = s->p.seq ? (s->n_waves + kWavesPerTimingHelper - 1) / kWavesPerTimingHelper : 0u;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(s->n_waves + helpers), dim3(64), lds_pad, s->stream, s->p.slots, s->p.logprobs, s->p.q, s->p.n_waves, s->p.n_slots, s->p);
  };
  auto launch_gather = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(s->n_waves + helpers), dim3(64), lds_pad, s->stream, s->p.slots, answers, inverse, n_unique, s->p.n_waves, s->p.n_slots, s->p);
  };
  // mode -> (NOISE, CACHE, SEARCH, HOLD) -> kernel.  A search and a hold session have ONE step kernel each: no noise, cache or
  // gather form (refused where they are asked for).
  with_planes(s->cfg.planes_dtype, [&](auto planes) {
    using P = decltype(planes);
    if (search_mode(s)) launch(c4_step_kernel<P, false, false, true>);
    else if (hold_mode(s)) launch(c4_step_kernel<P, false, false, false, true>);
    else with_flag(noise, [&](auto n) { with_flag(cache, [&](auto c) {
      constexpr bool NOISE = decltype(n)::value, CACHE = decltype(c)::value;
      if (inverse) launch_gather(c4_step_gather_kernel<P, NOISE, CACHE>); else launch(c4_step_kernel<P, NOISE, CACHE>);
    }); });
  });
  HIP_TRY(hipGetLastError());
  return maybe_reclaim(s);
}

}  // namespace

// One per-slot array of c4_session_hold_resume / c4_session_hold_undo as the kernel may use it: device memory and pinned host memory through
// device_view; pageable host memory (what HIP does not know) through the session's staging buffer `stage` (copied in now when
// `copy_in`).  *staged tells the caller which.
int hold_array(c4_session* s, const void* ptr, void** stage, bool copy_in, const char* what, void** out, bool* staged) {
  const size_t bytes = (size_t)s->cfg.n_slots * 4;
  *staged = false;
  hipPointerAttribute_t attr{};
  const hipError_t e = hipPointerGetAttributes(&attr, ptr);
  if (e == hipSuccess && attr.type != hipMemoryTypeUnregistered) return device_view(ptr, s->cfg.device, what, out);
  if (e != hipSuccess) (void)hipGetLastError();
  if (!*stage) HIP_TRY(hipMalloc(stage, bytes));
  if (copy_in) HIP_TRY(hipMemcpyAsync(*stage, ptr, bytes, hipMemcpyHostToDevice, s->stream));
  *out = *stage;
  *staged = true;
  return C4_OK;
}

int c4host::fail(int code, const std::string& msg) {
  g_last_error = msg;
  // HIP keeps a failed call's code as the thread's "last error" until somebody reads it; the launch checks of this library read it
  // (hipGetLastError after every launch), so a failed hipMalloc of ONE call -- device memory full -- used to surface as "out of
  // memory" in the next call's first launch, long after the memory was there again.  The failure is reported here: take it off.
  if (code == C4_ERR_HIP) (void)hipGetLastError();
  return code;
}

C4_TL_SETTER(c4_debug_timeline_session)

extern "C" {

const char* c4_last_error_string(void) { return g_last_error.c_str(); }
int c4_abi_version(void) { return C4_ABI_VERSION; }

#ifndef C4_SOURCE_HASH
#define C4_SOURCE_HASH "unknown"
#endif
// content hash of the sources this library was compiled from (c4a0_amd/csrc/build.py); the marker
// prefix lets the build script read it from the file's bytes without loading the library
const char* c4_source_hash(void) {
  static const char marked[] = "c4a0-src-hash:" C4_SOURCE_HASH;
  return marked + 14;
}

int c4_device_count(int* out) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) n = 0;
  if (out) *out = n;
  return C4_OK;
}

int c4_session_create(const c4_config* cfg, c4_session** out) {
  if (!cfg || !out) return fail(C4_ERR_BAD_ARG, "null argument");
  *out = nullptr;
  if (cfg->n_slots == 0) return fail(C4_ERR_BAD_ARG, "n_slots must be > 0");
  if (cfg->planes_dtype > 1) return fail(C4_ERR_BAD_ARG, "planes_dtype must be 0 (f32) or 1 (bf16)");
  if (cfg->blocks_per_slot > kMaxBlocksPerSlot) return fail(C4_ERR_BAD_ARG, "blocks_per_slot is limited to 65535 (16-bit child links)");
  // A game's arena is never reclaimed while it is played: every expansion of the whole game takes one
  // block, at most n_mcts_iterations per move and 42 moves, so 43 n + 8 blocks always suffice.  That
  // provable bound fits the 16-bit child links up to n = 1523 (the reference's own sweep tops out at
  // 1 500, src/c4a0/main.py:176).  Beyond it a long game could overflow its arena in the middle of a
  // job (C4_ERR_ARENA_OVERFLOW loses the whole call), so the default sizing is refused here, with the
  // reason; a caller who knows its games are short may still pass blocks_per_slot explicitly.
  // (From round 5 the default sizing switches to a RECLAIMED arena above 1 000 iterations, see C4_FLAG_RECLAIM: the live subtree is at
  // most n + a few blocks, so two halves of 2.5 n + 554 blocks (reclaim_half_min + 1.5 n of slack) serve any game and the links stay 16 bits wide up to n = 32 213.)
  // A search session (C4_FLAG_SEARCH) never moves: nothing to reclaim, nothing C4_FLAG_NO_MOVES would add, and a gate at 0 visits
  // would never be reached by a backup.
  if (cfg->flags & C4_FLAG_SEARCH) {
    if (cfg->flags & C4_FLAG_NO_MOVES) return fail(C4_ERR_BAD_ARG, "C4_FLAG_SEARCH and C4_FLAG_NO_MOVES exclude each other: a search ends at n_mcts_iterations visits and hands its slot on");
    if (cfg->flags & C4_FLAG_RECLAIM) return fail(C4_ERR_BAD_ARG, "C4_FLAG_SEARCH: a search never moves, so its arena (n_mcts_iterations + 8 blocks) has nothing to reclaim (C4_FLAG_RECLAIM)");
    if (cfg->n_mcts_iterations == 0) return fail(C4_ERR_BAD_ARG, "C4_FLAG_SEARCH needs n_mcts_iterations >= 1");
  }
  // A hold session (C4_FLAG_HOLD) moves when it is told to and searches up to a target: a step-kernel instantiation of its own, like
  // a search session's, with no noise, cache, reclaim or never-moving form; its never-reclaimed arena holds a root's n new
  // simulations for each of a game's 42 roots at most.
  if (cfg->flags & C4_FLAG_HOLD) {
    if (cfg->flags & C4_FLAG_SEARCH) return fail(C4_ERR_BAD_ARG, "C4_FLAG_HOLD and C4_FLAG_SEARCH exclude each other: a search hands its slot on after one record, a held game keeps it");
    if (cfg->flags & C4_FLAG_NO_MOVES) return fail(C4_ERR_BAD_ARG, "C4_FLAG_HOLD and C4_FLAG_NO_MOVES exclude each other: a held game parks at its target and moves when c4_session_hold_resume says so");
    if (cfg->flags & C4_FLAG_RECLAIM) return fail(C4_ERR_BAD_ARG, "C4_FLAG_HOLD: a held game's arena is never reclaimed (C4_FLAG_RECLAIM): the subtree under a move is kept in place");
    if (cfg->n_mcts_iterations == 0) return fail(C4_ERR_BAD_ARG, "C4_FLAG_HOLD needs n_mcts_iterations >= 1 (the largest target c4_session_set_iterations may ask for)");
  }
  if (reclaim_mode(cfg)) {
    const uint32_t period = cfg->reclaim_period ? cfg->reclaim_period : kReclaimPeriod;
    const uint64_t need = reclaim_half_min(cfg->n_mcts_iterations, period, 2);
    const uint64_t half = cfg->blocks_per_slot ? cfg->blocks_per_slot / 2 : kMaxBlocksPerSlot / 2;
    if (cfg->flags & C4_FLAG_NO_MOVES) return fail(C4_ERR_BAD_ARG, "C4_FLAG_RECLAIM: a search that never moves never frees anything (C4_FLAG_NO_MOVES)");
    if (cfg->flags & C4_FLAG_NO_RECLAIM) return fail(C4_ERR_BAD_ARG, "C4_FLAG_RECLAIM and C4_FLAG_NO_RECLAIM exclude each other");
    if (period > 4096) return fail(C4_ERR_BAD_ARG, "reclaim_period is limited to 4096 step launches");
    if (half < need)
      return fail(C4_ERR_BAD_ARG, "reclaimed arena too small: each half must hold the live subtree (n_mcts_iterations + simulations per launch + 8 blocks) and the blocks of 4 x "
                                  "reclaim_period step launches (" + std::to_string(need) + " blocks per half, i.e. blocks_per_slot >= " + std::to_string(2 * need) +
                                  "; a half is at most 32 767 blocks: n_mcts_iterations <= " + std::to_string(kMaxBlocksPerSlot / 2 - (need - cfg->n_mcts_iterations)) + ")");
  } else if ((cfg->flags & C4_FLAG_SEARCH) && cfg->blocks_per_slot == 0 && (uint64_t)cfg->n_mcts_iterations + 8 > kMaxBlocksPerSlot)
    return fail(C4_ERR_BAD_ARG, "C4_FLAG_SEARCH: n_mcts_iterations + 8 blocks per slot exceed 65535 (16-bit child links)");
  else if (!(cfg->flags & C4_FLAG_SEARCH) && cfg->blocks_per_slot == 0 && 43ull * cfg->n_mcts_iterations + 8 > kMaxBlocksPerSlot)
    return fail(C4_ERR_BAD_ARG, "n_mcts_iterations > 1523 is not supported with a never-reclaimed arena (C4_FLAG_NO_MOVES / C4_FLAG_NO_RECLAIM): a game's tree arena is limited to "
                                "65535 blocks (16-bit child links; up to 43 n + 8 blocks per game). "
                                "Pass blocks_per_slot explicitly to accept C4_ERR_ARENA_OVERFLOW on long searches");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(C4_ERR_NO_DEVICE, "no HIP device visible");
  if (cfg->device < 0 || cfg->device >= ndev) return fail(C4_ERR_BAD_ARG, "device ordinal out of range");
  C4_ON_DEVICE(cfg->device);
  c4_session* s = new c4_session();
  s->cfg = *cfg;
  const int rc = session_create_on_device(cfg, s);
  if (rc != C4_OK) {   // every failure path releases what was allocated (the message survives destroy)
    const std::string msg = g_last_error;
    c4_session_destroy(s);
    return fail(rc, msg);
  }
  *out = s;
  return C4_OK;
}

int c4_session_destroy(c4_session* s) {
  if (!s) return C4_OK;
  c4host::DeviceGuard guard(s->cfg.device);
  if (s->stream) (void)hipStreamSynchronize(s->stream); else (void)hipDeviceSynchronize();
  (void)hipFree(s->p.slots); arena_release(s->cfg.device, s->p.blocks, s->arena_bytes); (void)hipFree(s->p.wave_ctr); (void)hipFree(s->p.glob); (void)hipFree(s->p.stamps); (void)hipFree(s->p.clock_acc); (void)hipFree(s->p.phase); (void)hipFree(s->p.reclaim_ctr);
  (void)hipFree(s->p.samples); (void)hipFree(s->p.sample_counts); (void)hipFree(s->p.cache);
  (void)hipFree(s->plan_dev); (void)hipFree(s->pairs_dev); (void)hipFree(s->offsets_dev); (void)hipFree(s->ln_tab_dev);
  if (s->total_host) (void)hipHostFree(s->total_host);
  (void)hipFree(s->uniq_tab); (void)hipFree(s->uniq_cell); (void)hipFree(s->uniq_row); (void)hipFree(s->uniq_count);
  (void)hipFree(s->reqs_dev); (void)hipFree(s->start_mask_dev); (void)hipFree(s->start_value_dev);
  (void)hipFree(s->hold_cols_dev); (void)hipFree(s->hold_temps_dev); (void)hipFree(s->hold_results_dev); (void)hipFree(s->snap_dev);
  if (s->snap_host) (void)hipHostFree(s->snap_host);
  if (s->probe_host) (void)hipHostFree(s->probe_host);
  if (s->probe_event) (void)hipEventDestroy(s->probe_event);
  delete s;
  return C4_OK;
}

int c4_trim_cached_memory(void) {
  ArenaCache c;
  {
    std::lock_guard<std::mutex> lock(g_arena_mutex);
    c = g_arena_cache;
    g_arena_cache = ArenaCache{};
  }
  if (c.ptr) {
    c4host::DeviceGuard guard(c.device);
    HIP_TRY(hipFree(c.ptr));
  }
  return C4_OK;
}

int c4_session_set_games(c4_session* s, const c4_game_metadata* reqs, uint64_t n_games,
                         const uint64_t* start_masks, const uint64_t* start_values) {
  if (!s || (!reqs && n_games)) return fail(C4_ERR_BAD_ARG, "null argument");
  if ((start_masks == nullptr) != (start_values == nullptr)) return fail(C4_ERR_BAD_ARG, "start_masks and start_values go together");
  if (n_games >= (1ull << 32) - 1) return fail(C4_ERR_BAD_ARG, "too many games for one session");
  if (hold_mode(s) && n_games > s->cfg.n_slots)
    return fail(C4_ERR_BAD_ARG, "c4_session_set_games: a hold session (C4_FLAG_HOLD) keeps request i on slot i for good: " + std::to_string(n_games) +
                                    " games do not fit " + std::to_string(s->cfg.n_slots) + " slots");
  C4_ON_DEVICE(s->cfg.device);
  HIP_TRY(hipStreamSynchronize(s->stream));
  (void)hipFree(s->reqs_dev); (void)hipFree(s->start_mask_dev); (void)hipFree(s->start_value_dev);
  (void)hipFree(s->p.samples); (void)hipFree(s->p.sample_counts); (void)hipFree(s->offsets_dev);
  s->reqs_dev = nullptr; s->start_mask_dev = s->start_value_dev = nullptr;
  s->p.samples = nullptr; s->p.sample_counts = nullptr; s->offsets_dev = nullptr;
  const size_t ng = n_games ? n_games : 1;
  HIP_TRY(hipMalloc(&s->offsets_dev, (ng + 1) * sizeof(unsigned long long)));
  if (!s->total_host) HIP_TRY(hipHostMalloc(&s->total_host, sizeof(unsigned long long)));
  HIP_TRY(hipMalloc(&s->reqs_dev, ng * sizeof(c4_game_metadata)));
  HIP_TRY(hipMalloc(&s->p.samples, ng * C4_MAX_SAMPLES_PER_GAME * sizeof(c4_sample_rec)));
  HIP_TRY(hipMalloc(&s->p.sample_counts, ng * sizeof(uint32_t)));
  HIP_TRY(hipMemset(s->p.sample_counts, 0, ng * sizeof(uint32_t)));
  if (n_games) HIP_TRY(hipMemcpy(s->reqs_dev, reqs, n_games * sizeof(c4_game_metadata), hipMemcpyHostToDevice));
  if (start_masks && n_games) {
    HIP_TRY(hipMalloc(&s->start_mask_dev, n_games * 8));
    HIP_TRY(hipMalloc(&s->start_value_dev, n_games * 8));
    HIP_TRY(hipMemcpy(s->start_mask_dev, start_masks, n_games * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(s->start_value_dev, start_values, n_games * 8, hipMemcpyHostToDevice));
  }
  s->p.n_slots = s->cfg.n_slots;   // a compacted session goes back to its full width
  s->n_waves = s->p.n_waves = (s->cfg.n_slots + kGamesPerWave - 1) / kGamesPerWave;
  Globals g0{};
  g0.queue_head = n_games < s->cfg.n_slots ? n_games : s->cfg.n_slots;
  HIP_TRY(hipMemcpy(s->p.glob, &g0, sizeof g0, hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(s->p.wave_ctr, 0, (size_t)s->n_waves_cap * CTR_N * sizeof(unsigned long long)));
  s->p.reqs = s->reqs_dev;
  s->p.start_mask = s->start_mask_dev;
  s->p.start_value = s->start_value_dev;
  s->p.n_games = n_games;
  s->n_games = n_games;
  s->have_games = true;
  HIP_TRY(hipMemset(s->p.stamps, 0, (size_t)s->n_waves_cap * 4 * sizeof(unsigned long long)));
  HIP_TRY(reset_clock_acc(s->p.clock_acc));
  // a new list of games may come with new evaluator weights: forget the old evaluations
  if (s->p.cache) HIP_TRY(hipMemset(s->p.cache, 0, ((size_t)s->p.cache_mask + 1) * 64));
  s->seq = 0;
  s->reclaim_count = 0; s->reclaim_capture_id = 0;
  HIP_TRY(hipMemset(s->p.reclaim_ctr, 0, 2 * sizeof(unsigned long long)));
  s->probe_pending = false; s->probe_done = 0; s->probe_error = 0;
  s->hold_epoch++; s->hold_probe_valid = false;
  return C4_OK;
}

int c4_session_bind_io(c4_session* s, void* planes_dev, const float* logprobs_dev, const float* q_dev, void* stream) {
  if (!s || !planes_dev || !logprobs_dev || !q_dev) return fail(C4_ERR_BAD_ARG, "null argument");
  // the tensors and the stream must live on the session's device: a pointer of another device (or of
  // the host) would only fault later, inside a kernel, far from its cause
  C4_ON_DEVICE(s->cfg.device);
  const struct { const void* ptr; const char* name; } io[3] = {{planes_dev, "planes_dev"}, {logprobs_dev, "logprobs_dev"}, {q_dev, "q_dev"}};
  for (const auto& t : io) {
    hipPointerAttribute_t attr{};
    const hipError_t e = hipPointerGetAttributes(&attr, t.ptr);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      return fail(C4_ERR_BAD_ARG, std::string("c4_session_bind_io: ") + t.name + " is not a device pointer known to HIP (" + hipGetErrorString(e) + ")");
    }
    if (attr.type != hipMemoryTypeDevice && attr.type != hipMemoryTypeManaged)
      return fail(C4_ERR_BAD_ARG, std::string("c4_session_bind_io: ") + t.name + " is not device memory");
    if (attr.type == hipMemoryTypeDevice && attr.device != s->cfg.device)
      return fail(C4_ERR_BAD_ARG, std::string("c4_session_bind_io: ") + t.name + " lives on device " + std::to_string(attr.device) +
                                      ", the session on device " + std::to_string(s->cfg.device));
  }
  if (stream != nullptr) {
    int sdev = -1;
    if (hipStreamGetDevice((hipStream_t)stream, &sdev) == hipSuccess && sdev >= 0 && sdev != s->cfg.device)
      return fail(C4_ERR_BAD_ARG, "c4_session_bind_io: the stream belongs to device " + std::to_string(sdev) + ", the session to device " +
                                      std::to_string(s->cfg.device));
  }
  s->p.planes = planes_dev;
  s->p.logprobs = logprobs_dev;
  s->p.q = q_dev;
  s->stream = (hipStream_t)stream;
  s->bound = true;
  return C4_OK;
}

int c4_session_set_dirichlet(c4_session* s, float alpha, float epsilon) {
  if (!s) return fail(C4_ERR_BAD_ARG, "null session");
  if (!(epsilon >= 0.0f && epsilon <= 1.0f) || (epsilon > 0.0f && !(alpha > 0.0f))) return fail(C4_ERR_BAD_ARG, "need 0 <= epsilon <= 1 and alpha > 0");
  if (epsilon > 0.0f) if (int rc = refuse_search_hold(s, "c4_session_set_dirichlet", "has no Dirichlet-noise step kernel")) return rc;
  s->p.dir_alpha = alpha;
  s->p.dir_eps = epsilon;
  return C4_OK;
}

int c4_session_bind_leaf_models(c4_session* s, uint64_t* leaf_models_dev) {
  if (!s) return fail(C4_ERR_BAD_ARG, "null session");
  if (leaf_models_dev) if (int rc = refuse_search_hold(s, "c4_session_bind_leaf_models", "has ONE evaluator", " (a match is two sessions exchanging moves)")) return rc;
  if (leaf_models_dev && s->p.cache) return fail(C4_ERR_BAD_ARG, "the evaluation cache holds ONE evaluator's outputs: not with multi-model games");
  s->p.leaf_models = leaf_models_dev;
  return C4_OK;
}

int c4_session_set_eval_cache(c4_session* s, uint64_t n_entries, uint32_t max_sims_per_step) {
  if (!s) return fail(C4_ERR_BAD_ARG, "null session");
  if (n_entries && s->p.leaf_models) return fail(C4_ERR_BAD_ARG, "the evaluation cache holds ONE evaluator's outputs: not with multi-model games");
  if (n_entries > (1ull << 31)) return fail(C4_ERR_BAD_ARG, "at most 2^31 cache entries");
  if (n_entries) if (int rc = refuse_search_hold(s, "c4_session_set_eval_cache", "has no evaluation-cache step kernel")) return rc;
  C4_ON_DEVICE(s->cfg.device);
  HIP_TRY(hipStreamSynchronize(s->stream));
  (void)hipFree(s->p.cache);
  s->p.cache = nullptr;
  s->p.cache_mask = 0;
  const bool single = (s->cfg.flags & (C4_FLAG_NO_MOVES | C4_FLAG_ONE_SIM_PER_STEP)) != 0;
  s->p.max_sims = single ? 1u : 2u;
  if (n_entries == 0) return C4_OK;
  uint64_t n = 1024;
  while (n < n_entries) n <<= 1;
  HIP_TRY(hipMalloc(&s->p.cache, n * 64));
  HIP_TRY(hipMemset(s->p.cache, 0, n * 64));   // an all-zero entry does not validate (its dwords XOR to 0, not to the seal constant)
  s->p.cache_mask = (uint32_t)(n - 1);
  if (!single) s->p.max_sims = max_sims_per_step ? (max_sims_per_step > 64 ? 64u : max_sims_per_step) : 6u;   // measured at BASELINE config 2: 4 -> 43.3 k, 6 -> 45.5 k, 8 -> 44.8 k games/s
  if (s->p.half_blocks) {   // a reclaimed half holds the blocks of 4 x reclaim_period launches: as many simulations per launch as that allows
    if (s->p.max_sims > kReclaimMaxSims) s->p.max_sims = kReclaimMaxSims;
    while (s->p.max_sims > 2 && reclaim_half_min(s->p.n_iter, s->reclaim_period, s->p.max_sims) > s->p.half_blocks) s->p.max_sims--;
    // more simulations per launch = a larger margin to keep free: the next step launch is followed by a look at the arenas with
    // the new margin, whatever the count since the last one (a slot left with just over the OLD margin could otherwise
    // take reclaim_period launches of the new width before the next look)
    s->reclaim_count = 0;
  }
  return C4_OK;
}

int c4_session_start(c4_session* s) {
  if (!s) return fail(C4_ERR_BAD_ARG, "null session");
  if (!s->bound || !s->have_games) return fail(C4_ERR_NOT_BOUND, "bind_io and set_games must precede start");
  C4_ON_DEVICE(s->cfg.device);
  if (hold_mode(s)) return hold_launch_resume(s, nullptr, nullptr, nullptr, true);   // reset_slot + the one kernel that makes a game active
  with_planes(s->cfg.planes_dtype, [&](auto planes) {
    hipLaunchKernelGGL(c4_start_kernel<decltype(planes)>, dim3((s->p.n_slots + 7) / 8), dim3(64), 0, s->stream, s->p);
  });
  HIP_TRY(hipGetLastError());
  return C4_OK;
}

int c4_session_step(c4_session* s) { return launch_step(s, nullptr, nullptr, 0); }

int c4_session_step_gather(c4_session* s, const uint32_t* inverse_dev, const float* answers, uint32_t n_unique) {
  if (!s || !inverse_dev || (!answers && n_unique)) return fail(C4_ERR_BAD_ARG, "null argument");
  if (int rc = refuse_search_hold(s, "c4_session_step_gather", "takes a device evaluator, not the callback mode's batches")) return rc;
  if (!s->bound) return fail(C4_ERR_NOT_BOUND, "c4_session_step_gather: bind_io first");
  void *inv = nullptr, *ans = nullptr;
  {
    C4_ON_DEVICE(s->cfg.device);
    if (int rc = device_view(inverse_dev, s->cfg.device, "c4_session_step_gather: inverse_dev", &inv)) return rc;
    if (answers) if (int rc = device_view(answers, s->cfg.device, "c4_session_step_gather: answers", &ans)) return rc;
  }
  return launch_step(s, (const uint32_t*)inv, (const float*)ans, n_unique);
}

int c4_session_step_head_out(c4_session* s, const void* hidden_policy_dev, const void* hidden_value_dev, const void* w_policy_dev,
                             const void* w_value_dev, const float* b_policy_dev, const float* b_value_dev, uint32_t features,
                             uint32_t policy_row_stride, uint32_t value_row_stride) {
  if (!s) return fail(C4_ERR_BAD_ARG, "null session");
  if (!s->bound || !s->have_games) return fail(C4_ERR_NOT_BOUND, "bind_io and set_games must precede step");
  if (!hidden_policy_dev || !hidden_value_dev || !w_policy_dev || !w_value_dev || !b_policy_dev || !b_value_dev)
    return fail(C4_ERR_BAD_ARG, "c4_session_step_head_out: null argument");
  if (features % 8 != 0 || policy_row_stride % 8 != 0 || value_row_stride % 8 != 0 || (features / 8) % (4 * c4ho::kHeadSteps * c4ho::kHeadWaves) != 0)
    return fail(C4_ERR_BAD_ARG, "c4_session_step_head_out: features must be a multiple of 1 344 (42 x 32 channels) and the row strides of 8 elements");
  if (s->p.dir_eps > 0.0f || s->p.cache != nullptr || s->timing)
    return fail(C4_ERR_BAD_ARG, "c4_session_step_head_out: the fused launch exists for the default configuration only (no Dirichlet noise, no evaluation "
                                "cache, per-launch timing off): call c4_head_out_bf16 and c4_session_step");
  C4_ON_DEVICE(s->cfg.device);
  s->p.seq = 0;
  const uint32_t groups = (s->p.n_slots + 15) / 16;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(groups), dim3(64 * c4ho::kHeadWaves), 0, s->stream, (const uint4*)hidden_policy_dev, (const uint4*)hidden_value_dev,
                       (const uint4*)w_policy_dev, (const uint4*)w_value_dev, b_policy_dev, b_value_dev, s->p.slots, s->p.n_slots, features / 8,
                       policy_row_stride / 8, value_row_stride / 8, s->p);
  };
  // kGpw, mode -> kernel.  A search's and a hold session's fused launch exist for bf16 planes alone: refused here, not instantiated.
  if (search_mode(s) && s->cfg.planes_dtype == 0)
    return fail(C4_ERR_BAD_ARG, "c4_session_step_head_out: a search session's fused launch is built for bf16 planes (planes_dtype 1): call c4_head_out_bf16 and c4_session_step");
  if (hold_mode(s) && s->cfg.planes_dtype == 0)
    return fail(C4_ERR_BAD_ARG, "c4_session_step_head_out: a hold session's fused launch is built for bf16 planes (planes_dtype 1): call c4_head_out_bf16 and c4_session_step");
  with_flag(s->out_step_gpw == 4, [&](auto four) {
    constexpr uint32_t kGpw = decltype(four)::value ? 4 : 8;
    if (search_mode(s)) launch(c4_out_step_kernel<uint16_t, kGpw, true>);
    else if (hold_mode(s)) launch(c4_out_step_kernel<uint16_t, kGpw, false, true>);
    else with_planes(s->cfg.planes_dtype, [&](auto planes) { launch(c4_out_step_kernel<decltype(planes), kGpw>); });
  });
  HIP_TRY(hipGetLastError());
  return maybe_reclaim(s);
}

// Games per stepping wavefront of the fused output + step launch: 8 (default) or 4 (see c4_out_step_kernel).  A scheduling knob: the
// games' records do not depend on it.
int c4_session_set_step_shape(c4_session* s, uint32_t games_per_wavefront) {
  if (!s) return fail(C4_ERR_BAD_ARG, "null session");
  if (games_per_wavefront != 4 && games_per_wavefront != 8) return fail(C4_ERR_BAD_ARG, "c4_session_set_step_shape: games_per_wavefront must be 4 or 8");
  s->out_step_gpw = games_per_wavefront;
  return C4_OK;
}

int c4_session_set_timing(c4_session* s, int enable) {
  if (!s) return fail(C4_ERR_BAD_ARG, "null session");
  C4_ON_DEVICE(s->cfg.device);
  HIP_TRY(hipStreamSynchronize(s->stream));
  // fold nothing across the switch: restart the stamp buffers
  HIP_TRY(hipMemset(s->p.stamps, 0, (size_t)s->n_waves_cap * 4 * sizeof(unsigned long long)));
  if (enable && !s->timing) s->seq = 0;
  s->timing = enable != 0;
  return C4_OK;
}

int c4_session_counters(c4_session* s, c4_counters* out) {
  if (!s || !out) return fail(C4_ERR_BAD_ARG, "null argument");
  C4_ON_DEVICE(s->cfg.device);
  HIP_TRY(hipStreamSynchronize(s->stream));
  std::vector<unsigned long long> h((size_t)s->n_waves_cap * CTR_N);   // waves retired by a compaction keep their counts
  HIP_TRY(hipMemcpy(h.data(), s->p.wave_ctr, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  Globals g{};
  HIP_TRY(hipMemcpy(&g, s->p.glob, sizeof g, hipMemcpyDeviceToHost));
  unsigned long long sum[CTR_N] = {0};
  for (size_t w = 0; w < s->n_waves_cap; w++)
    for (int k = 0; k < CTR_N; k++) sum[k] += h[w * CTR_N + k];
  memset(out, 0, sizeof *out);
  out->sims = sum[CTR_SIMS]; out->select_levels = sum[CTR_S]; out->backup_nodes = sum[CTR_K];
  out->expansions = sum[CTR_E]; out->moves = sum[CTR_MOVES]; out->games_done = sum[CTR_DONE];
  out->ref_skipped_sims = sum[CTR_SKIPPED]; out->samples = sum[CTR_SAMPLES];
  out->eval_cache_probes = sum[CTR_PROBES]; out->eval_cache_hits = sum[CTR_HITS];
  out->games_started = g.queue_head < s->n_games ? g.queue_head : s->n_games;
  out->error = g.error; out->error_slot = g.error_slot;
  unsigned long long rc2[2] = {0, 0};
  HIP_TRY(hipMemcpy(rc2, s->p.reclaim_ctr, sizeof rc2, hipMemcpyDeviceToHost));
  out->reclaim_passes = rc2[0]; out->reclaim_blocks = rc2[1];
  // device-clock time of the step kernel: launches already folded in by the following launch,
  // plus the last one from its raw stamps
  unsigned long long acc[2] = {0, 0};
  HIP_TRY(hipMemcpy(acc, s->p.clock_acc, sizeof acc, hipMemcpyDeviceToHost));
  if (s->seq > 0) {
    std::vector<unsigned long long> st((size_t)s->n_waves * 2);
    HIP_TRY(hipMemcpy(st.data(), s->p.stamps + (size_t)(s->seq & 1) * s->n_waves * 2, st.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long lo = ~0ull, hi = 0ull;
    for (size_t w = 0; w < s->n_waves; w++) { if (st[2 * w] < lo) lo = st[2 * w]; if (st[2 * w + 1] > hi) hi = st[2 * w + 1]; }
    if (hi > lo) { acc[0] += hi - lo; acc[1] += 1; }
  }
  out->step_kernel_ns = acc[0] * 10ull;  // s_memrealtime ticks at 100 MHz
  out->step_launches = acc[1];
  return C4_OK;
}

int c4_session_poll(c4_session* s, uint64_t* games_done, uint32_t* error) {
  if (!s) return fail(C4_ERR_BAD_ARG, "null session");
  C4_ON_DEVICE(s->cfg.device);
  if (s->probe_pending && hipEventQuery(s->probe_event) == hipSuccess) {
    s->probe_done = s->probe_host->games_done;
    s->probe_started = s->probe_host->queue_head < s->n_games ? s->probe_host->queue_head : s->n_games;
    s->probe_error = s->probe_host->error;
    if (s->probe_epoch == s->hold_epoch) {   // (hold sessions) enqueued behind the last c4_session_hold_resume
      s->hold_probe_valid = true;
      s->hold_probe_active = s->probe_host->hold_active;
      s->hold_probe_need = s->probe_host->hold_need;
    }
    s->probe_pending = false;
  }
  if (!s->probe_pending) {
    HIP_TRY(hipMemcpyAsync(s->probe_host, s->p.glob, sizeof(Globals), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipEventRecord(s->probe_event, s->stream));
    s->probe_pending = true;
    s->probe_epoch = s->hold_epoch;
  }
  if (games_done) *games_done = s->probe_done;
  if (error) *error = s->probe_error;
  return C4_OK;
}

int c4_session_progress(c4_session* s, uint64_t* games_done, uint64_t* games_started, uint32_t* error) {
  const int rc = c4_session_poll(s, games_done, error);
  if (rc == C4_OK && games_started) *games_started = s->probe_started;
  return rc;
}

// ---- hold sessions (C4_FLAG_HOLD): target, moves from outside (snapshot and probe: c4_session_readout.hip) ----
int c4_session_set_iterations(c4_session* s, uint32_t n_mcts_iterations) {
  if (!s) return fail(C4_ERR_BAD_ARG, "null session");
  if (!hold_mode(s)) return fail(C4_ERR_BAD_ARG, "c4_session_set_iterations: not a hold session (C4_FLAG_HOLD); a session of games or searches keeps the n_mcts_iterations it was created with");
  if (n_mcts_iterations < 1 || n_mcts_iterations > s->cfg.n_mcts_iterations)
    return fail(C4_ERR_BAD_ARG, "c4_session_set_iterations: the target must be between 1 and the n_mcts_iterations the session was created with (" +
                                    std::to_string(s->cfg.n_mcts_iterations) + "), which sizes its tree arena and its table of logarithms");
  s->p.n_iter = n_mcts_iterations;   // a kernel argument of every later launch: stream-ordered by construction
  return C4_OK;
}

int c4_session_hold_resume(c4_session* s, const int32_t* cols, const float* temperatures, int32_t* results) {
  if (!s) return fail(C4_ERR_BAD_ARG, "null session");
  if (!hold_mode(s)) return fail(C4_ERR_BAD_ARG, "c4_session_hold_resume: not a hold session (C4_FLAG_HOLD)");
  if (!s->bound || !s->have_games) return fail(C4_ERR_NOT_BOUND, "bind_io and set_games must precede c4_session_hold_resume");
  if (!cols && (temperatures || results)) return fail(C4_ERR_BAD_ARG, "c4_session_hold_resume: temperatures and results go with cols");
  C4_ON_DEVICE(s->cfg.device);
  void *c = nullptr, *t = nullptr, *r = nullptr;
  bool sc = false, st = false, sr = false;
  if (cols) if (int rc = hold_array(s, cols, (void**)&s->hold_cols_dev, true, "c4_session_hold_resume: cols", &c, &sc)) return rc;
  if (temperatures) if (int rc = hold_array(s, temperatures, (void**)&s->hold_temps_dev, true, "c4_session_hold_resume: temperatures", &t, &st)) return rc;
  if (results) if (int rc = hold_array(s, results, (void**)&s->hold_results_dev, false, "c4_session_hold_resume: results", &r, &sr)) return rc;
  if (int rc = hold_launch_resume(s, (const int32_t*)c, (const float*)t, (int32_t*)r, false)) return rc;
  if (sr) HIP_TRY(hipMemcpyAsync(results, r, (size_t)s->cfg.n_slots * 4, hipMemcpyDeviceToHost, s->stream));
  if (sc || st || sr) HIP_TRY(hipStreamSynchronize(s->stream));   // pageable host memory: the caller's arrays are done with when the call returns
  return C4_OK;
}

// (the parity tests' entry point of k_dirichlet, see there)
int c4_dirichlet(const uint64_t* game_id_dev, const uint32_t* n_moves_dev, const uint32_t* legal_dev, float alpha, uint64_t n,
                 float* eta_dev, void* stream) {
  if (n == 0) return C4_OK;
  C4_ON_STREAM_DEVICE(stream);
  hipLaunchKernelGGL(k_dirichlet, grid_for(n, 64), dim3(64), 0, (hipStream_t)stream, game_id_dev, n_moves_dev, legal_dev, alpha, n, eta_dev);
  HIP_TRY(hipGetLastError());
  return C4_OK;
}

}  // extern "C"
