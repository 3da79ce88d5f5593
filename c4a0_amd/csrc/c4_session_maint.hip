// c4_session_maint.hip -- what keeps a running session's memory in shape between steps: tail compaction (c4_session_compact),
// the reclaimed arenas (C4_FLAG_RECLAIM: k_arena_reclaim behind every reclaim_period-th step launch) and a hold session's undo
// (c4_session_hold_undo: k_hold_undo in front of the resume launch).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/c4a0_hip.h"
#include "c4_device.hpp"
#include "c4_host.hpp"
#include "c4_session_impl.hpp"
#include "c4_tree.hpp"

#pragma clang fp contract(off)

namespace {

using c4host::fail;
using c4host::with_planes;

// ------------------------------------------------------------------------------------------
// Tail compaction: once the request queue is empty, finished slots stay empty and the evaluator
// would keep computing rows for them.  k_compact_plan pairs every active slot beyond the first A
// slots (A = number of active games) with an idle slot below A; k_compact_move copies the game
// (slot state, the used part of its arena, its evaluator input row) across.  All references inside
// a game's state are arena-relative, so nothing needs patching.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_compact_plan(const Slot* slots, uint32_t n_slots, CompactPlan* plan, uint2* pairs) {
  __shared__ uint32_t s_active, s_holes, s_movers;
  if (threadIdx.x == 0) { s_active = 0; s_holes = 0; s_movers = 0; }
  __syncthreads();
  uint32_t mine = 0;
  for (uint32_t g = threadIdx.x; g < n_slots; g += blockDim.x) mine += slot_status(slots[g].state) == kActive ? 1u : 0u;
  atomicAdd(&s_active, mine);
  __syncthreads();
  const uint32_t A = s_active;
  // any bijection between holes (< A, idle) and movers (>= A, active) will do: which slot plays a
  // game changes nothing a game records
  for (uint32_t g = threadIdx.x; g < n_slots; g += blockDim.x) {
    const bool act = slot_status(slots[g].state) == kActive;
    if (g < A && !act) pairs[atomicAdd(&s_holes, 1u)].y = g;
    if (g >= A && act) pairs[atomicAdd(&s_movers, 1u)].x = g;
  }
  __syncthreads();
  if (threadIdx.x == 0) { plan->n_active = A; plan->n_pairs = s_movers; }
}

template <typename PlaneT>
__global__ __launch_bounds__(256) void k_compact_move(Params p, const CompactPlan* plan, const uint2* pairs) {
  const uint32_t k = blockIdx.x;
  if (k >= plan->n_pairs) return;
  const uint32_t src = pairs[k].x, dst = pairs[k].y;
  const Slot* ss = p.slots + src;
  const uint32_t n_blocks = ss->arena & 0xFFFFu;
  const uint4* sb = reinterpret_cast<const uint4*>(p.blocks + (size_t)src * p.blocks_per_slot);
  uint4* db = reinterpret_cast<uint4*>(p.blocks + (size_t)dst * p.blocks_per_slot);
  for (uint32_t i = threadIdx.x; i < n_blocks * 8u; i += blockDim.x) db[i] = sb[i];
  PlaneT* pl = reinterpret_cast<PlaneT*>(p.planes);
  for (uint32_t e = threadIdx.x; e < C4_PLANES_LEN; e += blockDim.x) pl[(size_t)dst * C4_PLANES_LEN + e] = pl[(size_t)src * C4_PLANES_LEN + e];
  if (threadIdx.x < 16) reinterpret_cast<uint4*>(p.slots + dst)[threadIdx.x] = reinterpret_cast<const uint4*>(ss)[threadIdx.x];
  __syncthreads();
  if (threadIdx.x == 0) { p.slots[src].state = kIdle; p.slots[src].ordinal = 0xFFFFFFFFu; }
}

// ------------------------------------------------------------------------------------------
// Reclaimed arenas (C4_FLAG_RECLAIM).  The reference drops the siblings' subtrees at every move (mcts.rs:187-206: the new
// root's Rc is the only one left); the never-reclaimed arena keeps them, which is what bounds n_mcts_iterations by the 16-bit
// child links (43 n + 8 <= 65 535 blocks).  Here a slot's arena is two halves of half_blocks blocks.  A game allocates in one of
// them; when that half runs short, this kernel -- launched behind every reclaim_period-th step launch, between two steps, when
// every game waits for the evaluator with a recorded path -- copies what is still reachable into the other half, compactly:
//   new[0] = the block that holds the root's OWN entry (level 0 of every backup),  new[1] = the root's children block,
//   then breadth first: the workgroup walks the copied blocks in order; a block's children are copied to the next free
//   places and its links patched.  An old block's forwarding address goes into its tail's `legal` half-word (written by
//   expansion, read by nobody), from which the recorded path (entry refs = block << 3 | column) is translated at the end.
// Reachable blocks number at most (visits of the root + simulations of one launch + 2) <= half_blocks, so the copy always fits.
// One workgroup of 1 024 threads per slot (128 lane groups of 8: a block is one 16-byte load per lane, as everywhere);
// slots with room left return after one load.  Which block a node sits in changes nothing a game records.
// ------------------------------------------------------------------------------------------
constexpr int kReclaimThreads = 1024;
constexpr uint32_t kReclaimSlotsPerGroup = 16;            // slots one workgroup looks at (a look is one 8-byte load; few slots ever need more)
C4_DEV void reclaim_slot(const Params& p, const uint32_t g, const uint32_t min_free, uint32_t& s_tail, uint32_t& s_overflow) {
  Slot* st = p.slots + g;
  const uint32_t state = st->state, arena = st->arena;
  if (slot_status(state) != kActive) return;
  const uint32_t H = p.half_blocks;
  const uint32_t n_blocks = arena & 0xFFFFu, root_block = arena >> 16;
  const uint32_t cur = n_blocks > H ? H : 0u;             // the half in use (the upper one never holds fewer than H + 1)
  if (H - (n_blocks - cur) >= min_free) return;           // room until the next look
  Block* blocks = p.blocks + (size_t)g * p.blocks_per_slot;
  const uint32_t dst = cur ? 0u : H;
  const uint32_t tid = threadIdx.x, sub = tid & 7u, grp = tid >> 3;
  const int gbase = (int)(tid & 63u & ~7u);
  const uint32_t root_ref = st->root_ref, depth = (state >> 8) & 0xFFu;
  if (grp == 0) reinterpret_cast<uint4*>(blocks + dst)[sub] = load_block_lane(blocks, root_ref >> 3, sub);
  if (grp == 1 && root_block) {
    reinterpret_cast<uint4*>(blocks + dst + 1)[sub] = load_block_lane(blocks, root_block, sub);
    if (sub == 7) blocks[root_block].t.legal = (uint16_t)(dst + 1);
  }
  if (tid == 0) { s_tail = dst + (root_block ? 2u : 1u); s_overflow = 0u; }
  __syncthreads();
  uint32_t lo = dst + 1, hi = s_tail;
  while (lo < hi) {                                       // one level of the tree per trip
    for (uint32_t i = lo + grp; i < hi; i += kReclaimThreads / 8) {
      const uint4 tl = sub == 7 ? load_block_lane(blocks, i, 7) : make_uint4(0, 0, 0, 0);   // the copied block's links are still OLD block numbers
      uint32_t link[7], cnt = 0;
#pragma unroll
      for (int k = 0; k < 7; k++) {
        const uint32_t w = k >> 1;
        const uint32_t word = w == 0 ? tl.x : (w == 1 ? tl.y : (w == 2 ? tl.z : tl.w));
        link[k] = (shfl_u32(word, gbase + 7) >> (16u * (k & 1u))) & 0xFFFFu;
        cnt += link[k] ? 1u : 0u;
      }
      if (cnt == 0) continue;                             // (group-uniform)
      uint32_t base = sub == 0 ? atomicAdd(&s_tail, cnt) : 0u;
      base = shfl_u32(base, gbase);
      // The host sizes the halves so that the live subtree always fits (reclaim_half_min); should that ever not hold (a damaged
      // tree, a configuration changed under a running game), nothing is written past the destination half -- an upward copy
      // would run into the NEXT slot's arena, a downward one into the half still being read -- and the slot raises the error the
      // step kernel raises for a full arena, with its root, links and path left as they were.
      if (base + cnt > dst + H) {                         // (group-uniform)
        if (sub == 0) s_overflow = 1u;
        continue;
      }
      uint4 v[7];
#pragma unroll
      for (int k = 0; k < 7; k++) if (link[k]) v[k] = load_block_lane(blocks, link[k], sub);
      uint32_t r = 0, nl[7];
#pragma unroll
      for (int k = 0; k < 7; k++) {
        nl[k] = 0;
        if (link[k]) {
          nl[k] = base + r++;
          reinterpret_cast<uint4*>(blocks + nl[k])[sub] = v[k];
          if (sub == 7) blocks[link[k]].t.legal = (uint16_t)nl[k];        // forwarding address (after the load above: one wavefront, program order)
        }
      }
      if (sub == 7) {
        uint4 t2 = tl;
        t2.x = nl[0] | (nl[1] << 16); t2.y = nl[2] | (nl[3] << 16); t2.z = nl[4] | (nl[5] << 16); t2.w = nl[6] | (tl.w & 0xFFFF0000u);
        reinterpret_cast<uint4*>(blocks + i)[7] = t2;
      }
    }
    __syncthreads();                                      // this level's copies (and forwarding addresses) are visible to the workgroup
    lo = hi; hi = s_tail;
    if (s_overflow) hi = lo;                              // (workgroup-uniform: read between two barriers) stop walking
    __syncthreads();
  }
  if (s_overflow) {
    if (tid == 0) raise_error(p, st, g, C4_ERR_ARENA_OVERFLOW);
    return;
  }
  // the recorded path: level L sits at path[4 (L & 3) + (L >> 2)] (L < 16) or path_deep[L - 16]; level 0 is the root's own entry
  if (tid <= depth && tid < kMaxPath) {
    uint32_t* slot_word = tid < kHotPath ? &st->path[4 * (tid & 3u) + (tid >> 2)] : &st->path_deep[tid - kHotPath];
    const uint32_t ref = *slot_word;
    *slot_word = tid == 0 ? ((dst << 3) | (root_ref & 7u)) : (((uint32_t)blocks[ref >> 3].t.legal << 3) | (ref & 7u));
  }
  if (tid == 0) {
    st->root_ref = (dst << 3) | (root_ref & 7u);
    st->arena = hi | ((root_block ? dst + 1u : 0u) << 16);
    atomicAdd(&p.reclaim_ctr[0], 1ull);
    atomicAdd(&p.reclaim_ctr[1], (unsigned long long)(hi - dst));
  }
}

__global__ __launch_bounds__(kReclaimThreads) void k_arena_reclaim(Params p, uint32_t min_free) {
  __shared__ uint32_t s_tail, s_overflow;
  // one workgroup per 16 slots, one after the other (the test is workgroup-uniform): a launch that finds nothing to do is ~100
  // workgroups that return after 16 loads, not one 1 024-thread workgroup per slot
  for (uint32_t k = 0; k < kReclaimSlotsPerGroup; k++) {
    const uint32_t g = blockIdx.x * kReclaimSlotsPerGroup + k;
    if (g >= p.n_slots) return;
    reclaim_slot(p, g, min_free, s_tail, s_overflow);
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------
// Hold sessions (C4_FLAG_HOLD): MctsGame::undo_move (mcts.rs:230-245) / reset_game (mcts.rs:225-227) for every slot, 8 lanes per
// game like the step.  The reference pops the last RecordedMove (or all of them) and makes the root a FRESH node at the popped
// move's position -- Node::new(pos, Weak::new(), 1.0): the whole tree is dropped.  That position is in the game's own row of the
// sample store: record k was written when move k was made and holds the position it was made from.  The slot gets what reset_slot
// gives a new game there (block 0 = the root's own entry with prior 1.0, bump pointer at 1, leaf = root, terminal state 0: a move
// was made from that position), with game_id and ordinal its own and the state word carrying the shortened move count, and is left
// PARKED: the resume launch that follows (c4_session_hold_undo) is the one place where a game becomes active, and it selects the
// root as the pending leaf.  A finished game's finish is reversed: sample count 0, games_done and samples down by its share (the
// wavefront's counter row takes the negative amounts: the host's sum is modulo 2^64).  Records past the new count and the q
// values of the remaining ones stay as they are: the next finish rewrites them.  A refused slot is not written at all.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_hold_undo(Params p, const int32_t* __restrict__ requests, int32_t* __restrict__ results) {
  const uint32_t lane = threadIdx.x & 63, sub = lane & 7;
  const uint32_t g = blockIdx.x * kGamesPerWave + (lane >> 3);
  if (g >= p.n_slots) return;
  Slot* st = p.slots + g;
  const int32_t req = requests[g];
  const uint32_t state = st->state, ordinal = st->ordinal;
  const uint32_t status = slot_status(state), n_moves = (state >> 16) & 0xFFu;
  int32_t res = C4_HOLD_OK;
  if (req == C4_HOLD_UNDO_NONE) res = C4_HOLD_OK;
  else if (req != C4_HOLD_UNDO_ONE && req != C4_HOLD_UNDO_ALL) res = C4_HOLD_REFUSED_REQUEST;
  else if (status != kActive && status != kParked) res = C4_HOLD_NO_GAME;      // idle, or ended by a device error
  else if (n_moves == 0) res = C4_HOLD_REFUSED_NO_MOVES;                       // undo_move returns false (mcts.rs:231)
  if (sub == 0 && results) results[g] = res;
  if (req == C4_HOLD_UNDO_NONE || res != C4_HOLD_OK) return;
  const uint32_t new_count = req == C4_HOLD_UNDO_ONE ? n_moves - 1u : 0u;
  const c4_sample_rec* rec = p.samples + (size_t)ordinal * C4_MAX_SAMPLES_PER_GAME + new_count;
  const uint64_t m = rec->mask, v = rec->value;
  const uint32_t contributed = p.sample_counts[ordinal];                      // != 0: the game is finished
  // every lane has read the state line before lane 0 rewrites it (one wavefront, program order)
  Block* blocks = p.blocks + (size_t)g * p.blocks_per_slot;
  reinterpret_cast<uint4*>(blocks)[sub] = make_uint4(0, 0, 0, sub == 0 ? __float_as_uint(1.0f) : 0u);
  if (sub == 0) {
    st->root_mask = m; st->root_value = v;
    st->leaf_mask = m; st->leaf_value = v;
    st->root_n = 0;
    st->state = slot_state(kParked, 0, new_count, 0, 0);
    st->arena = 1;            // n_blocks = 1, root not expanded: the arena is given back
    st->root_ref = 0;
    st->path[0] = 0;
    if (status == kActive) atomicAdd(&p.glob->hold_active, 0xFFFFFFFFu);       // (the resume launch counts it again)
    if (contributed) {
      p.sample_counts[ordinal] = 0;
      atomicAdd(&p.glob->games_done, ~0ull);
      atomicAdd(&p.wave_ctr[(size_t)blockIdx.x * CTR_N + CTR_DONE], ~0ull);
      atomicAdd(&p.wave_ctr[(size_t)blockIdx.x * CTR_N + CTR_SAMPLES], 0ull - (unsigned long long)contributed);
    }
  }
}

}  // namespace

// Called behind every step launch of a reclaimed session: every `period`-th launch is followed by k_arena_reclaim on the same
// stream.  Launches are counted per capture while the stream is being captured into a HIP graph (the count restarts with the
// capture, so EVERY graph carries a look behind its first step and every `period` steps after it: replays never run longer
// than min(period, graph length) steps without one), and continuously otherwise.
int maybe_reclaim(c4_session* s) {
  if (!s->p.half_blocks) return C4_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  unsigned long long id = 0;
  if (hipStreamGetCaptureInfo(s->stream, &cs, &id) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; id = 0; }
  if (cs != hipStreamCaptureStatusActive) id = 0;
  if (id != s->reclaim_capture_id) { s->reclaim_capture_id = id; s->reclaim_count = 0; }
  if (s->reclaim_count++ % s->reclaim_period != 0) return C4_OK;
  hipLaunchKernelGGL(k_arena_reclaim, dim3((s->p.n_slots + kReclaimSlotsPerGroup - 1) / kReclaimSlotsPerGroup), dim3(kReclaimThreads), 0, s->stream, s->p,
                     reclaim_min_free(s->reclaim_period, s->p.max_sims));
  HIP_TRY(hipGetLastError());
  return C4_OK;
}

extern "C" {

int c4_session_compact(c4_session* s, uint32_t multiple, uint32_t* n_active, uint32_t* n_slots_now) {
  if (!s || !s->bound || !s->have_games) return fail(C4_ERR_BAD_ARG, "compact needs a bound session with games");
  if (s->p.leaf_models) return fail(C4_ERR_BAD_ARG, "compaction does not move the per-slot model ids of multi-model sessions");
  if (hold_mode(s)) return fail(C4_ERR_BAD_ARG, "c4_session_compact: a hold session (C4_FLAG_HOLD) keeps request i on slot i: its per-slot arrays are indexed by it");
  if (multiple == 0 || multiple % 8) return fail(C4_ERR_BAD_ARG, "multiple must be a positive multiple of 8");
  C4_ON_DEVICE(s->cfg.device);
  HIP_TRY(hipStreamSynchronize(s->stream));
  Globals g{};
  HIP_TRY(hipMemcpy(&g, s->p.glob, sizeof g, hipMemcpyDeviceToHost));
  if (n_slots_now) *n_slots_now = s->p.n_slots;
  if (g.queue_head < s->n_games) {   // slots are still being refilled: nothing to gain
    if (n_active) *n_active = s->p.n_slots;
    return C4_OK;
  }
  if (!s->plan_dev) {
    HIP_TRY(hipMalloc(&s->plan_dev, sizeof(CompactPlan)));
    HIP_TRY(hipMalloc(&s->pairs_dev, (size_t)s->cfg.n_slots * sizeof(uint2)));
  }
  hipLaunchKernelGGL(k_compact_plan, dim3(1), dim3(1024), 0, s->stream, s->p.slots, s->p.n_slots, s->plan_dev, s->pairs_dev);
  const uint32_t max_pairs = s->p.n_slots / 2 + 1;
  with_planes(s->cfg.planes_dtype, [&](auto planes) {
    hipLaunchKernelGGL(k_compact_move<decltype(planes)>, dim3(max_pairs), dim3(256), 0, s->stream, s->p, s->plan_dev, s->pairs_dev);
  });
  HIP_TRY(hipGetLastError());
  CompactPlan plan{};
  HIP_TRY(hipMemcpyAsync(&plan, s->plan_dev, sizeof plan, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  uint32_t want = ((plan.n_active + multiple - 1) / multiple) * multiple;
  if (want < multiple) want = multiple;
  if (want < s->p.n_slots) {
    s->p.n_slots = want;
    s->n_waves = (want + kGamesPerWave - 1) / kGamesPerWave;
    s->p.n_waves = s->n_waves;
    HIP_TRY(hipMemset(s->p.stamps, 0, (size_t)s->n_waves_cap * 4 * sizeof(unsigned long long)));   // the stamp stride changed
  }
  if (n_active) *n_active = plan.n_active;
  if (n_slots_now) *n_slots_now = s->p.n_slots;
  return C4_OK;
}

int c4_session_hold_undo(c4_session* s, const int32_t* requests, int32_t* results) {
  if (!s) return fail(C4_ERR_BAD_ARG, "null session");
  if (!hold_mode(s)) return fail(C4_ERR_BAD_ARG, "c4_session_hold_undo: not a hold session (C4_FLAG_HOLD)");
  if (!requests) return fail(C4_ERR_BAD_ARG, "c4_session_hold_undo: requests is NULL (one C4_HOLD_UNDO_* per slot of the C4_FLAG_HOLD session)");
  if (!s->bound || !s->have_games) return fail(C4_ERR_NOT_BOUND, "bind_io and set_games must precede c4_session_hold_undo");
  C4_ON_DEVICE(s->cfg.device);
  void *q = nullptr, *r = nullptr;
  bool sq = false, sr = false;
  if (int rc = hold_array(s, requests, (void**)&s->hold_cols_dev, true, "c4_session_hold_undo: requests", &q, &sq)) return rc;
  if (results) if (int rc = hold_array(s, results, (void**)&s->hold_results_dev, false, "c4_session_hold_undo: results", &r, &sr)) return rc;
  hipLaunchKernelGGL(k_hold_undo, dim3((s->p.n_slots + kGamesPerWave - 1) / kGamesPerWave), dim3(64), 0, s->stream, s->p, (const int32_t*)q, (int32_t*)r);
  HIP_TRY(hipGetLastError());
  // ensure_bg_thread for every slot: the undone games select their root and become active, the others park or go on as they are
  if (int rc = c4_session_hold_resume(s, nullptr, nullptr, nullptr)) return rc;
  if (sr) HIP_TRY(hipMemcpyAsync(results, r, (size_t)s->cfg.n_slots * 4, hipMemcpyDeviceToHost, s->stream));
  if (sq || sr) HIP_TRY(hipStreamSynchronize(s->stream));   // pageable host memory: the caller's arrays are done with when the call returns
  return C4_OK;
}

int c4_session_arena(c4_session* s, uint64_t* bytes, uint32_t* blocks_per_slot, uint32_t* reclaim_half_blocks) {
  if (!s) return fail(C4_ERR_BAD_ARG, "null session");
  if (bytes) *bytes = s->arena_bytes;
  if (blocks_per_slot) *blocks_per_slot = s->p.blocks_per_slot;
  if (reclaim_half_blocks) *reclaim_half_blocks = s->p.half_blocks;
  return C4_OK;
}

}  // extern "C"
