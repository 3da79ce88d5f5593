// c4_session_impl.hpp -- private to the session's translation units (c4_session.hip, c4_session_maint.hip,
// c4_session_callback.hip, c4_session_readout.hip): the session object, what kind of session it is, the sizing rules of a reclaimed arena and the few
// host functions that cross files.
#pragma once
#include <stdint.h>

#include <string>

#include "c4_host.hpp"
#include "c4_tree.hpp"

// The C ABI's opaque type.  Its members are of types that c4_tree.hpp keeps in an anonymous namespace (as the one-file session did,
// so that every kernel keeps its symbol): by the letter each translation unit sees a type of its own here; the layouts are the same
// by construction -- one definition, one set of flags -- and no object of it is created outside c4_session.hip.
struct c4_session {
  c4_config cfg{};
  Params p{};
  hipStream_t stream = nullptr;
  uint32_t n_waves = 0;       // wavefronts a step launches now (shrinks with c4_session_compact)
  uint32_t out_step_gpw = 8;  // games per stepping wavefront of the fused output + step launch (c4_session_set_step_shape)
  uint32_t n_waves_cap = 0;   // as created: size of the per-wavefront arrays
  uint32_t seq = 0;
  bool timing = true;
  bool bound = false, have_games = false;
  uint64_t n_games = 0;
  c4_game_metadata* reqs_dev = nullptr;
  uint64_t* start_mask_dev = nullptr;
  uint64_t* start_value_dev = nullptr;
  // pinned probe buffer for c4_session_poll
  Globals* probe_host = nullptr;
  hipEvent_t probe_event = nullptr;
  bool probe_pending = false;
  uint64_t probe_done = 0;
  uint64_t probe_started = 0;
  uint32_t probe_error = 0;
  CompactPlan* plan_dev = nullptr;   // tail compaction scratch
  uint2* pairs_dev = nullptr;
  float* ln_tab_dev = nullptr;                 // ln(visit count) table of select (Params::ln_tab)
  unsigned long long* offsets_dev = nullptr;   // pack_samples: [n_games] record offsets + [1] total, sized by set_games
  unsigned long long* total_host = nullptr;    // pinned
  // c4_session_unique_leaves scratch (first use): table of slot indices, each slot's cell, its row, the count
  size_t arena_bytes = 0;                      // of p.blocks (kept for the next session when this one is destroyed)
  uint32_t* uniq_tab = nullptr;
  uint32_t uniq_tab_mask = 0;
  uint32_t* uniq_cell = nullptr;
  uint32_t* uniq_row = nullptr;
  uint32_t* uniq_count = nullptr;
  // reclaimed arenas (C4_FLAG_RECLAIM): step launches since the last look at the arenas, and the capture they were counted in
  uint32_t reclaim_period = 0;
  uint32_t reclaim_count = 0;
  unsigned long long reclaim_capture_id = 0;
  // hold sessions (C4_FLAG_HOLD): staging for per-slot arrays handed over in pageable host memory (cols, temperatures, results),
  // the snapshot's device and pinned buffers, and the active-slot probe (valid once a probe enqueued after the last resume landed)
  int32_t* hold_cols_dev = nullptr;
  float* hold_temps_dev = nullptr;
  int32_t* hold_results_dev = nullptr;
  unsigned char* snap_dev = nullptr;
  unsigned char* snap_host = nullptr;
  uint32_t hold_epoch = 0, probe_epoch = 0;
  bool hold_probe_valid = false;
  uint32_t hold_probe_active = 0, hold_probe_need = 0;
};

#define C4_INTERNAL __attribute__((visibility("hidden")))   // crosses files, not the library's boundary
C4_INTERNAL int maybe_reclaim(c4_session* s);                                                  // c4_session_maint.hip
C4_INTERNAL int device_view(const void* ptr, int device, const char* what, void** out);        // c4_session_callback.hip
C4_INTERNAL int hold_array(c4_session* s, const void* ptr, void** stage, bool copy_in, const char* what, void** out, bool* staged);   // c4_session.hip

namespace {

// ---- reclaimed arenas (C4_FLAG_RECLAIM, k_arena_reclaim) ----
constexpr uint32_t kReclaimPeriod = 64;          // step launches between two looks at the arenas
constexpr uint32_t kReclaimAuto = 1000;          // blocks_per_slot == 0: reclaim above this many iterations per move
constexpr uint32_t kReclaimMaxSims = 8;          // simulations one game may run per launch in a reclaimed arena (evaluation cache)
// A half is compacted when fewer than this many blocks are free in it.  Between two looks a game takes at most
// max_sims blocks per step launch, and two looks are at most 2 x period launches apart (an eager step sequence that runs
// into a graph replay, or the other way round: each form alone keeps the period, see maybe_reclaim).
static uint32_t reclaim_min_free(uint32_t period, uint32_t max_sims) { return 2u * period * max_sims + 16u; }
// What a half must hold at the very least: the live subtree right after a compaction (<= n + max_sims + 2 blocks, + slack) and
// twice the trigger above, so that a freshly compacted half is not at its next trigger already.
static uint64_t reclaim_half_min(uint32_t n_iter, uint32_t period, uint32_t max_sims) {
  return (uint64_t)n_iter + max_sims + 8u + 2ull * reclaim_min_free(period, max_sims);
}
static bool reclaim_mode(const c4_config* cfg) {
  return (cfg->flags & C4_FLAG_RECLAIM) != 0 ||
         (cfg->blocks_per_slot == 0 && cfg->n_mcts_iterations > kReclaimAuto && !(cfg->flags & (C4_FLAG_NO_MOVES | C4_FLAG_NO_RECLAIM | C4_FLAG_SEARCH | C4_FLAG_HOLD)));
}
static bool search_mode(const c4_session* s) { return (s->cfg.flags & C4_FLAG_SEARCH) != 0; }
static bool hold_mode(const c4_session* s) { return (s->cfg.flags & C4_FLAG_HOLD) != 0; }

// "<entry>: a search session (C4_FLAG_SEARCH) <why>" / "... a hold session (C4_FLAG_HOLD) <why><hold_extra>" for the entry
// points neither kind of session has; C4_OK for a session of games.
inline int refuse_search_hold(const c4_session* s, const char* entry, const char* why, const char* hold_extra = "") {
  if (search_mode(s)) return c4host::fail(C4_ERR_BAD_ARG, std::string(entry) + ": a search session (C4_FLAG_SEARCH) " + why);
  if (hold_mode(s)) return c4host::fail(C4_ERR_BAD_ARG, std::string(entry) + ": a hold session (C4_FLAG_HOLD) " + why + hold_extra);
  return C4_OK;
}

}  // namespace
