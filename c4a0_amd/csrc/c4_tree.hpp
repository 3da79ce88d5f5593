// c4_tree.hpp -- what more than one translation unit of the session needs: the tree's HBM layout, the slot status and
// counter numbering, the parameter block the kernels take, and the 8-lane group primitives.  The step kernel family and
// the session itself are c4_session.hip; maintenance, callback mode and read-outs are c4_session_*.hip.
//
// Everything here sits in an anonymous namespace, as it did when the session was one file: each translation unit compiles
// its own copy, and no kernel's code depends on which file it is compiled in.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/c4a0_hip.h"
#include "c4_device.hpp"

#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------------------------------
// HBM layout
// ------------------------------------------------------------------------------------------
struct __attribute__((aligned(16))) Entry {
  uint32_t n;     // visit_count            (mcts.rs:335)
  float q_pen;    // q_sum_penalty          (mcts.rs:336)
  float q_nopen;  // q_sum_no_penalty       (mcts.rs:337)
  float prior;    // initial_policy_value   (mcts.rs:338)
};
struct __attribute__((aligned(16))) Tail {
  uint16_t child[7];  // per column: block holding that child's own children, 0 = not expanded (mcts.rs:339)
  uint16_t legal;     // legal-move mask of the parent position (informational)
};
// The 7 children of an expanded node: ONE 128-byte line.  Lane c < 7 of a game's lane group loads
// entry c, lane 7 the tail, in a single 16-byte-per-lane instruction; a backup touches one entry
// (one 32-byte sector).  16-bit child links bound an arena to 65 535 blocks per slot.
struct __attribute__((aligned(128))) Block {
  Entry e[7];
  Tail t;
};
constexpr uint32_t kMaxBlocksPerSlot = 65535;

constexpr uint32_t kMaxPath = 43;   // root + at most 42 moves below it
constexpr uint32_t kHotPath = 16;   // path levels kept in the slot's hot line
// A resident game's state.  Everything a simulation needs is ONE 128-byte line, read by the game's
// 8 lanes with one 16-byte-per-lane instruction at the start of the step kernel and written back
// with one at the end (lane k owns dwords 4k..4k+3):
//   lane 0: root position          lane 1: leaf position (waiting for the evaluator)
//   lane 2: game id, ordinal, root visit count
//   lane 3: state word, arena words, root ref, precomputed move RNG word
//   lanes 4..7: the recorded path, TRANSPOSED: lane 4 + j holds levels j, j + 4, j + 8, j + 12, so
//               the backup of level d runs on lane 4 + (d & 3) and the first four levels update in parallel
// The second line holds path levels 16..42 (deep searches only).
struct __attribute__((aligned(256))) Slot {
  uint64_t root_mask, root_value;  // MctsGame::root position
  uint64_t leaf_mask, leaf_value;  // MctsGame::leaf position
  uint64_t game_id;
  uint32_t ordinal;     // index into reqs / the sample store
  uint32_t root_n;      // mirror of the root entry's visit count
  uint32_t state;       // status[0:8] (0 idle, 1 active, >1 = c4_status error) | depth[8:16] (path[depth] = the leaf's entry)
                        // | n_moves[16:24] | terminal_state of the leaf [24:26] | rng_for[26:32] (n_moves + 1 rng_word is for; 0 = none)
  uint32_t arena;       // n_blocks[0:16] (bump pointer) | root_block[16:32] (the root's children block, 0 = not expanded)
  uint32_t root_ref;    // (block << 3 | column) of the root's own entry
  uint32_t rng_word;    // first ChaCha12 word for the NEXT move (mcts.rs:215-216), precomputed off the critical path
  uint32_t path[kHotPath];        // entry refs of levels 0..15, transposed: path[4 * j + i] = level j + 4 * i
  uint32_t path_deep[kMaxPath - kHotPath];   // levels 16..42
  uint32_t pad_[32 - (kMaxPath - kHotPath)];
};
static_assert(sizeof(Slot) == 256 && offsetof(Slot, path) == 64 && offsetof(Slot, path_deep) == 128, "slot state: one hot line + the deep path");
C4_DEV constexpr uint32_t slot_state(uint32_t status, uint32_t depth, uint32_t n_moves, uint32_t term, uint32_t rng_for) {
  return status | (depth << 8) | (n_moves << 16) | (term << 24) | (rng_for << 26);
}
C4_DEV uint32_t slot_status(uint32_t state) { return state & 0xFFu; }
static_assert(sizeof(Block) == 128 && sizeof(Entry) == 16 && sizeof(Tail) == 16 && sizeof(c4_sample_rec) == 64, "layout");
constexpr uint32_t kGamesPerWave = 8;   // one game <-> one 8-lane group of a wave64: the games of one stepping wavefront

enum : uint32_t { kIdle = 0, kActive = 1, kParked = C4_HOLD_PARKED };   // (kParked: hold sessions only, a status of its own)
enum : int { CTR_SIMS = 0, CTR_S, CTR_K, CTR_E, CTR_MOVES, CTR_DONE, CTR_SKIPPED, CTR_SAMPLES, CTR_PROBES, CTR_HITS, CTR_N = 16 };

struct Globals {             // one small device struct of cross-wave words
  unsigned long long queue_head;   // next game ordinal to start
  unsigned long long games_done;
  uint32_t error;            // first error status
  uint32_t error_slot;
  uint32_t hold_active;      // hold sessions (C4_FLAG_HOLD): slots whose status is active
  uint32_t hold_need;        // ... and the largest n_iter - root visits among them at the last c4_session_hold_resume
};

struct CompactPlan {         // tail compaction's device scratch (k_compact_plan -> k_compact_move and the host)
  uint32_t n_active;
  uint32_t n_pairs;
};

struct Params {
  Slot* slots;
  Block* blocks;
  unsigned long long* wave_ctr;  // [n_waves][CTR_N]
  unsigned long long* stamps;    // [2][n_waves][2] start/end device clock of each wavefront, by launch parity
  unsigned long long* clock_acc; // [0] sum of (last end - first start) over launches, [1] launches summed, [2..4] the timing helpers' scratch
  uint32_t n_waves;
  uint32_t seq;                  // launch sequence number
  unsigned long long* phase;     // diagnostic build: [n_waves][16] phase stamps of the last launch
  uint64_t* leaf_models;         // optional [n_slots]: model id that must evaluate each slot's leaf (mcts.rs:70-76)
  Globals* glob;
  const c4_game_metadata* reqs;
  const uint64_t* start_mask;    // may be null
  const uint64_t* start_value;
  c4_sample_rec* samples;        // [n_games][43]
  uint32_t* sample_counts;       // [n_games]
  void* planes;
  const float* logprobs;
  const float* q;
  unsigned long long n_games;
  uint32_t n_slots;
  uint32_t blocks_per_slot;
  uint32_t n_iter;
  float c_exploration;
  float c_ply_penalty;
  uint32_t flags;
  float dir_alpha, dir_eps;       // Dirichlet root noise (extension); dir_eps == 0 disables
  uint2* cache;                   // optional evaluation cache (extension): [cache_mask + 1] entries of 64 bytes, 8 x uint2
  uint32_t cache_mask;
  uint32_t max_sims;              // simulations one game may run in one launch (terminal / cached leaves need no evaluator)
  const float* ln_tab;            // ln_tab[k] = c4_logf((float)k), k < n_ln: the parent-visit term of uct_value (mcts.rs:379)
  uint32_t n_ln;
  uint32_t half_blocks;           // reclaimed arenas (C4_FLAG_RECLAIM): blocks per half, blocks_per_slot = 2 x this; 0 = never-reclaimed arena
  unsigned long long* reclaim_ctr;   // [2] passes, blocks copied (k_arena_reclaim)
  // hold sessions (C4_FLAG_HOLD), read by k_hold_resume alone: per-slot moves (null = none), their temperatures, where the
  // per-slot result codes go (may be null), and whether the launch is c4_session_start's (the slots were reset just now)
  const int32_t* hold_cols;
  const float* hold_temps;
  int32_t* hold_results;
  uint32_t hold_fresh;
};

// ------------------------------------------------------------------------------------------
// 8-lane group helpers
// ------------------------------------------------------------------------------------------
C4_DEV uint32_t shfl_u32(uint32_t v, int src_lane) { return (uint32_t)__shfl((int)v, src_lane, 64); }
C4_DEV float shfl_f32(float v, int src_lane) { return __shfl(v, src_lane, 64); }

// Exchanges inside an 8-lane group without the LDS crossbar (DPP): lane ^ 1, lane ^ 2, and 7 - lane.
// After the first two every lane of a quad holds the quad's combination, so the mirror step pairs
// the two quads: three steps reduce a group for any commutative, associative combination.
template <int kStep>
C4_DEV uint32_t grp_xchg(uint32_t v) {
  static_assert(kStep >= 0 && kStep < 3, "three butterfly steps");
  constexpr int ctrl = kStep == 0 ? 0xB1 /* quad_perm [1,0,3,2] */ : (kStep == 1 ? 0x4E /* quad_perm [2,3,0,1] */ : 0x141 /* row_half_mirror */);
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, 0xF, 0xF, true);
}
template <int kStep>
C4_DEV float grp_xchg(float v) { return __uint_as_float(grp_xchg<kStep>(__float_as_uint(v))); }

// lane `sub` of a group loads its 16 bytes of block `blk`: entry `sub` (sub < 7) or the tail (sub == 7)
C4_DEV uint4 load_block_lane(const Block* blocks, uint32_t blk, uint32_t sub) {
  return reinterpret_cast<const uint4*>(blocks + blk)[sub];
}
// child link of column `col` out of the tail held by lane 7 of the group (col is group-uniform)
C4_DEV uint32_t child_link(const uint4& raw, uint32_t col, int gbase) {
  const uint32_t w = col >> 1;
  const uint32_t mine = w == 0 ? raw.x : (w == 1 ? raw.y : (w == 2 ? raw.z : raw.w));
  return (shfl_u32(mine, gbase + 7) >> (16u * (col & 1u))) & 0xFFFFu;
}

C4_DEV void raise_error(const Params& p, Slot* st, uint32_t g, uint32_t code) {
  st->state = (st->state & ~0xFFu) | code;
  if (atomicCAS(&p.glob->error, 0u, code) == 0u) p.glob->error_slot = g;
}

template <typename PlaneT>
C4_DEV void store_plane(void* base, size_t idx, uint32_t bit);
template <>
C4_DEV void store_plane<float>(void* base, size_t idx, uint32_t bit) {
  ((float*)base)[idx] = bit ? 1.0f : 0.0f;
}
template <>
C4_DEV void store_plane<uint16_t>(void* base, size_t idx, uint32_t bit) {
  ((uint16_t*)base)[idx] = bit ? (uint16_t)0x3F80 : (uint16_t)0;  // bf16 1.0 / 0.0
}

}  // namespace
