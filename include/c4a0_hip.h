/*
 * c4a0_hip.h -- C ABI of the MI355X-native self-play generator (libc4a0_hip.so).
 *
 * Drop-in boundary for the reference's self-play hot path.  The reference has no C header:
 * its boundary is the PyO3 function `play_games` (rust/src/pybridge.rs:20-53) which calls
 * `self_play::self_play` (rust/src/self_play.rs:39-129).  The entry points below are what a
 * Rust host would bind with `extern "C"` to replace the body of `self_play()` (INTEGRATION.md
 * shows the binding); each one cites the reference code it replaces.
 *
 * Conventions: every function returns a c4_status (0 = ok); c4_last_error_string() gives the
 * detail for the calling thread.  All pointers named *_dev are DEVICE pointers owned by the
 * caller (e.g. PyTorch tensors) and must stay valid until the session is destroyed or rebound.
 * `stream` is a hipStream_t passed as void* (NULL = the default stream).  No function
 * synchronises the device unless its comment says so.
 */
#ifndef C4A0_HIP_H
#define C4A0_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of THIS interface: bumped whenever a signature or a struct layout below changes (version 3 added `config` in the
 * middle of c4_conv_tower_bf16's arguments, version 5 c4_session_step_head_out, version 8 the host-side record codecs c4_records_to_cbor / c4_cbor_to_records / c4_shuffle_games, version 9 c4_play_games_bf16, version 10 c4_play_games_cancel / C4_ERR_CANCELLED, version 11 the f32 evaluator c4_conv_tower_f32 / c4_linear_f32 / c4_head_out_f32, version 12 C4_FLAG_SEARCH / c4_search_positions_bf16, version 13 C4_FLAG_HOLD / c4_session_set_iterations / c4_session_hold_resume / c4_session_snapshot / c4_session_hold_poll, version 14 c4_session_route_leaves and the grouped bf16 chain c4_conv_tower_bf16_grouped / c4_linear_bf16_grouped / c4_head_out_bf16_grouped / c4_grouped_row_align).  A consumer compiled against this header checks it once at start-up --
 * `if (c4_abi_version() != C4_ABI_VERSION) refuse` -- because the dynamic linker compares names, not signatures
 * (tests/abi_consumer*.c and c4a0_amd/_lib.py do).  No reference counterpart: the reference's boundary is PyO3. */
#define C4_ABI_VERSION 14

#define C4_N_COLS 7          /* rust/src/c4r.rs:45, lib.rs:28 */
#define C4_N_ROWS 6          /* rust/src/c4r.rs:44, lib.rs:29 */
#define C4_BUF_N_CHANNELS 2  /* rust/src/c4r.rs:48, lib.rs:30 */
#define C4_PLANES_LEN 84     /* rust/src/c4r.rs:52 BUF_LEN */
#define C4_MAX_SAMPLES_PER_GAME 43 /* <= 42 moves + the terminal sample, mcts.rs:271-313 */

typedef enum {
  C4_OK = 0,
  C4_ERR_BAD_ARG = 1,
  C4_ERR_HIP = 2,               /* a HIP runtime call failed */
  C4_ERR_NAN_IN_TREE = 3,       /* reference panics: utils.rs:12 (OrdF32 on NaN) */
  C4_ERR_DEGENERATE_POLICY = 4, /* reference panics: mcts.rs:421-425, mcts.rs:219 */
  C4_ERR_ARENA_OVERFLOW = 5,    /* blocks_per_slot too small for this game's tree */
  C4_ERR_NOT_BOUND = 6,         /* step before bind_io / set_games */
  C4_ERR_NO_DEVICE = 7,
  C4_ERR_ILLEGAL_MOVE = 8,      /* reference panics: mcts.rs:196-200 (sampled a full column; only possible when the
                                   root's children have no visits, i.e. n_mcts_iterations <= 1) */
  C4_ERR_CANCELLED = 9          /* c4_play_games_bf16 stopped by c4_play_games_cancel (the host's Ctrl-C) */
} c4_status;

/* types.rs:37-48 GameMetadata */
typedef struct {
  uint64_t game_id;
  uint64_t player0_id;
  uint64_t player1_id;
} c4_game_metadata;

/* One training sample (types.rs:103-110 Sample + the game it belongs to), 64 bytes.
 * meta = sample index within the game (low 16 bits) | flags << 16 (bits 0 and 1 both: a c4_session_snapshot record, index = moves made; bit 0: terminal sample; bit 1: search record -- the one
 * record of a C4_FLAG_SEARCH request: policy = the root policy after n_mcts_iterations simulations, q_penalty / q_no_penalty = the
 * root's q values, mcts.rs:359-367, 396-412 -- not a training sample of a game). */
typedef struct {
  uint64_t game_id;
  uint64_t mask;   /* c4r.rs:13-17 Pos.mask  */
  uint64_t value;  /* c4r.rs:13-17 Pos.value */
  float policy[7];
  float q_penalty;
  float q_no_penalty;
  uint32_t meta;
} c4_sample_rec;

/* Arguments of self_play() (self_play.rs:39-46) that are fixed for a session, plus sizing. */
typedef struct {
  uint32_t n_slots;           /* games resident on the GPU and advanced in lock-step */
  uint32_t blocks_per_slot;   /* tree arena per slot, in 128-byte 7-children blocks, at most 65535 (16-bit child links).
                                 0 = automatic: up to n_mcts_iterations = 1000 the worst case of a never-reclaimed arena,
                                 43*n_mcts_iterations+8; beyond that (and up to 32 200) a RECLAIMED arena of two halves of
                                 2.5*n_mcts_iterations+554 blocks each (see C4_FLAG_RECLAIM); a search session (C4_FLAG_SEARCH):
                                 n_mcts_iterations+8; a hold session (C4_FLAG_HOLD): 43*n_mcts_iterations+8, never reclaimed */
  uint32_t n_mcts_iterations; /* self_play.rs:43 */
  float c_exploration;        /* self_play.rs:44 (f32, as pybridge.rs:26) */
  float c_ply_penalty;        /* self_play.rs:45 */
  uint32_t planes_dtype;      /* 0 = float32, 1 = bfloat16: element type of the NN input buffer */
  uint32_t flags;             /* C4_FLAG_* */
  int32_t device;             /* HIP device ordinal */
  uint32_t reclaim_period;    /* reclaimed arenas only: step launches between two looks at the arenas (0 = 64); tests use 1 */
} c4_config;

#define C4_FLAG_NO_MOVES 1u   /* never move: mcts.rs test helper `run_mcts` (mcts.rs:469-485) */
#define C4_FLAG_ONE_SIM_PER_STEP 2u /* exactly one simulation per game per c4_session_step.  Default: a game whose
                                       freshly selected leaf is terminal (no evaluator needed, mcts.rs:92-98) runs that
                                       simulation in the same step; samples are identical either way */

#define C4_FLAG_RECLAIM 4u    /* the tree arena is reclaimed while a game is played, as the reference frees the siblings' subtrees at
                                 every move (mcts.rs:187-206): a slot's arena is two halves; when the half in use runs short, the
                                 subtree below the current root (at most n_mcts_iterations + a few blocks) is copied compactly into
                                 the other half by a kernel of its own that follows every reclaim_period-th step launch on the
                                 session's stream (also inside HIP-graph captures).  Samples are identical with and without it; what
                                 it lifts is the limit n_mcts_iterations <= 1523 of the never-reclaimed arena, and the arena shrinks
                                 from 43 n + 8 to 2 x (2.5 n + 554) blocks per slot.  With blocks_per_slot == 0 the flag is implied
                                 for n_mcts_iterations > 1000; with an explicit blocks_per_slot that value is BOTH halves. */

#define C4_FLAG_NO_RECLAIM 8u /* keep the never-reclaimed arena where the default sizing would reclaim (n_mcts_iterations > 1000): 43 n + 8
                                 blocks per slot, refused beyond n = 1523 with the reason */

#define C4_FLAG_SEARCH 16u    /* every request is ONE search, not a game: n_mcts_iterations simulations from its start position as root
                                 (MctsGame::new_from_pos, mcts.rs:48-56, + the run_mcts helper of its tests, mcts.rs:469-485; what
                                 interactive_play.rs:33, 57 shows), then ONE record at the head of the request's 43 -- mask / value = the
                                 position, policy = root_policy (mcts.rs:396-412), q_penalty / q_no_penalty = q_sum / (visits + 1)
                                 (mcts.rs:359-367), meta = 2 << 16 -- sample count 1, and the slot takes the next request.  No move, no
                                 temperature, no move RNG.  A terminal position is searched n times like any other (its q is
                                 q_sum / (n + 1), not the terminal value), two simulations per launch.  Counters of a finished job of P
                                 positions: sims = P n, games_done = samples = games_started = P, moves = ref_skipped_sims = 0;
                                 select_levels leaves out the select behind each search's last simulation (nobody consumes its leaf),
                                 backup_nodes the simulations of a terminal root.  Automatic arena: n_mcts_iterations + 8 blocks per slot
                                 (one expansion per simulation at most, never a re-root), so the 1 523-iteration limit of whole games
                                 does not apply.  A step-kernel instantiation of its own: refused together with C4_FLAG_NO_MOVES,
                                 C4_FLAG_RECLAIM or n_mcts_iterations == 0, and c4_session_set_dirichlet (epsilon > 0),
                                 c4_session_set_eval_cache (n > 0), c4_session_bind_leaf_models, c4_session_step_gather and
                                 c4_session_unique_leaves return C4_ERR_BAD_ARG on such a session. */

#define C4_FLAG_HOLD 32u      /* GPU-resident interactive play: every request is ONE persistent game whose tree lives on across moves that come
                                 from outside -- the reference's InteractivePlay around one MctsGame (interactive_play.rs; what run_tui sits on).
                                 Request i lives on slot i for the session's whole life (c4_session_set_games: n_games <= n_slots, else
                                 C4_ERR_BAD_ARG; any start position, MctsGame::new_from_pos); no slot is ever refilled.
                                 Target: the session's n_mcts_iterations is InteractivePlay.max_mcts_iterations, an ABSOLUTE target for the
                                 root's visit count, changed by c4_session_set_iterations (at most the value the session was created with).
                                 After expand + backup a game whose root has that many visits is PARKED (State::bg_thread_should_stop,
                                 interactive_play.rs:188-191): slot status C4_HOLD_PARKED (c4_session_leaves; not idle, not active, not a
                                 c4_status), no leaf selected, no planes written, no move, no record; every later step skips it.  The gate sits
                                 inside the step's loop of (at most two) simulations, so a root never gets more visits than max(target, the
                                 visits it had when the target was set).  A game whose root is TERMINAL is never searched: it is parked from the
                                 start, or from the move that made its root terminal -- unlike C4_FLAG_SEARCH, which searches such a root n times.
                                 Becoming active: c4_session_start and c4_session_hold_resume, one kernel, which per slot applies the move asked
                                 for, parks, or selects the next leaf from the tree as it stands and writes it to planes_dev.
                                 Records: an accepted move writes what a self-play move writes (root position, untempered root policy, meta =
                                 moves made) into the game's row of the sample store, re-roots on the child KEEPING its subtree (mcts.rs:187-206)
                                 and, when the new root is terminal, completes the game's records as a finished self-play game's (to_result's q
                                 signs, the uniform terminal sample, sample count; counted in games_done): c4_session_sample_counts /
                                 _drain_samples / _pack_samples deliver finished games only, unchanged.  ref_skipped_sims stays 0.
                                 Taking moves back: c4_session_hold_undo (MctsGame::undo_move / reset_game) makes the root a FRESH node at the
                                 position an earlier move was made from -- the tree is dropped, the arena's bump pointer restarts -- and takes
                                 a finished game out of the records and out of games_done / samples again.
                                 Arena: 43 n + 8 blocks per slot by default, n the creation-time n_mcts_iterations (a root gets at most n new
                                 simulations, a game has at most 42 roots), never reclaimed -- above n = 1 523 pass blocks_per_slot;
                                 C4_ERR_ARENA_OVERFLOW stays the per-slot outcome of exhaustion.
                                 A step-kernel instantiation of its own: refused together with C4_FLAG_SEARCH, C4_FLAG_NO_MOVES, C4_FLAG_RECLAIM or
                                 n_mcts_iterations == 0, and c4_session_set_dirichlet (epsilon > 0), c4_session_set_eval_cache (n > 0),
                                 c4_session_bind_leaf_models, c4_session_compact, c4_session_step_gather and c4_session_unique_leaves return
                                 C4_ERR_BAD_ARG on such a session (one evaluator, one slot per game for good, device evaluators only).
                                 c4_session_step_head_out: bf16 planes.  Not part of c4_play_games_bf16. */
#define C4_HOLD_PARKED 64u    /* slot status of a parked game (c4_session_leaves, c4_session_snapshot) */
/* c4_session_hold_resume: a slot's move ... */
#define C4_HOLD_MOVE_NONE (-1)   /* none */
#define C4_HOLD_MOVE_SAMPLE (-2) /* make_random_move(temperatures[slot]) (mcts.rs:214-222); 0..6 = that column (mcts.rs:187-206) */
/* ... and its result */
#define C4_HOLD_OK 0                  /* accepted, or none asked */
#define C4_HOLD_REFUSED_TERMINAL 1    /* the root is terminal (interactive_play.rs:171, 180 return false) */
#define C4_HOLD_REFUSED_COLUMN 2      /* the column is outside 0..6 or full (interactive_play.rs:171) */
#define C4_HOLD_REFUSED_UNSEARCHED 3  /* the root has no children yet: not one simulation since it became the root (the reference panics, mcts.rs:196) */
#define C4_HOLD_REFUSED_SAMPLE 4      /* the sampled column is not legal (mcts.rs:196-200 panics; only while the root's children have no visits) */
#define C4_HOLD_NO_GAME 5             /* the slot holds no live game: never given one, or ended by a device error */
/* c4_session_hold_undo: what a slot is asked to take back ... */
#define C4_HOLD_UNDO_NONE 0      /* nothing */
#define C4_HOLD_UNDO_ONE 1       /* MctsGame::undo_move (mcts.rs:230-245): the last move */
#define C4_HOLD_UNDO_ALL 2       /* MctsGame::reset_game (mcts.rs:225-227): every move */
/* ... and the two results it adds to C4_HOLD_OK and C4_HOLD_NO_GAME */
#define C4_HOLD_REFUSED_NO_MOVES 6    /* the game has made no move (undo_move returns false; reset_game does nothing) */
#define C4_HOLD_REFUSED_REQUEST 7     /* requests[slot] is none of the three codes above */
#define C4_HOLD_POLL_UNKNOWN 0xFFFFFFFFu /* c4_session_hold_poll: no probe enqueued since the last resume has landed yet */

/* Device-side counters (the reference's progress bars, self_play.rs:352-381, plus the
 * roofline numerators of SURVEY 8d).  Sums over all games since set_games. */
typedef struct {
  uint64_t sims;            /* on_received_policy calls executed (self_play.rs:272) */
  uint64_t select_levels;   /* sum of S: children blocks scanned by select_new_leaf (mcts.rs:160-183) */
  uint64_t backup_nodes;    /* sum of K: nodes updated by backpropagate_value (mcts.rs:137-155) */
  uint64_t expansions;      /* sum of E: expand_leaf calls that created children (mcts.rs:114-132) */
  uint64_t moves;           /* make_random_move calls (mcts.rs:214-222) */
  uint64_t games_done;
  uint64_t ref_skipped_sims;/* terminal-root sims the reference would still run (self_play.rs:283-301): after a move
                               into a terminal position, and all n of a terminal start position */
  uint64_t samples;
  uint64_t games_started;
  uint64_t step_kernel_ns;  /* device-clock time inside c4_session_step's kernel, summed over launches:
                               last wavefront end - first wavefront start (s_memrealtime, 10 ns ticks) */
  uint64_t step_launches;   /* launches summed in step_kernel_ns */
  uint64_t eval_cache_probes; /* leaves looked up in the evaluation cache (extension, c4_session_set_eval_cache) */
  uint64_t eval_cache_hits;   /* ... and found: simulations that needed no evaluator row */
  uint64_t reclaim_passes;    /* reclaimed arenas (C4_FLAG_RECLAIM): live subtrees copied into the other half ... */
  uint64_t reclaim_blocks;    /* ... and the 128-byte blocks those copies moved */
  uint32_t error;           /* first c4_status raised on the device, 0 = none */
  uint32_t error_slot;
} c4_counters;

typedef struct c4_session c4_session;

const char* c4_last_error_string(void);
int c4_abi_version(void); /* == C4_ABI_VERSION of the header the library was compiled with */
/* Content hash of the sources the library was compiled from (no reference counterpart: build
 * hygiene; c4a0_amd/csrc/build.py rebuilds, and c4a0_amd/_lib.py refuses, a stale library). */
const char* c4_source_hash(void);
int c4_device_count(int* out);

/* Replaces the set-up half of self_play() (self_play.rs:47-58): allocates the tree arenas,
 * slot states and counters on `cfg->device`. */
int c4_session_create(const c4_config* cfg, c4_session** out);
int c4_session_destroy(c4_session* s);
/* c4_session_destroy keeps ONE tree arena (a session's largest allocation: n_slots x blocks_per_slot x 128 bytes) per
 * process for the next session on the same device that it fits -- the driver scrubs freed device memory before reuse,
 * which a session created right after a big one was destroyed would otherwise wait for (0.6 s for 13 GB).  This gives
 * the kept arena back to the device now.  C4_ARENA_CACHE=0 in the environment disables the cache. */
int c4_trim_cached_memory(void);

/* `reqs: Vec<GameMetadata>` of self_play() (self_play.rs:41).  Copies the list to the device,
 * allocates the sample store (43 records per game), resets queue and counters.
 * start_masks/start_values (host arrays of n_games, may be NULL = empty board, self_play.rs:56) give
 * every game its start position, MctsGame::new_from_pos (mcts.rs:48-56): ANY position, terminal ones
 * included, indexed like reqs.  Whole games from it are the reference's, sample for sample: the
 * temperature, the ply penalty and the leaf's model follow the ply of the position, the move seed, the
 * Dirichlet key, the record index and the sign of each sample's q the moves THIS game has made
 * (mcts.rs:215, 271-313).  A game whose start is terminal yields its one sample in the first step that
 * sees it; the n simulations the reference spends on such a root are counted in ref_skipped_sims
 * (with C4_FLAG_NO_MOVES they are run, as mcts.rs' run_mcts runs them).  Synchronises the stream. */
int c4_session_set_games(c4_session* s, const c4_game_metadata* reqs, uint64_t n_games,
                         const uint64_t* start_masks, const uint64_t* start_values);

/* Replaces EvalPosT / PyEvalPos / create_pos_batch (types.rs:24-34, pybridge.rs:161-221):
 * instead of a callback the evaluator's tensors are bound once.
 *   planes_dev   [n_slots][2][6][7]  written by the library (row g = leaf of slot g)
 *   logprobs_dev [n_slots][7] f32    read by the library (policy logits / log-probs)
 *   q_dev        [n_slots][2] f32    read by the library (q_penalty, q_no_penalty) */
int c4_session_bind_io(c4_session* s, void* planes_dev, const float* logprobs_dev, const float* q_dev,
                       void* stream);

/* Dirichlet root noise -- a BUILD EXTENSION named by BASELINE.json's north star; the reference has
 * none.  When epsilon > 0, the children of every search root get prior' = (1 - epsilon) * prior +
 * epsilon * eta with eta ~ Dir(alpha) over the legal columns, drawn from a private ChaCha12 stream
 * keyed by (game_id, moves played); specification = oracle/c4_oracle.c c4o_dirichlet, matched bit
 * for bit.  Off (epsilon = 0) by default and in every reference-parity run. */
int c4_session_set_dirichlet(c4_session* s, float alpha, float epsilon);

/* Multi-model games (player0_id != player1_id: tournaments, tournament.py:112-142): when bound,
 * every start/step also writes, for each slot, the id of the model that must evaluate its leaf
 * (MctsGame::leaf_model_id_to_play, mcts.rs:70-76) to leaf_models_dev [n_slots] (uint64), so the
 * caller can route rows to evaluators without leaving the device.  NULL unbinds. */
int c4_session_bind_leaf_models(c4_session* s, uint64_t* leaf_models_dev);

/* Evaluation cache -- a BUILD EXTENSION, off by default (the reference evaluates every leaf and only
 * dedups positions inside one batch, self_play.rs:203-208).  A direct-mapped table of n_entries
 * (rounded up to a power of two, 64 bytes each) in HBM keeps the evaluator's raw outputs by position;
 * a game whose freshly selected leaf is found there runs that simulation in the same launch, like a
 * terminal leaf, up to max_sims_per_step simulations per game per c4_session_step (0 = 6).  Samples
 * are unchanged provided the evaluator is a deterministic function of the position (a network in
 * inference mode is); one evaluator per session, so not together with c4_session_bind_leaf_models.
 * n_entries = 0 frees the table; c4_session_set_games empties it (new games may come with new weights).
 * Call before c4_session_start / graph capture.  Synchronises. */
int c4_session_set_eval_cache(c4_session* s, uint64_t n_entries, uint32_t max_sims_per_step);

/* Puts the first n_slots games on the slots and writes their first leaf (the start position)
 * to planes_dev: the state self_play() is in after self_play.rs:55-58. */
int c4_session_start(c4_session* s);

/* One MctsThread job (self_play.rs:268-323) for EVERY resident game: consume the evaluator
 * outputs for the current leaves (on_received_policy, mcts.rs:83-108), make a move when the
 * root has n_mcts_iterations visits (make_random_move, mcts.rs:214-222), finish and replace
 * finished games, select the next leaves and write them to planes_dev.  Asynchronous. */
int c4_session_step(c4_session* s);

/* Non-finite evaluator outputs, sessions of games and of searches alike (every step entry point: c4_session_step, _step_gather,
 * _step_head_out, with noise, cache, reclaimed arenas, HIP graphs).  No answer is rejected or clamped; a game ends as the reference
 * would panic, game by game: the slot's status byte (c4_session_leaves) becomes the code and stays, the slot is never refilled, the
 * game has no record, the first code raised is in c4_counters.error / error_slot, and every other game -- the seven of the same
 * wavefront included -- goes on and records the reference's bytes.  Pinned against the oracle by tests/test_gpu_nonfinite_regime.py
 * (games, every launch form) and tests/test_gpu_search_positions.py T5 (searches); the kinds are tests/helpers.py POISON_KINDS.
 *   NaN q_penalty        backed up along the path; C4_ERR_NAN_IN_TREE at the next select that compares it with another candidate
 *                        (utils.rs:12).  Down a chain of nodes with ONE legal column nothing is compared: no error, and a search
 *                        record's root q is NaN (a game's records hold terminal values only).
 *   NaN q_no_penalty     never compared: no error; a search record carries it.  A NaN's sign and payload are not specified.
 *   +Inf q_penalty       scores of +-Inf compare like any other; C4_ERR_NAN_IN_TREE once +Inf and -Inf have met in one q_sum.
 *   NaN legal logit      f32::max ignores it, its expf is NaN and so is every prior of the node: C4_ERR_NAN_IN_TREE when a select
 *                        reaches the node, if it has two or more children.  On the ONLY legal column the masked maximum is -Inf:
 *                        C4_ERR_DEGENERATE_POLICY at the expansion (mcts.rs:421-425).
 *   NaN / any value on a full column   masked before the softmax (c4r.rs:272-286): no effect.
 *   -Inf on some legal logits          priors of exactly 0.
 *   -Inf on all legal logits, +Inf on a legal one   C4_ERR_DEGENERATE_POLICY at the expansion; nothing is backed up.
 * One counted deviation: the reference selects a leaf BEHIND the simulation that completes a root's n visits
 * and throws it away (the move selects again from the new root; a search's caller reads the root).  The device leaves that select
 * out.  A NaN which that select alone would have compared therefore ends the game in the reference and not here: the game moves
 * on, and ends with C4_ERR_NAN_IN_TREE later if the NaN sits in the subtree the move keeps, or finishes (a search: writes its
 * record, root q possibly NaN).  The oracle plays either order (c4o_game_set_device_order); tests/test_nonfinite_regime.py pins
 * on the CPU which games differ: 6 of 800 at n = 8 with one position in 300 poisoned, none of 600 at n = 24. */

/* c4_head_out_bf16 (below) + c4_session_step as ONE launch: the heads' output layers (nn.py:84-85, 98-99) are computed by
 * workgroups of 16 boards whose first two wavefronts go on as the step of those 16 games (mcts.rs:83-108, self_play.rs:268-323):
 * one launch boundary and the step's argument fetch / state-line round trip leave the per-round chain.  The outputs are also
 * written to the bound logprobs / q tensors, and every result equals the two-launch form bit for bit (same code).  Operands as
 * for c4_head_out_bf16, rows = the session's current width, stream = the session's.  Default configuration only: returns
 * C4_ERR_BAD_ARG when Dirichlet noise, the evaluation cache or per-launch timing (c4_session_set_timing) is on, or when
 * `features` is not a multiple of 1 344 -- callers then use the two entry points. */
int c4_session_step_head_out(c4_session* s, const void* hidden_policy_dev, const void* hidden_value_dev, const void* w_policy_dev,
                             const void* w_value_dev, const float* b_policy_dev, const float* b_value_dev, uint32_t features,
                             uint32_t policy_row_stride, uint32_t value_row_stride);
/* How the fused launch above shares a workgroup's 16 games among its wavefronts: 8 games per stepping wavefront (default) or 4.
 * A scheduling knob -- the games' records do not depend on it: 4 is 0.5 % faster where a second session's kernels share the chip
 * (the paired graph of c4a0_amd.session.capture_pair asks for it), 8 where the session is alone. */
int c4_session_set_step_shape(c4_session* s, uint32_t games_per_wavefront);

/* Per-launch device-clock timing of the step kernel (c4_counters.step_kernel_ns) needs a launch
 * sequence number in the kernel arguments, which a HIP-graph capture would freeze: switch it
 * off before capturing c4_session_step into a graph, on again for eager launches.  On by
 * default.  Synchronises. */
int c4_session_set_timing(c4_session* s, int enable);

/* Synchronises the stream and sums the per-wavefront counters. */
int c4_session_counters(c4_session* s, c4_counters* out);
/* Non-blocking completion probe: enqueues a copy of (games_done, error) to pinned host
 * memory; *games_done / *error hold the values of the previous probe that has landed. */
int c4_session_poll(c4_session* s, uint64_t* games_done, uint32_t* error);
/* The same probe, also reporting how many games have been taken off the request list so far. */
int c4_session_progress(c4_session* s, uint64_t* games_done, uint64_t* games_started, uint32_t* error);

/* Tail of a job: once every request has been started, finished slots stay empty while the evaluator
 * still computes rows for them.  Moves the remaining active games into the lowest slots (slot state,
 * arena, evaluator input row; which slot plays a game changes none of its samples) and narrows the
 * session to the smallest multiple of `multiple` (itself a multiple of 8) slots that holds them:
 * c4_session_step then launches that many slots and the caller evaluates only rows [0, *n_slots_now).
 * A no-op (returning the unchanged width) while requests are still queued.  Not for sessions with
 * c4_session_bind_leaf_models.  HIP graphs captured before the call carry the old width: re-capture.
 * c4_session_set_games restores the full width.  Synchronises. */
int c4_session_compact(c4_session* s, uint32_t multiple, uint32_t* n_active, uint32_t* n_slots_now);

/* GameResult list (types.rs:63-71, mcts.rs:271-313).  Two-call pattern: n_samples of every
 * game (host array of n_games uint32, 0 = unfinished), then the records of finished games
 * packed in reqs order into dst_host (capacity cap records).  Both synchronise the stream. */
/* How the session's tree arena was sized: its bytes, the blocks per slot, and the blocks per half of a reclaimed arena
 * (C4_FLAG_RECLAIM; 0 = never-reclaimed arena).  Any of the outputs may be NULL. */
int c4_session_arena(c4_session* s, uint64_t* bytes, uint32_t* blocks_per_slot, uint32_t* reclaim_half_blocks);
int c4_session_sample_counts(c4_session* s, uint32_t* counts_host, uint64_t n_games);
int c4_session_drain_samples(c4_session* s, c4_sample_rec* dst_host, uint64_t cap, uint64_t* n_written);
/* K6: packs the records of finished games, in reqs order, into the
 * caller's DEVICE buffer dst_dev (capacity cap records) so that one rank's samples are one
 * contiguous tensor for the RCCL all-gather.  *n_written = records packed.  Synchronises (the
 * per-game counts are prefix-summed on the host). */
int c4_session_pack_samples(c4_session* s, c4_sample_rec* dst_dev, uint64_t cap, uint64_t* n_written);
/* Diagnostic builds (-DC4_PHASE_STAMPS) only: per-wavefront device-clock stamps [n_waves][16] of the
 * last step launch; all zero in the product build. */
int c4_session_debug_phase_stamps(c4_session* s, uint64_t* out_host, uint64_t cap_words, uint64_t* n_words);
/* Device views for collectives (RCCL all-gather of samples): records [n_games][43], counts [n_games]. */
int c4_session_sample_store(c4_session* s, const c4_sample_rec** recs_dev, const uint32_t** counts_dev, uint64_t* n_games);

/* ---- the body of self_play() as ONE call (rust/src/self_play.rs:39-129): for a host that keeps the folded bf16 network in device
 * memory and does not want to write the schedule itself (c4a0_amd/csrc/c4_selfplay_host.hip says what the schedule is: two paired
 * sessions in one HIP graph, the output layers inside the step's launch, long graphs while slots refill and short ones in the tail,
 * narrowing, records merged in request order on the device).  Uses nothing but the entry points of this header and the HIP runtime.
 *
 * The network in the layouts the evaluator's entry points below take (what c4a0_amd/nn.py::InferenceNet holds: eval-mode BatchNorm
 * folded, the tower's weights in MFMA fragment order -- pack_tower_weights --, the first Linear of each head with its input
 * dimension permuted to the tower's [cell][channel] feature order): F = 42 * channels features; the first hidden layer of BOTH heads
 * merged into one [2F][F] matrix (policy rows first), then n_policy_hidden / n_value_hidden further [F][F] hidden layers per head,
 * then the output layers [7][F] and [2][F].  All weights bf16, all biases f32, all DEVICE pointers. */
typedef struct {
  uint32_t channels;          /* 32 or 64 (nn.py ModelConfig.conv_filter_size) */
  uint32_t n_blocks;          /* residual blocks */
  const void* tower_w0;       /* c4_conv_tower_bf16's w0_dev / w_dev / bias_dev */
  const void* tower_w;
  const float* tower_bias;
  const void* w1;             /* merged first hidden layer [2F][F], b1 [2F] */
  const float* b1;
  uint32_t n_policy_hidden;   /* hidden layers of the policy head AFTER the merged one (nn.py n_policy_layers - 2), <= 8 */
  uint32_t n_value_hidden;    /* ... of the value head (n_value_layers - 2), <= 8 */
  const void* policy_w[8];
  const float* policy_b[8];
  const void* value_w[8];
  const float* value_b[8];
  const void* policy_out_w;   /* [7][F] */
  const void* value_out_w;    /* [2][F] */
  const float* policy_out_b;  /* [7] */
  const float* value_out_b;   /* [2] */
} c4_network_bf16;

/* Everything optional (zero-initialise for the defaults; NULL = all defaults, device 0). */
typedef struct {
  int32_t device;                /* HIP device ordinal */
  uint32_t resident_games;       /* games advanced in lock-step; 0 = by job size: 4 096 / 8 192 / 16 384 (c4a0_amd/api.py default_resident_games) */
  uint32_t concurrent_sessions;  /* 0 = two paired sessions from 2 048 resident games -- except one generation (no more games than slots) of a 32-channel network --, else one; 1 or 2 to force */
  uint32_t steps_per_graph;      /* rounds per HIP-graph replay while slots are refilled; 0 = by job length (64 / 32 / 8) */
  uint32_t tail_steps_per_graph; /* ... from the first narrowing of the tail on; 0 = 16 (8 for short jobs) */
  uint32_t blocks_per_slot;      /* c4_config.blocks_per_slot */
  uint32_t flags;                /* c4_config.flags (C4_FLAG_RECLAIM / C4_FLAG_NO_RECLAIM / C4_FLAG_ONE_SIM_PER_STEP) */
  uint32_t reclaim_period;       /* c4_config.reclaim_period */
  float dirichlet_alpha;         /* EXTENSION, off while epsilon == 0: c4_session_set_dirichlet */
  float dirichlet_epsilon;
  uint64_t eval_cache_entries;   /* EXTENSION, off at 0: c4_session_set_eval_cache (split over the sessions) */
} c4_play_options;

/* Where the call's wall time went (seconds; setup_s + steady_s + tail_s + drain_s = the call) and what it chose. */
typedef struct {
  double setup_s;                /* sessions, arenas, activation buffers, streams */
  double capture_s;              /* all graph captures (the first one and those after a narrowing: inside steady_s / tail_s too) */
  double steady_s;               /* from the end of set-up (the first capture, then the first replay) until every request had been started (all slots busy) */
  double tail_s;                 /* after that, until the last game ended */
  double drain_s;                /* counters, merge, transfer of the records */
  uint64_t rounds;               /* lock-step rounds replayed */
  uint64_t rounds_until_all_started;
  uint32_t graph_captures;
  uint32_t resident_games;
  uint32_t sessions;
  uint32_t rows_at_end;          /* sum of the sessions' widths after the last narrowing */
} c4_play_phases;

/* Plays every game of reqs[0 .. n_games) to the end (self_play.rs:39-129 with the arguments of self_play.rs:39-46) and returns the
 * samples in REQUEST order: counts_host[g] = samples of game g (<= 43), records_host = their records back to back -- host memory, or
 * DEVICE memory of options->device when the records are to stay on the GPU (one rank's input to the RCCL all-gather of samples) --
 * (capacity records_cap records: 43 * n_games always suffice; a smaller buffer that turns out too small -> C4_ERR_BAD_ARG with the number
 * needed in *n_records).  totals (may be NULL) = the sessions' counters summed; phases may be NULL.  Synchronous; the records are the
 * same bytes whatever resident_games / concurrent_sessions / graph lengths are chosen (the evaluator is a function of the position,
 * a game's samples do not depend on the slot or session that plays it).  A device-side error (C4_ERR_NAN_IN_TREE, ...) is returned
 * as the status, with the slot in totals->error_slot.  Thread-safe by exclusion: calls of concurrent threads run one after another
 * (a job captures HIP graphs, which another job's set-up on the same process would break; a job fills the device anyway). */
int c4_play_games_bf16(const c4_game_metadata* reqs, uint64_t n_games, uint32_t n_mcts_iterations, float c_exploration,
                       float c_ply_penalty, const c4_network_bf16* net, const c4_play_options* options, uint32_t* counts_host,
                       c4_sample_rec* records_host, uint64_t records_cap, uint64_t* n_records, c4_counters* totals,
                       c4_play_phases* phases);
/* Searches of given positions (ABI 12): MctsGame::new_from_pos (mcts.rs:48-56) + n_mcts_iterations x [leaf -> evaluator ->
 * on_received_policy] (the run_mcts helper, mcts.rs:469-485; InteractivePlay::new_from_pos / snapshot, interactive_play.rs:33, 57) for
 * EVERY position (masks[i], values[i]) -- any position, terminal ones included -- as one job of C4_FLAG_SEARCH sessions on
 * c4_play_games_bf16's schedule.  records[i] = position i's record (game_id = i, mask / value = the position, policy = the root policy,
 * q_penalty / q_no_penalty = the root's q, meta = 2 << 16), exactly n_positions of them, in host memory or DEVICE memory of
 * options->device.  records_cap < n_positions, n_mcts_iterations == 0, and options with Dirichlet noise, an evaluation cache or a
 * reclaim flag -> C4_ERR_BAD_ARG.  totals / phases may be NULL.  Synchronous; shares c4_play_games_bf16's one-job lock and
 * c4_play_games_cancel.  The positions are not validated (c4a0_amd.api.search_positions does that on the host). */
int c4_search_positions_bf16(const uint64_t* masks, const uint64_t* values, uint64_t n_positions, uint32_t n_mcts_iterations,
                             float c_exploration, float c_ply_penalty, const c4_network_bf16* net, const c4_play_options* options,
                             c4_sample_rec* records, uint64_t records_cap, c4_counters* totals, c4_play_phases* phases);
/* Asks the c4_play_games_bf16 / c4_search_positions_bf16 call that is running (on whatever thread) to stop: it returns C4_ERR_CANCELLED after the graph replays
 * in flight (milliseconds), with everything given back and no records.  For a host's interrupt handling -- the reference's job is
 * stopped by killing the process; a job here can be minutes of one library call.  Has no effect when no job is running (a job
 * clears the request when it starts), and none on the c4_session_* entry points.  Callable from any thread. */
void c4_play_games_cancel(void);

/* ---- the hand-off right after the path: PlayGamesResult's wire format on the packed records (HOST functions: no device is
 * touched, they work on a machine without a GPU). ----
 * PlayGamesResult::to_cbor / __getstate__ (rust/src/pybridge.rs:73-92: `serde_cbor::to_vec(self)`; what `pickle.dump(games, f)` of
 * src/c4a0/training.py:62-63 runs every generation): games g = 0 .. n_games-1 with metadata metas[g] (types.rs:37-48) and counts[g]
 * samples each, the samples being consecutive entries of recs (pos, policy, q_penalty, q_no_penalty of types.rs:103-110; game_id
 * and meta of the records are not part of the wire format), written to dst as serde_cbor 0.11.2 writes the derive(Serialize)
 * structs: definite-length maps keyed by field name in declaration order, shortest-form unsigned integers, f32 as a half float
 * where that is lossless.  Two-call pattern: dst == NULL -> *n_written = the size of the document; then written to dst (cap >= it). */
int c4_records_to_cbor(const c4_game_metadata* metas, const uint32_t* counts, uint64_t n_games, const c4_sample_rec* recs,
                       uint64_t n_records, uint8_t* dst, uint64_t cap, uint64_t* n_written);
/* PlayGamesResult::from_cbor / __setstate__ (pybridge.rs:80-92: `serde_cbor::from_slice`), for documents in the form above (what
 * to_cbor and the reference write; floats of any width and integers are accepted where an f32 is expected).  Two-call pattern:
 * with metas == counts == recs == NULL the document is validated and counted (*n_games, *n_records); with buffers of those
 * capacities it is decoded, records getting game_id = their game's and meta = index | terminal flag << 16 like the generator's.
 * Anything else -> C4_ERR_BAD_ARG with the byte offset in c4_last_error_string() (the reference raises ValueError, pybridge.rs:254-259). */
int c4_cbor_to_records(const uint8_t* src, uint64_t len, c4_game_metadata* metas, uint32_t* counts, uint64_t cap_games,
                       c4_sample_rec* recs, uint64_t cap_records, uint64_t* n_games, uint64_t* n_records);

/* PlayGamesResult::split_train_test's permutation (pybridge.rs:110-112: `results.shuffle(&mut StdRng::seed_from_u64(seed))`, rand
 * 0.10.1): order[i] = index of the game the shuffle leaves at position i of a list of n_games (< 2^32 - 1) games.  The caller then
 * takes the first round(n_games * train_frac) games as the training set (pybridge.rs:113-119). */
int c4_shuffle_games(uint64_t seed, uint64_t n_games, uint32_t* order);

/* Root statistics of slot `slot` (MctsGame::root_policy / root_q_with_penalty /
 * root_q_no_penalty / root_visit_count, mcts.rs:248-268).  Synchronises. */
int c4_session_root_stats(c4_session* s, uint32_t slot, float policy[7], float* q_penalty,
                          float* q_no_penalty, uint64_t* visit_count, uint64_t* root_mask, uint64_t* root_value);
/* One int64 per slot identifying the leaf position waiting for the evaluator (value bits | the 7
 * column heights << 42; -1 for an idle slot), written to the DEVICE array keys_dev[n_slots] on the
 * session's stream, no synchronisation.  The callback evaluator sorts these on the device to find
 * the unique positions of a batch (NNThread::loop_once's HashSet, self_play.rs:203-208) instead of
 * copying every slot to the host. */
int c4_session_leaf_keys(c4_session* s, int64_t* keys_dev);

/* The callback evaluator's batch, built on the device (NNThread::loop_once, self_play.rs:203-208: the
 * reference collects the waiting leaves in a HashSet<(ModelID, Pos)> and evaluates each pair once).
 * For the session's resident games, on its stream, without synchronising:
 *   inverse_dev[n_slots]      row of each slot's (model, leaf position) pair in the batch, 0xFFFFFFFF for idle slots;
 *   rows_out[n_unique][2][6][7] float32 evaluator input of each unique pair (c4r.rs:378-392, pybridge.rs:202-221);
 *   models_out[n_unique]      its model id (mcts.rs:70-76; 0 without c4_session_bind_leaf_models), may be NULL;
 *   *n_unique_out             the number of rows.
 * Rows are ordered by the lowest slot holding the pair, so the batch depends on the games alone.
 * inverse_dev is device memory; rows_out (capacity n_slots rows), models_out (n_slots) and n_unique_out may be
 * device memory or PINNED HOST memory (hipHostMalloc / torch pin_memory): the kernels then write the
 * batch across PCIe themselves and the host reads it after synchronising the stream.  Anything else
 * (pageable host memory, another device's memory) is refused. */
int c4_session_unique_leaves(c4_session* s, uint32_t* inverse_dev, float* rows_out, uint64_t* models_out, uint32_t* n_unique_out);
/* The other half: answers[n_unique][9] (7 policy log-probabilities, q_penalty, q_no_penalty per row of the
 * batch above; device or pinned host memory) to the bound logprobs / q rows of every slot that asked --
 * what PyEvalPos hands back per position (pybridge.rs:161-199).  On the session's stream, no synchronisation:
 * the caller keeps `answers` untouched until the stream has passed this point. */
int c4_session_scatter_outputs(c4_session* s, const uint32_t* inverse_dev, const float* answers, uint32_t n_unique);

/* c4_session_scatter_outputs + c4_session_step as ONE launch: every game takes its evaluator outputs from row inverse_dev[slot] of
 * `answers` (as for c4_session_scatter_outputs: device or pinned host memory, 9 floats per row) inside the step kernel itself
 * (self_play.rs:222-236 hands each waiting game its result, :268-323 runs its job).  The bound logprobs / q tensors are NOT
 * updated: callers that watch them keep the two entry points.  Every configuration of the session (noise, cache, timing). */
int c4_session_step_gather(c4_session* s, const uint32_t* inverse_dev, const float* answers, uint32_t n_unique);

/* ---- tournaments from a HIP graph (ABI 14): route the leaves of a multi-model session by model, on the device ---- */
#define C4_ROUTE_MAX_MODELS 32    /* models one routed batch may hold */
#define C4_GROUPED_ROW_ALIGN 128  /* c4_grouped_row_align(): the rows per workgroup of every grouped kernel divide it */
/* The resident games' leaves as ONE batch of rows_cap rows grouped by the model that must answer them (c4_session_bind_leaf_models:
 * mcts.rs:70-76), for the grouped bf16 chain below.  On the session's stream, no synchronisation, may be captured in a HIP graph;
 * no count reaches the host.  A session of games with bound leaf models and bf16 planes (planes_dtype 1); search and hold sessions
 * are refused.  For slot g:
 *   group     the index m with model_ids_dev[m] == the slot's leaf model.  An idle slot (decided from the slot, as
 *             c4_session_leaf_keys does: id 0 may be a real player) is not routed: inverse_dev[g] = 0xFFFFFFFF.  A slot whose id is
 *             not in the table is not routed either and is counted in *n_unrouted_dev.
 *   segments  seg_start_dev[0] = 0, seg_start_dev[m + 1] = seg_start_dev[m] + round_up(count_m, align); a model without rows has an
 *             empty segment.
 *   rows      inverse_dev[g] = seg_start_dev[m] + the slot's rank among the routed slots of model m in ASCENDING SLOT ORDER: the
 *             batch is a function of the games alone.
 *   planes    planes_out_dev[inverse_dev[g]] = the slot's 84 bf16 plane values; the pad rows between a segment's last row and the
 *             next segment become empty boards (zeros).  Rows from seg_start_dev[n_models] on are left as they are.
 * model_ids_dev [n_models], planes_out_dev bf16 [rows_cap][2][6][7], inverse_dev [n_slots], seg_start_dev [n_models + 1] and
 * n_unrouted_dev [1] are device memory of the session's device.  Refused (C4_ERR_BAD_ARG, the message names the bound): align not
 * a power of two in 16..256; n_models 0 or above C4_ROUTE_MAX_MODELS; rows_cap < round_up(n_slots + n_models * (align - 1), align)
 * (the sum of the rounded counts can never exceed it).  For the grouped chain align must be a multiple of c4_grouped_row_align(). */
int c4_session_route_leaves(c4_session* s, const uint64_t* model_ids_dev, uint32_t n_models, uint32_t align, void* planes_out_dev,
                            uint32_t rows_cap, uint32_t* inverse_dev, uint32_t* seg_start_dev, uint32_t* n_unrouted_dev);

/* ---- hold sessions (C4_FLAG_HOLD, ABI 13): InteractivePlay's operations for every slot at once ---- */
/* InteractivePlay::increase_mcts_iters (interactive_play.rs:63-67) as an absolute target: 1 <= n <= the n_mcts_iterations the session
 * was created with (which sizes the arena and the table of logarithms), else C4_ERR_BAD_ARG.  Takes effect with the next launch on
 * the session's stream (stream-ordered); parked games stay parked until c4_session_hold_resume.  HIP graphs captured earlier carry
 * the old target, as after c4_session_compact: re-capture. */
int c4_session_set_iterations(c4_session* s, uint32_t n_mcts_iterations);
/* InteractivePlay::make_move / make_random_move (interactive_play.rs:70-85, 169-185) + ensure_bg_thread for every slot, ONE launch on
 * the session's stream: per slot the move cols[slot] (C4_HOLD_MOVE_NONE, a column 0..6, or C4_HOLD_MOVE_SAMPLE: sampled from
 * apply_temperature(root policy, temperatures[slot]) with seed game_id * (42 + moves made), mcts.rs:214-222), then: park if the root
 * is terminal or has its target's visits, else select the next leaf from the tree as it stands, write it to planes_dev and make the
 * slot active.  A move that arrives while the slot is active drops the pending leaf and selects a new one, as make_move reselects
 * (mcts.rs:205).  A REFUSED move (results[slot] = C4_HOLD_REFUSED_*) leaves its slot byte for byte as it was -- InteractivePlay
 * returning false -- and raises no error; so does a slot that is active, has visits to go and was asked no move.
 * cols == NULL: no moves, just resume after a new target (temperatures and results must then be NULL).  temperatures == NULL: 1.0.
 * results may be NULL.  The arrays have one entry per slot (n_slots) and may be device memory, pinned host memory or ordinary host
 * memory (then the call copies and synchronises the stream); device or pinned arrays must stay untouched until the stream has passed
 * the launch.  The reference's panics stay errors of the slot: C4_ERR_DEGENERATE_POLICY from a sampled move's weights. */
int c4_session_hold_resume(c4_session* s, const int32_t* cols, const float* temperatures, int32_t* results);
/* InteractivePlay::undo_move / reset_game (interactive_play.rs; MctsGame::undo_move, mcts.rs:230-245, reset_game = undo_move until it
 * returns false, mcts.rs:225-227) + ensure_bg_thread for every slot, stream-ordered on the session's stream: per slot requests[slot]
 * (C4_HOLD_UNDO_NONE, _ONE or _ALL).  results[slot]: C4_HOLD_OK (accepted, or none asked); C4_HOLD_REFUSED_REQUEST for any other
 * request value; C4_HOLD_NO_GAME for a slot without a live game; C4_HOLD_REFUSED_NO_MOVES for a game that has made no move -- a game
 * finished at its start by a terminal start position among them, which keeps its one sample.  A refused slot stays byte for byte as
 * it was, pending leaf and evaluator row included.  An ACCEPTED undo leaves the game with moves - 1 (ONE) or 0 (ALL) moves made and,
 * as the reference does, a FRESH root (Node::new(pos, Weak::new(), 1.0): no visits, no children, leaf = root) at the position that
 * move was made from, read from the game's own row of the sample store (the record of that move); the whole tree is dropped, so the
 * slot's arena starts again at block 1.  game_id and ordinal stay; the seed of the next sampled move uses the shortened move count.
 * If the game was finished, the finish is reversed: its sample count is 0 again (c4_session_sample_counts / _drain_samples /
 * _pack_samples no longer deliver it) and the session's games_done and samples counters (c4_session_counters, c4_session_poll) drop
 * by the game's share.  Records past the new move count, and the q values of the remaining ones, are stale until the next finish
 * rewrites them.  Then every slot does what c4_session_hold_resume(s, NULL, NULL, NULL) does: an undone game selects its root as
 * the pending leaf and is active.  No argument of a captured launch changes: HIP graphs captured earlier stay valid.
 * The arrays follow c4_session_hold_resume's rules (n_slots entries; device, pinned or ordinary host memory -- then the call copies
 * and synchronises the stream); results may be NULL.  requests == NULL or a session without C4_FLAG_HOLD: C4_ERR_BAD_ARG. */
int c4_session_hold_undo(c4_session* s, const int32_t* requests, int32_t* results);
/* InteractivePlay::snapshot (interactive_play.rs:57, 145-166) of every slot, ONE launch and ONE copy: dst_host[slot] = (game_id, the
 * root position, root_policy (mcts.rs:396-412), the root's q_sum / (visits + 1) (mcts.rs:359-367; the arithmetic of
 * c4_session_root_stats), meta = moves made | 3 << 16), visits_host[slot] = the root's visit count, status_host[slot] = 0 idle (no
 * game: record all zero), 1 active, C4_HOLD_PARKED, or the c4_status that ended the game.  From the mover's perspective (the
 * player-0 view of interactive_play.rs:149-153 is the caller's to apply).  Host arrays of cap >= n_slots entries, any may be NULL.
 * Synchronises. */
int c4_session_snapshot(c4_session* s, c4_sample_rec* dst_host, uint32_t* visits_host, uint32_t* status_host, uint64_t cap);
/* Non-blocking probe in the style of c4_session_poll: *n_active = the number of active slots and *max_need = the largest
 * (target - root visits) any slot had at the last c4_session_hold_resume / c4_session_start -- a bound on the rounds still needed --
 * as of the last probe that has landed; C4_HOLD_POLL_UNKNOWN for both until a probe enqueued after that resume has.  *error as
 * c4_session_poll.  Any output may be NULL. */
int c4_session_hold_poll(c4_session* s, uint32_t* n_active, uint32_t* max_need, uint32_t* error);

/* Leaf position currently waiting for the evaluator, per slot (MctsGame::leaf_pos, mcts.rs:64-66);
 * status[g] = 1 active / 0 idle (a hold session: or C4_HOLD_PARKED), ordinal[g] = index of the slot's game in reqs.  Host arrays of
 * n_slots (any may be NULL).  Synchronises.  Used by the numpy-callback compatibility mode. */
int c4_session_leaves(c4_session* s, uint64_t* masks_host, uint64_t* values_host, uint32_t* status_host,
                      uint32_t* ordinals_host);

/* ---- element-wise device functions (SURVEY 8a kernel K1 and the arithmetic pieces), all on
 * device arrays of length n, launched on `stream`; used by the parity tests. ---- */
/* c4r.rs:58-72,228-238,253-263,266-269: for each position and column: moved position (0,0 if
 * illegal), legal mask, terminal state (0 none,1 PlayerWin,2 OpponentWin,3 Draw) and terminal values. */
int c4_pos_ops(const uint64_t* mask_dev, const uint64_t* value_dev, const int32_t* col_dev, uint64_t n,
               float c_ply_penalty, uint64_t* out_mask_dev, uint64_t* out_value_dev, uint32_t* out_legal_dev,
               uint32_t* out_terminal_dev, float* out_q_dev /* [n][2] */, void* stream);
/* c4r.rs:378-392 / pybridge.rs:202-221 */
int c4_encode_planes(const uint64_t* mask_dev, const uint64_t* value_dev, uint64_t n, uint32_t planes_dtype,
                     void* planes_dev, void* stream);
/* glibc expf/logf ports (what Rust f32::exp / f32::ln call) */
int c4_expf_logf(const float* x_dev, uint64_t n, int which /*0 expf, 1 logf*/, float* y_dev, void* stream);
/* mcts.rs:416-434 (with c4r.rs:272-286 masking when legal_dev != NULL); status per row in out_err_dev */
int c4_softmax7(const float* logits_dev, const uint32_t* legal_dev, uint64_t n, float* out_dev,
                uint32_t* out_err_dev, void* stream);
/* mcts.rs:439-454 */
int c4_apply_temperature(const float* policy_dev, const float* temperature_dev, uint64_t n, float* out_dev, void* stream);
/* extension: eta_dev[n][7] = Dir(alpha) noise for (game_id, n_moves, legal mask), see c4_session_set_dirichlet */
int c4_dirichlet(const uint64_t* game_id_dev, const uint32_t* n_moves_dev, const uint32_t* legal_dev, float alpha, uint64_t n,
                 float* eta_dev, void* stream);
/* mcts.rs:214-222 without the tree update: column sampled for (game_id, n_moves, policy, temperature);
 * out_col = -1 on DEGENERATE_POLICY.  out_u32 (may be NULL) = the RNG's first word. */
int c4_sample_move(const uint64_t* game_id_dev, const uint32_t* n_moves_dev, const float* policy_dev,
                   const float* temperature_dev, uint64_t n, int32_t* out_col_dev, uint32_t* out_u32_dev, void* stream);

/* ---- bf16 evaluator (c4_conv_tower_bf16, c4_linear_bf16, c4_head_out_bf16): where the chain rounds.  Every product of two bf16
 * operands is accumulated in f32 (MFMA, in an order of the kernel's own: only the f32 accumulation order is unspecified), and a
 * value is rounded to bf16 -- round to nearest, ties to even (v_cvt_pk_bf16_f32) -- at these points and nowhere else:
 *   conv0        y = bf16(s), s = the f32 sum of the products started at the bias (so in every tower layer; no activation)
 *   block conv 1 t = bf16(s)  (no activation: the ReLU comes after the second conv)
 *   block conv 2 y = bf16(x + relu(s)), s with the BN-folded weights and bias, x the block's bf16 input widened exactly to f32, the
 *                add one f32 operation
 *   linear       y = bf16(act(acc + bias[n])), act = relu or none, the bias added in f32 after the k-loop
 *   head out     v = acc + bias in f32 (no bf16 rounding); log-softmax and tanh in f32 (device expf / logf / tanhf)
 * Biases: the tower's (conv0, both convs of each block, BN folded) and the output layers' are f32; the hidden layers' biases are
 * rounded to bf16 by c4a0_amd/nn.py::InferenceNet (the weights and biases of the heads are bf16 tensors there) and widened back to f32
 * for c4_linear_bf16's epilogue.  Tower weights and hidden / output weights are bf16.  tests/bf16_ref.py restates the chain in
 * float64 and tests/test_gpu_bf16_exact.py holds the kernels to it bit for bit on data whose every partial sum is exact in f32. */

/* ---- fp8 hidden layers (c4_quantize_bf16_fp8, c4_linear_fp8; opt-in: c4a0_amd/nn.py::InferenceNet(head_dtype=torch.float8_e4m3fn)):
 * the numerics contract.  tests/fp8_ref.py restates it in float64 with integer arithmetic of its own, tests/test_gpu_fp8_exact.py
 * holds the kernels to it bit for bit.
 * Format.  FP8 is OCP e4m3fn: bias 7, largest finite 448, smallest subnormal 2^-9, no infinities, NaN = 0x7F / 0xFF (NOT the fnuz
 *   format).  q8(v) of an f32 v: NaN -> 0x7F; otherwise clamp to [-448, 448] (an explicit f32 operation in front of the convert
 *   instruction: no mode bit decides it), then round to nearest, ties to even; subnormals and the sign of zero are kept (a
 *   negative value that rounds to zero is 0x80).  A NaN is never laundered into a finite value.
 * Weights (host, at construction; nn.py::quantize_head_weights), from the BN-folded f32 weights (never rounded to bf16 first), the
 *   first layers in the tower's cell-major order: per output row n, e_w[n] = the largest integer in [-64, 64] with
 *   max_k |W[n][k]| * 2^e_w[n] <= 448 (an all-zero row: 0); Wq[n][k] = q8(W[n][k] * 2^e_w[n]).  Powers of two: scaling is exact.
 * Activations: ONE integer exponent per GEMM input tensor, x8 = q8(x * 2^e_x), static, chosen at construction from calibration
 *   positions and never from the batch: a row's result depends on that row alone.
 * Layer (c4_linear_fp8):
 *   1. acc[m][n] = sum_k x8[m][k] * Wq[n][k] in f32 by v_mfma_f32_16x16x128_f8f6f4 (e4m3 x e4m3, no block scales), k ascending in
 *      128-deep steps (a last step of 64 where k % 128 == 64: the upper half is zeros made in registers; nothing at or beyond
 *      column k of a row is read), no split-K, no atomics: one fixed order per element whatever m, the row index or `config`;
 *   2. v = acc * dq[n] + bias[n], dq[n] = 2^(-e_x - e_w[n]) an f32 array, bias f32 as folded: an exact multiply and ONE f32
 *      rounding in the add (fmaf would give the same value);
 *   3. r = relu ? (v <= 0 ? +0 : v) : v   (a NaN stays a NaN, -0 becomes +0 under relu);
 *   4. y = q8(r * out_scale), out_scale = 2^e_x of the consuming layer (exact multiply), or y = bf16(r), round to nearest even.
 * Chain: c4_conv_tower_bf16 (unchanged, bf16) -> c4_quantize_bf16_fp8 -> the merged 2F-wide first layer (fp8 -> fp8) -> each head's
 *   further hidden layers (fp8 -> fp8), the LAST hidden layer of each head writing bf16 -> c4_head_out_bf16 or the fused output +
 *   step launch, unchanged. */

/* y[m][c] = q8(x[m][c] * scale), x bf16 [m][ldx], y e4m3 [m][ldy], c < k; columns k .. ldy - 1 of y are not written.  scale = 2^e_x
 * (positive, finite).  k % 8 == 0, ldx % 8 == 0, ldy % 8 == 0, x_dev 16-byte and y_dev 8-byte aligned (a thread moves 8 elements:
 * a 16-byte load, an 8-byte store).  No synchronisation: capturable. */
int c4_quantize_bf16_fp8(const void* x_dev /*bf16 [m][ldx]*/, void* y_dev /*fp8 [m][ldy]*/, uint32_t m, uint32_t k,
                         uint32_t ldx, uint32_t ldy, float scale /*2^e_x*/, void* stream);
/* One fp8 hidden layer, see the contract above.  n % 192 == 0, k % 64 == 0; ldx >= k, ldx % 16 == 0, x8_dev and w8_dev 16-byte
 * aligned (rows are read 16 bytes at a time; x8 may be a column view of a wider tensor: nothing at or beyond column k of a row is
 * read); ldy >= n (in elements of the output type), ldy % 4 == 0, y_dev 4-byte (fp8) or 8-byte (bf16) aligned; dq_dev and bias_dev
 * 16-byte aligned; m at most 65 535 * 64.  out_fp8 != 0: y is e4m3 = q8(r * out_scale), out_scale positive and finite; else y is
 * bf16 and out_scale is ignored.  config: 0 = automatic; 3 / 4 = operands staged through LDS, 128 x 192 / 64 x 192 tiles (the automatic
 * choices); 1 / 2 = fragments read straight from global memory, 64- / 128-row tiles (measured alternatives); all compute the same
 * bits.  x8 and w8 below 4 GiB each.  No synchronisation: capturable.  Bad arguments: C4_ERR_BAD_ARG and a c4_last_error_string. */
int c4_linear_fp8(const void* x8_dev /*[m][ldx]*/, const void* w8_dev /*[n][k]*/, const float* dq_dev /*[n]*/, const float* bias_dev /*[n]*/,
                  void* y_dev /*fp8 or bf16 [m][ldy]*/, uint32_t m, uint32_t n, uint32_t k, uint32_t ldx, uint32_t ldy,
                  uint32_t relu, uint32_t out_fp8, float out_scale, uint32_t config, void* stream);

/* ---- evaluator building block: the residual conv tower of ConnectFourNet (src/c4a0/nn.py:64-70,
 * 184-195; eval-mode BatchNorm folded into the second conv of each block) as one MFMA kernel.
 *   planes_dev bf16 [n_boards][2][6][7] (what c4_session_step writes with planes_dtype = 1)
 *   w0_dev / w_dev / bias_dev: MFMA-fragment-ordered weights, see c4a0_amd/nn.py::pack_tower_weights
 *   out_dev    bf16 [n_boards][42][channels]  (cell-major, channels last)
 * channels must be 32 or 64.  config: 0 = the workgroup shape chosen from n_boards (32 channels: 2 boards up to 512 boards, 4 up to
 * 1 024, 8 up to 1 280, else 16; 64 channels: 2 up to 512, 4 up to 1 024, else 8); 32 channels: 1 / 2 / 3 = 16 boards, 8 boards, 16 boards on 12 wavefronts, 4 / 5 = 4 boards on 12
 * wavefronts, 2 boards on 6 (the narrow launches of a job's tail); 64 channels: 2 / 3 = four wavefronts (one per SIMD, whole boards and all 64 output channels each)
 * with a weight ring 6 / 3 k-steps deep instead of the default eight wavefronts in channel-splitting pairs, 4 = the eight wavefronts
 * with the weights fetched once per workgroup into an LDS ring (a workgroup barrier per tap), 5 / 6 = 4 boards on eight wavefronts, 2 boards
 * on four (narrow launches), 1 = the default shape at any size -- every shape computes the same bits. */
int c4_conv_tower_bf16(const void* planes_dev, const void* w0_dev, const void* w_dev, const float* bias_dev,
                       uint32_t n_boards, uint32_t channels, uint32_t n_blocks, void* out_dev, uint32_t config, void* stream);

/* A hidden layer of a head (nn.py:75-100: Linear(F, F) + BatchNorm1d + ReLU, BN folded by the caller):
 *   y[m][n] = act(sum_k x[m][k] * w[n][k] + bias[n]),  x bf16 [m][ldx], w bf16 [n][k] (nn.Linear's layout),
 *   bias f32 [n], y bf16 [m][ldy]; relu != 0 applies max(., 0).  Hand-written MFMA kernel whose result for
 * a row depends on that row and the weights ONLY (one fixed summation order per element whatever m, the row
 * index or `config`): the evaluator is a function of the position, as the reference's is (one forward per
 * unique position, self_play.rs:203-237).  n % 192 == 0, k % 64 == 0 (42 * C features, C a multiple of 32); n, k, ldx,
 * ldy < 65 536; ldx % 8 == 0, ldy % 8 == 0 and x_dev, y_dev 16-byte aligned (rows are moved 16 bytes at a time); each operand
 * below 2 GiB.  config 0 = automatic, 1..59 = a specific tile configuration (tools/gemm_probe.py; all compute the same bits). */
int c4_linear_bf16(const void* x_dev, const void* w_dev, const float* bias_dev, void* y_dev, uint32_t m, uint32_t n,
                   uint32_t k, uint32_t ldx, uint32_t ldy, uint32_t relu, uint32_t config, void* stream);
/* The block -> tile map c4_linear_bf16 launches with for an m x n output cut into bm x bn tiles (XCD-rectangle order), computed
 * on the HOST with the kernels' own formula; no device is touched.  tiles_out[2 b] / [2 b + 1] = row / column tile of block b
 * (tiles_out may be NULL to ask for *n_blocks only).  For tests: the map must be a bijection onto the tile grid. */
int c4_linear_bf16_tile_map(uint32_t m, uint32_t n, uint32_t bm, uint32_t bn, uint32_t* tiles_out, uint32_t cap_blocks,
                            uint32_t* n_blocks);

/* The entry of `forward_numpy` (nn.py:119-130: `torch.from_numpy(x).to(device)` under autocast): float32 positions
 * [n_boards][2][6][7] -> the tower's bf16 planes [n_rows_out][2][6][7] (round to nearest even; rows n_boards .. n_rows_out - 1
 * become empty boards, so that a launch sized for a bucket of rows serves any smaller batch).  The batch may live in device
 * memory or in PINNED host memory (then the kernel reads it over PCIe: no staging copy).  batch_slot != NULL: the kernel
 * takes the batch's address AND its board count from *batch_slot (pinned host or device memory) instead of `src` /
 * `n_boards`, so that a captured launch (one HIP-graph replay per call) serves a different array every call.  The slot's
 * n_boards <= n_rows_out is the caller's to keep.  n_rows_out even; arrays and the slot 16-byte aligned. */
typedef struct c4_f32_batch {
  const float* data;
  uint32_t n_boards;
  uint32_t reserved;
} c4_f32_batch;
int c4_planes_from_f32(const c4_f32_batch* batch_slot, const float* src, uint32_t n_boards, void* planes_dev, uint32_t n_rows_out,
                       void* stream);

/* Output layers of both heads in one launch (nn.py:84-85,98-99): policy Linear(F->7) + LogSoftmax
 * and value Linear(F->2) + Tanh.  hidden_*_dev bf16 [n_boards][features] with row strides
 * *_row_stride elements (the last hidden activation of each head; they may be two column ranges
 * of one merged tensor, or the same pointer twice when a head has no hidden layer), w_* bf16
 * [7|2][features], b_* f32; writes logprobs_dev f32 [n_boards][7] and q_dev f32 [n_boards][2]
 * (the tensors bound with c4_session_bind_io).  features % 8 == 0. */
int c4_head_out_bf16(const void* hidden_policy_dev, const void* hidden_value_dev, const void* w_policy_dev,
                     const void* w_value_dev, const float* b_policy_dev, const float* b_value_dev,
                     uint32_t n_boards, uint32_t features, uint32_t policy_row_stride, uint32_t value_row_stride,
                     float* logprobs_dev, float* q_dev, void* stream);

/* ---- grouped bf16 chain (ABI 14): the three kernels above for a batch whose rows are cut into one segment per model --
 * seg_start_dev [n_models + 1] in DEVICE memory (c4_session_route_leaves writes it; ascending from 0, every entry a multiple of
 * c4_grouped_row_align()), model m owns rows seg_start[m] .. seg_start[m + 1] - 1 -- each segment computed with ITS model's
 * weights, in one launch of a fixed shape that covers rows_cap rows (a multiple of c4_grouped_row_align(), 1 <= n_models <=
 * C4_ROUTE_MAX_MODELS).  Every weight / bias operand is the models' operands of the ungrouped entry point stacked along a new
 * leading dimension, one model's operand after the other (the stride per model is the operand's size).  A workgroup finds the m
 * with seg_start[m] <= its first row < seg_start[m + 1], moves its weight pointers by m strides and runs the ungrouped kernel's
 * code: a row's outputs are bit-identical to those of the ungrouped entry point run with that model's weights.  Rows at or
 * beyond seg_start[n_models] are not written; rows of a segment are all computed (pad rows too).  One workgroup shape per kernel
 * and channel count (all shapes compute the same bits).  No synchronisation; may be captured. */
int c4_grouped_row_align(void); /* == C4_GROUPED_ROW_ALIGN: a multiple of the tower's boards, the GEMM's rows and the output kernel's rows per workgroup */
/* c4_conv_tower_bf16: w0_dev [n_models][3][C/16][64][8], w_dev [n_models][2 n_blocks][9][C/16][C/32][64][8], bias_dev
 * [n_models][1 + 2 n_blocks][C]; out_dev bf16 [rows_cap][42][channels]. */
int c4_conv_tower_bf16_grouped(const void* planes_dev, const void* w0_dev, const void* w_dev, const float* bias_dev, const uint32_t* seg_start_dev,
                               uint32_t n_models, uint32_t rows_cap, uint32_t channels, uint32_t n_blocks, void* out_dev, void* stream);
/* c4_linear_bf16: w_dev bf16 [n_models][n][k], bias_dev f32 [n_models][n]; x_dev may be a column range of a wider tensor (ldx > k). */
int c4_linear_bf16_grouped(const void* x_dev, const void* w_dev, const float* bias_dev, void* y_dev, const uint32_t* seg_start_dev, uint32_t n_models,
                           uint32_t rows_cap, uint32_t n, uint32_t k, uint32_t ldx, uint32_t ldy, uint32_t relu, void* stream);
/* c4_head_out_bf16: w_policy_dev bf16 [n_models][7][features], w_value_dev [n_models][2][features], b_policy_dev f32 [n_models][7],
 * b_value_dev [n_models][2]; writes answers_dev f32 [rows_cap][9] -- 7 log-probabilities, q_penalty, q_no_penalty: the row format
 * of c4_session_step_gather and c4_session_scatter_outputs.  features % 1 344 == 0. */
int c4_head_out_bf16_grouped(const void* hidden_policy_dev, const void* hidden_value_dev, const void* w_policy_dev, const void* w_value_dev,
                             const float* b_policy_dev, const float* b_value_dev, const uint32_t* seg_start_dev, uint32_t n_models, uint32_t rows_cap,
                             uint32_t features, uint32_t policy_row_stride, uint32_t value_row_stride, float* answers_dev, void* stream);

/* ---- built-in players (additive, ABI 14): the tournament's two weightless evaluators (src/c4a0/tournament.py:54-77), as PURE
 * functions of (kind, seed, model id, position) -- an answer never depends on the batch, and a game can be replayed from outside.
 * (The reference's RandomPlayer draws from torch's global generator: another answer at every call.  Here the draw is keyed by
 * the position.)  One definition for the device kernels and the host twin: c4a0_amd/csrc/c4_builtin.hpp.
 *
 * The position is read from a row's two planes in their own order, cell i = 7 * row + col:
 *     value = sum over i of [plane0[i] != 0] << i          mask = value | sum over i of [plane1[i] != 0] << i
 * C4_BUILTIN_UNIFORM (tournament.py:67-77): seven logits of exactly 1.0f, q_penalty = q_no_penalty = 0.0f.
 * C4_BUILTIN_RANDOM (tournament.py:54-64: logits in [0, 1), one q in [-1, 1) for both values), all arithmetic modulo 2^64:
 *     G = 0x9E3779B97F4A7C15
 *     mix(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  return z ^ z >> 31
 *     k = mix(seed + G);  k = mix(k ^ model_id);  k = mix(k ^ mask);  k = mix(k ^ value)
 *     u[j] = mix(k + (j + 1) * G) >> 40                   j = 0..7   (24 bits)
 *     logit[j] = (float)u[j] * 2^-24                      j = 0..6
 *     q = (float)((int)u[7] - 2^23) * 2^-23               q_penalty = q_no_penalty = q
 * Every output is a dyadic rational that f32 holds exactly: no transcendental, no rounding; host and device agree bit for bit.
 * The logits are raw (the tree's masked softmax normalises them, as for every evaluator). */
#define C4_BUILTIN_UNIFORM 0
#define C4_BUILTIN_RANDOM 1
/* A plain batch, one lane per row: planes_dev [rows][2][6][7] in f32 (planes_dtype 0) or bf16 (1: the session's encoding), rows
 * 8-byte aligned (read as 8-byte words) -> logits_out_dev f32 [rows][7], q_out_dev f32 [rows][2] (q_penalty, q_no_penalty).
 * Nothing past `rows` is read or written.  rows == 0: C4_OK without a launch.  C4_ERR_BAD_ARG: another kind or dtype, a null or
 * misaligned pointer.  No synchronisation; may be captured. */
int c4_builtin_eval(const void* planes_dev, uint32_t planes_dtype, uint32_t rows, uint32_t kind, uint64_t seed, uint64_t model_id,
                    float* logits_out_dev, float* q_out_dev, void* stream);
/* The built-in players' segments of a grouped batch (the section above): planes_dev bf16 [rows_cap][2][6][7], segment m owns rows
 * seg_start_dev[m] .. seg_start_dev[m + 1] - 1 (n_segments + 1 bounds in DEVICE memory, multiples of c4_grouped_row_align(); a
 * tournament passes the router's array moved past the networks' segments) and is answered as player (kinds[m], seeds[m],
 * model_ids[m]) into answers_dev f32 [rows_cap][9]: 7 logits, q_penalty, q_no_penalty -- c4_head_out_bf16_grouped's rows.  kinds,
 * seeds and model_ids are HOST arrays of n_segments entries, read during the call and handed to the kernel BY VALUE in its
 * arguments (at most C4_ROUTE_MAX_MODELS): a captured launch owns them, no device memory is involved.  Rows outside the given
 * segments are not written; empty segments are legal; pad rows of a segment are computed like any row.  rows_cap a multiple of
 * c4_grouped_row_align(); n_segments == 0 or rows_cap == 0: C4_OK without a launch.  No synchronisation; may be captured. */
int c4_builtin_eval_grouped(const void* planes_dev, const uint32_t* seg_start_dev, uint32_t n_segments, const uint32_t* kinds,
                            const uint64_t* seeds, const uint64_t* model_ids, uint32_t rows_cap, float* answers_dev, void* stream);
/* The same code on the CPU (no device needed): planes f32 [rows][2][6][7] in host memory -> logits [rows][7], q_penalty [rows],
 * q_no_penalty [rows] -- the three arrays of the reference's forward_numpy. */
int c4_builtin_eval_host(const float* planes, uint64_t rows, uint32_t kind, uint64_t seed, uint64_t model_id, float* logits, float* q_penalty,
                         float* q_no_penalty);

/* ---- f32 evaluator (ABI 11): ConnectFourNet in f32 (the reference trains and evaluates in f32, nn.py:119-130) on gfx950's exact-f32
 * MFMA (v_mfma_f32_16x16x4_f32), for any width C = 1..64 (padded to Cp = 16 ceil(C / 16)), any number of residual blocks and any head
 * depth.  No bf16 anywhere: f32 planes, weights, activations, accumulation.  c4a0_amd/nn.py::pack_f32_weights packs the weights.
 *
 * Summation order (the contract: a row's outputs depend on that row and the weights only -- never on n_boards, the row's position, the
 * launch shape or timing).  Every matrix product is y[m][n] = act(s), s = chain(m, n) + bias[n] (one f32 add), where chain is ONE f32
 * fmaf chain started at +0.0f over the K inputs of the product (K a multiple of 16) visited in blocks of 16, inside a block in the
 * order k = kb + 4 h + j for j = 0..3, h = 0..3 (outer j):
 *     acc = 0.0f;  for kb in 0, 16, .., K - 16:  for j in 0..3:  for h in 0..3:  acc = fmaf(W[n][kb + 4h + j], X[m][kb + 4h + j], acc)
 * Zero-padded inputs and weights are part of the chain (they add +-0 products).  The K inputs of each product:
 *   conv0      X[(g, cell)][k], k = 2 tap + ci for k < 18 (tap = 3 (dr + 1) + (dc + 1), ci = input plane), 0 for k = 18..31: the plane
 *              value at the neighbour cell, 0 off the board; W = w0 [Cp][32]; act = none
 *   conv       X[(g, cell)][k], k = tap Cp + ci (K = 9 Cp): channel ci of the neighbour cell of the cell-major features, 0 off the board;
 *              W = [Cp][9 Cp]; the first conv of a block act = none, the second (BN folded) y = x + relu(s) (x = the block's input)
 *   linear     X = the layer's input row; act = relu(s) = (s > 0 ? s : 0) for hidden layers
 *   head out   policy v[0..6] = s, value v[7..8] = s (no activation), then logp[o] = v[o] - lse with mx = fmaxf over v[0..6] left to
 *              right, sum = ((0 + e0) + e1) + .. + e6, e_o = c4_expf(v[o] - mx) (glibc expf), lse = mx + c4_logf(sum) (glibc logf);
 *              q[i] = tanhf(v[7 + i]) (device libm)
 *
 * Non-finite values follow from these rules by IEEE 754 arithmetic (no input is rejected or clamped; a NaN's payload is not specified):
 *   chain      a NaN input or weight makes every sum it enters NaN, and so does Inf x 0 (a zero weight, a zero-padded input); Inf
 *              otherwise gives +-Inf, or NaN where both signs meet.  Only the sums an element enters are affected: in the tower the cells
 *              within the receptive field of a non-finite plane value, on its board; no other cell, board or row.
 *   linear     without ReLU a NaN sum comes through; relu(s) = (s > 0 ? s : 0) turns NaN and -Inf into +0.0 and keeps +Inf.
 *   head out   a NaN logit gives seven NaN log-probabilities (fmaxf skips it, so mx is the largest other logit, but its expf is NaN
 *              and so are the sum and lse); a +Inf logit gives seven NaN (Inf - Inf); -Inf logits give -Inf there and leave the others
 *              what they are without them (their expf is +0), unless all seven are -Inf (seven NaN).  q = tanhf: +-Inf give +-1.0
 *              exactly, NaN gives NaN. */

/* The tower (nn.py:64-70, 184-195): planes_dev f32 [n_boards][2][6][7] -> out_dev f32 [n_boards][42][channels] (cell-major, the padded
 * channels are 0).  channels = Cp (16, 32, 48 or 64); w0_dev [Cp][32], w_dev [2 n_blocks][Cp][9 Cp], bias_dev [1 + 2 n_blocks][Cp];
 * work_dev: a second buffer the size of out_dev (may be NULL when n_blocks = 0).  1 + 2 n_blocks launches on `stream`.
 * Arrays 16-byte aligned. */
int c4_conv_tower_f32(const float* planes_dev, const float* w0_dev, const float* w_dev, const float* bias_dev, uint32_t n_boards,
                      uint32_t channels, uint32_t n_blocks, float* out_dev, float* work_dev, void* stream);
/* A layer of a head: y[m][n] = act(chain + bias[n]), x f32 [m][ldx] (a strided row view is fine), w f32 [n][k], bias f32 [n], y f32
 * [m][ldy]; relu != 0: act = relu.  n % 32 == 0, k % 16 == 0, ldx and ldy multiples of 4, arrays 16-byte aligned. */
int c4_linear_f32(const float* x_dev, const float* w_dev, const float* bias_dev, float* y_dev, uint32_t m, uint32_t n, uint32_t k,
                  uint32_t ldx, uint32_t ldy, uint32_t relu, void* stream);
/* Output layers of both heads (nn.py:84-85, 98-99): hidden_policy [n_boards][policy_row_stride] x w_policy [7][policy_features],
 * hidden_value [n_boards][value_row_stride] x w_value [2][value_features] -> logprobs [n_boards][7] (log-softmax) and q [n_boards][2]
 * (tanh); preact (may be NULL) [n_boards][9] receives v (7 policy logits, 2 value pre-activations).  The outputs may be pinned host
 * memory.  features multiples of 16, row strides multiples of 4, hidden rows and weights 16-byte aligned. */
int c4_head_out_f32(const float* hidden_policy_dev, const float* hidden_value_dev, const float* w_policy_dev, const float* w_value_dev,
                    const float* b_policy_dev, const float* b_value_dev, uint32_t n_boards, uint32_t policy_features, uint32_t value_features,
                    uint32_t policy_row_stride, uint32_t value_row_stride, float* logprobs, float* q, float* preact, void* stream);

/* ---- training the heads' hidden blocks (added functions only: C4_ABI_VERSION stays what it was) ------------------------------------
 * One hidden block of a head is Linear(k, n) -> BatchNorm1d(n) in train mode -> ReLU (nn.py:75-100).  Its forward product z = x W^T + b
 * is c4_linear_f32(relu = 0); the calls below are the rest of a training step.  All f32, row-major, on `stream`; n % 32 == 0,
 * k % 16 == 0, leading dimensions multiples of 4 and at least the row length, arrays 16-byte aligned (else C4_ERR_BAD_ARG, nothing is
 * launched).  Every output is a fixed function of the inputs: each sum has one order that the shape alone decides, no atomics -- two
 * calls give the same bytes.  No [m][.] matrix is copied or transposed: activations and gradients are read where they lie. */

/* mean[c], var[c]: the batch mean and the BIASED batch variance (sum (z - mean)^2 / m, two passes) of column c of z [m][ldz];
 * y[r][c] = relu(((z[r][c] - mean[c]) * rstd[c]) * gamma[c] + beta[c]), rstd = 1 / sqrt(var + eps), y [m][ldy].  m >= 2. */
int c4_train_bn_relu_fwd_f32(const float* z_dev, const float* gamma_dev, const float* beta_dev, float eps, uint32_t m, uint32_t n, uint32_t ldz,
                             uint32_t ldy, float* y_dev, float* mean_dev, float* var_dev, void* stream);
/* The backward of the call above from dy [m][lddy], the z, mean and var it was given / wrote: with g = dy where the pre-activation,
 * recomputed by the forward's own operations, is > 0, else 0 (ReLU'(0) = 0), and xh = ((z - mean) - corr) * rstd, corr = the
 * mean of the deviations z - mean (what the f32 mean is off by: without it sum_r dz, 0 in real numbers, is rounding noise times rstd^2):
 *   dbeta = sum_r g,  dgamma = sum_r g xh,  dz = gamma rstd ((g - dbeta / m) - xh dgamma / m), dz [m][lddz].  m >= 2. */
int c4_train_bn_relu_bwd_f32(const float* dy_dev, const float* z_dev, const float* mean_dev, const float* var_dev, const float* gamma_dev,
                             const float* beta_dev, float eps, uint32_t m, uint32_t n, uint32_t lddy, uint32_t ldz, uint32_t lddz, float* dz_dev,
                             float* dgamma_dev, float* dbeta_dev, void* stream);
/* dx[r][c] = sum_j dz[r][j] w[j][c]: dz [m][ldz] (n columns), w [n][k], dx [m][ldx] (k columns).  One f32-MFMA chain per element over
 * j in the order of c4_linear_f32's k.  Any m (m == 0: nothing to do). */
int c4_train_linear_dgrad_f32(const float* dz_dev, const float* w_dev, float* dx_dev, uint32_t m, uint32_t n, uint32_t k, uint32_t ldz,
                              uint32_t ldx, void* stream);
/* dw[j][c] = sum_r dz[r][j] x[r][c] and db[j] = sum_r dz[r][j]: dz [m][ldz] (n columns), x [m][ldx] (k columns), dw [n][k] (dense),
 * db [n].  One f32-MFMA chain per element of dw over the batch rows; rows past m contribute nothing.  m >= 1. */
int c4_train_linear_wgrad_f32(const float* dz_dev, const float* x_dev, float* dw_dev, float* db_dev, uint32_t m, uint32_t n, uint32_t k,
                              uint32_t ldz, uint32_t ldx, void* stream);

/* ---- training the convolution tower (c4a0_amd/train_tower.py tower="hip"; added functions only: C4_ABI_VERSION stays what it was) ------
 * The tower in train mode (nn.py:64-70, 184-195): Conv2d(2, C), then per block Conv2d(C, C) -> Conv2d(C, C) -> BatchNorm2d with batch
 * statistics -> ReLU, added to the block's input.  All f32.  Activations and their gradients are cell-major [n_boards][42][C] -- a
 * row-major matrix [42 n_boards][C], dense -- which is what c4_conv_tower_f32 writes; BatchNorm2d is then a batch norm over the
 * m = 42 n_boards rows.  channels = C is 16, 32, 48 or 64, n_boards >= 1, 42 n_boards C < 2^31, arrays 16-byte aligned (else
 * C4_ERR_BAD_ARG, nothing is launched).  Weights are packed as pack_f32_weights packs them: w0 [C][32] with k = 2 tap + ci (zero from 18
 * on), w [C][9 C] with k = tap C + ci, tap = 3 (dr + 1) + (dc + 1).  No call allocates, copies or synchronises: each may be captured.
 * work_dev is the caller's, c4_train_tower_work_bytes(n_boards, channels) bytes, its contents meaningless between calls.
 *
 * The contract: every output is a fixed function of the inputs.  Each sum has ONE order, decided by (n_boards, C) alone -- never by the
 * device, its CU count, the launch or an environment variable -- and nothing is added with atomics: two calls give the same bytes.
 *   chunks     The rows are split into chunks of C4_TRAIN_TOWER_CHUNK_BOARDS = 16 whole boards (672 rows); the last chunk holds what is
 *              left.  n_chunks = ceil(n_boards / 16).
 *   forward    c4_train_conv0_f32 / c4_train_conv3x3_f32: z = chain + bias, the "f32 evaluator" chain above (conv0 / conv, act = none).
 *              c4_train_conv0_f32's bytes are c4_conv_tower_f32(n_blocks = 0)'s.
 *   dgrad      da[cell][ci] = sum_tap sum_co dz[cell - offset(tap)][co] W[co][tap][ci] is c4_train_conv3x3_f32 on dz with
 *              W'[ci][(8 - tap) C + co] = W[co][tap C + ci] and a zero bias: the same chain over k' = (8 - tap) C + co.
 *   wgrad      per chunk, dW_c[co][k] is ONE f32 fmaf chain from +0 over the chunk's rows in ascending order,
 *              acc = fmaf(X[row][k], dz[row][co], acc), X the im2col row the forward reads (0 off the board, 0 for conv0's k >= 18); rows
 *              past the batch and cells off the board enter as SELECTED zeros (+0 products of 0 x 0, never 0 x a value read).  db_c[co]:
 *              four sums s_h from +0 over the chunk's rows = h (mod 4) in ascending order, then (s_0 + s_1) + (s_2 + s_3).
 *              Then, per element of dW and db: group g = 0..7 adds the chunks g, g + 8, g + 16, .. in order, starting FROM its first chunk;
 *              the result is ((G_0 + G_1) + ..) + G_{min(8, n_chunks) - 1}.
 *   batch norm a reduction over rows [r0, r1) in a workgroup of RG = floor(256 / (C / 4)) row groups: group g starts from +0 and adds its
 *              rows r0 + g, r0 + g + RG, .. in ascending order, then the RG sums are added as a tree: for half = 32, 16, 8, 4, 2, 1,
 *              G_g += G_{g + half} for every g < half with g + half < RG; the result is G_0.  A column's total
 *              is that reduction over the chunk's rows, per chunk, and then THE SAME reduction over the n_chunks partial sums.
 *              Elementwise arithmetic is c4_train_bn_relu_*_f32's, operation for operation (separate multiplies and adds, no fma). */
#define C4_TRAIN_TOWER_CHUNK_BOARDS 16
/* *bytes_out = the bytes of work space any call below needs at (n_boards, channels): n_chunks (9 C^2 + C) floats. */
int c4_train_tower_work_bytes(uint32_t n_boards, uint32_t channels, uint64_t* bytes_out);
/* z [42 n_boards][C] = conv0(planes [n_boards][2][6][7]) + bias, no activation. */
int c4_train_conv0_f32(const float* planes_dev, const float* w0_dev, const float* bias_dev, float* z_dev, uint32_t n_boards, uint32_t channels,
                       void* stream);
/* z [42 n_boards][C] = conv3x3(x [42 n_boards][C]) + bias, no activation; z must not be x. */
int c4_train_conv3x3_f32(const float* x_dev, const float* w_dev, const float* bias_dev, float* z_dev, uint32_t n_boards, uint32_t channels,
                         void* stream);
/* dw0 [C][32] (columns 18..31 are +0) and db [C] of the first convolution from dz [42 n_boards][C] and the planes.  Two launches. */
int c4_train_conv0_wgrad_f32(const float* dz_dev, const float* planes_dev, float* dw0_dev, float* db_dev, uint32_t n_boards, uint32_t channels,
                             float* work_dev, void* stream);
/* dw [C][9 C] and db [C] of a 3x3 convolution from dz and its input x, both [42 n_boards][C].  Two launches. */
int c4_train_conv3x3_wgrad_f32(const float* dz_dev, const float* x_dev, float* dw_dev, float* db_dev, uint32_t n_boards, uint32_t channels,
                               float* work_dev, void* stream);
/* mean[c], var[c]: the batch mean and the BIASED batch variance (sum (z - mean)^2 / m, two passes) of column c of z over the m = 42 n_boards
 * rows; y = a + relu(((z - mean) * rstd) * gamma + beta), rstd = 1 / sqrt(var + eps), relu(p) = !(p <= 0) ? p : 0 (a NaN passes); a is the
 * residual block's input.  z, a, y [m][C].  Three launches. */
int c4_train_bn2d_relu_res_fwd_f32(const float* z_dev, const float* a_dev, const float* gamma_dev, const float* beta_dev, float eps,
                                   uint32_t n_boards, uint32_t channels, float* y_dev, float* mean_dev, float* var_dev, float* work_dev,
                                   void* stream);
/* The backward of the call above with respect to z, gamma and beta (the gradient with respect to a is dy itself) from dy [m][C] and the z,
 * mean and var it was given / wrote; the formulas are c4_train_bn_relu_bwd_f32's, corrected deviations included.  Three launches. */
int c4_train_bn2d_relu_res_bwd_f32(const float* dy_dev, const float* z_dev, const float* mean_dev, const float* var_dev, const float* gamma_dev,
                                   const float* beta_dev, float eps, uint32_t n_boards, uint32_t channels, float* dz_dev, float* dgamma_dev,
                                   float* dbeta_dev, float* work_dev, void* stream);

/* ---- bf16 mixed-precision training of the hidden blocks (c4a0_amd/train_heads.py heads="bf16"; added functions only: C4_ABI_VERSION
 * stays what it was): where a block rounds.  Parameters, optimiser state and running statistics stay f32.  Every rounding to bf16 is
 * round to nearest, ties to even (v_cvt_pk_bf16_f32); a value is rounded at the points below and nowhere else; all accumulation is
 * f32.  tests/train_bf16_ref.py restates this in float64 with a bf16 rounding in integer arithmetic at exactly these points.
 * Forward
 *   1. xb = bf16(x) when the block's input is f32 (the first block of a head, fed by the tower); a bf16 input is taken as it is;
 *   2. Wb = bf16(W) from the f32 master weights, every step;
 *   3. z = bf16(acc + b): c4_linear_bf16 with relu = 0, the f32 bias passed as it is, not rounded;
 *   4. mean, var (biased): f32 over z widened exactly, two passes (sum z / m, then sum (z - mean)^2 / m);
 *   5. pre = ((z - mean) * rstd) * gamma + beta in f32, rstd = 1 / sqrt(var + eps);
 *   6. y = bf16(relu(pre)); ReLU's predicate is !(pre <= 0), as in the f32 kernels: a NaN passes.
 * Backward, from dy in bf16 (an f32 dy is rounded once)
 *   1. g = dy where the pre-activation, recomputed by the forward's operations, passes the predicate, else 0;
 *   2. dbeta = sum_r g, dgamma = sum_r g xh, f32, xh = ((z - mean) - corr) * rstd with corr the mean of the deviations z - mean
 *      (c4_train_bn_relu_bwd_f32's corrected deviations);
 *   3. dz32 = gamma rstd ((g - dbeta / m) - xh dgamma / m), evaluated as (gamma rstd / m) ((m g - dbeta) - xh dgamma): m g is exact for a
 *      bf16 g, where g - fl(dbeta / m) would round every row of a binade the same way;
 *   4. db = sum_r dz32 in f32, from the values before the rounding: (gamma rstd / m) sum_r ((m g - dbeta) - xh dgamma), the column's
 *      factor applied once, after the sum, and the rounding error of every m g - dbeta (TwoSum gives it exactly; it is the same in every
 *      row of a binade, and no row can carry it) summed beside the rounded values: db is 0 in real numbers, and what is left is
 *      dbeta's own rounding.  The sum is kept two-fold (every addition's rounding error carried along): its summands cancel;
 *   5. dz = bf16(dz32);
 *   6. dx = bf16(sum_j dz[r][j] Wb[j][c]):  c4_linear_bf16(x = dz [m][n], w = Wb^T [k][n], zero bias);
 *   7. dw = bf16(sum_r dz[r][j] xb[r][c]):  c4_linear_bf16(x = dz^T [n][mp], w = xb^T [k][mp], zero bias), mp = 64 ceil(m / 64), the pad
 *      columns exact zeros; widened exactly to f32 for the parameter's gradient.
 * Every sum has one order that the shape alone decides, there are no atomics: two calls give the same bytes.  Non-finite input: a
 * column of z that holds a NaN or an infinity, or whose sum overflows, poisons that column's y, dz, dgamma and db; dbeta is the column
 * sum of dy; no other column changes.  A pad row or column is a selected zero, never a product with zero.
 * The calls below: n % 192 == 0 (what c4_linear_bf16 needs), leading dimensions multiples of 8 and at least the row length, arrays
 * 16-byte aligned, operands below 2^31 elements; a violation is C4_ERR_BAD_ARG with a c4_last_error_string and nothing is launched.
 * No synchronisation: capturable. */

/* src [m][lds] (c columns; f32, or bf16 where src_is_bf16 != 0) -> dst bf16 [m][ldd] and / or its transpose dst_t bf16 [c][ldt]
 * (either may be NULL, not both).  ldt >= 64 ceil(m / 64); columns m .. ldt - 1 of every row of dst_t are written as zeros.  A bf16
 * source is copied bit for bit.  c % 16 == 0, m >= 1. */
int c4_train_cast_bf16(const void* src_dev, uint32_t src_is_bf16, uint32_t m, uint32_t c, uint32_t lds, void* dst_dev /*bf16 [m][ldd]*/,
                       uint32_t ldd, void* dst_t_dev /*bf16 [c][ldt]*/, uint32_t ldt, void* stream);
/* Steps 4-6 of the forward: z bf16 [m][ldz] -> y bf16 [m][ldy], mean and var f32 [n]; y_t (may be NULL) bf16 [n][ldt] receives the
 * transpose of y, zero-padded as dst_t above.  m >= 2. */
int c4_train_bn_relu_fwd_bf16(const void* z_dev, const float* gamma_dev, const float* beta_dev, float eps, uint32_t m, uint32_t n, uint32_t ldz,
                              uint32_t ldy, void* y_dev, float* mean_dev, float* var_dev, void* y_t_dev, uint32_t ldt, void* stream);
/* Steps 1-5 of the backward: dy bf16 [m][lddy], z bf16 [m][ldz], the mean and var of the call above -> dz bf16 [m][lddz], its
 * zero-padded transpose dz_t bf16 [n][ldt], dgamma, dbeta and db f32 [n].  m >= 2. */
int c4_train_bn_relu_bwd_bf16(const void* dy_dev, const void* z_dev, const float* mean_dev, const float* var_dev, const float* gamma_dev,
                              const float* beta_dev, float eps, uint32_t m, uint32_t n, uint32_t lddy, uint32_t ldz, uint32_t lddz, void* dz_dev,
                              void* dz_t_dev, uint32_t ldt, float* dgamma_dev, float* dbeta_dev, float* db_dev, void* stream);

/* ---- training: the optimiser (c4a0_amd/train_graph.py HipAdam; added functions only: C4_ABI_VERSION stays what it was) -------------
 * Adam with coupled L2 -- torch.optim.Adam(lr, betas, eps, weight_decay) -- over every parameter of a network in ONE kernel launch,
 * plus a one-thread launch that advances the step count.  All arrays f32 in device memory.
 *
 * The table: n_segs segments in device memory, the table itself 16-byte aligned, built once.  Segment s is n >= 1 elements at p, g
 * (read only), m and v, each of the four 16-byte aligned, with first_block = sum over the segments before it of
 * ceil(n / C4_ADAM_BLOCK_ELEMS) (0 for the first); n_blocks is that sum over all segments.  A workgroup's elements belong to one
 * segment.  Whatever the table says, nothing outside [0, n) of a segment's arrays is read or written.
 *
 * The step count: step_dev[0], a uint32 in device memory.  The call computes step t = step_dev[0] + 1 and leaves t behind (t < 2^32),
 * so a replayed graph advances it and the host never reads it.  From t, in float64 and each rounded to f32 ONCE (PyTorch evaluates
 * the same expressions in host doubles): bc1 = 1 - beta1^t, bc2 = 1 - beta2^t (the powers by square-and-multiply in f64),
 *   step_size = f32(lr / bc1),  sqrt_bc2 = f32(sqrt(bc2));  also wd = f32(weight_decay), e = f32(eps), w1 = f32(1 - beta1),
 *   b2 = f32(beta2), w2 = f32(1 - beta2), the differences taken in f64.
 * Per element, in f32, these operations in this order (the library is built with -ffp-contract=off; fma(a, b, c) is ONE rounding of
 * a b + c and appears only where it is written):
 *   g' = fma(wd, p, g)                     (weight_decay == 0: g' = g, p is not multiplied)
 *   m' = fma(w1, g' - m, m)                (the lerp form m + (1 - beta1)(g' - m) of torch's lerp_, not beta1 m + (1 - beta1) g')
 *   v' = fma(w2 * g', g', b2 * v)
 *   p' = fma(-step_size, m' / (sqrt(v') / sqrt_bc2 + e), p)        (sqrt and both divisions correctly rounded)
 * and p', m', v' are stored.  tests/adam_ref.py restates this in float64.  Elements are independent and there are no atomics: two
 * calls from the same state give the same bytes; a NaN or an infinity in g poisons that element's p, m and v and no other.
 * The call does not synchronise, allocate or copy: it may be captured into a graph.  C4_ERR_BAD_ARG with a c4_last_error_string, and
 * nothing launched: a null table or step_dev, n_segs == 0, n_blocks == 0, n_blocks < n_segs, a table that is not 16-byte aligned, a
 * step_dev that is not 4-byte aligned. */
#define C4_ADAM_BLOCK_ELEMS 4096  /* c4_train_adam_block_elems(): the elements of one workgroup */
typedef struct c4_adam_segment {
  float* p;             /* the parameter, updated in place */
  const float* g;       /* its gradient */
  float* m;             /* exp_avg, updated in place */
  float* v;             /* exp_avg_sq, updated in place */
  uint64_t n;           /* elements */
  uint32_t first_block; /* the first workgroup of this segment */
  uint32_t reserved;    /* 0 */
} c4_adam_segment;      /* 48 bytes */
int c4_train_adam_f32(const c4_adam_segment* table_dev, uint32_t n_segs, uint32_t n_blocks, uint32_t* step_dev, double lr, double beta1,
                      double beta2, double eps, double weight_decay, void* stream);
int c4_train_adam_block_elems(void); /* == C4_ADAM_BLOCK_ELEMS */

/* ---- training: the output layers and the loss (c4a0_amd/train_out.py outputs="hip"; added functions only: C4_ABI_VERSION stays what
 * it was) -----
 * The end of a training step (nn.py:84-85, 98-99, 160-181): Linear(k, 7) + LogSoftmax on the policy head's last activations xp,
 * Linear(k, 2) + Tanh on the value head's xv, the KL divergence against the policy targets, the two mean squared errors, and the
 * gradients of all of it.  m >= 1 rows (m <= 2^30), k a multiple of 8 (k <= 2^20).  xp, xv [m][ldxp / ldxv] are f32, or bf16 where
 * x_is_bf16 != 0 (widened exactly; all arithmetic is f32), and may be the same buffer; wp [7][k], bp [7], wv [2][k], bv [2], the
 * targets policy_t [m][7], q_pen_t [m], q_nopen_t [m], out [m][9], dz [m][9], losses [4] and every gradient of a parameter are dense
 * f32.  Row strides are multiples of 4 elements (f32) or 8 (bf16) and at least k; every array is 16-byte aligned (scale: 4 bytes).  A
 * violation is C4_ERR_BAD_ARG with a c4_last_error_string that starts with the function's name, and nothing is launched.  No call
 * allocates, copies or synchronises: each may be captured.  work_dev is the caller's, c4_train_out_work_bytes(m, k) bytes, its
 * contents meaningless between calls.  The library is built with -ffp-contract=off: fma(a, b, c) is ONE rounding and appears only
 * where it is written.  EPS = 1e-8f.
 *
 * The contract: every output is a fixed function of the inputs; each sum has ONE order, decided by (m, k) alone; no atomics, no
 * counters: two calls give the same bytes.  A row's nine `out` values and nine `dz` values are a function of that row, the
 * weights, k and (dz only) m: not of where the row lies.
 *   dot        s = x[row] . w[j] over k columns: the columns are split into groups of 8 consecutive ones; lane l = 0..63 starts from +0
 *              and takes the groups l, l + 64, l + 128, .. in ascending order, within a group s_l = fma(x[c], w[c], s_l) in ascending
 *              column order; then for off = 32, 16, 8, 4, 2, 1: s_l += s_(l xor off), every lane at once.  The result is s_0.
 *   forward    per row: z_j = dot(xp, wp_j) + bp_j (j = 0..6), u_c = dot(xv, wv_c) + bv_c (c = 0, 1);
 *              mx = fmaxf over z_0 .. z_6 in order; se = sum_j expf(z_j - mx) from +0 in order; logp_j = (z_j - mx) - logf(se);
 *              q_c = tanhf(u_c); t'_j = t_j + EPS; kl_row = fma(t'_j, logf(t'_j) - logp_j, kl_row) from +0 over j in order;
 *              st = t'_0 + t'_1 + .. + t'_6 in order; d_0 = q_0 - q_pen_t, d_1 = q_1 - q_nopen_t; the row's terms are kl_row, d_0 d_0,
 *              d_1 d_1.  out[row] = (logp_0 .. logp_6, q_0, q_1).  With fm = (float)m, the gradient of `total` at the pre-activations:
 *              dz_j = fma(expf(logp_j), st, -t'_j) / fm;  dz_(7 + c) = ((2 d_c) (1 - q_c q_c)) / fm.
 *   chunks     The rows are split into chunks of C4_TRAIN_OUT_CHUNK_ROWS = 64 rows; the last chunk holds what is left.
 *              n_chunks = ceil(m / 64).  Per chunk every reduced element is ONE chain from +0 over the chunk's rows < m in ascending
 *              order: a loss term s = s + term[row]; db_c[j] = db_c[j] + dz[row][j]; dW_c[j][c] = fma(dz[row][j], x[row][c], dW_c[j][c]).
 *              A row past m enters no sum and no product.
 *   2nd stage  per element: group g = 0..7 adds the chunks g, g + 8, g + 16, .. in order, starting FROM its first chunk; the result is
 *              ((G_0 + G_1) + ..) + G_(min(8, n_chunks) - 1).
 *   losses     kl, mse_pen, mse_nopen = 2nd stage(term) / fm;  losses = ((kl + mse_pen) + mse_nopen, kl, mse_pen, mse_nopen).
 *   backward   with s = *scale_dev, read on the device only: dx[row][c] = (fma chain from +0 over the head's j in ascending order of
 *              dz[row][j] w[j][c]) * s, written f32, or bf16 rounded ONCE (nearest, ties to even) where x_is_bf16; dW = 2nd stage(dW_c) * s,
 *              db = 2nd stage(db_c) * s.  The policy head takes dz's columns 0..6, the value head 7 and 8.
 * Non-finite input goes where this arithmetic sends it: a NaN in xp[row] reaches that row's seven logp and dz, its dxp row, kl,
 * total, every element of dwp and dbp, and nothing of the value head; in xv[row] the same for q, dz_7, dz_8, both mean squared errors,
 * total, dwv, dbv and the dxv row; a NaN policy target leaves `out` finite and reaches kl, total, the row's seven dz and what they
 * reach.  fmaxf skips a NaN logit, whose expf is NaN all the same. */
#define C4_TRAIN_OUT_CHUNK_ROWS 64
/* *bytes_out = the bytes of work space either call below needs at (m, k): 4 max(4 m + 4 n_chunks, n_chunks (9 k + 12)). */
int c4_train_out_work_bytes(uint32_t m, uint32_t k, uint64_t* bytes_out);
int c4_train_out_chunk_rows(void); /* == C4_TRAIN_OUT_CHUNK_ROWS */
/* out, dz (at an upstream gradient of 1) and losses from the activations, the parameters and the targets.  Two launches. */
int c4_train_out_loss_fwd(const void* xp_dev, const void* xv_dev, uint32_t x_is_bf16, uint32_t ldxp, uint32_t ldxv, const float* wp_dev,
                          const float* bp_dev, const float* wv_dev, const float* bv_dev, const float* policy_t_dev, const float* q_pen_t_dev,
                          const float* q_nopen_t_dev, uint32_t m, uint32_t k, float* out_dev /*[m][9]*/, float* dz_dev /*[m][9]*/,
                          float* losses_dev /*[4]*/, float* work_dev, void* stream);
/* Every gradient of the output layers from dz and the upstream gradient of `total`, *scale_dev (one float in device memory).  dxp_dev and
 * dxv_dev, [m][lddxp / lddxv] in the type of x, may each be NULL: that head's dx is then not written.  Two launches. */
int c4_train_out_loss_bwd(const float* dz_dev, const float* scale_dev, const void* xp_dev, const void* xv_dev, uint32_t x_is_bf16, uint32_t ldxp,
                          uint32_t ldxv, const float* wp_dev, const float* wv_dev, uint32_t m, uint32_t k, void* dxp_dev, void* dxv_dev,
                          uint32_t lddxp, uint32_t lddxv, float* dwp_dev, float* dbp_dev, float* dwv_dev, float* dbv_dev, float* work_dev,
                          void* stream);

/* ---- exact solver ----------------------------------------------------------------------------------------------------------
 * What the reference gets from Pascal Pons' c4solver binary, its opening book and a rocksdb cache (rust/src/solver.rs): here a HIP
 * alpha-beta search with no binary, no book and no database.  These calls only ADD functions: C4_ABI_VERSION stays what it was.
 *
 * For a non-terminal position with s stones, scores[c] is what `c4solver -a` prints and solver.rs:167-172 reads as a Solution:
 *   a full column                      C4_SOLVE_FULL_COLUMN (-1000)
 *   a move that wins at once           (43 - s) / 2
 *   any other move                     -score(the position after it)
 * score(q) = the exact negamax value: +k if the side to move wins with its (22 - k)-th stone, 0 for a draw, -k symmetrically.
 *
 * Every legal child that is not answered at once is one task; one GPU lane searches one task (null-window alpha-beta, explicit stack)
 * against ONE lossy transposition table in device memory shared by all lanes and kept by the handle across calls (the role of the
 * reference's CachingSolver).  An entry is one aligned 64-bit word (49-bit key, 8-bit bound) read and written whole, so concurrent
 * writers change how many nodes are visited, never a score.  Nothing runs unbounded: a launch gives every lane nodes_per_launch node
 * visits (a visit = a node whose moves are generated; children answered at once by the rules, the window or the table belong to
 * their parent's visit); a task unfinished then keeps its stack (320 bytes, in device memory for the length of the call) and goes on in
 * the next launch; a task that has used max_nodes_per_position visits is given up.  A position with a task given up is returned with
 * solved = 0 and seven C4_SOLVE_UNSOLVED.  Positions with few stones end there unless tasks are split and a book is kept (below). */
#define C4_SOLVE_FULL_COLUMN (-1000)
#define C4_SOLVE_UNSOLVED (-32768)                    /* INT16_MIN */
#define C4_SOLVER_TT_ENTRIES (1ull << 24)             /* the default table: 2^24 entries = 128 MB */
#define C4_SOLVER_NODES_PER_LAUNCH 3072ull            /* the defaults that 0 selects: a launch of ~50 ms with every lane busy, and ~10 s for */
#define C4_SOLVER_MAX_NODES_PER_POSITION (1ull << 20) /* a position that ends unsolved (measured: DESIGN.md section 3, profiles/solver_rate.json) */
typedef struct c4_solver c4_solver;
typedef struct {
  uint64_t nodes;          /* node visits (expanded nodes), the unit of both budgets */
  uint64_t probes;         /* all nodes entered, the answered-at-once ones included */
  uint64_t launches;
  uint64_t tasks;
  uint64_t unsolved_tasks; /* tasks given up at max_nodes_per_position */
} c4_solver_stats;

/* A solver on `device` with a table of tt_entries entries (a power of two, 16 .. 2^32; 8 bytes each), zeroed. */
int c4_solver_create(uint64_t tt_entries, int32_t device, c4_solver** out);
int c4_solver_destroy(c4_solver* handle);
/* positions_host: uint64 [n_positions][2] (mask, value) as everywhere (bit = 7 row + col), each non-terminal and well formed --
 * C4_ERR_BAD_ARG names the first that is not.  scores_out int16 [n_positions][7], solved_out uint8 [n_positions], stats_out (may be
 * NULL): host memory.  nodes_per_launch / max_nodes_per_position: 0 = the defaults above.  The work runs on `stream`; the call waits
 * for that stream only and returns when the answer is in the host arrays.  n_positions == 0 is answered without touching the device.
 * One call at a time per handle (others wait). */
int c4_solver_solve(c4_solver* handle, const uint64_t* positions_host, uint64_t n_positions, uint64_t nodes_per_launch,
                    uint64_t max_nodes_per_position, int16_t* scores_out, uint8_t* solved_out, c4_solver_stats* stats_out, void* stream);

/* ---- exact solver: splitting and the book (added functions only: C4_ABI_VERSION stays what it was) ----------------------------
 * Splitting.  One lane per task is all the width a hard position gets, and a task given up at max_nodes_per_position leaves nothing
 * behind but bounds in a lossy table.  With split_stones > 0, a task that reaches max_nodes_per_position unsolved, has fewer than
 * split_stones stones and comes while the call has made fewer than split_max_tasks tasks by splitting is REPLACED by its children: one
 * task per non-losing move, a stone deeper and each far cheaper, with a fresh budget.  Equal and mirrored positions are one node of the
 * scheduler's graph; a node whose children are all known has the value max(-child).  A task that can neither finish nor split fails
 * with everything above it: the asked positions that depend on it come back solved = 0 with seven C4_SOLVE_UNSOLVED, as before, and
 * tasks that only they needed are dropped.  The task array and the stack store on the device grow between launches (392 bytes per
 * task in flight); split_max_tasks bounds them -- a memory bound, not a tuning result.
 *
 * The book.  A solver created with book_entries > 0 keeps every exact score it obtains for a position of at most book_max_stones
 * stones -- a finished task, a combined node, an asked position whose seven scores are known -- in a lossless open-addressed table:
 * one 64-bit word per entry, the canonical key (the smaller of the 49-bit key of the position and of its mirror image) | (score + 32)
 * << 56, 0 = empty.  Only the host inserts, between launches, and sends the new words to the device's copy before the next launch; the kernel only
 * reads: on entering a node with no more stones than the book's largest entry it probes, and a hit is a leaf with the exact score.
 * A child found in the book when tasks are made needs no task (book_hits_host): asking again for a solved position costs no launch.
 * Nothing is evicted; above half full nothing more is inserted (book_full counts what was turned away).  The book lives as long as
 * the handle and can be exported and imported. */
#define C4_SOLVER_SPLIT_MAX_TASKS (1ull << 18)        /* the default of split_max_tasks: ~100 MB of device memory at 392 bytes per task */
#define C4_SOLVER_BOOK_MAX_STONES 20u                 /* the default of book_max_stones */
typedef struct {
  uint64_t struct_size;             /* sizeof(c4_solver_options) */
  uint64_t nodes_per_launch;        /* 0 = C4_SOLVER_NODES_PER_LAUNCH */
  uint64_t max_nodes_per_position;  /* 0 = C4_SOLVER_MAX_NODES_PER_POSITION */
  uint64_t split_stones;            /* tasks with fewer stones may be split; 0 = never split (c4_solver_solve) */
  uint64_t split_max_tasks;         /* tasks one call may create by splitting; 0 = C4_SOLVER_SPLIT_MAX_TASKS */
} c4_solver_options;
typedef struct {
  uint64_t nodes, probes, launches, tasks, unsolved_tasks; /* as c4_solver_stats; tasks includes those made by splitting */
  uint64_t split_tasks;     /* tasks made by splitting */
  uint64_t combined_nodes;  /* split nodes whose value came from their children */
  uint64_t dropped_tasks;   /* tasks taken off the live list because every asked position that needed them had failed */
  uint64_t book_hits_host;  /* children answered from the book when tasks were made */
  uint64_t book_inserts;    /* entries the call added to the book */
  uint64_t book_full;       /* exact scores not kept because the book was half full */
} c4_solver_stats_ex;

/* c4_solver_create with a book of book_entries entries (0 = none; else a power of two, 16 .. 2^28; 8 bytes each on the device and on
 * the host) that keeps positions of at most book_max_stones stones (0 = C4_SOLVER_BOOK_MAX_STONES; at most 41). */
int c4_solver_create_ex(uint64_t tt_entries, uint64_t book_entries, uint32_t book_max_stones, int32_t device, c4_solver** out);
/* c4_solver_solve with options (NULL = all defaults, which is c4_solver_solve(.., 0, 0, ..)) and the longer statistics (may be NULL). */
int c4_solver_solve_ex(c4_solver* handle, const uint64_t* positions_host, uint64_t n_positions, const c4_solver_options* options,
                       int16_t* scores_out, uint8_t* solved_out, c4_solver_stats_ex* stats_out, void* stream);
/* The book's entries in table order: *n_out = how many there are, of which the first min(*n_out, cap) are written to out. */
int c4_solver_book_export(c4_solver* handle, uint64_t* out, uint64_t cap, uint64_t* n_out);
/* Add entries to the book: all of them or, with C4_ERR_BAD_ARG naming the index of the first bad one, none.  An entry is valid when its
 * key decodes to a legal position (bits 49..55 clear; no stones in the sentinel row; stone counts that fit the side
 * to move; no four on the board), is the canonical key of its mirror pair, has at most book_max_stones stones n, and its score lies in
 * [-(42 - n) / 2, (43 - n) / 2], and the book or an earlier entry does not hold the same position with another score (with the same
 * score it is a duplicate and adds nothing).  Entries that would fill the book beyond half are refused as a whole too. */
int c4_solver_book_import(c4_solver* handle, const uint64_t* entries, uint64_t n);

#ifdef __cplusplus
}
#endif
#endif
