/* solver_ref.c -- a deliberately plain exact Connect Four solver, the checker of the GPU solver (c4a0_amd.Solver).
 *
 * Negamax with alpha-beta on the project's own bitboards (bit = 7 row + col, row 0 = bottom; `value` = the stones of the side to
 * move, `mask` = all stones): no transposition table, no null windows, no move ordering beyond centre first, no threat analysis.
 * Scores are the scale `c4solver -a` prints: +k = the side to move wins with its (22 - k)-th stone, 0 = a draw, -k = it loses to
 * the opponent's (22 - k)-th stone.  Further down the same thing with no pruning at all, which pins the pruning, and once more with
 * a transposition table (solve_scores_tt), pinned to the first, for the stone counts the plain one cannot reach in any useful time.
 *
 * A row of solve_scores for a non-terminal position with s stones: a full column -1000, a move that wins at once (43 - s) / 2,
 * any other move -score(the position after it). */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define FULL_COLUMN (-1000)

static const uint64_t COL0 = 0x810204081ull; /* bits 0, 7, .., 35 */
static const int ORDER[7] = {3, 2, 4, 1, 5, 0, 6};

static int has_four(uint64_t x) {
  const uint64_t start03 = COL0 | (COL0 << 1) | (COL0 << 2) | (COL0 << 3); /* a run to the right must not wrap into the next row */
  const uint64_t h = x & (x >> 1) & (x >> 2) & (x >> 3) & start03;
  const uint64_t v = x & (x >> 7) & (x >> 14) & (x >> 21);
  const uint64_t d1 = x & (x >> 8) & (x >> 16) & (x >> 24) & start03;
  const uint64_t d2 = (x >> 3) & (x >> 9) & (x >> 15) & (x >> 21) & start03;
  return (h | v | d1 | d2) != 0;
}

static int popcount(uint64_t x) { return __builtin_popcountll(x); }

/* the cell a stone dropped into column c lands on, 0 if the column is full */
static uint64_t drop(uint64_t mask, int c) {
  const int h = popcount(mask & (COL0 << c));
  return h >= 6 ? 0 : 1ull << (7 * h + c);
}

/* exact score of (mask, me) for the side to move, whose stones are `me`; no four on the board */
static int negamax(uint64_t mask, uint64_t me, int s, int alpha, int beta, uint64_t* nodes) {
  ++*nodes;
  if (s == 42) return 0;
  for (int c = 0; c < 7; ++c) {
    const uint64_t bit = drop(mask, c);
    if (bit && has_four(me | bit)) return (43 - s) / 2;
  }
  const int best_possible = (41 - s) / 2; /* no win now, so at best a win with the mover's next stone but one */
  if (beta > best_possible) {
    beta = best_possible;
    if (alpha >= beta) return beta;
  }
  for (int i = 0; i < 7; ++i) {
    const uint64_t bit = drop(mask, ORDER[i]);
    if (!bit) continue;
    const int v = -negamax(mask | bit, mask ^ me, s + 1, -beta, -alpha, nodes);
    if (v >= beta) return v;
    if (v > alpha) alpha = v;
  }
  return alpha;
}

/* the same value by plain minimax: every line played out to a four or a full board */
static int brute(uint64_t mask, uint64_t me, int s) {
  if (s == 42) return 0;
  int best = -1000;
  for (int c = 0; c < 7; ++c) {
    const uint64_t bit = drop(mask, c);
    if (!bit) continue;
    const int v = has_four(me | bit) ? (43 - s) / 2 : -brute(mask | bit, mask ^ me, s + 1);
    if (v > best) best = v;
  }
  return best;
}

static void row(uint64_t mask, uint64_t value, int16_t* out, int use_brute, uint64_t* nodes) {
  const int s = popcount(mask);
  for (int c = 0; c < 7; ++c) {
    const uint64_t bit = drop(mask, c);
    if (!bit) out[c] = FULL_COLUMN;
    else if (has_four(value | bit)) out[c] = (int16_t)((43 - s) / 2);
    else if (use_brute) out[c] = (int16_t)-brute(mask | bit, mask ^ value, s + 1);
    else out[c] = (int16_t)-negamax(mask | bit, mask ^ value, s + 1, -1000, 1000, nodes);
  }
}

/* positions: uint64 [n][2] (mask, value), non-terminal; scores: int16 [n][7]; returns the nodes visited */
uint64_t solve_scores(const uint64_t* positions, uint64_t n, int16_t* scores) {
  uint64_t nodes = 0;
  for (uint64_t p = 0; p < n; ++p) row(positions[2 * p], positions[2 * p + 1], scores + 7 * p, 0, &nodes);
  return nodes;
}

void brute_scores(const uint64_t* positions, uint64_t n, int16_t* scores) {
  uint64_t nodes = 0;
  for (uint64_t p = 0; p < n; ++p) row(positions[2 * p], positions[2 * p + 1], scores + 7 * p, 1, &nodes);
}

/* The second checker: the same negamax (fail-soft) with a transposition table keyed by (mask, me), and nothing else -- no null
 * windows, no threat analysis, centre-first order.  It reaches the stone counts the plain one cannot; tests/test_solver_ref.py pins it
 * to the plain one and to the brute force.
 *
 * An entry is two words: a = mask | kind << 42 | (score + 64) << 44, b = me | generation << 42.  kind: 1 the score is exact, 2 a
 * lower bound, 3 an upper bound; an entry of another generation counts as empty.  Every position of solve_scores_tt starts a new
 * generation, so its row AND its node count depend on nothing solved before it.  Always replace. */
#define TT_LOG2 23
#define TT_EXACT 1
#define TT_LOWER 2
#define TT_UPPER 3
#define TT_GENERATIONS (1u << 20)
#define CELLS ((1ull << 42) - 1)

typedef struct { uint64_t a, b; } tt_entry;
static tt_entry* tt_table;
static uint64_t tt_generation;

static uint64_t tt_slot(uint64_t mask, uint64_t me) {
  return ((mask * 0x9E3779B97F4A7C15ull) ^ (me * 0xC2B2AE3D27D4EB4Full)) * 0xD6E8FEB86659FD93ull >> (64 - TT_LOG2);
}

static int negamax_tt(uint64_t mask, uint64_t me, int s, int alpha, int beta, uint64_t* nodes) {
  ++*nodes;
  if (s == 42) return 0;
  for (int c = 0; c < 7; ++c) {
    const uint64_t bit = drop(mask, c);
    if (bit && has_four(me | bit)) return (43 - s) / 2;
  }
  const int best_possible = (41 - s) / 2;
  if (beta > best_possible) {
    beta = best_possible;
    if (alpha >= beta) return beta; /* an upper bound of the score that is no more than alpha */
  }
  tt_entry* const e = tt_table + tt_slot(mask, me);
  if ((e->a & CELLS) == mask && e->b == (me | tt_generation << 42)) {
    const int kind = (int)(e->a >> 42) & 3, known = (int)((e->a >> 44) & 0xFF) - 64;
    if (kind == TT_EXACT) return known;
    if (kind == TT_LOWER) {
      if (known >= beta) return known;
      if (known > alpha) alpha = known;
    } else {
      if (known <= alpha) return known;
      if (known < beta) beta = known;
    }
  }
  /* the window searched is (alpha, beta) as it stands now: what comes back is judged against that very window */
  int best = -1000, a = alpha;
  for (int i = 0; i < 7 && best < beta; ++i) {
    const uint64_t bit = drop(mask, ORDER[i]);
    if (!bit) continue;
    const int v = -negamax_tt(mask | bit, mask ^ me, s + 1, -beta, -a, nodes);
    if (v > best) best = v;
    if (v > a) a = v;
  }
  const int kind = best <= alpha ? TT_UPPER : best >= beta ? TT_LOWER : TT_EXACT;
  e->a = mask | (uint64_t)kind << 42 | (uint64_t)(best + 64) << 44;
  e->b = me | tt_generation << 42;
  return best;
}

/* as solve_scores; returns the nodes visited, or UINT64_MAX if there is no memory for the table (128 MiB) */
uint64_t solve_scores_tt(const uint64_t* positions, uint64_t n, int16_t* scores) {
  if (!tt_table) {
    tt_table = calloc((size_t)1 << TT_LOG2, sizeof(tt_entry));
    if (!tt_table) return UINT64_MAX;
  }
  uint64_t nodes = 0;
  for (uint64_t p = 0; p < n; ++p) {
    if (++tt_generation == TT_GENERATIONS) {
      memset(tt_table, 0, sizeof(tt_entry) << TT_LOG2);
      tt_generation = 1;
    }
    const uint64_t mask = positions[2 * p], value = positions[2 * p + 1];
    const int s = popcount(mask);
    for (int c = 0; c < 7; ++c) {
      const uint64_t bit = drop(mask, c);
      int16_t* const out = scores + 7 * p + c;
      if (!bit) *out = FULL_COLUMN;
      else if (has_four(value | bit)) *out = (int16_t)((43 - s) / 2);
      else *out = (int16_t)-negamax_tt(mask | bit, mask ^ value, s + 1, -1000, 1000, &nodes);
    }
  }
  return nodes;
}
