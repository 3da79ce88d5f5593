/* solver_ref.c -- a deliberately plain exact Connect Four solver, the checker of the GPU solver (c4a0_amd.Solver).
 *
 * Negamax with alpha-beta on the project's own bitboards (bit = 7 row + col, row 0 = bottom; `value` = the stones of the side to
 * move, `mask` = all stones): no transposition table, no null windows, no move ordering beyond centre first, no threat analysis.
 * Scores are the scale `c4solver -a` prints: +k = the side to move wins with its (22 - k)-th stone, 0 = a draw, -k = it loses to
 * the opponent's (22 - k)-th stone.  Further down the same thing with no pruning at all, which pins the pruning.
 *
 * A row of solve_scores for a non-terminal position with s stones: a full column -1000, a move that wins at once (43 - s) / 2,
 * any other move -score(the position after it). */
#include <stdint.h>

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
