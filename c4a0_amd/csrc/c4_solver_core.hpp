// c4_solver_core.hpp -- the exact solver's search, one lane's worth, written once for the device (c4_solver.hip: one lane of a
// wavefront per task) and for the host (the same file builds the tasks there, and a CPU build can step a lane for checking).
//
// Board layout of the search (not the project's row-major one, c4_device.hpp): bit = 7 * col + row, row 0 = bottom, row 6 of
// every column a sentinel that stays empty.  `pos` = the stones of the side to move, `mask` = all stones.  In this layout
//   key = pos + mask            names the position AND the side to move in 49 bits (the carry-free sum sets, per column, the
//                               cell above the top stone: the mover's stones below it are then unambiguous),
//   (mask + kBottom) & kCells   are the playable cells, and the cells that complete a four are a few shifts (winning_cells).
// The search is the published alpha-beta solver of Pascal Pons (blog.gamesolver.org): negamax on null windows that narrow
// [lo, hi] at the root, non-losing moves only, centre-first move order refined by the number of winning cells a move opens, a
// lossy transposition table of bounds.  Scores are his: +k = the side to move wins with its (22 - k)-th stone, 0 = draw.
// Beside the table a search may read a book: exact scores under canonical keys, written by the host only (c4_solver_split.hpp).
//
// A lane keeps an explicit stack of at most kMaxDepth frames of two 32-bit words (the caller gives the memory: LDS on the
// device) and advances ONE node per call of step(): lanes of a wavefront that search different trees run the same code.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define C4S_HD __host__ __device__ __forceinline__
#else
#define C4S_HD inline
#endif

namespace c4s {

constexpr uint64_t kBottom = 0x40810204081ull;       // bit 7c, c = 0..6
constexpr uint64_t kCells = kBottom * 0x3Full;       // the 42 cells (rows 0..5 of every column)
constexpr uint32_t kOrder = 0x6051423u;              // nibble i = the i-th column tried: 3 2 4 1 5 0 6
constexpr int kMaxDepth = 40;                        // frames: a node is expanded with 1..39 stones, each level adds one
constexpr int kStackWords = 2 * kMaxDepth;           // 32-bit words of one lane's stack
constexpr uint64_t kKeyMask = (1ull << 56) - 1;      // a table entry = key (49 bits) | bound << 56; 0 = empty
constexpr int kUpperBias = 32, kLowerBias = 96;      // bound byte: score + 32 = "score <= ", score + 96 = "score >= "

// One unit of work: a position whose exact score is wanted.  72 bytes, the same on host and device.
struct Task {
  uint64_t pos, mask;       // the task's root
  uint64_t nodes, probes;   // expanded nodes / all nodes entered, so far (over every launch that touched the task)
  uint64_t cur_pos, cur_mask;   // saved != 0: the node the search stood on when its lane ran out of budget ...
  int8_t lo, hi;            // the score is known to lie in [lo, hi]
  int8_t value;             // the score, once status == 1
  uint8_t status;           // 0 unfinished, 1 solved
  uint8_t saved;            // ... and that a search is under way: sp frames of it are in the stack store, at `slot`
  int8_t sp, a, b;          // ... its depth and the window of that node
  int8_t med;               // ... the null window [med, med + 1] of the root being searched
  uint8_t pad[3];
  uint32_t owner;           // the caller's: which (position, column) asked for it
  uint32_t slot;            // the task's place in the stack store (kStackWords words each)
};
static_assert(sizeof(Task) == 72, "c4s::Task layout");

C4S_HD uint64_t col_cells(int c) { return 0x3Full << (7 * c); }

// Empty cells that would complete a four for the stones in `p` (all stones: mask).
C4S_HD uint64_t winning_cells(uint64_t p, uint64_t mask) {
  uint64_t r = (p << 1) & (p << 2) & (p << 3);                  // vertical
  uint64_t q = (p << 7) & (p << 14);                            // horizontal
  r |= q & (p << 21);
  r |= q & (p >> 7);
  q = (p >> 7) & (p >> 14);
  r |= q & (p << 7);
  r |= q & (p >> 21);
  q = (p << 6) & (p << 12);                                     // diagonal, down to the right
  r |= q & (p << 18);
  r |= q & (p >> 6);
  q = (p >> 6) & (p >> 12);
  r |= q & (p << 6);
  r |= q & (p >> 18);
  q = (p << 8) & (p << 16);                                     // diagonal, up to the right
  r |= q & (p << 24);
  r |= q & (p >> 8);
  q = (p >> 8) & (p >> 16);
  r |= q & (p << 8);
  r |= q & (p >> 24);
  return r & (kCells ^ mask);
}

C4S_HD uint64_t playable(uint64_t mask) { return (mask + kBottom) & kCells; }
C4S_HD bool can_win_next(uint64_t pos, uint64_t mask) { return (winning_cells(pos, mask) & playable(mask)) != 0; }

// Playable cells that do not let the opponent win with the next stone (0: every move loses).  The mover has no winning cell.
C4S_HD uint64_t non_losing_moves(uint64_t pos, uint64_t mask) {
  uint64_t possible = playable(mask);
  const uint64_t opp = winning_cells(pos ^ mask, mask);
  const uint64_t forced = possible & opp;
  if (forced) {
    if (forced & (forced - 1)) return 0;     // two threats at once
    possible = forced;
  }
  return possible & ~(opp >> 1);             // never play right below an opponent's winning cell
}

C4S_HD uint64_t tt_index(uint64_t key, uint32_t log2_entries) { return (key * 0x9E3779B97F4A7C15ull) >> (64 - log2_entries); }

// The book (c4_solver_split.hpp): a lossless open-addressed table of exact scores that only the host writes, between launches.
// An entry = canonical key (49 bits) | (score + kUpperBias) << 56; 0 = empty.  The canonical key is the smaller of pos + mask and
// the same of the mirror image: the sum is carry-free per column, so reversing the seven 7-bit columns of the key mirrors it.
C4S_HD uint64_t mirror_columns(uint64_t x) {
  const uint64_t c = 0x7Full;
  return ((x & c) << 42) | ((x & (c << 7)) << 28) | ((x & (c << 14)) << 14) | (x & (c << 21)) | ((x >> 14) & (c << 14)) | ((x >> 28) & (c << 7)) |
         ((x >> 42) & c);
}
C4S_HD uint64_t canonical_key(uint64_t pos, uint64_t mask) {
  const uint64_t k = pos + mask, m = mirror_columns(k);
  return k < m ? k : m;
}
// Linear probing from the key's hash; the table is never more than half full, and the trip count is bounded by its size anyway.
C4S_HD bool book_probe(const uint64_t* book, uint32_t log2_book, uint64_t key, int& score) {
  const uint64_t last = (1ull << log2_book) - 1;
  uint64_t i = tt_index(key, log2_book);
  for (uint64_t trip = 0; trip <= last; ++trip) {
    const uint64_t e = book[i];
    if (e == 0) return false;
    if ((e & kKeyMask) == key) { score = (int)(e >> 56) - kUpperBias; return true; }
    i = (i + 1) & last;
  }
  return false;
}

// Row-major (bit = 7 row + col, c4_device.hpp) -> this layout.
C4S_HD uint64_t from_row_major(uint64_t x) {
  uint64_t r = 0;
  for (int row = 0; row < 6; ++row)
    for (int col = 0; col < 7; ++col) r |= ((x >> (7 * row + col)) & 1ull) << (7 * col + row);
  return r;
}

enum StepResult { kRunning = 0, kSolved = 1, kOutOfBudget = 2 };

struct Lane {
  uint64_t pos, mask;       // the node the lane stands on
  uint64_t nodes, probes;   // of this task, this launch
  int n;                    // its stones
  int sp;                   // frames on the stack
  int a, b;                 // window of the node about to be entered
  int ret;                  // value handed up when !enter
  int lo, hi, med;          // the root's bounds and the null window [med, med + 1] being searched
  bool enter;

  C4S_HD void next_window() {
    med = lo + (hi - lo) / 2;
    if (med <= 0 && lo / 2 < med) med = lo / 2;
    else if (med >= 0 && hi / 2 > med) med = hi / 2;
    a = med;
    b = med + 1;
    enter = true;
  }

  // The task's root must have no winning cell for the side to move and lo < hi.  A task with saved != 0 goes on where save()
  // left it (the caller has put its sp frames back on the stack).
  C4S_HD void start(const Task& t) {
    nodes = 0; probes = 0; ret = 0; lo = t.lo; hi = t.hi;
    if (t.saved) {
      pos = t.cur_pos; mask = t.cur_mask; sp = t.sp; a = t.a; b = t.b; med = t.med; enter = true;
    } else {
      pos = t.pos; mask = t.mask; sp = 0;
      next_window();
    }
    n = __builtin_popcountll(mask);
  }

  // After kOutOfBudget: what start() needs to go on (the caller keeps the sp frames of the stack).
  C4S_HD void save(Task& t) const {
    t.cur_pos = pos; t.cur_mask = mask; t.sp = (int8_t)sp; t.a = (int8_t)a; t.b = (int8_t)b; t.med = (int8_t)med; t.saved = 1;
  }

  // One node.  stk: the lane's stack, word w of frame f at stk[(2 f + w) * stride]; tt: the shared table; budget: expanded nodes
  // the lane may still spend (decremented).  kSolved: lo == hi == the score.  kOutOfBudget: the lane stands at the node it could
  // not expand, nothing changed; save() and the stack's sp frames are the whole search.
  template <typename Word>
  C4S_HD StepResult step(Word* stk, int stride, uint64_t* tt, uint32_t log2_entries, int64_t& budget) {
    return step_impl<false>(stk, stride, tt, log2_entries, budget, nullptr, 0, 0);
  }

  // The same with a book (book_probe): a node entered with at most book_stones stones -- the largest stone count the book holds --
  // is looked up by its canonical key, and a hit is a leaf with the exact score.
  template <typename Word>
  C4S_HD StepResult step(Word* stk, int stride, uint64_t* tt, uint32_t log2_entries, int64_t& budget, const uint64_t* book, uint32_t log2_book,
                         int book_stones) {
    return step_impl<true>(stk, stride, tt, log2_entries, budget, book, log2_book, book_stones);
  }

  template <bool BOOK, typename Word>
  C4S_HD StepResult step_impl(Word* stk, int stride, uint64_t* tt, uint32_t log2_entries, int64_t& budget, const uint64_t* book, uint32_t log2_book,
                              int book_stones) {
    bool have_ret = !enter;
    uint32_t w0 = 0;
    if (enter) {
      ++probes;
      const uint64_t possible = non_losing_moves(pos, mask);
      bool leaf = true;
      int v = 0;
      if (possible == 0) v = -(42 - n) / 2;            // the opponent wins with the next stone
      else if (n >= 40) v = 0;                         // two cells left and nobody can win
      else {
        leaf = false;
        const int mn = -(40 - n) / 2, mx = (41 - n) / 2;   // the opponent cannot win next; the mover cannot win now
        if (a < mn) { a = mn; if (a >= b) { v = a; leaf = true; } }
        if (!leaf && b > mx) { b = mx; if (a >= b) { v = b; leaf = true; } }
        if (BOOK && !leaf && n <= book_stones) {
          int exact = 0;
          if (book_probe(book, log2_book, canonical_key(pos, mask), exact)) { v = exact; leaf = true; }
        }
        if (!leaf) {
          const uint64_t key = pos + mask;
          const uint64_t e = tt[tt_index(key, log2_entries)];       // one 8-byte load: an entry is whole or absent
          if ((e & kKeyMask) == key) {
            const int val = (int)(e >> 56);
            if (val >= 64) { const int l = val - kLowerBias; if (a < l) { a = l; if (a >= b) { v = a; leaf = true; } } }
            else { const int u = val - kUpperBias; if (b > u) { b = u; if (a >= b) { v = b; leaf = true; } } }
          }
        }
        if (!leaf) {
          if (budget <= 0) { --probes; return kOutOfBudget; }     // the node is entered again when the search goes on
          --budget;
          ++nodes;
          // nibble i: 0 = column kOrder[i] is not to be tried, else 1 + the winning cells the move opens
          for (int i = 0; i < 7; ++i) {
            const int col = (kOrder >> (4 * i)) & 7;
            const uint64_t move = possible & col_cells(col);
            int s = __builtin_popcountll(winning_cells(pos | move, mask));
            s = s > 14 ? 14 : s;
            w0 |= (move ? (uint32_t)(s + 1) : 0u) << (4 * i);
          }
          stk[(2 * sp + 1) * stride] = (Word)(((uint32_t)(a & 0xFF)) | ((uint32_t)(b & 0xFF) << 8));
          ++sp;
        }
      }
      if (leaf) { ret = v; have_ret = true; }
    }
    if (have_ret) {
      if (sp == 0) {                                   // a null window of the root is answered
        if (ret <= med) hi = ret; else lo = ret;
        if (lo >= hi) return kSolved;
        next_window();
        return kRunning;
      }
      w0 = (uint32_t)stk[(2 * (sp - 1)) * stride];
      const uint32_t w1 = (uint32_t)stk[(2 * (sp - 1) + 1) * stride];
      a = (int)(int8_t)(w1 & 0xFF);
      b = (int)(int8_t)((w1 >> 8) & 0xFF);
      const int col = (kOrder >> (4 * ((w0 >> 28) & 7))) & 7;    // take the move back
      const uint64_t in_col = mask & col_cells(col);
      const uint64_t top = in_col ^ ((in_col >> 1) & col_cells(col));
      mask &= ~top;
      pos ^= mask;
      --n;
      const int score = -ret;
      if (score >= b) {                                // cut: a lower bound of this node
        tt[tt_index(pos + mask, log2_entries)] = (pos + mask) | ((uint64_t)(score + kLowerBias) << 56);
        ret = score; --sp; enter = false;
        return kRunning;
      }
      if (score > a) {
        a = score;
        stk[(2 * (sp - 1) + 1) * stride] = (Word)(((uint32_t)(a & 0xFF)) | ((uint32_t)(b & 0xFF) << 8));
      }
    }
    // the next move of the top frame: the largest nibble, the first among equals (centre first)
    uint32_t best = 0, bi = 0;
    for (uint32_t i = 0; i < 7; ++i) {
      const uint32_t nib = (w0 >> (4 * i)) & 15u;
      if (nib > best) { best = nib; bi = i; }
    }
    if (best == 0) {                                   // every move tried: an upper bound of this node
      tt[tt_index(pos + mask, log2_entries)] = (pos + mask) | ((uint64_t)(a + kUpperBias) << 56);
      ret = a; --sp; enter = false;
      return kRunning;
    }
    w0 = (w0 & ~(15u << (4 * bi)) & 0x0FFFFFFFu) | (bi << 28);
    stk[(2 * (sp - 1)) * stride] = (Word)w0;
    const int col = (kOrder >> (4 * bi)) & 7;
    const uint64_t move = (mask + (1ull << (7 * col))) & col_cells(col);
    pos ^= mask;
    mask |= move;
    ++n;
    const int na = -b, nb = -a;
    a = na; b = nb; enter = true;
    return kRunning;
  }
};

}  // namespace c4s
