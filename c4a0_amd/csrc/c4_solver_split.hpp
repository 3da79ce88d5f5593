// c4_solver_split.hpp -- the exact solver's host side, free of HIP: the book of exact scores and the scheduler that turns asked
// positions into tasks, runs launches over them and, where a task exhausts its budget, replaces it by its children.
//
// The scheduler is written once for the device and for a CPU build: solve() takes a callable that runs ONE launch over an array of
// tasks (c4_solver.hip: upload, solver_kernel, download; tests/solver_split_host.cpp: a loop over Lane::step).
//
// A node is a position with the side to move.  While splitting is on, nodes are keyed by their canonical key (c4_solver_core.hpp), so
// equal and mirrored positions are one node with several parents.  A node is
//   live     a task searches it;
//   split    its task reached max_nodes_per_position unsolved, and it now waits for its children -- one per non-losing move, each a
//            stone deeper: those the rules answer at once, those in the book and those already in the graph are linked, the rest
//            become live nodes with a fresh budget.  When every child is known its value is max(-child);
//   done     its exact score is known: it goes to the book and to whoever waits for it;
//   failed   it could neither finish nor split (too many stones for split_stones, or the call has made split_max_tasks tasks by
//            splitting), or a child of it failed.  An asked position that depends on a failed node is returned unsolved as a whole;
//   dropped  no asked position that can still be solved depends on it: its task left the live list.
// While splitting is off there is no graph: a task's owner is the output that asked for it, and the loop is the plain one -- run a
// launch, take out what finished or reached its budget, go on with the rest.
// Every launch spends budget or finishes a task, every task ends at max_nodes_per_position, and splitting makes at most
// split_max_tasks + 6 tasks: the loop is bounded.
#pragma once
#include <stdint.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "c4_solver_core.hpp"

namespace c4split {

constexpr int16_t kFullColumn = -1000, kUnsolved = INT16_MIN;
constexpr uint64_t kCellsRowMajor = (1ull << 42) - 1;
constexpr uint32_t kNone = 0xFFFFFFFFu;
constexpr int kDefaultBookMaxStones = 20;

enum Status { kOk = 0, kBadArg = 1, kRunFailed = 2, kNoProgress = 3 };

struct Options {              // all resolved: no field means "the default" here
  uint64_t nodes_per_launch;
  uint64_t max_nodes_per_position;
  uint64_t split_stones;      // tasks with fewer stones may be split; 0 = never
  uint64_t split_max_tasks;   // tasks the call may create by splitting
};

struct Stats {                // include/c4a0_hip.h c4_solver_stats_ex, field for field
  uint64_t nodes, probes, launches, tasks, unsolved_tasks;
  uint64_t split_tasks, combined_nodes, dropped_tasks, book_hits_host, book_inserts, book_full;
};

inline bool has_four_row_major(uint64_t x) {
  const uint64_t col0 = 0x810204081ull, start03 = col0 | (col0 << 1) | (col0 << 2) | (col0 << 3);
  const uint64_t h = x & (x >> 1) & (x >> 2) & (x >> 3) & start03;
  const uint64_t v = x & (x >> 7) & (x >> 14) & (x >> 21);
  const uint64_t d1 = x & (x >> 8) & (x >> 16) & (x >> 24) & start03;
  const uint64_t d2 = (x >> 3) & (x >> 9) & (x >> 15) & (x >> 21) & start03;
  return (h | v | d1 | d2) != 0;
}

// Why a row-major (mask, value) cannot be solved, or nullptr.
inline const char* refuse_position(uint64_t rm, uint64_t rv) {
  if ((rm | rv) & ~kCellsRowMajor) return "bits outside the 42 cells";
  if (rv & ~rm) return "value has bits outside mask";
  if (((rm >> 7) & ~rm) & kCellsRowMajor) return "a stone above an empty cell";
  if (has_four_row_major(rv) || has_four_row_major(rm & ~rv) || rm == kCellsRowMajor) return "the position is terminal";
  return nullptr;
}

// A four among the stones `p`, in the search's layout (bit = 7 col + row).
inline bool has_four(uint64_t p) {
  for (int s : {1, 6, 7, 8}) {
    const uint64_t m = p & (p >> s);
    if (m & (m >> (2 * s))) return true;
  }
  return false;
}

// The book on the host: the array the device reads a copy of.  Only insert() writes; `changed` lists the words written since the
// owner of the device copy last brought it up to date (and cleared the list).
struct Book {
  std::vector<uint64_t> words;
  uint32_t log2_entries = 0;
  uint64_t count = 0;
  int max_stones = kDefaultBookMaxStones;     // positions with more stones are not kept
  int top_stones = -1;                        // the largest stone count present
  std::vector<uint64_t> changed;              // indices into words

  void create(uint64_t entries, int max_stones_) {
    words.assign(entries, 0);
    log2_entries = 0;
    while ((1ull << log2_entries) < entries) ++log2_entries;
    count = 0; top_stones = -1; changed.clear();
    max_stones = max_stones_;
  }
  bool enabled() const { return !words.empty(); }
  bool find(uint64_t key, int& score) const { return enabled() && c4s::book_probe(words.data(), log2_entries, key, score); }

  // 0 inserted, 1 already there, 2 refused: the book is half full.
  int insert(uint64_t key, int score, int stones) {
    int have = 0;
    if (find(key, have)) return 1;
    if (2 * (count + 1) > words.size()) return 2;
    const uint64_t last = words.size() - 1;
    uint64_t i = c4s::tt_index(key, log2_entries);
    while (words[i] != 0) i = (i + 1) & last;
    words[i] = key | ((uint64_t)(score + c4s::kUpperBias) << 56);
    ++count;
    if (stones > top_stones) top_stones = stones;
    changed.push_back(i);
    return 0;
  }

  // Why `e` is no entry of a book that keeps positions of up to max_stones stones, or nullptr; *stones_out: its stone count.
  static const char* refuse_entry(uint64_t e, int max_stones, int* stones_out) {
    const uint64_t key = e & c4s::kKeyMask;
    if (key >> 49) return "bits between the key and the score";
    uint64_t pos = 0, mask = 0;
    for (int c = 0; c < 7; ++c) {
      // a column of h stones adds pos + 2^h - 1 to the key: one more is the marker bit 2^h above the mover's stones
      const uint32_t col = ((uint32_t)(key >> (7 * c)) & 0x7Fu) + 1;
      const int h = 31 - __builtin_clz(col);
      if (h > 6) return "stones in the sentinel row";
      mask |= (uint64_t)((1u << h) - 1) << (7 * c);
      pos |= (uint64_t)(col - (1u << h)) << (7 * c);
    }
    const int n = __builtin_popcountll(mask);
    if (__builtin_popcountll(pos) != n / 2) return "the stone counts of the two sides do not fit the side to move";
    if (has_four(pos) || has_four(pos ^ mask)) return "a position with a four on the board";
    if (key != c4s::canonical_key(pos, mask)) return "not the canonical key of the position and its mirror image";
    if (n > max_stones) return "more stones than book_max_stones";
    const int score = (int)(e >> 56) - c4s::kUpperBias;
    if (score < -(42 - n) / 2 || score > (43 - n) / 2) return "a score outside the range of the stone count";
    if (stones_out) *stones_out = n;
    return nullptr;
  }

  // All of `entries` or none: kBadArg names the first entry refused.
  Status import(const uint64_t* entries, uint64_t n, std::string& err) {
    std::vector<int> stones(n);
    for (uint64_t i = 0; i < n; ++i)
      if (const char* why = refuse_entry(entries[i], max_stones, &stones[i])) {
        err = "entry " + std::to_string(i) + ": " + why;
        return kBadArg;
      }
    // a key the book or an earlier entry already has: the same score is a duplicate and adds nothing, another score is refused
    std::unordered_map<uint64_t, int> seen;
    uint64_t fresh = 0;
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t key = entries[i] & c4s::kKeyMask;
      const int score = (int)(entries[i] >> 56) - c4s::kUpperBias;
      int have = 0;
      const auto it = seen.find(key);
      bool known = it != seen.end();
      if (known) have = it->second;
      else known = find(key, have);
      if (known && have != score) {
        err = "entry " + std::to_string(i) + ": the position is already known with the score " + std::to_string(have);
        return kBadArg;
      }
      if (!known) { seen.emplace(key, score); ++fresh; }
    }
    if (2 * (count + fresh) > words.size()) {
      err = std::to_string(n) + " entries do not fit a book of " + std::to_string(words.size()) + " that stays at most half full";
      return kBadArg;
    }
    for (uint64_t i = 0; i < n; ++i) insert(entries[i] & c4s::kKeyMask, (int)(entries[i] >> 56) - c4s::kUpperBias, stones[i]);
    return kOk;
  }

  uint64_t export_to(uint64_t* out, uint64_t cap) const {      // returns the number of entries; writes min(that, cap)
    uint64_t k = 0;
    for (uint64_t w : words)
      if (w != 0) { if (k < cap) out[k] = w; ++k; }
    return k;
  }
};

namespace detail {

enum NodeState : uint8_t { kLive, kSplit, kDone, kFailed, kDropped };

struct Link { uint32_t value, next; };      // one element of a list kept in Graph::links (no allocation per node)

struct Node {
  uint64_t pos, mask;
  uint32_t parents = kNone;          // list: split nodes that wait for this one (a node twice where two of its moves lead here)
  uint32_t owners = kNone;           // list: outputs 7 p + c of asked positions that wait for it
  uint32_t child[7];
  uint8_t n_children = 0;
  NodeState state = kLive;
  int8_t best = -128;                // split: max(-child) over the children known so far
  uint8_t pending = 0;               // split: children not known yet
};

struct Graph {
  const uint64_t* positions;
  uint64_t n_positions;
  const Options& opt;
  Book& book;
  Stats& st;
  int16_t* scores;
  uint8_t* solved;
  const bool splitting;
  std::vector<Node> nodes;
  std::vector<Link> links;
  std::unordered_map<uint64_t, uint32_t> by_key;     // splitting only
  std::vector<uint32_t> roots;                       // splitting only: node of output 7 p + c, or kNone
  std::vector<uint8_t> waiting;                      // per asked position: outputs not known yet
  std::vector<c4s::Task> live, next;
  std::vector<uint32_t> free_slots;
  uint32_t n_slots = 0;
  bool new_failure = false;

  Graph(const uint64_t* positions_, uint64_t n, const Options& o, Book& b, Stats& s, int16_t* scores_, uint8_t* solved_)
      : positions(positions_), n_positions(n), opt(o), book(b), st(s), scores(scores_), solved(solved_), splitting(o.split_stones != 0) {}

  void push(uint32_t& head, uint32_t value) {
    links.push_back(Link{value, head});
    head = (uint32_t)links.size() - 1;
  }

  void remember(uint64_t pos, uint64_t mask, int value) {
    const int n = __builtin_popcountll(mask);
    if (!book.enabled() || n > book.max_stones) return;
    const int r = book.insert(c4s::canonical_key(pos, mask), value, n);
    if (r == 0) ++st.book_inserts;
    else if (r == 2) ++st.book_full;
  }

  // An asked position whose seven outputs are known is itself a position with an exact score.
  void remember_asked(uint64_t p) {
    int best = -128;
    for (int c = 0; c < 7; ++c)
      if (scores[7 * p + c] != kFullColumn && scores[7 * p + c] > best) best = scores[7 * p + c];
    remember(c4s::from_row_major(positions[2 * p + 1]), c4s::from_row_major(positions[2 * p]), best);
  }

  // owner: the node made for the task while splitting is on, else `out`, the output 7 p + c that asked for it.
  uint32_t new_task(uint64_t pos, uint64_t mask, std::vector<c4s::Task>& to, uint32_t out = kNone) {
    uint32_t id = out;
    if (splitting) {
      id = (uint32_t)nodes.size();
      nodes.emplace_back();
      nodes.back().pos = pos;
      nodes.back().mask = mask;
    }
    const int n = __builtin_popcountll(mask);
    c4s::Task t{};
    t.pos = pos; t.mask = mask;
    t.lo = (int8_t)(-(42 - n) / 2);
    t.hi = (int8_t)((43 - n) / 2);
    t.owner = id;
    if (free_slots.empty()) t.slot = n_slots++;
    else { t.slot = free_slots.back(); free_slots.pop_back(); }
    to.push_back(t);
    return id;
  }

  void answer(uint32_t out, int score) {
    scores[out] = (int16_t)score;
    if (--waiting[out / 7] == 0 && solved[out / 7]) remember_asked(out / 7);
  }

  void finish(uint32_t id, int value) {      // recursion: one level per stone at the most
    nodes[id].state = kDone;
    nodes[id].best = (int8_t)value;
    remember(nodes[id].pos, nodes[id].mask, value);
    for (uint32_t l = nodes[id].owners; l != kNone; l = links[l].next) answer(links[l].value, -value);
    for (uint32_t l = nodes[id].parents; l != kNone; l = links[l].next) {
      const uint32_t p = links[l].value;
      Node& pa = nodes[p];
      if (pa.state != kSplit) continue;
      if (-value > pa.best) pa.best = (int8_t)(-value);
      if (--pa.pending == 0) { ++st.combined_nodes; finish(p, pa.best); }
    }
  }

  void fail(uint32_t id) {
    if (nodes[id].state == kFailed) return;
    nodes[id].state = kFailed;
    new_failure = true;
    for (uint32_t l = nodes[id].owners; l != kNone; l = links[l].next) solved[links[l].value / 7] = 0;
    for (uint32_t l = nodes[id].parents; l != kNone; l = links[l].next) fail(links[l].value);
  }

  // The task of node `id` reached its budget: its children take its place.
  void split(uint32_t id) {
    const uint64_t pos = nodes[id].pos, mask = nodes[id].mask;
    const int n = __builtin_popcountll(mask);
    const uint64_t moves = c4s::non_losing_moves(pos, mask);
    nodes[id].state = kSplit;
    bool child_failed = false;
    for (int c = 0; c < 7 && moves; ++c) {
      const uint64_t move = moves & c4s::col_cells(c);
      if (!move) continue;
      const uint64_t cpos = pos ^ mask, cmask = mask | move;
      int v = 0;
      bool known = true;
      if (c4s::non_losing_moves(cpos, cmask) == 0) v = -(42 - (n + 1)) / 2;      // what step() answers without spending budget
      else if (n + 1 >= 40) v = 0;
      else if (book.find(c4s::canonical_key(cpos, cmask), v)) ++st.book_hits_host;
      else known = false;
      uint32_t kid = kNone;
      if (!known) {
        const uint64_t key = c4s::canonical_key(cpos, cmask);
        const auto it = by_key.find(key);
        if (it != by_key.end()) kid = it->second;
        else {
          kid = new_task(cpos, cmask, next);
          by_key.emplace(key, kid);
          ++st.split_tasks;
          ++st.tasks;
        }
        if (nodes[kid].state == kDone) { v = nodes[kid].best; known = true; }
        else if (nodes[kid].state == kFailed) child_failed = true;
      }
      Node& nd = nodes[id];                    // new_task may have moved the nodes
      if (kid != kNone) nd.child[nd.n_children++] = kid;
      if (known) { if (-v > nd.best) nd.best = (int8_t)(-v); }
      else { ++nd.pending; push(nodes[kid].parents, id); }
    }
    if (child_failed) fail(id);
    else if (nodes[id].pending == 0) {
      ++st.combined_nodes;
      finish(id, moves ? nodes[id].best : -(42 - n) / 2);
    }
  }

  // Tasks that no asked position still to be solved depends on leave `next`.
  void drop_unneeded() {
    std::vector<uint8_t> need(nodes.size(), 0);
    std::vector<uint32_t> stack;
    for (uint64_t p = 0; p < n_positions; ++p) {
      if (!solved[p]) continue;
      for (int c = 0; c < 7; ++c) {
        const uint32_t r = roots[7 * p + c];
        if (r != kNone && !need[r]) { need[r] = 1; stack.push_back(r); }
      }
    }
    while (!stack.empty()) {
      const Node& nd = nodes[stack.back()];
      stack.pop_back();
      if (nd.state != kSplit) continue;
      for (int i = 0; i < nd.n_children; ++i)
        if (!need[nd.child[i]]) { need[nd.child[i]] = 1; stack.push_back(nd.child[i]); }
    }
    size_t kept = 0;
    for (const c4s::Task& t : next) {
      if (need[t.owner]) { next[kept++] = t; continue; }
      ++st.dropped_tasks;
      st.nodes += t.nodes; st.probes += t.probes;
      free_slots.push_back(t.slot);
      Node& nd = nodes[t.owner];
      nd.state = kDropped;
      const auto it = by_key.find(c4s::canonical_key(nd.pos, nd.mask));
      if (it != by_key.end() && it->second == t.owner) by_key.erase(it);
    }
    next.resize(kept);
    // a split node nobody needs waits for children that are gone: a later split must not link to it
    for (size_t i = 0; i < nodes.size(); ++i) {
      if (need[i] || nodes[i].state != kSplit) continue;
      nodes[i].state = kDropped;
      const auto it = by_key.find(c4s::canonical_key(nodes[i].pos, nodes[i].mask));
      if (it != by_key.end() && it->second == i) by_key.erase(it);
    }
  }

  // The tasks of the asked positions: what a position itself answers is answered here.
  Status make_roots(std::string& err) {
    waiting.assign(n_positions, 0);
    if (splitting) roots.assign(7 * n_positions, kNone);
    live.reserve(n_positions * 4);
    if (splitting) {
      nodes.reserve(n_positions * 4);
      links.reserve(n_positions * 4);
    }
    for (uint64_t p = 0; p < n_positions; ++p) {
      const uint64_t rm = positions[2 * p], rv = positions[2 * p + 1];
      if (const char* why = refuse_position(rm, rv)) {
        err = "position " + std::to_string(p) + ": " + why;
        return kBadArg;
      }
      const uint64_t mask = c4s::from_row_major(rm), pos = c4s::from_row_major(rv);
      const int stones = __builtin_popcountll(mask);
      const uint64_t wins = c4s::winning_cells(pos, mask);
      solved[p] = 1;
      for (int c = 0; c < 7; ++c) {
        const uint32_t o = (uint32_t)(7 * p + c);
        int16_t& out = scores[o];
        const uint64_t move = c4s::playable(mask) & c4s::col_cells(c);
        if (!move) { out = kFullColumn; continue; }
        if (move & wins) { out = (int16_t)((43 - stones) / 2); continue; }
        const uint64_t cpos = pos ^ mask, cmask = mask | move;      // the child: the other side to move
        if (stones + 1 == 42) { out = 0; continue; }
        if (c4s::can_win_next(cpos, cmask)) { out = (int16_t)(-((43 - (stones + 1)) / 2)); continue; }
        int v = 0;
        if (book.enabled() && book.find(c4s::canonical_key(cpos, cmask), v)) { out = (int16_t)(-v); ++st.book_hits_host; continue; }
        out = kUnsolved;
        ++waiting[p];
        if (splitting) {
          const uint64_t key = c4s::canonical_key(cpos, cmask);
          const auto it = by_key.find(key);
          uint32_t id = kNone;
          if (it != by_key.end()) id = it->second;
          else by_key.emplace(key, id = new_task(cpos, cmask, live));
          roots[o] = id;
          push(nodes[id].owners, o);
        } else {
          new_task(cpos, cmask, live, o);
        }
      }
      if (waiting[p] == 0) remember_asked(p);
    }
    st.tasks = live.size();
    return kOk;
  }
};

}  // namespace detail

// Solve `positions` (uint64 [n][2], row-major mask and value) into scores int16 [n][7] and solved uint8 [n].
// run(tasks, n_tasks, n_slots) -> 0 or an error: one launch over tasks[0 .. n_tasks), whose slots are all < n_slots; it may read
// `book` (and must bring a copy of it up to date from book.changed).  Slots keep their content from launch to launch.
template <typename Run>
Status solve(const uint64_t* positions, uint64_t n_positions, const Options& opt, Book& book, int16_t* scores, uint8_t* solved, Stats& st,
             std::string& err, Run&& run) {
  st = Stats{};
  detail::Graph g(positions, n_positions, opt, book, st, scores, solved);
  if (const Status s = g.make_roots(err)) return s;
  uint64_t spent_before = 0;
  while (!g.live.empty()) {
    if (run(g.live.data(), (uint32_t)g.live.size(), g.n_slots) != 0) return kRunFailed;
    ++st.launches;
    uint64_t spent = 0, finished = 0;
    for (const c4s::Task& t : g.live) { spent += t.nodes; finished += t.status; }
    if (spent == spent_before && finished == 0) {     // every launch spends budget or finishes a task: anything else must not loop
      err = "a launch made no progress";
      return kNoProgress;
    }
    g.next.clear();
    for (size_t i = 0; i < g.live.size(); ++i) {
      const c4s::Task t = g.live[i];
      if (t.status != 1 && t.nodes < opt.max_nodes_per_position) { g.next.push_back(t); continue; }
      st.nodes += t.nodes; st.probes += t.probes;
      if (!g.splitting) {
        if (t.status == 1) { g.remember(t.pos, t.mask, t.value); g.answer(t.owner, -(int)t.value); }
        else { ++st.unsolved_tasks; solved[t.owner / 7] = 0; }
        continue;
      }
      g.free_slots.push_back(t.slot);                 // a split drops the saved search: the children start afresh
      if (t.status == 1) g.finish(t.owner, t.value);
      else if ((uint64_t)__builtin_popcountll(t.mask) < opt.split_stones && st.split_tasks < opt.split_max_tasks) g.split(t.owner);
      else { ++st.unsolved_tasks; g.fail(t.owner); }
    }
    if (g.splitting && g.new_failure) g.drop_unneeded();
    g.new_failure = false;
    g.live.swap(g.next);
    spent_before = 0;
    for (const c4s::Task& t : g.live) spent_before += t.nodes;
  }
  for (uint64_t p = 0; p < n_positions; ++p) {
    if (solved[p] && g.waiting[p] != 0) {             // never: every node ends done, failed or dropped
      err = "position " + std::to_string(p) + " was left waiting";
      return kNoProgress;
    }
    if (!solved[p])
      for (int c = 0; c < 7; ++c) scores[7 * p + c] = kUnsolved;
  }
  return kOk;
}

}  // namespace c4split
