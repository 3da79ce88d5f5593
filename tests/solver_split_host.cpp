// solver_split_host.cpp -- the solver's scheduler and book (c4a0_amd/csrc/c4_solver_split.hpp) driven on the CPU: the "one launch" it
// asks for is a loop over the Lane::step the kernel runs, one lane per task, with the launch budget, the stack store that grows with
// its content kept, the lossy table and -- once the book holds something -- the step overload that probes it.
// Built by tests/test_solver_split_host.py with g++: as a shared library for ctypes, and with -DSPLIT_HOST_MAIN as a stand-alone
// program (compiled with -fsanitize=address,undefined there) that checks itself on playout positions of its own.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../c4a0_amd/csrc/c4_solver_split.hpp"

namespace {

struct Emu {
  std::vector<uint64_t> tt;
  uint32_t log2_entries;
  c4split::Book book;
  std::vector<uint32_t> store;      // kStackWords words per slot
  bool bounds_broken = false;
};

int run_launch(Emu& e, const c4split::Options& opt, c4s::Task* tasks, uint32_t n, uint32_t n_slots) {
  if (e.store.size() < (size_t)n_slots * c4s::kStackWords) e.store.resize((size_t)n_slots * c4s::kStackWords);      // keeps what it holds
  e.book.changed.clear();                                                                                            // the lanes read the book itself
  for (uint32_t i = 0; i < n; ++i) {
    c4s::Task& t = tasks[i];
    if (t.slot >= n_slots) { e.bounds_broken = true; return 1; }
    const uint64_t left = t.nodes >= opt.max_nodes_per_position ? 0 : opt.max_nodes_per_position - t.nodes;
    int64_t budget = (int64_t)(left < opt.nodes_per_launch ? left : opt.nodes_per_launch);
    c4s::Lane lane;
    uint32_t* const stk = e.store.data() + (size_t)t.slot * c4s::kStackWords;
    lane.start(t);
    c4s::StepResult r;
    uint64_t trips = 0;
    for (;;) {
      r = e.book.top_stones >= 0 ? lane.step(stk, 1, e.tt.data(), e.log2_entries, budget, e.book.words.data(), e.book.log2_entries, e.book.top_stones)
                                 : lane.step(stk, 1, e.tt.data(), e.log2_entries, budget);
      if (r != c4s::kRunning) break;
      if (lane.sp > c4s::kMaxDepth - 1 || ++trips > 64 * (opt.nodes_per_launch + 64)) { e.bounds_broken = true; return 1; }   // what the kernel relies on
    }
    t.nodes += lane.nodes; t.probes += lane.probes;
    t.lo = (int8_t)lane.lo; t.hi = (int8_t)lane.hi;
    if (r == c4s::kSolved) { t.value = (int8_t)lane.lo; t.status = 1; }
    else lane.save(t);
  }
  return 0;
}

void say(char* err, uint64_t cap, const std::string& what) {
  if (err && cap) snprintf(err, cap, "%s", what.c_str());
}

}  // namespace

extern "C" {

void* sp_create(uint32_t log2_entries, uint64_t book_entries, int book_max_stones) {
  Emu* e = new Emu;
  e->log2_entries = log2_entries;
  e->tt.assign(1ull << log2_entries, 0);
  e->book.create(book_entries, book_max_stones);
  return e;
}

void sp_destroy(void* h) { delete static_cast<Emu*>(h); }

// stats: the eleven words of c4split::Stats.  Returns a c4split::Status, or -1 when a lane broke a bound the kernel relies on.
int sp_solve(void* h, const uint64_t* positions, uint64_t n, uint64_t nodes_per_launch, uint64_t max_nodes, uint64_t split_stones,
             uint64_t split_max_tasks, int16_t* scores, uint8_t* solved, uint64_t* stats, char* err, uint64_t err_cap) {
  Emu& e = *static_cast<Emu*>(h);
  const c4split::Options opt{nodes_per_launch, max_nodes, split_stones, split_max_tasks};
  c4split::Stats st{};
  std::string why;
  const c4split::Status r = c4split::solve(positions, n, opt, e.book, scores, solved, st, why,
                                           [&](c4s::Task* tasks, uint32_t n_tasks, uint32_t n_slots) { return run_launch(e, opt, tasks, n_tasks, n_slots); });
  memcpy(stats, &st, sizeof(st));
  say(err, err_cap, why);
  return e.bounds_broken ? -1 : (int)r;
}

uint64_t sp_canonical_key(uint64_t mask_row_major, uint64_t value_row_major) {
  return c4s::canonical_key(c4s::from_row_major(value_row_major), c4s::from_row_major(mask_row_major));
}

uint64_t sp_book_size(void* h) { return static_cast<Emu*>(h)->book.count; }
uint64_t sp_book_export(void* h, uint64_t* out, uint64_t cap) { return static_cast<Emu*>(h)->book.export_to(out, cap); }
int sp_book_import(void* h, const uint64_t* entries, uint64_t n, char* err, uint64_t err_cap) {
  std::string why;
  const c4split::Status r = static_cast<Emu*>(h)->book.import(entries, n, why);
  say(err, err_cap, why);
  return (int)r;
}

}  // extern "C"

#ifdef SPLIT_HOST_MAIN
namespace {

// Distinct non-terminal positions of `stones` stones from random playouts (row-major mask, value of the side to move).
std::vector<uint64_t> playouts(int count, int stones, uint64_t seed) {
  std::vector<uint64_t> out;
  while ((int)out.size() < 2 * count) {
    uint64_t mask = 0, mover = 0;
    int height[7] = {0, 0, 0, 0, 0, 0, 0};
    bool dead = false;
    for (int n = 0; n < stones && !dead; ++n) {
      int col;
      do {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        col = (int)((seed >> 33) % 7);
      } while (height[col] == 6);
      const uint64_t stone = 1ull << (7 * height[col]++ + col);
      mask |= stone;
      mover |= stone;
      dead = c4split::has_four_row_major(mover);
      mover = mask & ~mover;                       // the other side moves next
    }
    if (dead) continue;
    bool seen = false;
    for (size_t i = 0; i < out.size(); i += 2) seen |= out[i] == mask && out[i + 1] == mover;
    if (!seen) { out.push_back(mask); out.push_back(mover); }
  }
  return out;
}

int failures = 0;
#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) { ++failures; printf("line %d: %s\n", __LINE__, #cond); } \
  } while (0)

struct Answer {
  std::vector<int16_t> scores;
  std::vector<uint8_t> solved;
  uint64_t stats[11];
  int status;
};

Answer ask(void* h, const std::vector<uint64_t>& pos, uint64_t per_launch, uint64_t max_nodes, uint64_t split_stones, uint64_t cap) {
  Answer a;
  const uint64_t n = pos.size() / 2;
  a.scores.assign(7 * n, 0);
  a.solved.assign(n, 0);
  char err[200];
  a.status = sp_solve(h, pos.data(), n, per_launch, max_nodes, split_stones, cap, a.scores.data(), a.solved.data(), a.stats, err, sizeof(err));
  return a;
}

bool all_or_nothing(const Answer& a, const Answer& want) {
  bool ok = true;
  for (size_t p = 0; p < a.solved.size(); ++p)
    for (int c = 0; c < 7; ++c) ok &= a.scores[7 * p + c] == (a.solved[p] ? want.scores[7 * p + c] : c4split::kUnsolved);
  return ok;
}

uint64_t count(const std::vector<uint8_t>& v) {
  uint64_t k = 0;
  for (uint8_t x : v) k += x;
  return k;
}

}  // namespace

int main() {
  const std::vector<uint64_t> pos = playouts(40, 24, 7);
  const uint64_t n = pos.size() / 2;
  void* plain = sp_create(16, 0, 20);
  const Answer want = ask(plain, pos, 1ull << 30, 1ull << 30, 0, 1);      // the search itself is pinned by tests/test_solver_core_host.py
  EXPECT(want.status == 0 && count(want.solved) == n);
  sp_destroy(plain);

  void* a = sp_create(12, 1 << 17, 41);
  const Answer unsplit = ask(a, pos, 8, 64, 0, 1);
  EXPECT(unsplit.status == 0 && count(unsplit.solved) < n && all_or_nothing(unsplit, want));
  const Answer capped = ask(a, pos, 8, 64, 42, 20);
  EXPECT(capped.status == 0 && all_or_nothing(capped, want) && capped.stats[5] >= 20 && capped.stats[5] < 27);
  const Answer split = ask(a, pos, 8, 64, 42, 1 << 18);
  EXPECT(split.status == 0 && count(split.solved) == n && split.scores == want.scores);
  const Answer again = ask(a, pos, 8, 64, 42, 1 << 18);
  EXPECT(again.status == 0 && again.stats[2] == 0 && again.scores == want.scores);

  std::vector<uint64_t> entries(sp_book_size(a));
  EXPECT(sp_book_export(a, entries.data(), entries.size()) == entries.size() && !entries.empty());
  void* b = sp_create(12, 1 << 17, 41);
  char err[200];
  EXPECT(sp_book_import(b, entries.data(), entries.size(), err, sizeof(err)) == 0 && sp_book_size(b) == entries.size());
  const Answer loaded = ask(b, pos, 8, 64, 42, 1 << 18);
  EXPECT(loaded.status == 0 && loaded.stats[2] == 0 && loaded.scores == want.scores);
  std::vector<uint64_t> bad = entries;
  bad[bad.size() / 2] |= 1ull << 50;
  void* c = sp_create(12, 1 << 17, 41);
  EXPECT(sp_book_import(c, bad.data(), bad.size(), err, sizeof(err)) == 1 && sp_book_size(c) == 0);
  EXPECT(std::string(err).find("entry " + std::to_string(bad.size() / 2) + ":") == 0);

  void* tiny = sp_create(12, 16, 41);
  const Answer full = ask(tiny, pos, 8, 64, 42, 1 << 18);
  EXPECT(full.status == 0 && full.scores == want.scores && full.stats[10] > 0 && sp_book_size(tiny) == 8);
  for (void* h : {a, b, c, tiny}) sp_destroy(h);
  if (failures) printf("FAILED: %d\n", failures);
  else printf("solver_split_host ok\n");
  return failures != 0;
}
#endif
