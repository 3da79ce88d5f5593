// solver_core_host.cpp -- the GPU solver's search (c4a0_amd/csrc/c4_solver_core.hpp) stepped on the CPU: the same Lane::step the
// kernel runs, one lane after another, with the launch budget, the saved stacks and the lossy table of the device path.
// Task building restates c4_solver_solve's.  Built by tests/test_solver_core_host.py with g++.
#include <cstdint>
#include <vector>

#include "../c4a0_amd/csrc/c4_solver_core.hpp"

extern "C" int emu_solve(const uint64_t* positions, uint64_t n_positions, uint64_t nodes_per_launch, uint64_t max_nodes, uint32_t log2_entries,
                         int16_t* scores, uint8_t* solved, uint64_t* stats /* nodes, probes, launches, tasks, unsolved, the most nodes of one task */) {
  static std::vector<uint64_t> tt;
  tt.assign(1ull << log2_entries, 0);
  std::vector<c4s::Task> live, next;
  for (uint64_t p = 0; p < n_positions; ++p) {
    const uint64_t mask = c4s::from_row_major(positions[2 * p]), pos = c4s::from_row_major(positions[2 * p + 1]);
    const int stones = __builtin_popcountll(mask);
    const uint64_t wins = c4s::winning_cells(pos, mask);
    solved[p] = 1;
    for (int c = 0; c < 7; ++c) {
      int16_t& out = scores[7 * p + c];
      const uint64_t move = c4s::playable(mask) & c4s::col_cells(c);
      if (!move) { out = -1000; continue; }
      if (move & wins) { out = (int16_t)((43 - stones) / 2); continue; }
      const uint64_t cpos = pos ^ mask, cmask = mask | move;
      if (stones + 1 == 42) { out = 0; continue; }
      if (c4s::can_win_next(cpos, cmask)) { out = (int16_t)(-((43 - (stones + 1)) / 2)); continue; }
      c4s::Task t{};
      t.pos = cpos; t.mask = cmask;
      t.lo = (int8_t)(-(42 - (stones + 1)) / 2);
      t.hi = (int8_t)((43 - (stones + 1)) / 2);
      t.owner = (uint32_t)(7 * p + c);
      t.slot = (uint32_t)live.size();
      out = INT16_MIN;
      live.push_back(t);
    }
  }
  for (int i = 0; i < 6; ++i) stats[i] = 0;
  stats[3] = live.size();
  std::vector<uint32_t> store(live.size() * c4s::kStackWords);     // one stack per task: an unfinished search waits here
  while (!live.empty()) {
    ++stats[2];
    for (c4s::Task& t : live) {     // one lane per task, each with a fresh launch budget
      const uint64_t left = t.nodes >= max_nodes ? 0 : max_nodes - t.nodes;
      int64_t budget = (int64_t)(left < nodes_per_launch ? left : nodes_per_launch);
      c4s::Lane lane;
      uint32_t* const stk = store.data() + (uint64_t)t.slot * c4s::kStackWords;
      lane.start(t);
      c4s::StepResult r;
      uint64_t trips = 0;
      while ((r = lane.step(stk, 1, tt.data(), log2_entries, budget)) == c4s::kRunning)
        if (lane.sp > c4s::kMaxDepth - 1 || ++trips > 64 * (nodes_per_launch + 64)) return 1;   // the bounds the kernel relies on
      t.nodes += lane.nodes; t.probes += lane.probes;
      if (t.nodes > stats[5]) stats[5] = t.nodes;
      t.lo = (int8_t)lane.lo; t.hi = (int8_t)lane.hi;
      if (r == c4s::kSolved) { t.value = (int8_t)lane.lo; t.status = 1; }
      else lane.save(t);
    }
    next.clear();
    for (const c4s::Task& t : live) {
      if (t.status == 1) { scores[t.owner] = (int16_t)(-(int)t.value); stats[0] += t.nodes; stats[1] += t.probes; }
      else if (t.nodes >= max_nodes) { ++stats[4]; solved[t.owner / 7] = 0; stats[0] += t.nodes; stats[1] += t.probes; }
      else next.push_back(t);
    }
    live.swap(next);
  }
  for (uint64_t p = 0; p < n_positions; ++p)
    if (!solved[p]) for (int c = 0; c < 7; ++c) scores[7 * p + c] = INT16_MIN;
  return 0;
}
