// c4_solver.hip -- the exact solver (include/c4a0_hip.h, "exact solver"): c4_solver_create / c4_solver_solve / c4_solver_destroy.
//
// Every legal child of an input position that neither wins at once nor is won at once by the reply is one task (c4_solver_core.hpp);
// one lane of a wavefront searches one task with an explicit stack in LDS, one node per trip of the kernel's only loop, and takes
// the next task index from a global counter when it is done.  All lanes share one lossy transposition table in HBM whose entries
// are single aligned 64-bit words, read and written with plain 8-byte loads and stores: a racing writer replaces a whole entry by
// another whole entry, every bound is true whoever stored it, so races change node counts and never scores.  A launch gives each
// lane a budget of expanded nodes; a lane that runs out writes its task back unfinished -- with the few words that say where
// the search stood, and its stack into the task's slot of a stack store in device memory -- and exits; the host loop below compacts
// the unfinished tasks and launches again, and whichever lane picks such a task up goes on from there.  (Starting an unfinished
// task again from its root and trusting the table to lead back was measured first: with a table much smaller than the number of
// lanes writing to it, tasks larger than a launch budget never finished.)
#include "c4_host.hpp"
#include "c4_solver_core.hpp"

#include <algorithm>
#include <mutex>
#include <vector>

namespace {

constexpr int kLanes = 64;                       // one wavefront per workgroup: 40 frames x 2 words x 64 lanes = 20 KB of LDS
constexpr uint32_t kMaxBlocks = 256 * 8;         // 8 such workgroups fit the LDS of each of the 256 CUs
constexpr uint64_t kCellsRowMajor = (1ull << 42) - 1;

__global__ __launch_bounds__(kLanes) void solver_kernel(c4s::Task* __restrict__ tasks, uint32_t n_tasks, uint32_t* __restrict__ next_task,
                                                        uint32_t* __restrict__ stack_store, uint32_t n_slots, uint64_t* __restrict__ tt,
                                                        uint32_t log2_entries, int64_t nodes_per_launch, uint64_t max_nodes_per_task) {
  __shared__ uint32_t stack[c4s::kMaxDepth * 2 * kLanes];
  uint32_t* const stk = stack + threadIdx.x;
  c4s::Lane lane;
  int64_t lane_budget = nodes_per_launch;
  int64_t budget = 0;          // of the task in hand: what the lane has left, or less where the task nears its own cap
  int64_t granted = 0;
  uint64_t nodes_before = 0, probes_before = 0;
  uint32_t idx = 0;
  bool have_task = false;
  // every trip is one node (or one task fetch); a trip either spends budget or pops a frame, so the loop is bounded by the budget
  for (;;) {
    if (!have_task) {
      if (lane_budget <= 0) break;
      idx = atomicAdd(next_task, 1u);
      if (idx >= n_tasks) break;
      const c4s::Task t = tasks[idx];
      if (t.slot >= n_slots || t.sp < 0 || t.sp >= c4s::kMaxDepth) break;      // never: the host made the slots
      if (t.saved)
        for (int w = 0; w < 2 * t.sp; ++w) stk[w * kLanes] = stack_store[(size_t)t.slot * c4s::kStackWords + w];
      lane.start(t);
      nodes_before = t.nodes;
      probes_before = t.probes;
      const uint64_t left = t.nodes >= max_nodes_per_task ? 0 : max_nodes_per_task - t.nodes;
      granted = budget = left < (uint64_t)lane_budget ? (int64_t)left : lane_budget;
      have_task = true;
    }
    const c4s::StepResult r = lane.step(stk, kLanes, tt, log2_entries, budget);
    if (r != c4s::kRunning) {
      c4s::Task* t = tasks + idx;
      t->nodes = nodes_before + lane.nodes;
      t->probes = probes_before + lane.probes;
      t->lo = (int8_t)lane.lo;
      t->hi = (int8_t)lane.hi;
      if (r == c4s::kSolved) { t->value = (int8_t)lane.lo; t->status = 1; }
      else {
        lane.save(*t);
        for (int w = 0; w < 2 * lane.sp; ++w) stack_store[(size_t)t->slot * c4s::kStackWords + w] = stk[w * kLanes];
      }
      lane_budget -= granted - budget;   // a task that stopped at its own cap leaves the lane budget for the next one
      have_task = false;
    }
  }
}

struct Solver {
  int device = 0;
  uint64_t* tt = nullptr;
  uint32_t log2_entries = 0;
  c4s::Task* tasks_dev = nullptr;
  uint32_t* stacks_dev = nullptr;      // kStackWords words per task of the call: where an unfinished search waits for its next launch
  uint32_t* counter_dev = nullptr;
  size_t tasks_cap = 0;
  std::mutex mu;
};

bool has_four_row_major(uint64_t x) {
  const uint64_t col0 = 0x810204081ull, start03 = col0 | (col0 << 1) | (col0 << 2) | (col0 << 3);
  const uint64_t h = x & (x >> 1) & (x >> 2) & (x >> 3) & start03;
  const uint64_t v = x & (x >> 7) & (x >> 14) & (x >> 21);
  const uint64_t d1 = x & (x >> 8) & (x >> 16) & (x >> 24) & start03;
  const uint64_t d2 = (x >> 3) & (x >> 9) & (x >> 15) & (x >> 21) & start03;
  return (h | v | d1 | d2) != 0;
}

}  // namespace

extern "C" {

int c4_solver_create(uint64_t tt_entries, int32_t device, c4_solver** out) {
  if (!out) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_create: out is NULL");
  *out = nullptr;
  if (tt_entries < 16 || tt_entries > (1ull << 32) || (tt_entries & (tt_entries - 1)))
    return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_create: tt_entries must be a power of two between 16 and 2^32");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return c4host::fail(C4_ERR_NO_DEVICE, "c4_solver_create: no HIP device");
  if (device < 0 || device >= n_dev) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_create: no such device");
  C4_ON_DEVICE(device);
  Solver* s = new Solver;
  s->device = device;
  while ((1ull << s->log2_entries) < tt_entries) ++s->log2_entries;
  hipError_t e = hipMalloc(&s->tt, tt_entries * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMemset(s->tt, 0, tt_entries * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMalloc(&s->counter_dev, sizeof(uint32_t));
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    (void)hipFree(s->tt);
    (void)hipFree(s->counter_dev);
    delete s;
    return c4host::fail(C4_ERR_HIP, std::string("c4_solver_create: ") + hipGetErrorString(e));
  }
  *out = reinterpret_cast<c4_solver*>(s);
  return C4_OK;
}

int c4_solver_destroy(c4_solver* handle) {
  if (!handle) return C4_OK;
  Solver* s = reinterpret_cast<Solver*>(handle);
  C4_ON_DEVICE(s->device);
  (void)hipFree(s->tt);
  (void)hipFree(s->tasks_dev);
  (void)hipFree(s->stacks_dev);
  (void)hipFree(s->counter_dev);
  delete s;
  return C4_OK;
}

int c4_solver_solve(c4_solver* handle, const uint64_t* positions_host, uint64_t n_positions, uint64_t nodes_per_launch,
                    uint64_t max_nodes_per_position, int16_t* scores_out, uint8_t* solved_out, c4_solver_stats* stats_out, void* stream_) {
  if (!handle) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_solve: handle is NULL");
  if (stats_out) *stats_out = c4_solver_stats{};
  if (n_positions == 0) return C4_OK;
  if (!positions_host || !scores_out || !solved_out) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_solve: NULL array");
  if (n_positions > (1ull << 28)) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_solve: more than 2^28 positions in one call");
  if (nodes_per_launch == 0) nodes_per_launch = C4_SOLVER_NODES_PER_LAUNCH;
  if (max_nodes_per_position == 0) max_nodes_per_position = C4_SOLVER_MAX_NODES_PER_POSITION;
  if (nodes_per_launch > (1ull << 40)) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_solve: nodes_per_launch above 2^40");
  Solver* s = reinterpret_cast<Solver*>(handle);
  hipStream_t stream = (hipStream_t)stream_;
  std::lock_guard<std::mutex> lock(s->mu);
  C4_ON_DEVICE(s->device);

  // the tasks: what the position itself answers is answered here
  std::vector<c4s::Task> tasks;
  tasks.reserve(n_positions * 4);
  for (uint64_t p = 0; p < n_positions; ++p) {
    const uint64_t rm = positions_host[2 * p], rv = positions_host[2 * p + 1];
    const char* why = nullptr;
    if ((rm | rv) & ~kCellsRowMajor) why = "bits outside the 42 cells";
    else if (rv & ~rm) why = "value has bits outside mask";
    else if (((rm >> 7) & ~rm) & kCellsRowMajor) why = "a stone above an empty cell";
    else if (has_four_row_major(rv) || has_four_row_major(rm & ~rv) || rm == kCellsRowMajor) why = "the position is terminal";
    if (why) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_solve: position " + std::to_string(p) + ": " + why);
    const uint64_t mask = c4s::from_row_major(rm), pos = c4s::from_row_major(rv);
    const int stones = __builtin_popcountll(mask);
    const uint64_t wins = c4s::winning_cells(pos, mask);
    solved_out[p] = 1;
    for (int c = 0; c < 7; ++c) {
      int16_t& out = scores_out[7 * p + c];
      const uint64_t move = c4s::playable(mask) & c4s::col_cells(c);
      if (!move) { out = C4_SOLVE_FULL_COLUMN; continue; }
      if (move & wins) { out = (int16_t)((43 - stones) / 2); continue; }
      const uint64_t cpos = pos ^ mask, cmask = mask | move;      // the child: the other side to move
      if (stones + 1 == 42) { out = 0; continue; }
      if (c4s::can_win_next(cpos, cmask)) { out = (int16_t)(-((43 - (stones + 1)) / 2)); continue; }
      c4s::Task t{};
      t.pos = cpos; t.mask = cmask;
      t.lo = (int8_t)(-(42 - (stones + 1)) / 2);
      t.hi = (int8_t)((43 - (stones + 1)) / 2);
      t.owner = (uint32_t)(7 * p + c);
      t.slot = (uint32_t)tasks.size();
      out = C4_SOLVE_UNSOLVED;
      tasks.push_back(t);
    }
  }
  c4_solver_stats st{};
  st.tasks = tasks.size();
  const uint32_t n_slots = (uint32_t)tasks.size();
  if (tasks.size() > s->tasks_cap) {
    (void)hipFree(s->tasks_dev);
    (void)hipFree(s->stacks_dev);
    s->tasks_dev = nullptr;
    s->stacks_dev = nullptr;
    s->tasks_cap = 0;
    HIP_TRY(hipMalloc(&s->tasks_dev, tasks.size() * sizeof(c4s::Task)));
    HIP_TRY(hipMalloc(&s->stacks_dev, tasks.size() * c4s::kStackWords * sizeof(uint32_t)));
    s->tasks_cap = tasks.size();
  }
  std::vector<c4s::Task> live = tasks, next;
  uint64_t spent_before = 0;
  while (!live.empty()) {
    const uint32_t n = (uint32_t)live.size();
    HIP_TRY(hipMemcpyAsync(s->tasks_dev, live.data(), n * sizeof(c4s::Task), hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemsetAsync(s->counter_dev, 0, sizeof(uint32_t), stream));
    const uint32_t blocks = std::min<uint32_t>((n + kLanes - 1) / kLanes, kMaxBlocks);
    solver_kernel<<<dim3(blocks), dim3(kLanes), 0, stream>>>(s->tasks_dev, n, s->counter_dev, s->stacks_dev, n_slots, s->tt, s->log2_entries, (int64_t)nodes_per_launch,
                                                             max_nodes_per_position);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(live.data(), s->tasks_dev, n * sizeof(c4s::Task), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    ++st.launches;
    uint64_t spent = 0, finished = 0;
    for (const c4s::Task& t : live) { spent += t.nodes; finished += t.status; }
    if (spent == spent_before && finished == 0)      // every launch spends budget or finishes a task: anything else must not loop
      return c4host::fail(C4_ERR_HIP, "c4_solver_solve: a launch made no progress");
    next.clear();
    for (const c4s::Task& t : live) {
      if (t.status == 1) {
        scores_out[t.owner] = (int16_t)(-(int)t.value);
        st.nodes += t.nodes; st.probes += t.probes;
      } else if (t.nodes >= max_nodes_per_position) {
        ++st.unsolved_tasks;
        solved_out[t.owner / 7] = 0;
        st.nodes += t.nodes; st.probes += t.probes;
      } else {
        next.push_back(t);
      }
    }
    live.swap(next);
    spent_before = 0;
    for (const c4s::Task& t : live) spent_before += t.nodes;
  }
  for (uint64_t p = 0; p < n_positions; ++p)
    if (!solved_out[p])
      for (int c = 0; c < 7; ++c) scores_out[7 * p + c] = C4_SOLVE_UNSOLVED;
  if (stats_out) *stats_out = st;
  return C4_OK;
}

}  // extern "C"
