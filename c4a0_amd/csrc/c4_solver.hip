// c4_solver.hip -- the exact solver (include/c4a0_hip.h, "exact solver"): c4_solver_create[_ex] / c4_solver_solve[_ex] /
// c4_solver_book_export / c4_solver_book_import / c4_solver_destroy.
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
//
// The host loop is c4_solver_split.hpp's scheduler (c4_solver_solve_ex), which is handed run_launch() below: with split_stones set,
// a task that reaches max_nodes_per_position is replaced by its children instead of being given up, so that one hard position
// becomes thousands of tasks that fill the chip, and their exact scores are combined by minimax; the task array and the stack
// store grow between launches, the saved stacks kept.  A solver created with a book (c4_solver_create_ex) keeps every exact score
// of a position with few enough stones in a lossless table: the host inserts between launches and sends the new words to the
// device's copy (book_update_kernel), solver_kernel<true> only reads it -- a node found there is a leaf.  Limits: every level of splitting first spends a whole
// max_nodes_per_position on the task it then drops, split nodes are searched with a full window, and split_max_tasks bounds the
// tasks (device memory); without a book, or with one that holds nothing yet, the launch is solver_kernel<false>, the kernel and
// arguments of a solver that knows neither.
#include "c4_host.hpp"
#include "c4_solver_core.hpp"
#include "c4_solver_split.hpp"

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace {

constexpr int kLanes = 64;                       // one wavefront per workgroup: 40 frames x 2 words x 64 lanes = 20 KB of LDS
constexpr uint32_t kMaxBlocks = 256 * 8;         // 8 such workgroups fit the LDS of each of the 256 CUs

// BOOK: three more arguments -- the book's device copy, log2 of its entries and the largest stone count it holds -- go on to the
// Lane::step that probes it; without them the kernel and its arguments are those of a solver that has no book.
template <bool BOOK, typename... BookArgs>
__global__ __launch_bounds__(kLanes) void solver_kernel(c4s::Task* __restrict__ tasks, uint32_t n_tasks, uint32_t* __restrict__ next_task,
                                                        uint32_t* __restrict__ stack_store, uint32_t n_slots, uint64_t* __restrict__ tt,
                                                        uint32_t log2_entries, int64_t nodes_per_launch, uint64_t max_nodes_per_task,
                                                        BookArgs... book) {
  static_assert(sizeof...(BookArgs) == (BOOK ? 3 : 0), "solver_kernel<true> takes (const uint64_t* book, uint32_t log2_book, int book_stones)");
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
    const c4s::StepResult r = lane.step(stk, kLanes, tt, log2_entries, budget, book...);
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

// The book's device copy follows the host's: pairs[2 i] = the index of a word the host wrote, pairs[2 i + 1] = the word.
__global__ void book_update_kernel(uint64_t* __restrict__ book, uint64_t book_entries, const uint64_t* __restrict__ pairs, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && pairs[2 * i] < book_entries) book[pairs[2 * i]] = pairs[2 * i + 1];
}

struct Solver {
  int device = 0;
  uint64_t* tt = nullptr;
  uint32_t log2_entries = 0;
  c4s::Task* tasks_dev = nullptr;
  uint32_t* stacks_dev = nullptr;      // kStackWords words per slot: where an unfinished search waits for its next launch
  uint32_t* counter_dev = nullptr;
  uint64_t* book_dev = nullptr;        // the device's copy of book.words: before a launch it gets the words the host wrote since the last
  uint64_t* pairs_dev = nullptr;       // ... as (index, word) pairs, staged here
  std::vector<uint64_t> pairs;
  size_t tasks_cap = 0, slots_cap = 0, pairs_cap = 0;
  c4split::Book book;
  std::mutex mu;
};

void free_solver(Solver* s) {
  (void)hipFree(s->tt);
  (void)hipFree(s->tasks_dev);
  (void)hipFree(s->stacks_dev);
  (void)hipFree(s->counter_dev);
  (void)hipFree(s->book_dev);
  (void)hipFree(s->pairs_dev);
  delete s;
}

// One launch over tasks[0 .. n): upload, solver_kernel, download.  The task array grows to n, the stack store to n_slots slots
// with what it holds kept: saved searches wait there between launches.
int run_launch(Solver* s, c4s::Task* tasks, uint32_t n, uint32_t n_slots, const c4split::Options& opt, hipStream_t stream) {
  if (n > s->tasks_cap) {
    const size_t cap = std::max<size_t>(n, 2 * s->tasks_cap);
    (void)hipFree(s->tasks_dev);
    s->tasks_dev = nullptr;
    s->tasks_cap = 0;
    HIP_TRY(hipMalloc(&s->tasks_dev, cap * sizeof(c4s::Task)));
    s->tasks_cap = cap;
  }
  if (n_slots > s->slots_cap) {
    const size_t cap = std::max<size_t>(n_slots, 2 * s->slots_cap), words = c4s::kStackWords;
    uint32_t* grown = nullptr;
    HIP_TRY(hipMalloc(&grown, cap * words * sizeof(uint32_t)));
    hipError_t e = hipSuccess;
    if (s->slots_cap) e = hipMemcpyAsync(grown, s->stacks_dev, s->slots_cap * words * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
      (void)hipFree(grown);
      HIP_TRY(e);
    }
    (void)hipFree(s->stacks_dev);
    s->stacks_dev = grown;
    s->slots_cap = cap;
  }
  if (!s->book.changed.empty()) {        // only what changed travels: 16 bytes an insert, not the whole table
    const size_t k = s->book.changed.size();
    if (k > s->pairs_cap) {
      const size_t cap = std::max<size_t>(k, 2 * s->pairs_cap);
      (void)hipFree(s->pairs_dev);
      s->pairs_dev = nullptr;
      s->pairs_cap = 0;
      HIP_TRY(hipMalloc(&s->pairs_dev, cap * 2 * sizeof(uint64_t)));
      s->pairs_cap = cap;
    }
    s->pairs.resize(2 * k);
    for (size_t i = 0; i < k; ++i) {
      s->pairs[2 * i] = s->book.changed[i];
      s->pairs[2 * i + 1] = s->book.words[s->book.changed[i]];
    }
    HIP_TRY(hipMemcpyAsync(s->pairs_dev, s->pairs.data(), 2 * k * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    book_update_kernel<<<dim3((uint32_t)((k + 255) / 256)), dim3(256), 0, stream>>>(s->book_dev, s->book.words.size(), s->pairs_dev, (uint32_t)k);
    HIP_TRY(hipGetLastError());
    s->book.changed.clear();
  }
  HIP_TRY(hipMemcpyAsync(s->tasks_dev, tasks, n * sizeof(c4s::Task), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemsetAsync(s->counter_dev, 0, sizeof(uint32_t), stream));
  const uint32_t blocks = std::min<uint32_t>((n + kLanes - 1) / kLanes, kMaxBlocks);
  if (s->book.top_stones >= 0)
    solver_kernel<true, const uint64_t*, uint32_t, int><<<dim3(blocks), dim3(kLanes), 0, stream>>>(
        s->tasks_dev, n, s->counter_dev, s->stacks_dev, (uint32_t)s->slots_cap, s->tt, s->log2_entries, (int64_t)opt.nodes_per_launch,
        opt.max_nodes_per_position, s->book_dev, s->book.log2_entries, s->book.top_stones);
  else
    solver_kernel<false><<<dim3(blocks), dim3(kLanes), 0, stream>>>(s->tasks_dev, n, s->counter_dev, s->stacks_dev, (uint32_t)s->slots_cap, s->tt,
                                                                    s->log2_entries, (int64_t)opt.nodes_per_launch, opt.max_nodes_per_position);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(tasks, s->tasks_dev, n * sizeof(c4s::Task), hipMemcpyDeviceToHost, stream));
  HIP_TRY(hipStreamSynchronize(stream));
  return C4_OK;
}

static_assert(sizeof(c4_solver_stats_ex) == sizeof(c4split::Stats), "c4_solver_stats_ex and c4split::Stats are one layout");

}  // namespace

extern "C" {

int c4_solver_create_ex(uint64_t tt_entries, uint64_t book_entries, uint32_t book_max_stones, int32_t device, c4_solver** out) {
  if (!out) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_create: out is NULL");
  *out = nullptr;
  if (tt_entries < 16 || tt_entries > (1ull << 32) || (tt_entries & (tt_entries - 1)))
    return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_create: tt_entries must be a power of two between 16 and 2^32");
  if (book_entries != 0 && (book_entries < 16 || book_entries > (1ull << 28) || (book_entries & (book_entries - 1))))
    return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_create: book_entries must be 0 or a power of two between 16 and 2^28");
  if (book_max_stones == 0) book_max_stones = C4_SOLVER_BOOK_MAX_STONES;
  if (book_max_stones > 41) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_create: book_max_stones above 41");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return c4host::fail(C4_ERR_NO_DEVICE, "c4_solver_create: no HIP device");
  if (device < 0 || device >= n_dev) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_create: no such device");
  C4_ON_DEVICE(device);
  Solver* s = new Solver;
  s->device = device;
  while ((1ull << s->log2_entries) < tt_entries) ++s->log2_entries;
  s->book.create(book_entries, (int)book_max_stones);
  hipError_t e = hipMalloc(&s->tt, tt_entries * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMemset(s->tt, 0, tt_entries * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMalloc(&s->counter_dev, sizeof(uint32_t));
  if (e == hipSuccess && book_entries) e = hipMalloc(&s->book_dev, book_entries * sizeof(uint64_t));
  if (e == hipSuccess && book_entries) e = hipMemset(s->book_dev, 0, book_entries * sizeof(uint64_t));
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    free_solver(s);
    return c4host::fail(C4_ERR_HIP, std::string("c4_solver_create: ") + hipGetErrorString(e));
  }
  *out = reinterpret_cast<c4_solver*>(s);
  return C4_OK;
}

int c4_solver_create(uint64_t tt_entries, int32_t device, c4_solver** out) { return c4_solver_create_ex(tt_entries, 0, 0, device, out); }

int c4_solver_destroy(c4_solver* handle) {
  if (!handle) return C4_OK;
  Solver* s = reinterpret_cast<Solver*>(handle);
  C4_ON_DEVICE(s->device);
  free_solver(s);
  return C4_OK;
}

int c4_solver_solve_ex(c4_solver* handle, const uint64_t* positions_host, uint64_t n_positions, const c4_solver_options* options,
                       int16_t* scores_out, uint8_t* solved_out, c4_solver_stats_ex* stats_out, void* stream_) {
  if (!handle) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_solve: handle is NULL");
  if (stats_out) *stats_out = c4_solver_stats_ex{};
  if (options && options->struct_size != sizeof(c4_solver_options))
    return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_solve: options->struct_size is not sizeof(c4_solver_options)");
  if (n_positions == 0) return C4_OK;
  if (!positions_host || !scores_out || !solved_out) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_solve: NULL array");
  if (n_positions > (1ull << 28)) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_solve: more than 2^28 positions in one call");
  c4split::Options opt{};
  if (options) opt = {options->nodes_per_launch, options->max_nodes_per_position, options->split_stones, options->split_max_tasks};
  if (opt.nodes_per_launch == 0) opt.nodes_per_launch = C4_SOLVER_NODES_PER_LAUNCH;
  if (opt.max_nodes_per_position == 0) opt.max_nodes_per_position = C4_SOLVER_MAX_NODES_PER_POSITION;
  if (opt.split_max_tasks == 0) opt.split_max_tasks = C4_SOLVER_SPLIT_MAX_TASKS;
  if (opt.nodes_per_launch > (1ull << 40)) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_solve: nodes_per_launch above 2^40");
  if (opt.split_stones > 42) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_solve: split_stones above 42");
  if (opt.split_max_tasks > (1ull << 24)) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_solve: split_max_tasks above 2^24");
  Solver* s = reinterpret_cast<Solver*>(handle);
  hipStream_t stream = (hipStream_t)stream_;
  std::lock_guard<std::mutex> lock(s->mu);
  C4_ON_DEVICE(s->device);

  c4split::Stats st{};
  std::string err;
  const c4split::Status r = c4split::solve(positions_host, n_positions, opt, s->book, scores_out, solved_out, st, err,
                                           [&](c4s::Task* tasks, uint32_t n, uint32_t n_slots) { return run_launch(s, tasks, n, n_slots, opt, stream); });
  if (r == c4split::kBadArg) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_solve: " + err);
  if (r == c4split::kRunFailed) return C4_ERR_HIP;      // run_launch has said what failed
  if (r != c4split::kOk) return c4host::fail(C4_ERR_HIP, "c4_solver_solve: " + err);
  if (stats_out) memcpy(stats_out, &st, sizeof(st));
  return C4_OK;
}

int c4_solver_solve(c4_solver* handle, const uint64_t* positions_host, uint64_t n_positions, uint64_t nodes_per_launch,
                    uint64_t max_nodes_per_position, int16_t* scores_out, uint8_t* solved_out, c4_solver_stats* stats_out, void* stream) {
  c4_solver_options opt{};
  opt.struct_size = sizeof(opt);
  opt.nodes_per_launch = nodes_per_launch;
  opt.max_nodes_per_position = max_nodes_per_position;
  c4_solver_stats_ex st{};
  const int r = c4_solver_solve_ex(handle, positions_host, n_positions, &opt, scores_out, solved_out, &st, stream);
  if (stats_out) memcpy(stats_out, &st, sizeof(*stats_out));      // the five fields the two have in common come first
  return r;
}

int c4_solver_book_export(c4_solver* handle, uint64_t* out, uint64_t cap, uint64_t* n_out) {
  if (!handle || !n_out || (cap && !out)) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_book_export: NULL argument");
  Solver* s = reinterpret_cast<Solver*>(handle);
  std::lock_guard<std::mutex> lock(s->mu);
  *n_out = s->book.export_to(out, cap);
  return C4_OK;
}

int c4_solver_book_import(c4_solver* handle, const uint64_t* entries, uint64_t n) {
  if (!handle || (n && !entries)) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_book_import: NULL argument");
  Solver* s = reinterpret_cast<Solver*>(handle);
  std::lock_guard<std::mutex> lock(s->mu);
  if (n == 0) return C4_OK;
  if (!s->book.enabled()) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_book_import: this solver was created without a book");
  std::string err;
  if (s->book.import(entries, n, err) != c4split::kOk) return c4host::fail(C4_ERR_BAD_ARG, "c4_solver_book_import: " + err);
  return C4_OK;
}

}  // extern "C"
