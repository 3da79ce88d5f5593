// c4_session_route.hip -- the device-side router of multi-model sessions (c4_session_route_leaves): the resident games' leaves as
// ONE fixed-shape batch whose rows are grouped by the model that must answer them, for the grouped bf16 chain
// (c4_conv_tower_bf16_grouped, c4_linear_bf16_grouped, c4_head_out_bf16_grouped).  Where api._MultiModelEvaluator sorts the slots
// with torch.argsort and reads the groups' sizes on the host, here no count ever leaves the device: the segment bounds stay in
// device memory, the launches that follow cover `rows_cap` rows whatever the counts are, and the whole round can be captured.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "../../include/c4a0_hip.h"
#include "c4_device.hpp"
#include "c4_host.hpp"
#include "c4_session_impl.hpp"
#include "c4_tree.hpp"

namespace {

using c4host::fail;

constexpr uint32_t kNoRow = 0xFFFFFFFFu;
constexpr uint32_t kPlaneChunks = C4_PLANES_LEN * 2 / 8;   // a slot's bf16 planes as 8-byte pieces (rows are 168 bytes apart)
static_assert(C4_PLANES_LEN * 2 % 8 == 0, "plane rows are moved 8 bytes at a time");

// Group of slot g: the index of its model id in the table; kNoRow for an idle slot (decided from the slot, as leaf_key_of does:
// id 0 may be a real player) and for an id the table does not hold (counted).
C4_DEV uint32_t route_group(const Slot* slots, const uint64_t* leaf_models, const uint64_t* ids, uint32_t n_models, uint32_t g, bool* unrouted) {
  *unrouted = false;
  if (slot_status(slots[g].state) != kActive) return kNoRow;
  const uint64_t id = leaf_models[g];
  for (uint32_t m = 0; m < n_models; m++)
    if (ids[m] == id) return m;
  *unrouted = true;
  return kNoRow;
}

// One workgroup (as k_unique_rank and k_sample_offsets): ranks every routed slot among the slots of its model IN SLOT ORDER, so the
// batch is a function of the games alone; then the segment bounds, every slot's row, and zeros into the pad rows of every segment.
__global__ __launch_bounds__(1024) void k_route_rank(const Slot* __restrict__ slots, const uint64_t* __restrict__ leaf_models, uint32_t n_slots,
                                                     const uint64_t* __restrict__ model_ids, uint32_t n_models, uint32_t align, uint32_t rows_cap,
                                                     uint32_t* __restrict__ inverse, uint32_t* __restrict__ seg_start, uint32_t* __restrict__ n_unrouted,
                                                     uint2* __restrict__ planes_out) {
  __shared__ uint64_t ids[C4_ROUTE_MAX_MODELS];
  __shared__ uint32_t wave_cnt[16][C4_ROUTE_MAX_MODELS];
  __shared__ uint32_t carry[C4_ROUTE_MAX_MODELS];      // slots of model m seen so far; after the loop: its count
  __shared__ uint32_t start[C4_ROUTE_MAX_MODELS + 1];
  __shared__ uint32_t lost;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < n_models) { ids[tid] = model_ids[tid]; carry[tid] = 0; }
  if (tid == 0) lost = 0;
  __syncthreads();
  for (uint32_t base = 0; base < n_slots; base += 1024) {
    const uint32_t g = base + tid;
    bool unrouted = false;
    const uint32_t mine = g < n_slots ? route_group(slots, leaf_models, ids, n_models, g, &unrouted) : kNoRow;
    uint32_t within = 0;
    for (uint32_t m = 0; m < n_models; m++) {
      const unsigned long long b = __ballot(mine == m);
      if (lane == 0) wave_cnt[wave][m] = (uint32_t)__popcll(b);
      if (mine == m) within = (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    }
    const unsigned long long bl = __ballot(unrouted);
    if (lane == 0 && bl) atomicAdd(&lost, (uint32_t)__popcll(bl));
    __syncthreads();
    if (g < n_slots) {
      uint32_t rank = kNoRow;
      if (mine != kNoRow) {
        rank = carry[mine] + within;
        for (uint32_t w = 0; w < wave; w++) rank += wave_cnt[w][mine];
      }
      inverse[g] = rank;                                 // (the second pass below reads it back in the same thread)
    }
    __syncthreads();
    if (tid < n_models) {
      uint32_t c = carry[tid];
      for (uint32_t w = 0; w < 16; w++) c += wave_cnt[w][tid];
      carry[tid] = c;
    }
    __syncthreads();
  }
  if (tid == 0) {
    uint32_t at = 0;
    for (uint32_t m = 0; m < n_models; m++) {
      start[m] = at;
      seg_start[m] = at;
      at += (carry[m] + align - 1) / align * align;
    }
    start[n_models] = at;
    seg_start[n_models] = at;
    *n_unrouted = lost;
  }
  __syncthreads();
  for (uint32_t base = 0; base < n_slots; base += 1024) {
    const uint32_t g = base + tid;
    if (g >= n_slots) break;
    const uint32_t rank = inverse[g];
    if (rank == kNoRow) continue;
    bool unrouted;
    const uint32_t m = route_group(slots, leaf_models, ids, n_models, g, &unrouted);   // (as in the first pass: nothing has changed)
    const uint32_t row = start[m] + rank;
    inverse[g] = row < rows_cap ? row : kNoRow;          // (the host's bound on rows_cap makes this always true)
  }
  // pad rows -- between a segment's last row and the next segment -- become empty boards
  for (uint32_t m = 0; m < n_models; m++) {
    const uint32_t lo = start[m] + carry[m], hi = start[m + 1] < rows_cap ? start[m + 1] : rows_cap;
    for (uint32_t i = lo * kPlaneChunks + tid; i < hi * kPlaneChunks && lo < hi; i += 1024) planes_out[i] = make_uint2(0u, 0u);
  }
}

// every routed slot's 84 bf16 plane values to its row of the batch
__global__ __launch_bounds__(256) void k_route_planes(const uint2* __restrict__ planes, const uint32_t* __restrict__ inverse, uint32_t n_slots,
                                                      uint32_t rows_cap, uint2* __restrict__ planes_out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const uint32_t g = i / kPlaneChunks, c = i - g * kPlaneChunks;
  if (g >= n_slots) return;
  const uint32_t row = inverse[g];
  if (row >= rows_cap) return;                           // idle, or its model is not in the table
  planes_out[(size_t)row * kPlaneChunks + c] = planes[(size_t)g * kPlaneChunks + c];
}

}  // namespace

extern "C" int c4_session_route_leaves(c4_session* s, const uint64_t* model_ids_dev, uint32_t n_models, uint32_t align, void* planes_out_dev,
                                       uint32_t rows_cap, uint32_t* inverse_dev, uint32_t* seg_start_dev, uint32_t* n_unrouted_dev) {
  if (!s || !model_ids_dev || !planes_out_dev || !inverse_dev || !seg_start_dev || !n_unrouted_dev) return fail(C4_ERR_BAD_ARG, "c4_session_route_leaves: null argument");
  if (int rc = refuse_search_hold(s, "c4_session_route_leaves", "has ONE evaluator: nothing to route")) return rc;
  if (!s->bound || !s->have_games) return fail(C4_ERR_NOT_BOUND, "c4_session_route_leaves: bind_io and set_games first");
  if (!s->p.leaf_models) return fail(C4_ERR_BAD_ARG, "c4_session_route_leaves: no leaf models bound (c4_session_bind_leaf_models first)");
  if (s->cfg.planes_dtype != 1) return fail(C4_ERR_BAD_ARG, "c4_session_route_leaves: the session's planes must be bf16 (planes_dtype 1)");
  if (align < 16 || align > 256 || (align & (align - 1))) return fail(C4_ERR_BAD_ARG, "c4_session_route_leaves: align must be a power of two in 16..256");
  if (n_models == 0 || n_models > C4_ROUTE_MAX_MODELS)
    return fail(C4_ERR_BAD_ARG, "c4_session_route_leaves: n_models must be between 1 and " + std::to_string(C4_ROUTE_MAX_MODELS) + " (C4_ROUTE_MAX_MODELS)");
  const uint32_t n = s->cfg.n_slots;
  const uint64_t need = ((uint64_t)n + (uint64_t)n_models * (align - 1) + align - 1) / align * align;
  if (rows_cap < need)
    return fail(C4_ERR_BAD_ARG, "c4_session_route_leaves: rows_cap " + std::to_string(rows_cap) + " is below round_up(n_slots + n_models * (align - 1), align) = " +
                                    std::to_string(need));
  if (((uintptr_t)planes_out_dev | (uintptr_t)s->p.planes) & 7) return fail(C4_ERR_BAD_ARG, "c4_session_route_leaves: plane rows must be 8-byte aligned");
  C4_ON_DEVICE(s->cfg.device);
  hipLaunchKernelGGL(k_route_rank, dim3(1), dim3(1024), 0, s->stream, s->p.slots, s->p.leaf_models, n, model_ids_dev, n_models, align, rows_cap, inverse_dev,
                     seg_start_dev, n_unrouted_dev, (uint2*)planes_out_dev);
  hipLaunchKernelGGL(k_route_planes, c4host::grid_for((uint64_t)n * kPlaneChunks), dim3(256), 0, s->stream, (const uint2*)s->p.planes, inverse_dev, n, rows_cap,
                     (uint2*)planes_out_dev);
  HIP_TRY(hipGetLastError());
  return C4_OK;
}
