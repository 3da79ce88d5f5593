// c4_builtin_players.hip -- the tournament's two weightless players on the device (c4_builtin.hpp: uniform and random, pure
// functions of kind, seed, model id and position): c4_builtin_eval answers a plain batch, c4_builtin_eval_grouped the built-in
// players' segments of a routed batch (c4_session_route_leaves) beside the grouped network chain, c4_builtin_eval_host is the
// same header code in a loop on the CPU.
//
// One lane per row.  A row is 21 (bf16) or 42 (f32) 8-byte words that the lane loads as such and folds into the position's two
// bitboards; the answer is four rounds of a 64-bit mixer and eight draws -- a few hundred integer operations per row, nine f32
// stores.  Nothing here is worth tuning: at 4 096 rows the launch is bounded by its own latency.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>

#include "../../include/c4a0_hip.h"
#include "c4_builtin.hpp"
#include "c4_grouped.hpp"
#include "c4_host.hpp"

static_assert(c4b::kUniform == C4_BUILTIN_UNIFORM && c4b::kRandom == C4_BUILTIN_RANDOM, "c4_builtin.hpp and c4a0_hip.h name the same kinds");
static_assert(C4_PLANES_LEN == 84 && c4b::kBf16Words * 4 == C4_PLANES_LEN && c4b::kF32Words * 2 == C4_PLANES_LEN, "a row is 84 plane values");

namespace {

using c4host::fail;

constexpr int kRowsPerGroup = 64;   // rows (= lanes) per workgroup of both kernels: one wavefront
static_assert(C4_GROUPED_ROW_ALIGN % kRowsPerGroup == 0, "a workgroup of the grouped kernel never straddles two segments");

// the position of row `row`: T = uint16_t (bf16 planes) or float
template <typename T>
__device__ __forceinline__ c4b::Cells load_cells(const uint2* __restrict__ planes, uint32_t row) {
  constexpr uint32_t kWords = sizeof(T) == 2 ? c4b::kBf16Words : c4b::kF32Words;
  const uint2* p = planes + (size_t)row * kWords;
  c4b::Cells cells;
#pragma unroll
  for (uint32_t w = 0; w < kWords; w++) {
    const uint2 v = p[w];
    const uint64_t word = (uint64_t)v.x | ((uint64_t)v.y << 32);
    if (sizeof(T) == 2) cells.add_bf16x4(w, word); else cells.add_f32x2(w, word);
  }
  return cells;
}

template <typename T>
__global__ __launch_bounds__(kRowsPerGroup) void k_builtin_eval(const uint2* __restrict__ planes, uint32_t rows, uint32_t kind, uint64_t seed,
                                                                uint64_t model_id, float* __restrict__ logits, float* __restrict__ q) {
  const uint32_t row = blockIdx.x * kRowsPerGroup + threadIdx.x;
  if (row >= rows) return;
  const c4b::Cells cells = load_cells<T>(planes, row);
  float out[9];
  c4b::answer(kind, seed, model_id, cells.mask(), cells.value(), out);
#pragma unroll
  for (int j = 0; j < 7; j++) logits[(size_t)row * 7 + j] = out[j];
  q[(size_t)row * 2] = out[7];
  q[(size_t)row * 2 + 1] = out[8];
}

// the segments' players, by value in the kernel's arguments: a captured launch owns them
struct Players {
  uint64_t seed[C4_ROUTE_MAX_MODELS];
  uint64_t model_id[C4_ROUTE_MAX_MODELS];
  uint8_t kind[C4_ROUTE_MAX_MODELS];
};

__global__ __launch_bounds__(kRowsPerGroup) void k_builtin_eval_grouped(const uint2* __restrict__ planes, const uint32_t* __restrict__ seg_start,
                                                                        uint32_t n_segments, float* __restrict__ answers, Players players) {
  const int m = c4grp::Segments{seg_start, n_segments}.model_of(blockIdx.x * kRowsPerGroup);   // (below n_segments, whatever the array holds)
  if (m < 0) return;
  const uint32_t row = blockIdx.x * kRowsPerGroup + threadIdx.x;                                // (< rows_cap: the grid covers exactly rows_cap rows)
  const c4b::Cells cells = load_cells<uint16_t>(planes, row);
  float out[9];
  c4b::answer(players.kind[m], players.seed[m], players.model_id[m], cells.mask(), cells.value(), out);
#pragma unroll
  for (int j = 0; j < 9; j++) answers[(size_t)row * 9 + j] = out[j];
}

}  // namespace

extern "C" int c4_builtin_eval(const void* planes_dev, uint32_t planes_dtype, uint32_t rows, uint32_t kind, uint64_t seed, uint64_t model_id,
                               float* logits_out_dev, float* q_out_dev, void* stream) {
  if (!c4b::valid_kind(kind)) return fail(C4_ERR_BAD_ARG, "c4_builtin_eval: kind must be C4_BUILTIN_UNIFORM (0) or C4_BUILTIN_RANDOM (1), got " + std::to_string(kind));
  if (planes_dtype > 1) return fail(C4_ERR_BAD_ARG, "c4_builtin_eval: planes_dtype must be 0 (f32) or 1 (bf16), got " + std::to_string(planes_dtype));
  if (rows == 0) return C4_OK;
  if (!planes_dev || !logits_out_dev || !q_out_dev) return fail(C4_ERR_BAD_ARG, "c4_builtin_eval: null argument");
  if ((uintptr_t)planes_dev & 7) return fail(C4_ERR_BAD_ARG, "c4_builtin_eval: plane rows must be 8-byte aligned");
  if (((uintptr_t)logits_out_dev | (uintptr_t)q_out_dev) & 3) return fail(C4_ERR_BAD_ARG, "c4_builtin_eval: the outputs must be 4-byte aligned");
  C4_ON_STREAM_DEVICE(stream);
  const dim3 grid((rows + kRowsPerGroup - 1) / kRowsPerGroup), block(kRowsPerGroup);
  c4host::with_planes(planes_dtype, [&](auto t) {
    hipLaunchKernelGGL(k_builtin_eval<decltype(t)>, grid, block, 0, (hipStream_t)stream, (const uint2*)planes_dev, rows, kind, seed, model_id, logits_out_dev,
                       q_out_dev);
  });
  HIP_TRY(hipGetLastError());
  return C4_OK;
}

extern "C" int c4_builtin_eval_grouped(const void* planes_dev, const uint32_t* seg_start_dev, uint32_t n_segments, const uint32_t* kinds,
                                       const uint64_t* seeds, const uint64_t* model_ids, uint32_t rows_cap, float* answers_dev, void* stream) {
  if (n_segments > C4_ROUTE_MAX_MODELS) return fail(C4_ERR_BAD_ARG, "c4_builtin_eval_grouped: n_segments must be at most " + std::to_string(C4_ROUTE_MAX_MODELS) + " (C4_ROUTE_MAX_MODELS)");
  if (rows_cap % C4_GROUPED_ROW_ALIGN) return fail(C4_ERR_BAD_ARG, "c4_builtin_eval_grouped: rows_cap must be a multiple of C4_GROUPED_ROW_ALIGN");
  if (n_segments == 0 || rows_cap == 0) return C4_OK;
  if (!planes_dev || !seg_start_dev || !kinds || !seeds || !model_ids || !answers_dev) return fail(C4_ERR_BAD_ARG, "c4_builtin_eval_grouped: null argument");
  if ((uintptr_t)planes_dev & 7) return fail(C4_ERR_BAD_ARG, "c4_builtin_eval_grouped: plane rows must be 8-byte aligned");
  if (((uintptr_t)answers_dev | (uintptr_t)seg_start_dev) & 3) return fail(C4_ERR_BAD_ARG, "c4_builtin_eval_grouped: answers and seg_start must be 4-byte aligned");
  Players players;
  memset(&players, 0, sizeof(players));
  for (uint32_t m = 0; m < n_segments; m++) {
    if (!c4b::valid_kind(kinds[m])) return fail(C4_ERR_BAD_ARG, "c4_builtin_eval_grouped: kinds[" + std::to_string(m) + "] must be C4_BUILTIN_UNIFORM (0) or C4_BUILTIN_RANDOM (1)");
    players.kind[m] = (uint8_t)kinds[m];
    players.seed[m] = seeds[m];
    players.model_id[m] = model_ids[m];
  }
  C4_ON_STREAM_DEVICE(stream);
  hipLaunchKernelGGL(k_builtin_eval_grouped, dim3(rows_cap / kRowsPerGroup), dim3(kRowsPerGroup), 0, (hipStream_t)stream, (const uint2*)planes_dev, seg_start_dev,
                     n_segments, answers_dev, players);
  HIP_TRY(hipGetLastError());
  return C4_OK;
}

extern "C" int c4_builtin_eval_host(const float* planes, uint64_t rows, uint32_t kind, uint64_t seed, uint64_t model_id, float* logits, float* q_penalty,
                                    float* q_no_penalty) {
  if (!c4b::valid_kind(kind)) return fail(C4_ERR_BAD_ARG, "c4_builtin_eval_host: kind must be C4_BUILTIN_UNIFORM (0) or C4_BUILTIN_RANDOM (1), got " + std::to_string(kind));
  if (rows == 0) return C4_OK;
  if (!planes || !logits || !q_penalty || !q_no_penalty) return fail(C4_ERR_BAD_ARG, "c4_builtin_eval_host: null argument");
  for (uint64_t r = 0; r < rows; r++) {
    c4b::Cells cells;
    for (uint32_t w = 0; w < c4b::kF32Words; w++) {
      uint64_t word;
      memcpy(&word, planes + r * C4_PLANES_LEN + 2 * w, 8);   // (any alignment; little endian, as the device reads it)
      cells.add_f32x2(w, word);
    }
    float out[9];
    c4b::answer(kind, seed, model_id, cells.mask(), cells.value(), out);
    memcpy(logits + r * 7, out, 7 * sizeof(float));
    q_penalty[r] = out[7];
    q_no_penalty[r] = out[8];
  }
  return C4_OK;
}
