// c4_train_adam.hip -- the optimiser of a training step as one launch: Adam with coupled L2 over every parameter of a network
// (c4a0_amd/train_graph.py HipAdam; the numerics contract is include/c4a0_hip.h's "training: the optimiser").
//
//   train_adam        one workgroup of 256 threads owns kAdamBlock = 4 096 consecutive elements of ONE segment {p, g, m, v, n}: the
//                     grouped pattern of c4_grouped.hpp -- the table carries every segment's first workgroup (a prefix sum the caller
//                     made once), a workgroup finds its segment by a binary search over it (uniform: scalar loads), then walks its
//                     elements in 4 rounds of 256 x 16 bytes.  A thread moves one aligned group of 4 floats per round: 16-byte loads
//                     of p, g, m, v, 16-byte stores of p, m, v -- 28 bytes a parameter, one pass, nothing else.  The last group of a
//                     segment whose n is no multiple of 4 is walked element by element by the one thread that owns it.
//   train_adam_bump   one thread: step[0] += 1, in stream order behind train_adam, which read step[0] as t.
//
// The step count lives on the device so that a replayed graph advances it; thread 0 of every workgroup turns it into the two f32
// scalars of the step in float64 (beta^t by square-and-multiply: a fixed sequence of f64 products, no library call) and hands them
// to the others through LDS.  Elements are independent: no atomics, two calls give the same bytes, a non-finite g stays in its element.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/c4a0_hip.h"
#include "c4_host.hpp"

namespace {

constexpr int kThreads = 256, kRounds = 4;
constexpr uint32_t kAdamBlock = C4_ADAM_BLOCK_ELEMS;
static_assert(kAdamBlock == kThreads * 4 * kRounds, "a workgroup walks C4_ADAM_BLOCK_ELEMS elements");
static_assert(sizeof(c4_adam_segment) == 48, "c4_adam_segment is 48 bytes");

struct AdamScalars {
  float step_size, sqrt_bc2;   // lr / (1 - beta1^t) and sqrt(1 - beta2^t), each evaluated in f64 and rounded once
  float eps, wd, w1, b2, w2;   // eps, weight_decay, 1 - beta1, beta2, 1 - beta2 (the differences taken in f64), rounded once
};

// the table's pointers are device memory: say so, and the accesses are global_load / global_store, not flat ones
typedef float __attribute__((ext_vector_type(4))) vfloat4;
typedef __attribute__((address_space(1))) vfloat4 gfloat4;
typedef __attribute__((address_space(1))) float gfloat;
__device__ __forceinline__ vfloat4 load4(const float* p) { return *(const gfloat4*)p; }
__device__ __forceinline__ void store4(float* p, const vfloat4 x) { *(gfloat4*)p = x; }
__device__ __forceinline__ float load1(const float* p) { return *(const gfloat*)p; }
__device__ __forceinline__ void store1(float* p, float x) { *(gfloat*)p = x; }

// b^e for an integer e: square-and-multiply from the lowest bit, r and b in f64
__device__ __forceinline__ double pow_u32(double b, uint32_t e) {
  double r = 1.0;
  while (e) {
    if (e & 1u) r *= b;
    b *= b;
    e >>= 1;
  }
  return r;
}

// the element's update: the operations and their order are the header's
__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const AdamScalars& a) {
  const float g2 = a.wd != 0.0f ? __builtin_fmaf(a.wd, p, g) : g;
  const float m2 = __builtin_fmaf(a.w1, g2 - m, m);
  const float v2 = __builtin_fmaf(a.w2 * g2, g2, a.b2 * v);
  const float denom = sqrtf(v2) / a.sqrt_bc2 + a.eps;
  p = __builtin_fmaf(-a.step_size, m2 / denom, p);
  m = m2;
  v = v2;
}

__global__ __launch_bounds__(kThreads) void train_adam(const c4_adam_segment* __restrict__ table, uint32_t n_segs,
                                                       const uint32_t* __restrict__ step, double lr, double beta1, double beta2, float eps,
                                                       float wd, float w1, float b2, float w2) {
  __shared__ float s_scal[2];
  if (threadIdx.x == 0) {
    const uint32_t t = step[0] + 1u;
    const double bc1 = 1.0 - pow_u32(beta1, t), bc2 = 1.0 - pow_u32(beta2, t);
    s_scal[0] = (float)(lr / bc1);
    s_scal[1] = (float)__builtin_sqrt(bc2);
  }
  // the segment whose workgroups hold blockIdx.x: the last one with first_block <= blockIdx.x
  uint32_t lo = 0, hi = n_segs;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (table[mid].first_block <= blockIdx.x) lo = mid; else hi = mid;
  }
  const c4_adam_segment seg = table[lo];
  __syncthreads();
  const AdamScalars a{s_scal[0], s_scal[1], eps, wd, w1, b2, w2};
  if (blockIdx.x < seg.first_block) return;   // a table whose first segment does not begin at workgroup 0: nothing is this workgroup's
  const uint64_t base = (uint64_t)(blockIdx.x - seg.first_block) * kAdamBlock;
#pragma unroll
  for (int r = 0; r < kRounds; r++) {
    const uint64_t i = base + (uint64_t)(r * kThreads + threadIdx.x) * 4;
    if (i + 4 <= seg.n) {
      vfloat4 p = load4(seg.p + i);
      const vfloat4 g = load4(seg.g + i);
      vfloat4 m = load4(seg.m + i), v = load4(seg.v + i);
#pragma unroll
      for (int e = 0; e < 4; e++) {
        float pe = p[e], me = m[e], ve = v[e];
        adam1(pe, g[e], me, ve, a);
        p[e] = pe;
        m[e] = me;
        v[e] = ve;
      }
      store4(seg.p + i, p);
      store4(seg.m + i, m);
      store4(seg.v + i, v);
    } else {
      for (uint64_t j = i; j < seg.n; j++) {   // at most 3 elements: the segment's tail
        float p = load1(seg.p + j), m = load1(seg.m + j), v = load1(seg.v + j);
        adam1(p, load1(seg.g + j), m, v, a);
        store1(seg.p + j, p);
        store1(seg.m + j, m);
        store1(seg.v + j, v);
      }
    }
  }
}

__global__ void train_adam_bump(uint32_t* step) { step[0] = step[0] + 1u; }

}  // namespace

extern "C" int c4_train_adam_f32(const c4_adam_segment* table_dev, uint32_t n_segs, uint32_t n_blocks, uint32_t* step_dev, double lr, double beta1,
                                 double beta2, double eps, double weight_decay, void* stream) {
  const char* me = "c4_train_adam_f32";
  if (!table_dev || !step_dev) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": null argument (table, step)");
  if (n_segs == 0 || n_blocks == 0) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": n_segs >= 1 and n_blocks >= 1");
  if (n_blocks < n_segs) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": n_blocks < n_segs (every segment has at least one workgroup)");
  if (((uintptr_t)table_dev & 15) != 0) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": the table must be 16-byte aligned");
  if (((uintptr_t)step_dev & 3) != 0) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": the step counter must be 4-byte aligned");
  C4_ON_STREAM_DEVICE(stream);
  train_adam<<<dim3(n_blocks), dim3(kThreads), 0, (hipStream_t)stream>>>(table_dev, n_segs, step_dev, lr, beta1, beta2, (float)eps,
                                                                        (float)weight_decay, (float)(1.0 - beta1), (float)beta2,
                                                                        (float)(1.0 - beta2));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return c4host::fail(C4_ERR_HIP, std::string(me) + " launch: " + hipGetErrorString(e));
  train_adam_bump<<<dim3(1), dim3(1), 0, (hipStream_t)stream>>>(step_dev);
  e = hipGetLastError();
  if (e != hipSuccess) return c4host::fail(C4_ERR_HIP, std::string(me) + " counter launch: " + hipGetErrorString(e));
  return C4_OK;
}

extern "C" int c4_train_adam_block_elems(void) { return (int)kAdamBlock; }
