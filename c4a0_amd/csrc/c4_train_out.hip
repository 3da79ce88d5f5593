// c4_train_out.hip -- training kernels for the heads' output layers and the loss (reference src/c4a0/nn.py:84-85, 98-99, 160-181):
// Linear(F, 7) + LogSoftmax, Linear(F, 2) + Tanh, the KL divergence and the two mean squared errors, forward and backward, in f32
// arithmetic from f32 or bf16 activations.  About 27 FMAs per activation loaded: plain fmaf on 16-byte loads, no MFMA.
//
//   out_fwd_rows      one wavefront per kFwdRows rows: the nine dot products of a row, its log-softmax, tanh, loss terms and dz
//   out_loss_reduce   one workgroup: the rows' loss terms added per chunk, the chunks in the fixed second-stage order, / m
//   out_bwd_tile      one wavefront per (chunk of rows, 64 column groups, head): reads x once, writes dx once and the chunk's dW from
//                     the same tile; db is added beside them from the dz values the tile loads anyway
//   out_chunk_reduce  the chunks' dW and db added in the fixed second-stage order, times the upstream gradient
//
// A chunk is C4_TRAIN_OUT_CHUNK_ROWS = 64 rows, the last chunk what is left: the split depends on m alone.  Every sum has one order
// that (m, k) decides and nothing is accumulated with atomics; the orders are include/c4a0_hip.h's "training: the output layers and
// the loss".  No kernel multiplies a value it read for a row past m: the forward computes such a row from row m - 1 and drops it, the
// backward's row loops end at m.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/c4a0_hip.h"
#include "c4_host.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kChunkRows = C4_TRAIN_OUT_CHUNK_ROWS;
constexpr uint32_t kReduceGroups = 8;   // chunk groups of the second stage
constexpr uint32_t kFwdRows = 2;        // rows a forward wavefront computes together (they share the weights it loads)
constexpr uint32_t kNP = 7, kNV = 2, kNO = kNP + kNV;
constexpr float kEps = 1e-8f;

// 8 consecutive elements as f32: two 16-byte loads of f32, one of bf16 (widened exactly)
__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; e++) {
    v[e] = a[e];
    v[4 + e] = b[e];
  }
}
__device__ __forceinline__ void load8(const uint16_t* p, float (&v)[8]) {
  const u32x4 a = *reinterpret_cast<const u32x4*>(p);
#pragma unroll
  for (int e = 0; e < 4; e++) {
    v[2 * e] = __uint_as_float(a[e] << 16);
    v[2 * e + 1] = __uint_as_float(a[e] & 0xFFFF0000u);
  }
}

// round to nearest, ties to even; a NaN stays a (quiet) NaN
__device__ __forceinline__ uint32_t bf16_rne(float f) {
  const uint32_t u = __float_as_uint(f);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

__device__ __forceinline__ void store_vec(float* p, const float (&v)[4]) { *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]}; }
__device__ __forceinline__ void store_vec(uint16_t* p, const float (&v)[8]) {
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; e++) o[e] = bf16_rne(v[2 * e]) | (bf16_rne(v[2 * e + 1]) << 16);
  *reinterpret_cast<u32x4*>(p) = o;
}
__device__ __forceinline__ void load_vec(const float* p, float (&v)[4]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
  for (int e = 0; e < 4; e++) v[e] = a[e];
}
__device__ __forceinline__ void load_vec(const uint16_t* p, float (&v)[8]) { load8(p, v); }
__device__ __forceinline__ void load_vec(const float* p, float (&v)[8]) { load8(p, v); }   // f32 weights beside 8 bf16 columns
__device__ __forceinline__ void store_vec(float* p, const float (&v)[8]) {
  *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
}

// every lane gets the sum of the 64 lanes' values: s += the lane 32, 16, 8, 4, 2, 1 away (a + b is b + a: all lanes hold the same bits)
__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  return s;
}

// ---------------------------------------------------------------------------------------------------------------- forward
// acc[r][j] += the lane's part of x[r] . w[j]: per group of 8 columns one fmaf chain in ascending column order
template <typename T, int NJ>
__device__ __forceinline__ void dot_part(const T* __restrict__ x, uint32_t ldx, const float* __restrict__ w, uint32_t k, uint32_t col,
                                         const uint32_t (&rows)[kFwdRows], float (&acc)[kFwdRows][kNO], int j0) {
  float xv[kFwdRows][8];
#pragma unroll
  for (uint32_t r = 0; r < kFwdRows; r++) load8(x + (size_t)rows[r] * ldx + col, xv[r]);
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    float wv[8];
    load8(w + (size_t)j * k + col, wv);
#pragma unroll
    for (uint32_t r = 0; r < kFwdRows; r++)
#pragma unroll
      for (int e = 0; e < 8; e++) acc[r][j0 + j] = fmaf(xv[r][e], wv[e], acc[r][j0 + j]);
  }
}

// terms [m][4]: a row's (kl, (q0 - tp)^2, (q1 - tn)^2, 0)
template <typename T>
__global__ __launch_bounds__(256) void out_fwd_rows(const T* __restrict__ xp, const T* __restrict__ xv, uint32_t ldxp, uint32_t ldxv,
                                                    const float* __restrict__ wp, const float* __restrict__ bp, const float* __restrict__ wv,
                                                    const float* __restrict__ bv, const float* __restrict__ pt, const float* __restrict__ tp,
                                                    const float* __restrict__ tn, uint32_t m, uint32_t k, float* __restrict__ out,
                                                    float* __restrict__ dz, float* __restrict__ terms) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t first = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * kFwdRows;
  if (first >= m) return;   // a whole wavefront past the last row (no barrier in this kernel)
  uint32_t rows[kFwdRows];
#pragma unroll
  for (uint32_t r = 0; r < kFwdRows; r++) rows[r] = (uint32_t)min(first + r, (uint64_t)m - 1);   // past m: row m - 1 again, dropped below
  float acc[kFwdRows][kNO];
#pragma unroll
  for (uint32_t r = 0; r < kFwdRows; r++)
#pragma unroll
    for (uint32_t j = 0; j < kNO; j++) acc[r][j] = 0.f;
  for (uint32_t col = 8 * lane; col < k; col += 8 * 64) {
    dot_part<T, kNP>(xp, ldxp, wp, k, col, rows, acc, 0);
    dot_part<T, kNV>(xv, ldxv, wv, k, col, rows, acc, kNP);
  }
  const float fm = (float)m;
#pragma unroll
  for (uint32_t r = 0; r < kFwdRows; r++) {
    if (first + r >= m) break;   // uniform over the wavefront
    const size_t row = rows[r];
    float z[kNO];
#pragma unroll
    for (uint32_t j = 0; j < kNO; j++) z[j] = wave_sum(acc[r][j]) + (j < kNP ? bp[j] : bv[j - kNP]);
    float mx = z[0];
#pragma unroll
    for (uint32_t j = 1; j < kNP; j++) mx = fmaxf(mx, z[j]);
    float se = 0.f;
#pragma unroll
    for (uint32_t j = 0; j < kNP; j++) se += expf(z[j] - mx);
    const float lse = logf(se);
    float o[kNO], g[kNO], t[kNP];
    float kl = 0.f, st = 0.f;
#pragma unroll
    for (uint32_t j = 0; j < kNP; j++) {
      o[j] = (z[j] - mx) - lse;
      t[j] = pt[row * kNP + j] + kEps;
      kl = fmaf(t[j], logf(t[j]) - o[j], kl);
      st = j == 0 ? t[0] : st + t[j];
    }
#pragma unroll
    for (uint32_t j = 0; j < kNP; j++) g[j] = fmaf(expf(o[j]), st, -t[j]) / fm;
    float sq[kNV];
#pragma unroll
    for (uint32_t c = 0; c < kNV; c++) {
      const float q = tanhf(z[kNP + c]);
      const float d = q - (c == 0 ? tp[row] : tn[row]);
      o[kNP + c] = q;
      sq[c] = d * d;
      g[kNP + c] = ((2.f * d) * (1.f - q * q)) / fm;
    }
    // lane j stores element j (selected by compares: the arrays stay in registers)
    float vo = 0.f, vg = 0.f;
#pragma unroll
    for (uint32_t j = 0; j < kNO; j++) {
      vo = lane == j ? o[j] : vo;
      vg = lane == j ? g[j] : vg;
    }
    if (lane < kNO) {
      out[row * kNO + lane] = vo;
      dz[row * kNO + lane] = vg;
    }
    if (lane == 0) *reinterpret_cast<f32x4*>(terms + row * 4) = f32x4{kl, sq[0], sq[1], 0.f};
  }
}

// the second stage over the chunks' partial values part[chunk * stride]: group g adds the chunks g, g + 8, .. in order starting from its
// first chunk, then the groups' sums are added in order g = 0 .. min(8, n_chunks) - 1
__device__ __forceinline__ float second_stage(const float* part, size_t stride, uint32_t n_chunks) {
  float t = 0.f;
  const uint32_t groups = min(kReduceGroups, n_chunks);
  for (uint32_t g = 0; g < groups; g++) {
    float s = part[(size_t)g * stride];
    for (uint32_t c = g + kReduceGroups; c < n_chunks; c += kReduceGroups) s += part[(size_t)c * stride];
    t = g == 0 ? s : t + s;
  }
  return t;
}

// losses[4] = (total, kl, mse_pen, mse_nopen) from terms [m][4]; part [n_chunks][4] is work space.  One workgroup.
__global__ __launch_bounds__(256) void out_loss_reduce(const float* terms, float* part, float* __restrict__ losses, uint32_t m, uint32_t n_chunks) {
  __shared__ float mean[4];
  for (uint64_t i = threadIdx.x; i < (uint64_t)n_chunks * 4; i += 256) {
    const uint32_t chunk = (uint32_t)(i >> 2), comp = (uint32_t)(i & 3);
    const size_t row0 = (size_t)chunk * kChunkRows, row1 = min((size_t)m, row0 + kChunkRows);
    float s = 0.f;
    for (size_t row = row0; row < row1; row++) s += terms[row * 4 + comp];
    part[i] = s;
  }
  __syncthreads();   // the partial sums, written to global memory by this workgroup, are visible to it
  if (threadIdx.x < 3) mean[threadIdx.x] = second_stage(part + threadIdx.x, 4, n_chunks) / (float)m;
  __syncthreads();
  if (threadIdx.x == 0) {
    losses[0] = (mean[0] + mean[1]) + mean[2];
    losses[1] = mean[0];
    losses[2] = mean[1];
    losses[3] = mean[2];
  }
}

// ---------------------------------------------------------------------------------------------------------------- backward
// One head's tile: this thread's VEC columns of the chunk's rows.  dz [m][9] (this head's columns from j0), part: the chunk's
// [9 k + 12] partial results (dWp [7][k], dWv [2][k], dbp [7], dbv [2], 3 unused).
template <typename T, int NJ>
__device__ __forceinline__ void bwd_head(const float* __restrict__ dz, float scale, const T* __restrict__ x, uint32_t ldx, const float* __restrict__ w,
                                         uint32_t m, uint32_t k, T* __restrict__ dx, uint32_t lddx, float* __restrict__ part, uint32_t j0) {
  constexpr int VEC = 16 / sizeof(T);
  const uint32_t chunk = blockIdx.x, lane = threadIdx.x;
  const size_t row0 = (size_t)chunk * kChunkRows, row1 = min((size_t)m, row0 + kChunkRows);
  const uint32_t col = (blockIdx.y * 64 + lane) * VEC;
  if (col >= k) return;
  float wr[NJ][VEC], acc[NJ][VEC], sdb[NJ];   // sdb: db, one chain over the chunk's rows in ascending order (the same in every lane)
#pragma unroll
  for (int j = 0; j < NJ; j++) {
    load_vec(w + (size_t)j * k + col, wr[j]);
    sdb[j] = 0.f;
#pragma unroll
    for (int e = 0; e < VEC; e++) acc[j][e] = 0.f;
  }
#pragma unroll 4
  for (size_t row = row0; row < row1; row++) {
    float xr[VEC], d[VEC], g[NJ];
    load_vec(x + row * ldx + col, xr);
#pragma unroll
    for (int j = 0; j < NJ; j++) {
      g[j] = dz[row * kNO + j0 + j];
      sdb[j] += g[j];
    }
#pragma unroll
    for (int e = 0; e < VEC; e++) d[e] = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; j++)
#pragma unroll
      for (int e = 0; e < VEC; e++) {
        acc[j][e] = fmaf(g[j], xr[e], acc[j][e]);
        d[e] = fmaf(g[j], wr[j][e], d[e]);
      }
    if (dx) {   // uniform
#pragma unroll
      for (int e = 0; e < VEC; e++) d[e] *= scale;
      store_vec(dx + row * lddx + col, d);
    }
  }
#pragma unroll
  for (int j = 0; j < NJ; j++) store_vec(part + (size_t)(j0 + j) * k + col, acc[j]);
  if (blockIdx.y == 0 && lane == 0) {   // the wavefront of the first column groups writes db (lane 0 always owns a column)
#pragma unroll
    for (int j = 0; j < NJ; j++) part[(size_t)kNO * k + j0 + j] = sdb[j];
  }
}

// grid (n_chunks, column blocks of 64 threads, 2 heads), one wavefront a workgroup
template <typename T>
__global__ __launch_bounds__(64) void out_bwd_tile(const float* __restrict__ dz, const float* __restrict__ scale, const T* __restrict__ xp,
                                                   const T* __restrict__ xv, uint32_t ldxp, uint32_t ldxv, const float* __restrict__ wp,
                                                   const float* __restrict__ wv, uint32_t m, uint32_t k, T* __restrict__ dxp, T* __restrict__ dxv,
                                                   uint32_t lddxp, uint32_t lddxv, float* __restrict__ work) {
  const float sc = *scale;
  float* part = work + (size_t)blockIdx.x * ((size_t)kNO * k + 12);
  if (blockIdx.z == 0) bwd_head<T, kNP>(dz, sc, xp, ldxp, wp, m, k, dxp, lddxp, part, 0);
  else bwd_head<T, kNV>(dz, sc, xv, ldxv, wv, m, k, dxv, lddxv, part, kNP);
}

// one thread per element of (dWp, dWv, dbp, dbv): the second stage over the chunks, times the upstream gradient
__global__ __launch_bounds__(256) void out_chunk_reduce(const float* __restrict__ work, const float* __restrict__ scale, float* __restrict__ dwp,
                                                        float* __restrict__ dbp, float* __restrict__ dwv, float* __restrict__ dbv,
                                                        uint32_t n_chunks, uint32_t k) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x, wpe = kNP * k, we = kNO * k;
  if (e >= we + kNO) return;
  const float t = second_stage(work + e, (size_t)we + 12, n_chunks) * *scale;
  if (e < wpe) dwp[e] = t;
  else if (e < we) dwv[e - wpe] = t;
  else if (e < we + kNP) dbp[e - we] = t;
  else dbv[e - we - kNP] = t;
}

// ---------------------------------------------------------------------------------------------------------------- host
using c4host::aligned16;
using c4host::launched;

uint32_t chunks_of(uint32_t m) { return (m + kChunkRows - 1) / kChunkRows; }

uint64_t work_floats(uint32_t m, uint32_t k) {
  const uint64_t n_chunks = chunks_of(m), fwd = 4ull * m + 4 * n_chunks, bwd = n_chunks * (9ull * k + 12);
  return fwd > bwd ? fwd : bwd;
}

int shape_refusal(const char* me, uint32_t m, uint32_t k) {
  if (m == 0) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": m >= 1");
  if (m > (1u << 30)) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": m <= 2^30");
  if (k == 0 || k % 8) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": k must be a positive multiple of 8");
  if (k > (1u << 20)) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": k <= 2^20");
  return C4_OK;
}

int stride_refusal(const char* me, const char* name, uint32_t ld, uint32_t k, uint32_t x_is_bf16) {
  const uint32_t mult = x_is_bf16 ? 8 : 4;
  if (ld % mult || ld < k)
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": row stride " + name + " must be a multiple of " + (x_is_bf16 ? "8" : "4") + " and at least k");
  return C4_OK;
}

}  // namespace

extern "C" int c4_train_out_chunk_rows(void) { return (int)kChunkRows; }

extern "C" int c4_train_out_work_bytes(uint32_t m, uint32_t k, uint64_t* bytes_out) {
  const char* me = "c4_train_out_work_bytes";
  if (!bytes_out) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": null argument");
  if (const int rc = shape_refusal(me, m, k)) return rc;
  *bytes_out = work_floats(m, k) * sizeof(float);
  return C4_OK;
}

extern "C" int c4_train_out_loss_fwd(const void* xp_dev, const void* xv_dev, uint32_t x_is_bf16, uint32_t ldxp, uint32_t ldxv, const float* wp_dev,
                                     const float* bp_dev, const float* wv_dev, const float* bv_dev, const float* policy_t_dev,
                                     const float* q_pen_t_dev, const float* q_nopen_t_dev, uint32_t m, uint32_t k, float* out_dev, float* dz_dev,
                                     float* losses_dev, float* work_dev, void* stream) {
  const char* me = "c4_train_out_loss_fwd";
  if (!xp_dev || !xv_dev || !wp_dev || !bp_dev || !wv_dev || !bv_dev || !policy_t_dev || !q_pen_t_dev || !q_nopen_t_dev || !out_dev || !dz_dev ||
      !losses_dev || !work_dev)
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": null argument");
  if (const int rc = shape_refusal(me, m, k)) return rc;
  if (const int rc = stride_refusal(me, "ldxp", ldxp, k, x_is_bf16)) return rc;
  if (const int rc = stride_refusal(me, "ldxv", ldxv, k, x_is_bf16)) return rc;
  if (!aligned16(xp_dev) || !aligned16(xv_dev) || !aligned16(wp_dev) || !aligned16(bp_dev) || !aligned16(wv_dev) || !aligned16(bv_dev) ||
      !aligned16(policy_t_dev) || !aligned16(q_pen_t_dev) || !aligned16(q_nopen_t_dev) || !aligned16(out_dev) || !aligned16(dz_dev) ||
      !aligned16(losses_dev) || !aligned16(work_dev))
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": arrays must be 16-byte aligned");
  C4_ON_STREAM_DEVICE(stream);
  const hipStream_t s = (hipStream_t)stream;
  const uint32_t n_chunks = chunks_of(m);
  const dim3 grid((m + 4 * kFwdRows - 1) / (4 * kFwdRows)), block(256);
  float* terms = work_dev;
  float* part = work_dev + 4 * (size_t)m;
  if (x_is_bf16)
    out_fwd_rows<uint16_t><<<grid, block, 0, s>>>((const uint16_t*)xp_dev, (const uint16_t*)xv_dev, ldxp, ldxv, wp_dev, bp_dev, wv_dev, bv_dev,
                                                  policy_t_dev, q_pen_t_dev, q_nopen_t_dev, m, k, out_dev, dz_dev, terms);
  else
    out_fwd_rows<float><<<grid, block, 0, s>>>((const float*)xp_dev, (const float*)xv_dev, ldxp, ldxv, wp_dev, bp_dev, wv_dev, bv_dev, policy_t_dev,
                                               q_pen_t_dev, q_nopen_t_dev, m, k, out_dev, dz_dev, terms);
  if (const int rc = launched(me, hipGetLastError())) return rc;
  out_loss_reduce<<<dim3(1), block, 0, s>>>(terms, part, losses_dev, m, n_chunks);
  return launched(me, hipGetLastError());
}

extern "C" int c4_train_out_loss_bwd(const float* dz_dev, const float* scale_dev, const void* xp_dev, const void* xv_dev, uint32_t x_is_bf16,
                                     uint32_t ldxp, uint32_t ldxv, const float* wp_dev, const float* wv_dev, uint32_t m, uint32_t k, void* dxp_dev,
                                     void* dxv_dev, uint32_t lddxp, uint32_t lddxv, float* dwp_dev, float* dbp_dev, float* dwv_dev, float* dbv_dev,
                                     float* work_dev, void* stream) {
  const char* me = "c4_train_out_loss_bwd";
  if (!dz_dev || !scale_dev || !xp_dev || !xv_dev || !wp_dev || !wv_dev || !dwp_dev || !dbp_dev || !dwv_dev || !dbv_dev || !work_dev)
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": null argument");
  if (const int rc = shape_refusal(me, m, k)) return rc;
  if (const int rc = stride_refusal(me, "ldxp", ldxp, k, x_is_bf16)) return rc;
  if (const int rc = stride_refusal(me, "ldxv", ldxv, k, x_is_bf16)) return rc;
  if (dxp_dev)
    if (const int rc = stride_refusal(me, "lddxp", lddxp, k, x_is_bf16)) return rc;
  if (dxv_dev)
    if (const int rc = stride_refusal(me, "lddxv", lddxv, k, x_is_bf16)) return rc;
  if (!aligned16(dz_dev) || !aligned16(xp_dev) || !aligned16(xv_dev) || !aligned16(wp_dev) || !aligned16(wv_dev) || !aligned16(dxp_dev) ||
      !aligned16(dxv_dev) || !aligned16(dwp_dev) || !aligned16(dbp_dev) || !aligned16(dwv_dev) || !aligned16(dbv_dev) || !aligned16(work_dev))
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": arrays must be 16-byte aligned");
  if ((uintptr_t)scale_dev & 3) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": scale must be 4-byte aligned");
  C4_ON_STREAM_DEVICE(stream);
  const hipStream_t s = (hipStream_t)stream;
  const uint32_t n_chunks = chunks_of(m), vec = x_is_bf16 ? 8 : 4;
  const dim3 grid(n_chunks, (k / vec + 63) / 64, 2), block(64);
  if (x_is_bf16)
    out_bwd_tile<uint16_t><<<grid, block, 0, s>>>(dz_dev, scale_dev, (const uint16_t*)xp_dev, (const uint16_t*)xv_dev, ldxp, ldxv, wp_dev, wv_dev, m,
                                                  k, (uint16_t*)dxp_dev, (uint16_t*)dxv_dev, lddxp, lddxv, work_dev);
  else
    out_bwd_tile<float><<<grid, block, 0, s>>>(dz_dev, scale_dev, (const float*)xp_dev, (const float*)xv_dev, ldxp, ldxv, wp_dev, wv_dev, m, k,
                                               (float*)dxp_dev, (float*)dxv_dev, lddxp, lddxv, work_dev);
  if (const int rc = launched(me, hipGetLastError())) return rc;
  out_chunk_reduce<<<dim3((kNO * k + kNO + 255) / 256), dim3(256), 0, s>>>(work_dev, scale_dev, dwp_dev, dbp_dev, dwv_dev, dbv_dev, n_chunks, k);
  return launched(me, hipGetLastError());
}
