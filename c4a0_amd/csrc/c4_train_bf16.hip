// c4_train_bf16.hip -- the memory-bound kernels of bf16 mixed-precision training of the heads' hidden blocks (heads="bf16",
// c4a0_amd/train_heads.py; the numerics contract is in include/c4a0_hip.h).  The three products of a step -- forward x W^T, dgrad
// dz W, wgrad dz^T x -- are c4_linear_bf16 (c4_head_gemm.hip) as it is; it reads both operands k-major, so every matrix a product
// reduces over its ROWS is needed transposed: W^T for dgrad, x^T and dz^T (the batch as k) for wgrad.  This file holds
//
//   train_cast          f32 or bf16 [m][lds] -> bf16 [m][ldd] and / or its transpose [c][ldt], the batch padded with zeros
//   train_bn_fwd_bf16   batch mean and biased variance of every column of z (bf16), y = bf16(relu(...)), optionally y^T
//   train_bn_bwd_bf16   dz = bf16(dz32) and dz^T, dgamma, dbeta, db = sum_r dz32 (before the rounding; gamma rstd / m applied after the sum)
//
// One walk serves all three: a workgroup of 512 threads owns 16 columns and visits the rows in blocks of 256; thread
// (rg = t >> 1, ch = t & 1) moves the 8 columns 8 ch .. 8 ch + 7 of row 256 blk + rg with one 16-byte access (two for an f32
// source).  The transpose of a block goes through an LDS tile [16][256 + 8] of bf16: a thread puts its 8 values at [8 ch + i][rg]
// (2-byte stores; the 132-dword row puts the two column halves 32 banks apart, the rows of a wavefront share dwords pairwise), then
// thread (col = t >> 5, chunk = t & 31) reads 16 aligned bytes [col][8 chunk ..] and stores them to dst_t[col][256 blk + 8 chunk ..]:
// 512 contiguous bytes per half wavefront.  A row at or past m is a SELECTED zero -- never loaded, never a product with zero --
// so columns m .. ldt - 1 of every transposed row are written as zeros, which is what makes them exact no-ops in the GEMM's k.
// Column sums: per thread over its rows rg, rg + 256, .. in order, then 16 sums of 16 row groups in order, then those 16 in order:
// one order that the shape alone decides, no atomics.  The batch-norm arithmetic is c4_train.hip's, operation for operation
// (-ffp-contract=off), on z widened exactly to f32: the two-pass variance, the predicate !(pre <= 0) that lets a NaN pass, the
// corrected deviations xh = ((z - mean) - corr) * rstd of the backward.  Non-finite columns behave as there: a NaN, an infinity or an
// overflowing sum in a column of z makes its mean or variance non-finite, every pre-activation of the column NaN, so y, dz, dgamma
// and db of that column are NaN and dbeta is the column sum of dy; no other column is touched.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/c4a0_hip.h"
#include "c4_host.hpp"

namespace {

constexpr int kCols = 16, kRows = 256, kThreads = 2 * kRows, kTileLd = kRows + 8, kGroups = 16;

// round to nearest, ties to even: v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t to_bf16(float f) { return (uint32_t)__builtin_bit_cast(uint16_t, static_cast<__bf16>(f)); }
__device__ __forceinline__ float widen(uint32_t h) { return __uint_as_float(h << 16); }

__device__ __forceinline__ uint4 pack8(const uint32_t (&h)[8]) {
  return uint4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
}

__device__ __forceinline__ void unpack8(const uint4 q, float (&v)[8]) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
  for (int i = 0; i < 4; i++) {
    v[2 * i] = widen(w[i] & 0xFFFFu);
    v[2 * i + 1] = widen(w[i] >> 16);
  }
}

__device__ __forceinline__ void load8_bf16(const uint16_t* p, float (&v)[8]) { unpack8(*reinterpret_cast<const uint4*>(p), v); }

__device__ __forceinline__ void load8_f32(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

struct Tile {
  uint16_t e[kCols][kTileLd];
};

// the block's 256 x 16 values into dst_t[col0 + col][row0 ..]; chunks that begin at or past ldt (a multiple of 8) are not written
__device__ __forceinline__ void transpose_out(Tile& tile, const uint32_t (&h)[8], uint16_t* __restrict__ dst_t, uint32_t col0, uint32_t row0,
                                              uint32_t ldt) {
  const uint32_t rg = threadIdx.x >> 1, ch = threadIdx.x & 1;
#pragma unroll
  for (int i = 0; i < 8; i++) tile.e[8 * ch + i][rg] = (uint16_t)h[i];
  __syncthreads();
  const uint32_t col = threadIdx.x >> 5, r = row0 + 8 * (threadIdx.x & 31);
  if (r < ldt) *reinterpret_cast<uint4*>(dst_t + (size_t)(col0 + col) * ldt + r) = *reinterpret_cast<const uint4*>(&tile.e[col][8 * (threadIdx.x & 31)]);
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void train_cast(const void* __restrict__ src, uint32_t src_bf16, uint32_t m, uint32_t lds,
                                                       uint16_t* __restrict__ dst, uint32_t ldd, uint16_t* __restrict__ dst_t, uint32_t ldt) {
  __shared__ __attribute__((aligned(16))) Tile tile;
  const uint32_t rg = threadIdx.x >> 1, ch = threadIdx.x & 1, col0 = blockIdx.x * kCols, c = col0 + 8 * ch;
  const uint32_t row0 = blockIdx.y * kRows, row = row0 + rg;
  uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (row < m) {
    if (src_bf16) {
      const uint4 q = *reinterpret_cast<const uint4*>(reinterpret_cast<const uint16_t*>(src) + (size_t)row * lds + c);
      h[0] = q.x & 0xFFFFu; h[1] = q.x >> 16; h[2] = q.y & 0xFFFFu; h[3] = q.y >> 16;
      h[4] = q.z & 0xFFFFu; h[5] = q.z >> 16; h[6] = q.w & 0xFFFFu; h[7] = q.w >> 16;
    } else {
      float v[8];
      load8_f32(reinterpret_cast<const float*>(src) + (size_t)row * lds + c, v);
#pragma unroll
      for (int i = 0; i < 8; i++) h[i] = to_bf16(v[i]);
    }
    if (dst) *reinterpret_cast<uint4*>(dst + (size_t)row * ldd + c) = pack8(h);
  }
  if (dst_t) transpose_out(tile, h, dst_t, col0, row0, ldt);   // uniform over the workgroup
}

struct Red {
  float a[kRows][kCols];
  float b[kGroups][kCols];
};

// s[j] <- the sum over all row groups of column 8 ch + j; every thread of a column half gets the same values
__device__ __forceinline__ void column_sums(Red& red, float (&s)[8]) {
  const uint32_t rg = threadIdx.x >> 1, ch = threadIdx.x & 1;
  __syncthreads();   // the previous use of `red` is over
#pragma unroll
  for (int j = 0; j < 8; j++) red.a[rg][8 * ch + j] = s[j];
  __syncthreads();
  if (threadIdx.x < kGroups * kCols) {
    const uint32_t col = threadIdx.x & (kCols - 1), grp = threadIdx.x / kCols;
    float t = red.a[grp * (kRows / kGroups)][col];
#pragma unroll
    for (int q = 1; q < kRows / kGroups; q++) t += red.a[grp * (kRows / kGroups) + q][col];
    red.b[grp][col] = t;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 8; j++) {
    float t = red.b[0][8 * ch + j];
#pragma unroll
    for (int g = 1; g < kGroups; g++) t += red.b[g][8 * ch + j];
    s[j] = t;
  }
}

// s = fl(a + b) and e with a + b = s + e exactly (Knuth's TwoSum; -ffp-contract=off and no fast-math keep it as written)
__device__ __forceinline__ void two_sum(float a, float b, float& s, float& e) {
  const float t = a + b, bv = t - a, av = t - bv;
  e = (a - av) + (b - bv);
  s = t;
}

// column_sums of hi + lo in two-float arithmetic, the same order: every addition of two hi parts hands its rounding error to lo.  For
// summands that cancel (the bias gradient is 0 in real numbers while its partial sums are not) the plain sum keeps the partial sums' ulps.
__device__ __forceinline__ void column_sums_twofold(Red& rh, Red& rl, float (&hi)[8], float (&lo)[8]) {
  const uint32_t rg = threadIdx.x >> 1, ch = threadIdx.x & 1;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 8; j++) {
    rh.a[rg][8 * ch + j] = hi[j];
    rl.a[rg][8 * ch + j] = lo[j];
  }
  __syncthreads();
  if (threadIdx.x < kGroups * kCols) {
    const uint32_t col = threadIdx.x & (kCols - 1), base = (threadIdx.x / kCols) * (kRows / kGroups);
    float h = rh.a[base][col], l = rl.a[base][col], e;
#pragma unroll
    for (int q = 1; q < kRows / kGroups; q++) {
      two_sum(h, rh.a[base + q][col], h, e);
      l += e;
      l += rl.a[base + q][col];
    }
    rh.b[threadIdx.x / kCols][col] = h;
    rl.b[threadIdx.x / kCols][col] = l;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 8; j++) {
    float h = rh.b[0][8 * ch + j], l = rl.b[0][8 * ch + j], e;
#pragma unroll
    for (int g = 1; g < kGroups; g++) {
      two_sum(h, rh.b[g][8 * ch + j], h, e);
      l += e;
      l += rl.b[g][8 * ch + j];
    }
    hi[j] = h;
    lo[j] = l;
  }
}

__global__ __launch_bounds__(kThreads) void train_bn_fwd_bf16(const uint16_t* __restrict__ z, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps, uint32_t m, uint32_t ldz, uint32_t ldy,
                                                              uint16_t* __restrict__ y, float* __restrict__ mean_out, float* __restrict__ var_out,
                                                              uint16_t* __restrict__ y_t, uint32_t ldt) {
  __shared__ Red red;
  __shared__ __attribute__((aligned(16))) Tile tile;
  const uint32_t rg = threadIdx.x >> 1, ch = threadIdx.x & 1, col0 = blockIdx.x * kCols, c = col0 + 8 * ch;
  const uint16_t* zc = z + c;
  float s[8], v[8], mean[8], rstd[8], g[8], b[8];
#pragma unroll
  for (int j = 0; j < 8; j++) s[j] = 0.f;
  for (uint32_t row = rg; row < m; row += kRows) {
    load8_bf16(zc + (size_t)row * ldz, v);
#pragma unroll
    for (int j = 0; j < 8; j++) s[j] += v[j];
  }
  column_sums(red, s);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    mean[j] = s[j] / (float)m;
    s[j] = 0.f;
  }
  for (uint32_t row = rg; row < m; row += kRows) {
    load8_bf16(zc + (size_t)row * ldz, v);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float d = v[j] - mean[j];
      s[j] += d * d;
    }
  }
  column_sums(red, s);
  load8_f32(gamma + c, g);
  load8_f32(beta + c, b);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    s[j] = s[j] / (float)m;   // the biased variance
    rstd[j] = 1.0f / sqrtf(s[j] + eps);
  }
  if (rg == 0) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      mean_out[c + j] = mean[j];
      var_out[c + j] = s[j];
    }
  }
  const uint32_t rows = y_t ? max(m, ldt) : m;   // the transpose's zero columns reach ldt
  for (uint32_t row0 = 0; row0 < rows; row0 += kRows) {
    const uint32_t row = row0 + rg;
    uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (row < m) {
      load8_bf16(zc + (size_t)row * ldz, v);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float pre = (v[j] - mean[j]) * rstd[j] * g[j] + b[j];
        h[j] = to_bf16(!(pre <= 0.f) ? pre : 0.f);   // a NaN passes
      }
      *reinterpret_cast<uint4*>(y + (size_t)row * ldy + c) = pack8(h);
    }
    if (y_t) transpose_out(tile, h, y_t, col0, row0, ldt);
  }
}

__global__ __launch_bounds__(kThreads) void train_bn_bwd_bf16(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ z,
                                                              const float* __restrict__ mean_in, const float* __restrict__ var_in,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta, float eps, uint32_t m,
                                                              uint32_t lddy, uint32_t ldz, uint32_t lddz, uint16_t* __restrict__ dz,
                                                              uint16_t* __restrict__ dz_t, uint32_t ldt, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta, float* __restrict__ db) {
  __shared__ Red red, red_lo;
  __shared__ __attribute__((aligned(16))) Tile tile;
  const uint32_t rg = threadIdx.x >> 1, ch = threadIdx.x & 1, col0 = blockIdx.x * kCols, c = col0 + 8 * ch;
  const uint16_t* zc = z + c;
  const uint16_t* dyc = dy + c;
  float s[8], t[8], v[8], w[8], mean[8], rstd[8], g[8], b[8], corr[8];
  load8_f32(mean_in + c, mean);
  load8_f32(var_in + c, rstd);
  load8_f32(gamma + c, g);
  load8_f32(beta + c, b);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    rstd[j] = 1.0f / sqrtf(rstd[j] + eps);
    s[j] = 0.f;
  }
  // the mean of the deviations: what the f32 mean is off the column's true mean by (c4_train.hip, train_bn_relu_bwd)
  for (uint32_t row = rg; row < m; row += kRows) {
    load8_bf16(zc + (size_t)row * ldz, v);
#pragma unroll
    for (int j = 0; j < 8; j++) s[j] += v[j] - mean[j];
  }
  column_sums(red, s);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    corr[j] = s[j] / (float)m;
    s[j] = t[j] = 0.f;
  }
  for (uint32_t row = rg; row < m; row += kRows) {
    load8_bf16(zc + (size_t)row * ldz, v);
    load8_bf16(dyc + (size_t)row * lddy, w);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const float d = v[j] - mean[j];
      const float pre = d * rstd[j] * g[j] + b[j];          // the forward's operations in the forward's order
      const float gr = !(pre <= 0.f) ? w[j] : 0.f;          // ReLU'(0) = 0; the forward's predicate
      s[j] += gr;
      t[j] += gr * ((d - corr[j]) * rstd[j]);
    }
  }
  column_sums(red, s);
  column_sums(red, t);
  // dz32 = gamma rstd ((g - dbeta / m) - xh dgamma / m) is evaluated as (gamma rstd / m) ((m g - dbeta) - xh dgamma): dy is bf16, so m g
  // is exact and m g - dbeta keeps the bits that g - fl(dbeta / m) would round away THE SAME WAY in every row of a binade -- a bias
  // of m half-ulps in sum_r dz32, the bias gradient, which is 0 in real numbers
  // ... which is 0 in real numbers.  What m g - dbeta still rounds away (dbeta, an f32 sum, has lower bits than m g) it also rounds
  // the same way in every row of a binade; no row can carry that residue, but the bias gradient can: TwoSum gives the subtraction's
  // rounding error exactly, and db sums it beside the rounded values.  The sum itself is two-fold (sdb + sde, every addition's
  // rounding error kept): its summands cancel, and a plain f32 sum would be left with the ulps of partial sums m times the result's.
  const float mf = (float)m;
  float scale[8], sdb[8], sde[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    scale[j] = g[j] * rstd[j] / mf;
    sdb[j] = sde[j] = 0.f;
  }
  const uint32_t rows = max(m, ldt);
  for (uint32_t row0 = 0; row0 < rows; row0 += kRows) {
    const uint32_t row = row0 + rg;
    uint32_t h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (row < m) {
      load8_bf16(zc + (size_t)row * ldz, v);
      load8_bf16(dyc + (size_t)row * lddy, w);
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const float d = v[j] - mean[j];
        const float pre = d * rstd[j] * g[j] + b[j];
        const float gr = !(pre <= 0.f) ? w[j] : 0.f;
        float u, eu, es;
        two_sum(mf * gr, -s[j], u, eu);                        // m g - dbeta, and what the subtraction rounded away
        const float t32 = u - ((d - corr[j]) * rstd[j]) * t[j];
        // the bias gradient sums the values before the rounding, the column's factor gamma rstd / m applied once, after the sum
        two_sum(sdb[j], t32, sdb[j], es);
        sde[j] += eu + es;
        h[j] = to_bf16(scale[j] * t32);
      }
      *reinterpret_cast<uint4*>(dz + (size_t)row * lddz + c) = pack8(h);
    }
    transpose_out(tile, h, dz_t, col0, row0, ldt);
  }
  column_sums_twofold(red, red_lo, sdb, sde);
  if (rg == 0) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      dbeta[c + j] = s[j];
      dgamma[c + j] = t[j];
      db[c + j] = scale[j] * (sdb[j] + sde[j]);
    }
  }
}

using c4host::aligned16;
using c4host::below_2_31;
using c4host::launched;

uint32_t padded(uint32_t m) { return 64 * ((m + 63) / 64); }

uint32_t row_blocks(uint32_t rows) { return (rows + kRows - 1) / kRows; }

}  // namespace

extern "C" int c4_train_cast_bf16(const void* src_dev, uint32_t src_is_bf16, uint32_t m, uint32_t c, uint32_t lds, void* dst_dev, uint32_t ldd,
                                  void* dst_t_dev, uint32_t ldt, void* stream) {
  const char* me = "c4_train_cast_bf16";
  if (!src_dev || (!dst_dev && !dst_t_dev)) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": null argument (src, and at least one of dst and dst_t)");
  if (m == 0) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": m >= 1");
  if (c == 0 || c % kCols || lds % 8 || lds < c) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": c % 16 == 0, lds >= c, lds a multiple of 8");
  if (dst_dev && (ldd % 8 || ldd < c)) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": ldd >= c, ldd a multiple of 8");
  if (dst_t_dev && (ldt % 8 || ldt < padded(m))) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": ldt >= 64 ceil(m / 64), ldt a multiple of 8");
  if (!aligned16(src_dev) || !aligned16(dst_dev) || !aligned16(dst_t_dev)) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": arrays must be 16-byte aligned");
  if (!below_2_31(m, lds) || (dst_dev && !below_2_31(m, ldd)) || (dst_t_dev && !below_2_31(c, ldt)))
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": operands must stay below 2^31 elements");
  C4_ON_STREAM_DEVICE(stream);
  const uint32_t rows = dst_t_dev ? (ldt > m ? ldt : m) : m;
  train_cast<<<dim3(c / kCols, row_blocks(rows)), dim3(kThreads), 0, (hipStream_t)stream>>>(src_dev, src_is_bf16, m, lds, (uint16_t*)dst_dev, ldd,
                                                                                           (uint16_t*)dst_t_dev, ldt);
  return launched(me, hipGetLastError());
}

extern "C" int c4_train_bn_relu_fwd_bf16(const void* z_dev, const float* gamma_dev, const float* beta_dev, float eps, uint32_t m, uint32_t n,
                                         uint32_t ldz, uint32_t ldy, void* y_dev, float* mean_dev, float* var_dev, void* y_t_dev, uint32_t ldt,
                                         void* stream) {
  const char* me = "c4_train_bn_relu_fwd_bf16";
  if (!z_dev || !gamma_dev || !beta_dev || !y_dev || !mean_dev || !var_dev) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": null argument");
  if (m < 2) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": batch statistics need m >= 2 rows");
  if (n == 0 || n % 192 || ldz % 8 || ldy % 8 || ldz < n || ldy < n)
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": n % 192 == 0, ldz >= n, ldy >= n, ldz and ldy multiples of 8");
  if (y_t_dev && (ldt % 8 || ldt < padded(m))) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": ldt >= 64 ceil(m / 64), ldt a multiple of 8");
  if (!aligned16(z_dev) || !aligned16(gamma_dev) || !aligned16(beta_dev) || !aligned16(y_dev) || !aligned16(mean_dev) || !aligned16(var_dev) ||
      !aligned16(y_t_dev))
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": arrays must be 16-byte aligned");
  if (!below_2_31(m, ldz) || !below_2_31(m, ldy) || (y_t_dev && !below_2_31(n, ldt)))
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": operands must stay below 2^31 elements");
  C4_ON_STREAM_DEVICE(stream);
  train_bn_fwd_bf16<<<dim3(n / kCols), dim3(kThreads), 0, (hipStream_t)stream>>>((const uint16_t*)z_dev, gamma_dev, beta_dev, eps, m, ldz, ldy,
                                                                                (uint16_t*)y_dev, mean_dev, var_dev, (uint16_t*)y_t_dev, ldt);
  return launched(me, hipGetLastError());
}

extern "C" int c4_train_bn_relu_bwd_bf16(const void* dy_dev, const void* z_dev, const float* mean_dev, const float* var_dev, const float* gamma_dev,
                                         const float* beta_dev, float eps, uint32_t m, uint32_t n, uint32_t lddy, uint32_t ldz, uint32_t lddz,
                                         void* dz_dev, void* dz_t_dev, uint32_t ldt, float* dgamma_dev, float* dbeta_dev, float* db_dev, void* stream) {
  const char* me = "c4_train_bn_relu_bwd_bf16";
  if (!dy_dev || !z_dev || !mean_dev || !var_dev || !gamma_dev || !beta_dev || !dz_dev || !dz_t_dev || !dgamma_dev || !dbeta_dev || !db_dev)
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": null argument");
  if (m < 2) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": batch statistics need m >= 2 rows");
  if (n == 0 || n % 192 || lddy % 8 || ldz % 8 || lddz % 8 || lddy < n || ldz < n || lddz < n)
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": n % 192 == 0, lddy, ldz and lddz >= n and multiples of 8");
  if (ldt % 8 || ldt < padded(m)) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": ldt >= 64 ceil(m / 64), ldt a multiple of 8");
  if (!aligned16(dy_dev) || !aligned16(z_dev) || !aligned16(mean_dev) || !aligned16(var_dev) || !aligned16(gamma_dev) || !aligned16(beta_dev) ||
      !aligned16(dz_dev) || !aligned16(dz_t_dev) || !aligned16(dgamma_dev) || !aligned16(dbeta_dev) || !aligned16(db_dev))
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": arrays must be 16-byte aligned");
  if (!below_2_31(m, lddy) || !below_2_31(m, ldz) || !below_2_31(m, lddz) || !below_2_31(n, ldt))
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": operands must stay below 2^31 elements");
  C4_ON_STREAM_DEVICE(stream);
  train_bn_bwd_bf16<<<dim3(n / kCols), dim3(kThreads), 0, (hipStream_t)stream>>>((const uint16_t*)dy_dev, (const uint16_t*)z_dev, mean_dev, var_dev,
                                                                                gamma_dev, beta_dev, eps, m, lddy, ldz, lddz, (uint16_t*)dz_dev,
                                                                                (uint16_t*)dz_t_dev, ldt, dgamma_dev, dbeta_dev, db_dev);
  return launched(me, hipGetLastError());
}
