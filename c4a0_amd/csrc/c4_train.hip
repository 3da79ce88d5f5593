// c4_train.hip -- training kernels for the heads' hidden blocks (Linear(F, F) -> BatchNorm1d in train mode -> ReLU; reference
// src/c4a0/nn.py:75-100), f32 throughout, on gfx950's exact-f32 MFMA v_mfma_f32_16x16x4_f32.  The forward product z = x W^T + b is
// c4_linear_f32 (c4_f32_net.hip); this file holds what a training step needs besides:
//
//   train_bn_relu_fwd   batch mean and biased variance of every column of z, y = relu((z - mean) * rstd * gamma + beta)
//   train_bn_relu_bwd   dz, dgamma, dbeta from dy (the pre-activation is recomputed from z with the forward's own operations)
//   train_dgrad         dx[m][k] = sum_n dz[m][n] w[n][k]
//   train_wgrad         dw[n][k] = sum_m dz[m][n] x[m][k],  db[n] = sum_m dz[m][n]
//
// Every output is a fixed function of the inputs: each sum has one order, set by the shape alone, and nothing is accumulated with
// atomics.  Both products read the [m][.] matrices where they lie (row-major, strided rows allowed):
//   * wgrad reduces over the batch.  The 16x16x4 operand map wants, from lane (r = l & 15, h = l >> 4), A[i = r][kk = h] and
//     B[kk = h][j = r]: with kk = the batch row mb + h these are x[mb + h][k0 + r] and dz[mb + h][n0 + r], 64 contiguous bytes per
//     lane group.  D[i = 4 h + e][j = r] is then dw[n0 + r][k0 + 4 h + e]: one 16-byte store per tile.  Rows past the batch are fed
//     as zeros on both sides.
//   * dgrad reduces over n.  dz is read like f32_gemm's X (one float4 of row m0 + r at n = nb + 4 h .. + 3, element j in MFMA step
//     j), the weights one float per step from w[nb + 4 h + j][k0 + r].  D is dx[m0 + r][k0 + 4 h + e].
// The batch-norm kernels give one workgroup 32 columns: 16 row groups x 32 columns of threads, per-thread sums over rows
// rg, rg + 16, .., then the 16 partial sums added in order by the column's first thread.
// Non-finite input: ReLU's predicate, in the forward and in the backward's mask, is PyTorch's !(pre <= 0), not pre > 0.  0 and -0 give 0
// and ReLU'(0) = 0 as before, and for finite pre no bit differs; a NaN pre-activation passes: y is NaN and dy goes through the mask.
// A column of z that holds a NaN or an infinity, or whose sum overflows, has a non-finite mean and variance, so all its
// pre-activations are NaN: y, dz and dgamma of that column are NaN, dbeta is the column sum of dy, and no other column is touched
// (F.batch_norm(training=True) + relu and their autograd do the same).  A poisoned batch shows in the loss; it is not trained on as zeros.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/c4a0_hip.h"
#include "c4_host.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kBnCols = 32, kBnGroups = 16;

// sum over the row groups of this thread's column; every thread of the column returns the same value
__device__ __forceinline__ float bn_column_sum(float (*red)[kBnCols], float s, uint32_t c, uint32_t rg) {
  __syncthreads();   // the previous use of `red` is over
  red[rg][c] = s;
  __syncthreads();
  float t = red[0][c];
#pragma unroll
  for (int g = 1; g < kBnGroups; g++) t += red[g][c];
  return t;
}

__global__ __launch_bounds__(kBnCols * kBnGroups) void train_bn_relu_fwd(const float* __restrict__ z, const float* __restrict__ gamma,
                                                                         const float* __restrict__ beta, float eps, uint32_t m, uint32_t n,
                                                                         uint32_t ldz, uint32_t ldy, float* __restrict__ y,
                                                                         float* __restrict__ mean_out, float* __restrict__ var_out) {
  __shared__ float red[kBnGroups][kBnCols];
  const uint32_t c = threadIdx.x & (kBnCols - 1), rg = threadIdx.x / kBnCols, col = blockIdx.x * kBnCols + c;   // col < n: n % 32 == 0
  const float* zc = z + col;
  float s = 0.f;
  for (uint32_t row = rg; row < m; row += kBnGroups) s += zc[(size_t)row * ldz];
  const float mean = bn_column_sum(red, s, c, rg) / (float)m;
  s = 0.f;
  for (uint32_t row = rg; row < m; row += kBnGroups) {
    const float d = zc[(size_t)row * ldz] - mean;
    s += d * d;
  }
  const float var = bn_column_sum(red, s, c, rg) / (float)m;
  const float rstd = 1.0f / sqrtf(var + eps), g = gamma[col], b = beta[col];
  for (uint32_t row = rg; row < m; row += kBnGroups) {
    const float pre = (zc[(size_t)row * ldz] - mean) * rstd * g + b;
    y[(size_t)row * ldy + col] = !(pre <= 0.f) ? pre : 0.f;   // a NaN passes
  }
  if (rg == 0) {
    mean_out[col] = mean;
    var_out[col] = var;
  }
}

__global__ __launch_bounds__(kBnCols * kBnGroups) void train_bn_relu_bwd(const float* __restrict__ dy, const float* __restrict__ z,
                                                                         const float* __restrict__ mean_in, const float* __restrict__ var_in,
                                                                         const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                                         uint32_t m, uint32_t n, uint32_t lddy, uint32_t ldz, uint32_t lddz,
                                                                         float* __restrict__ dz, float* __restrict__ dgamma,
                                                                         float* __restrict__ dbeta) {
  __shared__ float red[kBnGroups][kBnCols];
  const uint32_t c = threadIdx.x & (kBnCols - 1), rg = threadIdx.x / kBnCols, col = blockIdx.x * kBnCols + c;
  const float mean = mean_in[col], rstd = 1.0f / sqrtf(var_in[col] + eps), g = gamma[col], b = beta[col];
  // The f32 mean is off the column's true mean by up to half an ulp of it, so the deviations z - mean do not sum to zero: where rstd
  // is large (a column that hardly varies) that residue, times rstd^2, would be what sum_r dz -- exactly 0 in real numbers, the
  // bias gradient of the layer before -- consists of.  The deviations themselves are (nearly) exact, so their mean `corr` is known
  // to f32 accuracy and the gradient arithmetic uses xh = ((z - mean) - corr) * rstd.  The ReLU mask stays the forward's own.
  float sd = 0.f;
  for (uint32_t row = rg; row < m; row += kBnGroups) sd += z[(size_t)row * ldz + col] - mean;
  const float corr = bn_column_sum(red, sd, c, rg) / (float)m;
  float sb = 0.f, sg = 0.f;
  for (uint32_t row = rg; row < m; row += kBnGroups) {
    const float d = z[(size_t)row * ldz + col] - mean;
    const float pre = d * rstd * g + b;                               // the forward's operations in the forward's order
    const float gr = !(pre <= 0.f) ? dy[(size_t)row * lddy + col] : 0.f;   // ReLU'(0) = 0; the forward's predicate
    sb += gr;
    sg += gr * ((d - corr) * rstd);
  }
  const float db = bn_column_sum(red, sb, c, rg);
  const float dg = bn_column_sum(red, sg, c, rg);
  const float c1 = db / (float)m, c2 = dg / (float)m, scale = g * rstd;
  for (uint32_t row = rg; row < m; row += kBnGroups) {
    const float d = z[(size_t)row * ldz + col] - mean;
    const float pre = d * rstd * g + b;
    const float gr = !(pre <= 0.f) ? dy[(size_t)row * lddy + col] : 0.f;
    dz[(size_t)row * lddz + col] = scale * ((gr - c1) - ((d - corr) * rstd) * c2);
  }
  if (rg == 0) {
    dgamma[col] = dg;
    dbeta[col] = db;
  }
}

// dx[m][k] for a tile of 16 KT columns x 16 MT rows per wavefront; the chain of an element visits n = nb + 4 h + j for j = 0..3,
// h = 0..3 in every block nb of 16 (f32_gemm's order).  Rows beyond the batch read the last row (in bounds) and are never stored.
template <int KT, int MT>
__global__ __launch_bounds__(256) void train_dgrad(const float* __restrict__ dz, const float* __restrict__ w, float* __restrict__ dx, uint32_t m,
                                                   uint32_t n, uint32_t k, uint32_t ldz, uint32_t ldx) {
  const uint32_t lane = threadIdx.x & 63, r = lane & 15, h = lane >> 4;
  const uint32_t k_tiles = k / (16 * KT);
  const uint32_t tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t mt = tile / k_tiles, kt = tile - mt * k_tiles;
  const uint32_t m0 = mt * 16 * MT, k0 = kt * 16 * KT;
  if (m0 >= m) return;   // a whole wavefront past the last tile (no barrier in this kernel)
  const float* zl[MT];
#pragma unroll
  for (int s = 0; s < MT; s++) zl[s] = dz + (size_t)min(m0 + 16 * s + r, m - 1) * ldz + 4 * h;
  const float* wl = w + (size_t)(4 * h) * k + k0 + r;
  f32x4 acc[KT][MT];
#pragma unroll
  for (int t = 0; t < KT; t++)
#pragma unroll
    for (int s = 0; s < MT; s++) acc[t][s] = f32x4{0.f, 0.f, 0.f, 0.f};
  float a[KT][4];
  f32x4 b[MT];
#pragma unroll
  for (int t = 0; t < KT; t++)
#pragma unroll
    for (int j = 0; j < 4; j++) a[t][j] = wl[(size_t)j * k + 16 * t];
#pragma unroll
  for (int s = 0; s < MT; s++) b[s] = *reinterpret_cast<const f32x4*>(zl[s]);
  for (uint32_t nb = 0; nb < n; nb += 16) {
    // the next block's operands are requested before this block's MFMAs (the last iteration re-reads block 0: in bounds, unused)
    const uint32_t nn = nb + 16 < n ? nb + 16 : 0;
    float an[KT][4];
    f32x4 bn[MT];
#pragma unroll
    for (int t = 0; t < KT; t++)
#pragma unroll
      for (int j = 0; j < 4; j++) an[t][j] = wl[(size_t)(nn + j) * k + 16 * t];
#pragma unroll
    for (int s = 0; s < MT; s++) bn[s] = *reinterpret_cast<const f32x4*>(zl[s] + nn);
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int t = 0; t < KT; t++)
#pragma unroll
        for (int s = 0; s < MT; s++) acc[t][s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][j], b[s][j], acc[t][s], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < KT; t++)
#pragma unroll
      for (int j = 0; j < 4; j++) a[t][j] = an[t][j];
#pragma unroll
    for (int s = 0; s < MT; s++) b[s] = bn[s];
  }
#pragma unroll
  for (int s = 0; s < MT; s++) {
    const uint32_t row = m0 + 16 * s + r;
    if (row >= m) continue;
#pragma unroll
    for (int t = 0; t < KT; t++) *reinterpret_cast<f32x4*>(dx + (size_t)row * ldx + k0 + 16 * t + 4 * h) = acc[t][s];
  }
}

// dw[n][k] for a tile of 16 NT rows x 16 KT columns per wavefront; the chain of an element visits the batch rows in order (MFMA
// step j of a block of 16 rows feeds row mb + 4 j + h, lane groups h = 0..3 inside the instruction).  Wavefronts of the first column
// tile also sum db: per lane its rows mb + 4 j + h in order, then (h0 + h1) + (h2 + h3).
template <int NT, int KT>
__global__ __launch_bounds__(256) void train_wgrad(const float* __restrict__ dz, const float* __restrict__ x, float* __restrict__ dw,
                                                   float* __restrict__ db, uint32_t m, uint32_t n, uint32_t k, uint32_t ldz, uint32_t ldx) {
  const uint32_t lane = threadIdx.x & 63, r = lane & 15, h = lane >> 4;
  const uint32_t k_tiles = k / (16 * KT), n_tiles = n / (16 * NT);
  const uint32_t tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t nt = tile / k_tiles, kt = tile - nt * k_tiles;
  if (nt >= n_tiles) return;   // a whole wavefront past the last tile (no barrier in this kernel)
  const uint32_t n0 = nt * 16 * NT, k0 = kt * 16 * KT;
  const float* xl = x + k0 + r;
  const float* zl = dz + n0 + r;
  f32x4 acc[NT][KT];
#pragma unroll
  for (int u = 0; u < NT; u++)
#pragma unroll
    for (int t = 0; t < KT; t++) acc[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float sdb[NT];
#pragma unroll
  for (int u = 0; u < NT; u++) sdb[u] = 0.f;
  // one block = 16 batch rows: step j feeds row mb + 4 j + h; a row past the batch is zero on both sides (its address is clamped)
  float a[4][KT], b[4][NT];
  auto load = [&](uint32_t mb, float (&aa)[4][KT], float (&bb)[4][NT]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t row = mb + 4 * j + h;
      const bool in = row < m;
      const size_t rc = in ? row : m - 1;
#pragma unroll
      for (int t = 0; t < KT; t++) {
        const float v = xl[rc * ldx + 16 * t];
        aa[j][t] = in ? v : 0.f;
      }
#pragma unroll
      for (int u = 0; u < NT; u++) {
        const float v = zl[rc * ldz + 16 * u];
        bb[j][u] = in ? v : 0.f;
      }
    }
  };
  load(0, a, b);
  for (uint32_t mb = 0; mb < m; mb += 16) {
    // the next block's operands are requested before this block's MFMAs (the last iteration re-reads block 0: in bounds, unused)
    float an[4][KT], bn[4][NT];
    load(mb + 16 < m ? mb + 16 : 0, an, bn);
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
      for (int u = 0; u < NT; u++) {
        sdb[u] += b[j][u];
#pragma unroll
        for (int t = 0; t < KT; t++) acc[u][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][t], b[j][u], acc[u][t], 0, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
      for (int t = 0; t < KT; t++) a[j][t] = an[j][t];
#pragma unroll
      for (int u = 0; u < NT; u++) b[j][u] = bn[j][u];
    }
  }
#pragma unroll
  for (int u = 0; u < NT; u++) {
#pragma unroll
    for (int t = 0; t < KT; t++) *reinterpret_cast<f32x4*>(dw + (size_t)(n0 + 16 * u + r) * k + k0 + 16 * t + 4 * h) = acc[u][t];
    if (kt == 0) {   // uniform over the wavefront
      const float p = sdb[u] + __shfl_xor(sdb[u], 16);
      const float q = p + __shfl_xor(p, 32);
      if (h == 0) db[n0 + 16 * u + r] = q;
    }
  }
}

using c4host::aligned16;
using c4host::below_2_31;
using c4host::launched;

}  // namespace

extern "C" int c4_train_bn_relu_fwd_f32(const float* z_dev, const float* gamma_dev, const float* beta_dev, float eps, uint32_t m, uint32_t n,
                                        uint32_t ldz, uint32_t ldy, float* y_dev, float* mean_dev, float* var_dev, void* stream) {
  const char* me = "c4_train_bn_relu_fwd_f32";
  if (!z_dev || !gamma_dev || !beta_dev || !y_dev || !mean_dev || !var_dev) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": null argument");
  if (m < 2) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": batch statistics need m >= 2 rows");
  if (n == 0 || n % 32 || ldz % 4 || ldy % 4 || ldz < n || ldy < n)
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": n % 32 == 0, ldz >= n, ldy >= n, ldz and ldy multiples of 4");
  if (!aligned16(z_dev) || !aligned16(gamma_dev) || !aligned16(beta_dev) || !aligned16(y_dev) || !aligned16(mean_dev) || !aligned16(var_dev))
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": arrays must be 16-byte aligned");
  if (!below_2_31(m, ldz) || !below_2_31(m, ldy)) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": operands must stay below 2^31 elements");
  C4_ON_STREAM_DEVICE(stream);
  train_bn_relu_fwd<<<dim3(n / kBnCols), dim3(kBnCols * kBnGroups), 0, (hipStream_t)stream>>>(z_dev, gamma_dev, beta_dev, eps, m, n, ldz, ldy, y_dev,
                                                                                             mean_dev, var_dev);
  return launched(me, hipGetLastError());
}

extern "C" int c4_train_bn_relu_bwd_f32(const float* dy_dev, const float* z_dev, const float* mean_dev, const float* var_dev, const float* gamma_dev,
                                        const float* beta_dev, float eps, uint32_t m, uint32_t n, uint32_t lddy, uint32_t ldz, uint32_t lddz,
                                        float* dz_dev, float* dgamma_dev, float* dbeta_dev, void* stream) {
  const char* me = "c4_train_bn_relu_bwd_f32";
  if (!dy_dev || !z_dev || !mean_dev || !var_dev || !gamma_dev || !beta_dev || !dz_dev || !dgamma_dev || !dbeta_dev)
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": null argument");
  if (m < 2) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": batch statistics need m >= 2 rows");
  if (n == 0 || n % 32 || lddy % 4 || ldz % 4 || lddz % 4 || lddy < n || ldz < n || lddz < n)
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": n % 32 == 0, lddy, ldz and lddz >= n and multiples of 4");
  if (!aligned16(dy_dev) || !aligned16(z_dev) || !aligned16(mean_dev) || !aligned16(var_dev) || !aligned16(gamma_dev) || !aligned16(beta_dev) ||
      !aligned16(dz_dev) || !aligned16(dgamma_dev) || !aligned16(dbeta_dev))
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": arrays must be 16-byte aligned");
  if (!below_2_31(m, lddy) || !below_2_31(m, ldz) || !below_2_31(m, lddz))
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": operands must stay below 2^31 elements");
  C4_ON_STREAM_DEVICE(stream);
  train_bn_relu_bwd<<<dim3(n / kBnCols), dim3(kBnCols * kBnGroups), 0, (hipStream_t)stream>>>(dy_dev, z_dev, mean_dev, var_dev, gamma_dev, beta_dev, eps,
                                                                                             m, n, lddy, ldz, lddz, dz_dev, dgamma_dev, dbeta_dev);
  return launched(me, hipGetLastError());
}

extern "C" int c4_train_linear_dgrad_f32(const float* dz_dev, const float* w_dev, float* dx_dev, uint32_t m, uint32_t n, uint32_t k, uint32_t ldz,
                                         uint32_t ldx, void* stream) {
  const char* me = "c4_train_linear_dgrad_f32";
  if (!dz_dev || !w_dev || !dx_dev) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": null argument");
  if (n == 0 || k == 0 || n % 32 || k % 16 || ldz % 4 || ldx % 4 || ldz < n || ldx < k)
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": n % 32 == 0, k % 16 == 0, ldz >= n, ldx >= k, ldz and ldx multiples of 4");
  if (!aligned16(dz_dev) || !aligned16(w_dev) || !aligned16(dx_dev)) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": arrays must be 16-byte aligned");
  if (!below_2_31(m, ldz) || !below_2_31(m, ldx) || !below_2_31(n, k))
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": operands must stay below 2^31 elements");
  if (m == 0) return C4_OK;
  C4_ON_STREAM_DEVICE(stream);
  const hipStream_t s = (hipStream_t)stream;
  // 32 x 32 tiles (16 x 32 where k is an odd multiple of 16); both compute the same bits
  const uint32_t kt = k % 32 ? 1 : 2;
  const uint64_t tiles = (uint64_t)((m + 31) / 32) * (k / (16 * kt));
  const dim3 grid((uint32_t)((tiles + 3) / 4));
  if (kt == 2)
    train_dgrad<2, 2><<<grid, dim3(256), 0, s>>>(dz_dev, w_dev, dx_dev, m, n, k, ldz, ldx);
  else
    train_dgrad<1, 2><<<grid, dim3(256), 0, s>>>(dz_dev, w_dev, dx_dev, m, n, k, ldz, ldx);
  return launched(me, hipGetLastError());
}

extern "C" int c4_train_linear_wgrad_f32(const float* dz_dev, const float* x_dev, float* dw_dev, float* db_dev, uint32_t m, uint32_t n, uint32_t k,
                                         uint32_t ldz, uint32_t ldx, void* stream) {
  const char* me = "c4_train_linear_wgrad_f32";
  if (!dz_dev || !x_dev || !dw_dev || !db_dev) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": null argument");
  if (m == 0) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": m >= 1");
  if (n == 0 || k == 0 || n % 32 || k % 16 || ldz % 4 || ldx % 4 || ldz < n || ldx < k)
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": n % 32 == 0, k % 16 == 0, ldz >= n, ldx >= k, ldz and ldx multiples of 4");
  if (!aligned16(dz_dev) || !aligned16(x_dev) || !aligned16(dw_dev) || !aligned16(db_dev))
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": arrays must be 16-byte aligned");
  if (!below_2_31(m, ldz) || !below_2_31(m, ldx) || !below_2_31(n, k))
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": operands must stay below 2^31 elements");
  C4_ON_STREAM_DEVICE(stream);
  const hipStream_t s = (hipStream_t)stream;
  const uint32_t kt = k % 32 ? 1 : 2;
  const uint64_t tiles = (uint64_t)(n / 32) * (k / (16 * kt));
  const dim3 grid((uint32_t)((tiles + 3) / 4));
  if (kt == 2)
    train_wgrad<2, 2><<<grid, dim3(256), 0, s>>>(dz_dev, x_dev, dw_dev, db_dev, m, n, k, ldz, ldx);
  else
    train_wgrad<2, 1><<<grid, dim3(256), 0, s>>>(dz_dev, x_dev, dw_dev, db_dev, m, n, k, ldz, ldx);
  return launched(me, hipGetLastError());
}
