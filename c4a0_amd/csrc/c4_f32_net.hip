// c4_f32_net.hip -- ConnectFourNet's forward pass for f32 networks (reference src/c4a0/nn.py:64-117, the reference's own
// training and evaluation precision) on gfx950's exact-f32 MFMA, v_mfma_f32_16x16x4_f32.  No bf16 anywhere: f32 planes,
// weights, activations and accumulation.  Any width from 1 to 64 channels (padded to Cp = a multiple of 16), any number of
// residual blocks, any head depth.
//
// Every matrix product is one kernel, f32_gemm: y[m][n] = epilogue(chain(m, n) + bias[n]), where chain(m, n) is ONE fmaf
// chain over k in the order include/c4a0_hip.h documents ("f32 evaluator: summation order").  A wavefront owns a tile of
// 16 NT output columns x 16 MT rows (NT x MT independent accumulators) and walks k in blocks of 16:
//   * lane l (r = l & 15, h = l >> 4) loads ONE float4 per column tile -- weights W[n0 + 16 u + r][kb + 4 h .. 4 h + 3] --
//     and one per row tile -- inputs X[m0 + 16 t + r][kb + 4 h .. 4 h + 3];
//   * MFMA step j (0..3) feeds element j of those float4s, so lane group h supplies k = kb + 4 h + j, and the instruction
//     accumulates its four k in lane-group order h = 0..3: the chain visits k = kb + 4 h + j for j = 0..3, h = 0..3
//     (a 4 x 4 transpose inside each block of 16).
//   * D leaves the MFMA as output column block n0 + 16 u + 4 h .. + 3 of row m0 + 16 t + r: bias, activation and (conv)
//     the residual add happen in registers, one 16-byte store per tile.
// The chain of an element depends on its row and column only: not on the batch, the row's position, the tile shape or
// the launch.  Rows beyond the batch read the last row (in bounds) and are never stored.
//
// The tower is 1 + 2 n_blocks launches of f32_gemm (implicit-GEMM convolutions over cell-major features [G][42][Cp]); the
// heads' hidden layers are f32_gemm on dense rows; the output layers + log-softmax + tanh are f32_head_out.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/c4a0_hip.h"
#include "c4_device.hpp"
#include "c4_host.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

enum { kLinear = 0, kConv = 1, kConv0 = 2 };          // how the B operand (the layer's input) is read
enum { kEpiNone = 0, kEpiRelu = 1, kEpiResidual = 2 };  // s = chain + bias;  s  |  relu(s)  |  y_old + relu(s)

__device__ __forceinline__ float relu(float s) { return s > 0.f ? s : 0.f; }

// One 16-block of the input row `m` for lane group h: elements k = kb + 4 h + e, e = 0..3.
//   kLinear: x[m * ldx + k]
//   kConv:   k = tap * Cp + ci; the neighbour cell (row + tap / 3 - 1, col + tap % 3 - 1) of cell m % 42 of board m / 42, channel ci
//            of x [G][42][Cp] (ldx = Cp), zero outside the board
//   kConv0:  k = 2 tap + ci (k < 18, zero beyond); planes [G][2][6][7]
template <int MODE>
__device__ __forceinline__ f32x4 load_b(const float* __restrict__ x, uint32_t m, uint32_t kb, uint32_t h, uint32_t ldx) {
  if (MODE == kLinear) return *reinterpret_cast<const f32x4*>(x + (size_t)m * ldx + kb + 4 * h);
  const uint32_t board = m / 42, cell = m - board * 42, row = cell / 7, col = cell - row * 7;
  if (MODE == kConv) {
    const uint32_t tap = kb / ldx, ci = kb - tap * ldx + 4 * h;
    const int rr = (int)row + (int)(tap / 3) - 1, cc = (int)col + (int)(tap % 3) - 1;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (rr >= 0 && rr < 6 && cc >= 0 && cc < 7) v = *reinterpret_cast<const f32x4*>(x + ((size_t)board * 42 + rr * 7 + cc) * ldx + ci);
    return v;
  }
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; e++) {
    const uint32_t k = kb + 4 * h + e, tap = k >> 1, ci = k & 1;
    const int rr = (int)row + (int)(tap / 3) - 1, cc = (int)col + (int)(tap % 3) - 1;
    if (k < 18 && rr >= 0 && rr < 6 && cc >= 0 && cc < 7) v[e] = x[(size_t)board * 84 + ci * 42 + rr * 7 + cc];
  }
  return v;
}

// y[m][n] (row stride ldy) for m < n_rows, n < n_cols (a multiple of 16 NT), k < k_len (a multiple of 16); w [n_cols][k_len].
// 256 threads = four independent wavefronts, each one tile.
template <int MODE, int NT, int MT, int EPI>
__global__ __launch_bounds__(256) void f32_gemm(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                float* y, uint32_t n_rows, uint32_t n_cols, uint32_t k_len, uint32_t ldx, uint32_t ldy) {
  const uint32_t lane = threadIdx.x & 63, r = lane & 15, h = lane >> 4;
  const uint32_t n_tiles = n_cols / (16 * NT);
  const uint32_t tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t mt = tile / n_tiles, nt = tile - mt * n_tiles;
  const uint32_t m0 = mt * 16 * MT, n0 = nt * 16 * NT;
  if (m0 >= n_rows) return;                 // a whole wavefront past the last tile (no barrier in this kernel)
  const float* wl[NT];
#pragma unroll
  for (int u = 0; u < NT; u++) wl[u] = w + (size_t)(n0 + 16 * u + r) * k_len + 4 * h;
  uint32_t mrow[MT];
#pragma unroll
  for (int t = 0; t < MT; t++) mrow[t] = min(m0 + 16 * t + r, n_rows - 1);
  f32x4 acc[NT][MT];
#pragma unroll
  for (int u = 0; u < NT; u++)
#pragma unroll
    for (int t = 0; t < MT; t++) acc[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 a[NT], b[MT];
#pragma unroll
  for (int u = 0; u < NT; u++) a[u] = *reinterpret_cast<const f32x4*>(wl[u]);
#pragma unroll
  for (int t = 0; t < MT; t++) b[t] = load_b<MODE>(x, mrow[t], 0, h, ldx);
  for (uint32_t kb = 0; kb < k_len; kb += 16) {
    // the next block's operands are requested before this block's MFMAs (the last iteration re-reads block 0: in bounds, unused)
    const uint32_t kn = kb + 16 < k_len ? kb + 16 : 0;
    f32x4 an[NT], bn[MT];
#pragma unroll
    for (int u = 0; u < NT; u++) an[u] = *reinterpret_cast<const f32x4*>(wl[u] + kn);
#pragma unroll
    for (int t = 0; t < MT; t++) bn[t] = load_b<MODE>(x, mrow[t], kn, h, ldx);
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
      for (int u = 0; u < NT; u++)
#pragma unroll
        for (int t = 0; t < MT; t++) acc[u][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][j], b[t][j], acc[u][t], 0, 0, 0);
#pragma unroll
    for (int u = 0; u < NT; u++) a[u] = an[u];
#pragma unroll
    for (int t = 0; t < MT; t++) b[t] = bn[t];
  }
#pragma unroll
  for (int t = 0; t < MT; t++) {
    const uint32_t m = m0 + 16 * t + r;
    if (m >= n_rows) continue;
#pragma unroll
    for (int u = 0; u < NT; u++) {
      const uint32_t n = n0 + 16 * u + 4 * h;
      const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + n);
      f32x4* dst = reinterpret_cast<f32x4*>(y + (size_t)m * ldy + n);
      f32x4 o;
      if (EPI == kEpiResidual) o = *dst;    // in place: this lane reads and writes these four elements only
#pragma unroll
      for (int e = 0; e < 4; e++) {
        const float s = acc[u][t][e] + bv[e];
        o[e] = EPI == kEpiNone ? s : (EPI == kEpiRelu ? relu(s) : o[e] + relu(s));
      }
      *dst = o;
    }
  }
}

template <int MODE, int NT, int MT, int EPI>
hipError_t launch_gemm(const float* x, const float* w, const float* bias, float* y, uint32_t m, uint32_t n, uint32_t k, uint32_t ldx,
                       uint32_t ldy, hipStream_t stream) {
  const uint64_t tiles = (uint64_t)((m + 16 * MT - 1) / (16 * MT)) * (n / (16 * NT));
  f32_gemm<MODE, NT, MT, EPI><<<dim3((uint32_t)((tiles + 3) / 4)), dim3(256), 0, stream>>>(x, w, bias, y, m, n, k, ldx, ldy);
  return hipGetLastError();
}

// One convolution of the tower: NT = Cp / 16 (a wavefront computes every output channel of its 64 cells).
template <int MODE, int EPI>
hipError_t launch_conv(const float* x, const float* w, const float* bias, float* y, uint32_t cells, uint32_t cp, hipStream_t stream) {
  const uint32_t k = MODE == kConv0 ? 32 : 9 * cp;
  switch (cp) {
    case 16: return launch_gemm<MODE, 1, 4, EPI>(x, w, bias, y, cells, cp, k, cp, cp, stream);
    case 32: return launch_gemm<MODE, 2, 4, EPI>(x, w, bias, y, cells, cp, k, cp, cp, stream);
    case 48: return launch_gemm<MODE, 3, 4, EPI>(x, w, bias, y, cells, cp, k, cp, cp, stream);
    default: return launch_gemm<MODE, 4, 4, EPI>(x, w, bias, y, cells, cp, k, cp, cp, stream);
  }
}

// Output layers of both heads for the 16 rows of one wavefront: policy [7][kp] and value [2][kv] weights as the A operand
// (lanes past the 7 / 2 outputs re-read row 0: their columns of D are independent chains, never read), the hidden rows as
// B; the same chain as f32_gemm.  Then per row: pre-activations
// v = chain + bias, log-softmax in the order of c4_head_out_bf16 with the glibc ports, tanh from the device libm.
__global__ __launch_bounds__(64) void f32_head_out(const float* __restrict__ hp, const float* __restrict__ hv, const float* __restrict__ wp,
                                                   const float* __restrict__ wv, const float* __restrict__ bp, const float* __restrict__ bv,
                                                   uint32_t n_rows, uint32_t kp, uint32_t kv, uint32_t ldp, uint32_t ldv, float* logprobs, float* q,
                                                   float* preact) {
  __shared__ float tile[2][16][17];
  const uint32_t lane = threadIdx.x, r = lane & 15, h = lane >> 4;
  const uint32_t m0 = blockIdx.x * 16, mrow = min(m0 + r, n_rows - 1);
  const float* xp = hp + (size_t)mrow * ldp + 4 * h;
  const float* xv = hv + (size_t)mrow * ldv + 4 * h;
  const float* wpl = wp + (size_t)(r < 7 ? r : 0) * kp + 4 * h;
  const float* wvl = wv + (size_t)(r < 2 ? r : 0) * kv + 4 * h;
  f32x4 accp = {0.f, 0.f, 0.f, 0.f}, accv = {0.f, 0.f, 0.f, 0.f};
  // kDepth blocks of 16 features are requested together (one memory round trip per 16 kDepth features: the two chains alone
  // cannot hide a load's latency); past a head's last block the loads re-read it (in bounds) and its MFMAs are skipped
  constexpr int kDepth = 8;
  const uint32_t k_len = kp > kv ? kp : kv;
  for (uint32_t k0 = 0; k0 < k_len; k0 += 16 * kDepth) {
    f32x4 a_p[kDepth], b_p[kDepth], a_v[kDepth], b_v[kDepth];
#pragma unroll
    for (int i = 0; i < kDepth; i++) {
      const uint32_t kbp = min(k0 + 16 * i, kp - 16), kbv = min(k0 + 16 * i, kv - 16);
      a_p[i] = *reinterpret_cast<const f32x4*>(wpl + kbp);
      b_p[i] = *reinterpret_cast<const f32x4*>(xp + kbp);
      a_v[i] = *reinterpret_cast<const f32x4*>(wvl + kbv);
      b_v[i] = *reinterpret_cast<const f32x4*>(xv + kbv);
    }
#pragma unroll
    for (int i = 0; i < kDepth; i++) {
      const uint32_t kb = k0 + 16 * i;
      if (kb < kp) {
#pragma unroll
        for (int j = 0; j < 4; j++) accp = __builtin_amdgcn_mfma_f32_16x16x4f32(a_p[i][j], b_p[i][j], accp, 0, 0, 0);
      }
      if (kb < kv) {
#pragma unroll
        for (int j = 0; j < 4; j++) accv = __builtin_amdgcn_mfma_f32_16x16x4f32(a_v[i][j], b_v[i][j], accv, 0, 0, 0);
      }
    }
  }
  // lane holds outputs 4 h .. 4 h + 3 of row r
#pragma unroll
  for (int e = 0; e < 4; e++) {
    tile[0][r][4 * h + e] = accp[e];
    tile[1][r][4 * h + e] = accv[e];
  }
  __syncthreads();
  const uint32_t m = m0 + lane;
  if (lane < 16 && m < n_rows) {
    float v[7];
#pragma unroll
    for (int o = 0; o < 7; o++) v[o] = tile[0][lane][o] + bp[o];
    const float v0 = tile[1][lane][0] + bv[0], v1 = tile[1][lane][1] + bv[1];
    float mx = v[0];
#pragma unroll
    for (int o = 1; o < 7; o++) mx = fmaxf(mx, v[o]);
    float sm = 0.f;
#pragma unroll
    for (int o = 0; o < 7; o++) sm += c4::c4_expf(v[o] - mx);
    const float lse = mx + c4::c4_logf(sm);
#pragma unroll
    for (int o = 0; o < 7; o++) logprobs[(size_t)m * 7 + o] = v[o] - lse;
    q[(size_t)m * 2 + 0] = tanhf(v0);
    q[(size_t)m * 2 + 1] = tanhf(v1);
    if (preact) {
#pragma unroll
      for (int o = 0; o < 7; o++) preact[(size_t)m * 9 + o] = v[o];
      preact[(size_t)m * 9 + 7] = v0;
      preact[(size_t)m * 9 + 8] = v1;
    }
  }
}

using c4host::aligned16;
using c4host::launched;

}  // namespace

// The tower's convolution for c4_train_tower.hip: the same launch as c4_conv_tower_f32's (same tiles, same chain), no activation.
hipError_t c4f32::launch_train_conv(bool first, const float* x, const float* w, const float* bias, float* y, uint32_t cells, uint32_t cp,
                                    hipStream_t stream) {
  return first ? launch_conv<kConv0, kEpiNone>(x, w, bias, y, cells, cp, stream) : launch_conv<kConv, kEpiNone>(x, w, bias, y, cells, cp, stream);
}

extern "C" int c4_conv_tower_f32(const float* planes_dev, const float* w0_dev, const float* w_dev, const float* bias_dev, uint32_t n_boards,
                                 uint32_t channels, uint32_t n_blocks, float* out_dev, float* work_dev, void* stream) {
  if (!planes_dev || !w0_dev || !bias_dev || !out_dev || (n_blocks && (!w_dev || !work_dev)))
    return c4host::fail(C4_ERR_BAD_ARG, "c4_conv_tower_f32: null argument");
  if (channels == 0 || channels > 64 || channels % 16)
    return c4host::fail(C4_ERR_BAD_ARG, "c4_conv_tower_f32: channels (padded) must be 16, 32, 48 or 64");
  if (!aligned16(w0_dev) || !aligned16(w_dev) || !aligned16(bias_dev) || !aligned16(out_dev) || !aligned16(work_dev))
    return c4host::fail(C4_ERR_BAD_ARG, "c4_conv_tower_f32: weights, biases, out and work must be 16-byte aligned");
  if ((uint64_t)n_boards * 42 * channels >= (1ull << 31)) return c4host::fail(C4_ERR_BAD_ARG, "c4_conv_tower_f32: n_boards too large");
  if (n_boards == 0) return C4_OK;
  const int device = c4host::stream_device((hipStream_t)stream);
  c4host::DeviceGuard guard(device);
  if (guard.error() != hipSuccess) return c4host::fail(C4_ERR_HIP, std::string("c4_conv_tower_f32: hipSetDevice: ") + hipGetErrorString(guard.error()));
  const hipStream_t s = (hipStream_t)stream;
  const uint32_t cells = n_boards * 42, cp = channels;
  int rc = launched("c4_conv_tower_f32", launch_conv<kConv0, kEpiNone>(planes_dev, w0_dev, bias_dev, out_dev, cells, cp, s));
  for (uint32_t i = 0; i < n_blocks && rc == C4_OK; i++) {
    const float* w1 = w_dev + (size_t)(2 * i) * cp * 9 * cp;
    const float* w2 = w1 + (size_t)cp * 9 * cp;
    rc = launched("c4_conv_tower_f32", launch_conv<kConv, kEpiNone>(out_dev, w1, bias_dev + (1 + 2 * i) * cp, work_dev, cells, cp, s));
    if (rc == C4_OK)
      rc = launched("c4_conv_tower_f32", launch_conv<kConv, kEpiResidual>(work_dev, w2, bias_dev + (2 + 2 * i) * cp, out_dev, cells, cp, s));
  }
  return rc;
}

extern "C" int c4_linear_f32(const float* x_dev, const float* w_dev, const float* bias_dev, float* y_dev, uint32_t m, uint32_t n, uint32_t k,
                             uint32_t ldx, uint32_t ldy, uint32_t relu, void* stream) {
  if (!x_dev || !w_dev || !bias_dev || !y_dev) return c4host::fail(C4_ERR_BAD_ARG, "c4_linear_f32: null argument");
  if (n == 0 || k == 0 || n % 32 || k % 16 || ldx % 4 || ldy % 4 || ldx < k || ldy < n)
    return c4host::fail(C4_ERR_BAD_ARG, "c4_linear_f32: n % 32 == 0, k % 16 == 0, ldx >= k, ldy >= n, ldx and ldy multiples of 4");
  if (!aligned16(x_dev) || !aligned16(w_dev) || !aligned16(bias_dev) || !aligned16(y_dev))
    return c4host::fail(C4_ERR_BAD_ARG, "c4_linear_f32: arrays must be 16-byte aligned");
  if ((uint64_t)m * ldx >= (1ull << 31) || (uint64_t)m * ldy >= (1ull << 31) || (uint64_t)n * k >= (1ull << 31))
    return c4host::fail(C4_ERR_BAD_ARG, "c4_linear_f32: operands must stay below 2^31 elements");
  if (m == 0) return C4_OK;
  const int device = c4host::stream_device((hipStream_t)stream);
  c4host::DeviceGuard guard(device);
  if (guard.error() != hipSuccess) return c4host::fail(C4_ERR_HIP, std::string("c4_linear_f32: hipSetDevice: ") + hipGetErrorString(guard.error()));
  const hipStream_t s = (hipStream_t)stream;
  // 32 x 64 tiles; up to 2 048 rows 32 x 32 (twice the wavefronts for the CUs).  Both compute the same bits.
  hipError_t e;
  if (m > 2048)
    e = relu ? launch_gemm<kLinear, 2, 4, kEpiRelu>(x_dev, w_dev, bias_dev, y_dev, m, n, k, ldx, ldy, s)
             : launch_gemm<kLinear, 2, 4, kEpiNone>(x_dev, w_dev, bias_dev, y_dev, m, n, k, ldx, ldy, s);
  else
    e = relu ? launch_gemm<kLinear, 2, 2, kEpiRelu>(x_dev, w_dev, bias_dev, y_dev, m, n, k, ldx, ldy, s)
             : launch_gemm<kLinear, 2, 2, kEpiNone>(x_dev, w_dev, bias_dev, y_dev, m, n, k, ldx, ldy, s);
  return launched("c4_linear_f32", e);
}

extern "C" int c4_head_out_f32(const float* hidden_policy_dev, const float* hidden_value_dev, const float* w_policy_dev, const float* w_value_dev,
                               const float* b_policy_dev, const float* b_value_dev, uint32_t n_boards, uint32_t policy_features,
                               uint32_t value_features, uint32_t policy_row_stride, uint32_t value_row_stride, float* logprobs, float* q,
                               float* preact, void* stream) {
  if (!hidden_policy_dev || !hidden_value_dev || !w_policy_dev || !w_value_dev || !b_policy_dev || !b_value_dev || !logprobs || !q)
    return c4host::fail(C4_ERR_BAD_ARG, "c4_head_out_f32: null argument");
  if (policy_features == 0 || value_features == 0 || policy_features % 16 || value_features % 16 || policy_row_stride % 4 ||
      value_row_stride % 4 || policy_row_stride < policy_features || value_row_stride < value_features)
    return c4host::fail(C4_ERR_BAD_ARG, "c4_head_out_f32: features multiples of 16, row strides multiples of 4 and >= features");
  if (!aligned16(hidden_policy_dev) || !aligned16(hidden_value_dev) || !aligned16(w_policy_dev) || !aligned16(w_value_dev))
    return c4host::fail(C4_ERR_BAD_ARG, "c4_head_out_f32: hidden rows and weights must be 16-byte aligned");
  if ((uint64_t)n_boards * policy_row_stride >= (1ull << 31) || (uint64_t)n_boards * value_row_stride >= (1ull << 31))
    return c4host::fail(C4_ERR_BAD_ARG, "c4_head_out_f32: operands must stay below 2^31 elements");
  if (n_boards == 0) return C4_OK;
  const int device = c4host::stream_device((hipStream_t)stream);
  c4host::DeviceGuard guard(device);
  if (guard.error() != hipSuccess) return c4host::fail(C4_ERR_HIP, std::string("c4_head_out_f32: hipSetDevice: ") + hipGetErrorString(guard.error()));
  f32_head_out<<<dim3((n_boards + 15) / 16), dim3(64), 0, (hipStream_t)stream>>>(
      hidden_policy_dev, hidden_value_dev, w_policy_dev, w_value_dev, b_policy_dev, b_value_dev, n_boards, policy_features, value_features,
      policy_row_stride, value_row_stride, logprobs, q, preact);
  return launched("c4_head_out_f32", hipGetLastError());
}
