// c4_fp8_gemm.hip -- the opt-in FP8 form of the heads' hidden layers (include/c4a0_hip.h, "fp8 hidden layers": the numerics
// contract) for gfx950:
//
//     Y[M, N] = out(act(acc[M, N] * dq[N] + bias[N])),   acc = X8[M, K] . W8[N, K]^T in f32
//
// X8 and W8 are OCP e4m3fn bytes, dq and bias f32, Y either e4m3fn (q8(r * out_scale)) or bf16.  One v_mfma_f32_16x16x128_f8f6f4
// (e4m3 x e4m3, no block scales: the scale operands are literal zeros) per 128-deep k-step -- twice the MACs per clock of the bf16
// MFMA -- k-steps ascending, no split-K, no atomics: an output element is ONE fixed chain whatever M, the row or `config`.
//
// Mapping, as in c4_head_gemm.hip: D[n][m] = sum_k W[n][k] X[m][k], the weights are the MFMA's A operand, so a lane ends with 4
// consecutive features of one board: one 4-byte fp8 store or one 8-byte bf16 store.
//
// Operand lane map of the 16x16x128 form: lane l holds row l & 15 and 32 bytes of the row's 128-byte k-step.  WHICH 32 bytes a lane
// holds does not change the dot product as long as A and B are loaded the same way (they share the map), so every kernel here
// gives lane group g = l >> 4 the 16-byte pieces g and 4 + g of the k-step (registers 0-3 and 4-7): the one assignment under
// which c4_head_gemm.hip's XOR-swizzled LDS image is read without bank conflicts.  ONE assignment for all kernels: the MFMA's own
// order of the 128 products is then the same in every configuration, and so are the bits.
//
// Two forms, same bits:
//   * LDS (configs 3, 4; the automatic choice): a 128 x 192 (or 64 x 192) tile on four wavefronts, 64 (32) x 96 each.  A k-step of
//     both operands ((BM + 192) rows of 128 bytes) goes global -> registers -> LDS (ds_write_b128; piece g of row r in slot
//     g ^ (r & 7)) into a two-stage ring: k-step kt + 2 is in flight to registers and k-step kt + 1 is written to the other stage
//     while k-step kt is multiplied; one barrier per k-step.
//   * direct (configs 1, 2: 64- and 128-row tiles; kept as measured alternatives): no LDS, a wavefront reads its fragments straight
//     from global memory one k-step ahead; bound by the CU's vector cache.
//
// K % 128 == 64 (K = 1 344: 10.5 k-steps): in the last step pieces 4-7 hold k >= K.  They are ZEROS made in registers (the LDS form
// writes those zeros into its stage) and their loads are not issued past column K (the address is pulled back into the row):
// nothing at or beyond column k of a row is read, so neither a NaN byte behind a column view nor the end of an allocation can matter.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/c4a0_hip.h"
#include "c4_host.hpp"

#pragma clang fp contract(off)

namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// q8 of four f32 values, packed low byte first.  The clamp is an explicit f32 operation in front of the convert (no mode bit decides
// what an overflow becomes) and a NaN is selected by hand: fminf / fmaxf would launder it into a finite value.
__device__ __forceinline__ uint32_t q8x4(float v0, float v1, float v2, float v3) {
  const float c0 = fminf(fmaxf(v0, -448.f), 448.f), c1 = fminf(fmaxf(v1, -448.f), 448.f);
  const float c2 = fminf(fmaxf(v2, -448.f), 448.f), c3 = fminf(fmaxf(v3, -448.f), 448.f);
  int p = __builtin_amdgcn_cvt_pk_fp8_f32(c0, c1, 0, false);
  p = __builtin_amdgcn_cvt_pk_fp8_f32(c2, c3, p, true);
  uint32_t u = (uint32_t)p;
  if (v0 != v0) u = (u & 0xFFFFFF00u) | 0x0000007Fu;
  if (v1 != v1) u = (u & 0xFFFF00FFu) | 0x00007F00u;
  if (v2 != v2) u = (u & 0xFF00FFFFu) | 0x007F0000u;
  if (v3 != v3) u = (u & 0x00FFFFFFu) | 0x7F000000u;
  return u;
}

// relu that keeps a NaN (the tree kernels' C4_ERR_NAN_IN_TREE needs it to survive the evaluator) and turns -0 into +0
__device__ __forceinline__ float relu_keep_nan(float v) { return v <= 0.f ? 0.f : v; }

// ---- bf16 [m][ldx] -> e4m3 [m][ldy]: y = q8(x * scale).  One thread per 8 elements: a 16-byte load, an 8-byte store.
__global__ __launch_bounds__(256) void c4_quantize_bf16_fp8_kernel(const uint16_t* __restrict__ x, uint8_t* __restrict__ y, uint32_t m, uint32_t k8,
                                                                   uint32_t ldx, uint32_t ldy, float scale) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)m * k8) return;
  const uint32_t row = (uint32_t)(i / k8), c = (uint32_t)(i % k8);
  const uint4 in = *reinterpret_cast<const uint4*>(x + (size_t)row * ldx + 8u * c);
  const uint32_t wds[4] = {in.x, in.y, in.z, in.w};
  float v[8];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    v[2 * j] = __uint_as_float(wds[j] << 16) * scale;
    v[2 * j + 1] = __uint_as_float(wds[j] & 0xFFFF0000u) * scale;
  }
  uint2 out;
  out.x = q8x4(v[0], v[1], v[2], v[3]);
  out.y = q8x4(v[4], v[5], v[6], v[7]);
  *reinterpret_cast<uint2*>(y + (size_t)row * ldy + 8u * c) = out;
}

// ---- epilogue shared by both forms: the lane holds features n0 + 16 a + 4 lg + {0..3} of board m0 + 16 b + li (C/D map: row =
// 4 (lane >> 4) + reg, col = lane & 15)
template <int TM_, int TN_>
__device__ __forceinline__ void fp8_epilogue(const f32x4 (&acc)[TN_][TM_], const float* __restrict__ dq, const float* __restrict__ bias, void* __restrict__ y,
                                             uint32_t M, uint32_t ldy, bool relu, bool out_fp8, float out_scale, int m0, int n0, int li, int lg) {
#pragma unroll
  for (int a = 0; a < TN_; a++) {
    const int n = n0 + 16 * a + 4 * lg;
    const f32x4 dq4 = *reinterpret_cast<const f32x4*>(dq + n), b4 = *reinterpret_cast<const f32x4*>(bias + n);
#pragma unroll
    for (int b = 0; b < TM_; b++) {
      const int mrow = m0 + 16 * b + li;
      float r[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float v = acc[a][b][j] * dq4[j] + b4[j];           // an exact multiply (a power of two), one rounding in the add
        r[j] = relu ? relu_keep_nan(v) : v;
      }
      if (mrow < (int)M) {
        if (out_fp8) {
          *reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(y) + (size_t)mrow * ldy + n) =
              q8x4(r[0] * out_scale, r[1] * out_scale, r[2] * out_scale, r[3] * out_scale);
        } else {
          const f32x4 rv = {r[0], r[1], r[2], r[3]};
          *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(y) + (size_t)mrow * ldy + n) = __builtin_bit_cast(uint2, __builtin_convertvector(rv, bf16x4));
        }
      }
    }
  }
}

// ---- the GEMM, direct form.  A workgroup is four wavefronts side by side along N: 16 TM rows x 192 features, 48 features per wavefront.
constexpr int TN = 3;

template <int TM>
__global__ __launch_bounds__(256) void c4_fp8_gemm_kernel(const uint8_t* __restrict__ x, const uint8_t* __restrict__ w, const float* __restrict__ dq,
                                                          const float* __restrict__ bias, void* __restrict__ y, uint32_t M, uint32_t K, uint32_t ldx,
                                                          uint32_t ldy, uint32_t flags, float out_scale) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int n0 = (int)blockIdx.x * 192 + wave * 48, m0 = (int)blockIdx.y * (16 * TM);
  const bool relu = flags & 1u, out_fp8 = flags & 2u;

  // row bases of this lane's fragments; rows past the end re-read the last one (never stored)
  const uint8_t* xrow[TM];
  const uint8_t* wrow[TN];
#pragma unroll
  for (int b = 0; b < TM; b++) {
    int r = m0 + 16 * b + li;
    r = r < (int)M ? r : (int)M - 1;
    xrow[b] = x + (size_t)r * ldx;
  }
#pragma unroll
  for (int a = 0; a < TN; a++) wrow[a] = w + (size_t)(n0 + 16 * a + li) * K;

  const int KT = ((int)K + 127) / 128;
  // this lane's pieces lg and 4 + lg of k-step kt of a row -- the second one zeros, made here, where it lies at or beyond column K
  auto frag = [&](const uint8_t* row, int kt) __attribute__((always_inline)) {
    const uint32_t col = (uint32_t)kt * 128u + 16u * (uint32_t)lg;
    const bool valid = col + 64u < K;                            // K % 64 == 0: the upper half of a k-step is all below K or all beyond
    const uint4 lo = *reinterpret_cast<const uint4*>(row + col);
    uint4 hi = *reinterpret_cast<const uint4*>(row + (valid ? col + 64u : col));
    if (!valid) hi = uint4{0u, 0u, 0u, 0u};
    return i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
  };

  f32x4 acc[TN][TM];
#pragma unroll
  for (int a = 0; a < TN; a++)
#pragma unroll
    for (int b = 0; b < TM; b++) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  i32x8 afr[TN], bfr[TM], afn[TN], bfn[TM];
#pragma unroll
  for (int b = 0; b < TM; b++) bfr[b] = frag(xrow[b], 0);
#pragma unroll
  for (int a = 0; a < TN; a++) afr[a] = frag(wrow[a], 0);
  for (int kt = 0; kt < KT; kt++) {
    const int nk = kt + 1 < KT ? kt + 1 : kt;                    // (the last step re-reads itself: no branch around the loads)
#pragma unroll
    for (int b = 0; b < TM; b++) bfn[b] = frag(xrow[b], nk);
#pragma unroll
    for (int a = 0; a < TN; a++) afn[a] = frag(wrow[a], nk);
#pragma unroll
    for (int a = 0; a < TN; a++)
#pragma unroll
      for (int b = 0; b < TM; b++)
        acc[a][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(afr[a], bfr[b], acc[a][b], 0, 0, 0, 0, 0, 0);
#pragma unroll
    for (int b = 0; b < TM; b++) bfr[b] = bfn[b];
#pragma unroll
    for (int a = 0; a < TN; a++) afr[a] = afn[a];
  }

  fp8_epilogue<TM, TN>(acc, dq, bias, y, M, ldy, relu, out_fp8, out_scale, m0, n0, li, lg);
}

// ---- the GEMM, LDS form: BM x 192 tile, four wavefronts as 2 x 2, (BM / 2) x 96 each; see the head of the file.
template <int BM>
__global__ __launch_bounds__(256, 2) void c4_fp8_gemm_lds_kernel(const uint8_t* __restrict__ x, const uint8_t* __restrict__ w, const float* __restrict__ dq,
                                                                 const float* __restrict__ bias, void* __restrict__ y, uint32_t M, uint32_t K, uint32_t ldx,
                                                                 uint32_t ldy, uint32_t flags, float out_scale) {
  constexpr int BN = 192, ROWS = BM + BN, STAGE = ROWS * 128;
  constexpr int L = ROWS * 8 / 256;                              // 16-byte pieces per thread and k-step: piece tid + 256 i
  constexpr int LX = BM * 8 / 256;                               // ... of which the first LX are rows of X, the others rows of W
  constexpr int LTM = BM / 2 / 16, LTN = 6;
  extern __shared__ __attribute__((aligned(1024))) uint8_t fp8_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4, wm = wave & 1, wn = wave >> 1;
  const int n0 = (int)blockIdx.x * BN, m0 = (int)blockIdx.y * BM;

  // staging: piece tid + 256 i is row (tid >> 3) + 32 i of the stage, 16-byte piece g = tid & 7 of that row's k-step
  const int g = tid & 7, r0 = tid >> 3;
  uint32_t src[L], dst[L];
#pragma unroll
  for (int i = 0; i < L; i++) {
    const int row = r0 + 32 * i;
    if (i < LX) {
      int gr = m0 + row;
      gr = gr < (int)M ? gr : (int)M - 1;                         // rows past the end re-read the last one (never stored)
      src[i] = (uint32_t)gr * ldx;
    } else {
      src[i] = (uint32_t)(n0 + row - BM) * K;
    }
    dst[i] = (uint32_t)row * 128u + (uint32_t)((g ^ (row & 7)) * 16);
  }
  auto gload = [&](int kt, uint4 (&r)[L]) __attribute__((always_inline)) {
    const uint32_t col = (uint32_t)kt * 128u + 16u * (uint32_t)g;
    const bool valid = col < K;                                  // K % 64 == 0 and pieces are 16 bytes: all below K or all beyond
    const uint32_t c = valid ? col : 0u;                         // (nothing at or beyond column K is read)
#pragma unroll
    for (int i = 0; i < L; i++) {
      r[i] = *reinterpret_cast<const uint4*>((i < LX ? x : w) + (size_t)src[i] + c);
      if (!valid) r[i] = uint4{0u, 0u, 0u, 0u};
    }
  };
  auto lstore = [&](int stage, const uint4 (&r)[L]) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < L; i++) *reinterpret_cast<uint4*>(fp8_lds + stage * STAGE + dst[i]) = r[i];
  };
  auto publish = [&]() __attribute__((always_inline)) {          // my LDS traffic is done; then everybody's is
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  };

  f32x4 acc[LTN][LTM];
#pragma unroll
  for (int a = 0; a < LTN; a++)
#pragma unroll
    for (int b = 0; b < LTM; b++) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fragment reads: row = tile base (a multiple of 16) + li, so row & 7 == li & 7; lane group lg holds pieces lg and 4 + lg
  const uint32_t off_lo = (uint32_t)li * 128u + (uint32_t)((lg ^ (li & 7)) * 16), off_hi = (uint32_t)li * 128u + (uint32_t)(((4 + lg) ^ (li & 7)) * 16);
  const uint32_t x_base = (uint32_t)(wm * (BM / 2)) * 128u, w_base = (uint32_t)(BM + wn * 96) * 128u;
  auto frag = [&](const uint8_t* st, uint32_t base, int t) __attribute__((always_inline)) {
    const uint4 lo = *reinterpret_cast<const uint4*>(st + base + t * 2048 + off_lo), hi = *reinterpret_cast<const uint4*>(st + base + t * 2048 + off_hi);
    return i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
  };

  const int KT = ((int)K + 127) / 128;
  uint4 r[L];
  gload(0, r);
  lstore(0, r);
  if (KT > 1) gload(1, r);
  publish();
  for (int kt = 0; kt < KT; kt++) {
    const int st = kt & 1;
    if (kt + 1 < KT) lstore(st ^ 1, r);                           // k-step kt + 1: the stage everybody left before the last barrier
    if (kt + 2 < KT) gload(kt + 2, r);
    const uint8_t* sp = fp8_lds + st * STAGE;
    i32x8 bfr[LTM];
#pragma unroll
    for (int b = 0; b < LTM; b++) bfr[b] = frag(sp, x_base, b);
#pragma unroll
    for (int a = 0; a < LTN; a++) {
      const i32x8 afr = frag(sp, w_base, a);
#pragma unroll
      for (int b = 0; b < LTM; b++)
        acc[a][b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(afr, bfr[b], acc[a][b], 0, 0, 0, 0, 0, 0);
    }
    publish();
  }
  fp8_epilogue<LTM, LTN>(acc, dq, bias, y, M, ldy, flags & 1u, flags & 2u, out_scale, m0 + wm * (BM / 2), n0 + wn * 96, li, lg);
}

template <int BM>
int launch_fp8_gemm_lds(const void* x, const void* w, const float* dq, const float* bias, void* y, uint32_t m, uint32_t n, uint32_t k, uint32_t ldx,
                        uint32_t ldy, uint32_t flags, float out_scale, hipStream_t st, int device) {
  constexpr int kLds = 2 * (BM + 192) * 128;
  HIP_TRY(c4host::opt_in_lds(reinterpret_cast<const void*>(&c4_fp8_gemm_lds_kernel<BM>), kLds, device));
  const dim3 grid(n / 192, (m + BM - 1) / BM);
  c4_fp8_gemm_lds_kernel<BM><<<grid, dim3(256), kLds, st>>>((const uint8_t*)x, (const uint8_t*)w, dq, bias, y, m, k, ldx, ldy, flags, out_scale);
  HIP_TRY(hipGetLastError());
  return C4_OK;
}

template <int TM>
int launch_fp8_gemm(const void* x, const void* w, const float* dq, const float* bias, void* y, uint32_t m, uint32_t n, uint32_t k, uint32_t ldx,
                    uint32_t ldy, uint32_t flags, float out_scale, hipStream_t st) {
  const dim3 grid(n / 192, (m + 16 * TM - 1) / (16 * TM));
  c4_fp8_gemm_kernel<TM><<<grid, dim3(256), 0, st>>>((const uint8_t*)x, (const uint8_t*)w, dq, bias, y, m, k, ldx, ldy, flags, out_scale);
  HIP_TRY(hipGetLastError());
  return C4_OK;
}

}  // namespace

extern "C" int c4_quantize_bf16_fp8(const void* x_dev, void* y_dev, uint32_t m, uint32_t k, uint32_t ldx, uint32_t ldy, float scale, void* stream) {
  if (!x_dev || !y_dev) return c4host::fail(C4_ERR_BAD_ARG, "c4_quantize_bf16_fp8: null argument");
  if (k == 0 || k % 8) return c4host::fail(C4_ERR_BAD_ARG, "c4_quantize_bf16_fp8: k must be a positive multiple of 8");
  if (ldx < k || ldy < k || ldx % 8 || ldy % 8 || ((uintptr_t)x_dev & 15) || ((uintptr_t)y_dev & 7))
    return c4host::fail(C4_ERR_BAD_ARG, "c4_quantize_bf16_fp8: row strides must cover a row and be multiples of 8; x 16-byte, y 8-byte aligned");
  if (!(scale > 0.f) || !(scale < __builtin_inff())) return c4host::fail(C4_ERR_BAD_ARG, "c4_quantize_bf16_fp8: scale must be positive and finite (a power of two)");
  if (m == 0) return C4_OK;
  C4_ON_STREAM_DEVICE(stream);
  const uint64_t n_threads = (uint64_t)m * (k / 8);
  if (n_threads > 0x7FFFFFFFull * 256ull) return c4host::fail(C4_ERR_BAD_ARG, "c4_quantize_bf16_fp8: too many elements for one launch");
  c4_quantize_bf16_fp8_kernel<<<c4host::grid_for(n_threads), dim3(256), 0, (hipStream_t)stream>>>((const uint16_t*)x_dev, (uint8_t*)y_dev, m, k / 8, ldx, ldy,
                                                                                                 scale);
  HIP_TRY(hipGetLastError());
  return C4_OK;
}

extern "C" int c4_linear_fp8(const void* x8_dev, const void* w8_dev, const float* dq_dev, const float* bias_dev, void* y_dev, uint32_t m, uint32_t n,
                             uint32_t k, uint32_t ldx, uint32_t ldy, uint32_t relu, uint32_t out_fp8, float out_scale, uint32_t config, void* stream) {
  if (!x8_dev || !w8_dev || !dq_dev || !bias_dev || !y_dev) return c4host::fail(C4_ERR_BAD_ARG, "c4_linear_fp8: null argument");
  if (k == 0 || k % 64) return c4host::fail(C4_ERR_BAD_ARG, "c4_linear_fp8: K must be a positive multiple of 64");
  if (n == 0 || n % 192) return c4host::fail(C4_ERR_BAD_ARG, "c4_linear_fp8: N must be a positive multiple of 192 (42 x C features, C a multiple of 32)");
  if (ldx < k || ldx % 16 || ((uintptr_t)x8_dev & 15) || ((uintptr_t)w8_dev & 15))
    return c4host::fail(C4_ERR_BAD_ARG, "c4_linear_fp8: ldx must cover a row and be a multiple of 16; x8 and w8 16-byte aligned (rows are read 16 bytes at a time)");
  if (ldy < n || ldy % 4 || ((uintptr_t)y_dev & (out_fp8 ? 3 : 7)))
    return c4host::fail(C4_ERR_BAD_ARG, "c4_linear_fp8: ldy must cover a row and be a multiple of 4; y 4-byte (fp8) or 8-byte (bf16) aligned");
  if (((uintptr_t)dq_dev & 15) || ((uintptr_t)bias_dev & 15)) return c4host::fail(C4_ERR_BAD_ARG, "c4_linear_fp8: dq and bias must be 16-byte aligned");
  if (out_fp8 && (!(out_scale > 0.f) || !(out_scale < __builtin_inff())))
    return c4host::fail(C4_ERR_BAD_ARG, "c4_linear_fp8: out_scale must be positive and finite (a power of two) for fp8 output");
  if (config > 4) return c4host::fail(C4_ERR_BAD_ARG, "c4_linear_fp8: unknown config (0 = automatic; 1 / 2 = direct form, 64- / 128-row tiles; 3 / 4 = LDS form, 128 / 64 x 192 tiles)");
  if ((m + 63) / 64 > 65535u) return c4host::fail(C4_ERR_BAD_ARG, "c4_linear_fp8: m too large (more than 65 535 row tiles)");
  if ((uint64_t)m * ldx >= (1ull << 32) || (uint64_t)n * k >= (1ull << 32)) return c4host::fail(C4_ERR_BAD_ARG, "c4_linear_fp8: operands are addressed with 32-bit row offsets (< 4 GiB each)");
  if (m == 0) return C4_OK;
  const int device = c4host::stream_device((hipStream_t)stream);
  C4_ON_DEVICE(device);
  const uint32_t flags = (relu ? 1u : 0u) | (out_fp8 ? 2u : 0u);
  // automatic: the LDS form; 128 x 192 tiles once they give each of the chip's 256 CUs a workgroup, else 64 x 192 tiles, of which a CU
  // holds two (measured at 2 048 rows, profiles/fp8_heads.json: 224 tiles of 128 rows take 21.7 / 30.7 us where 448 of 64 rows take
  // 19.0 / 27.9; 448 of 128 rows 40.6 where 896 of 64 rows take 51.7).  All the same bits.
  if (config == 0) config = (uint64_t)((m + 127) / 128) * (n / 192) >= 256 ? 3 : 4;
  hipStream_t st = (hipStream_t)stream;
  switch (config) {
    case 1: return launch_fp8_gemm<4>(x8_dev, w8_dev, dq_dev, bias_dev, y_dev, m, n, k, ldx, ldy, flags, out_scale, st);
    case 2: return launch_fp8_gemm<8>(x8_dev, w8_dev, dq_dev, bias_dev, y_dev, m, n, k, ldx, ldy, flags, out_scale, st);
    case 3: return launch_fp8_gemm_lds<128>(x8_dev, w8_dev, dq_dev, bias_dev, y_dev, m, n, k, ldx, ldy, flags, out_scale, st, device);
    default: return launch_fp8_gemm_lds<64>(x8_dev, w8_dev, dq_dev, bias_dev, y_dev, m, n, k, ldx, ldy, flags, out_scale, st, device);
  }
}
