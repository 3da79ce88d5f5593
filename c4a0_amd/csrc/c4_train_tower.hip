// c4_train_tower.hip -- training kernels for the convolution tower (Conv2d(2, C) and per block Conv2d(C, C) -> Conv2d(C, C) ->
// BatchNorm2d in train mode -> ReLU, plus the block's input; reference src/c4a0/nn.py:64-70, 184-195), f32 throughout, on gfx950's
// exact-f32 MFMA v_mfma_f32_16x16x4_f32.  Activations are cell-major [B][42][C], i.e. a row-major matrix [42 B][C]; C is 16, 32, 48 or 64.
//
//   conv forward / dgrad   c4_f32_net.hip's f32_gemm<kConv0 | kConv, NT, 4, kEpiNone> (c4f32::launch_train_conv): nothing new here
//   tower_wgrad_partial    per chunk of rows, dW[co][k] = sum_row dz[row][co] X[row][k] and db[co] = sum_row dz[row][co], X the implicit
//                          im2col row that f32_gemm's load_b reads (zero off the board; the first convolution's k >= 18 are zero columns)
//   tower_chunk_reduce     the chunks' partial results added in a fixed order
//   bn2d_*                 batch mean, biased variance, y = a + relu(bn(z)) and its backward over the 42 B rows, three launches each way:
//                          every reduction is per chunk first, and the launch that needs a total adds the chunks' partial sums itself
//
// A chunk is kChunkBoards = 16 whole boards = 672 rows (42 MFMA blocks of 16 rows), the last chunk what is left: the split depends on
// B alone.  Every sum has one order that (B, C) decides and nothing is accumulated with atomics; the orders are include/c4a0_hip.h's
// "training the convolution tower".  The MFMA operand map is train_wgrad's (c4_train.hip): from lane (r = l & 15, h = l >> 4) step j of a
// block of 16 rows takes A = X[mb + 4 j + h][k0 + r] and B = dz[mb + 4 j + h][n0 + r]; D[4 h + e][r] is dW[n0 + r][k0 + 4 h + e].  Rows past
// the chunk and cells off the board are fed as selected zeros (their addresses are replaced by an address inside the arrays), never as
// products with zero, so a NaN next to the data cannot enter a sum.
// The batch-norm arithmetic is c4_train.hip's: two-pass variance, the corrected deviations of the backward, ReLU's predicate
// !(pre <= 0) so that a NaN passes, and a non-finite column stays in its column.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/c4a0_hip.h"
#include "c4_host.hpp"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kChunkBoards = C4_TRAIN_TOWER_CHUNK_BOARDS, kChunkRows = 42 * kChunkBoards;
constexpr uint32_t kReduceGroups = 8;   // tower_chunk_reduce: chunk groups per element

// ---------------------------------------------------------------------------------------------------------------- wgrad
// One wavefront: chunk `wave / k_tiles`, columns k0 .. k0 + 16 KT of X, all C = 16 NT output channels.  FIRST: the first convolution
// (X from planes [B][2][6][7], k = 2 tap + ci, K = 32 of which 18 are live), else a 3x3 convolution of x [42 B][C] (k = tap C + ci, K = 9 C).
// part [n_chunks][C K + C]: the chunk's dW [C][K], then its db [C] (written by the wavefront of the first column tile).
template <bool FIRST, int NT, int KT>
__global__ __launch_bounds__(256) void tower_wgrad_partial(const float* __restrict__ dz, const float* __restrict__ x, float* __restrict__ part,
                                                           uint32_t m, uint32_t n_chunks) {
  constexpr uint32_t C = 16 * NT, K = FIRST ? 32 : 9 * C, k_tiles = K / (16 * KT);
  const uint32_t lane = threadIdx.x & 63, r = lane & 15, h = lane >> 4;
  const uint32_t wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t chunk = wave / k_tiles, kt = wave - chunk * k_tiles;
  if (chunk >= n_chunks) return;   // a whole wavefront past the last tile (no barrier in this kernel)
  const uint32_t row0 = chunk * kChunkRows, row1 = min(m, row0 + kChunkRows), k0 = kt * 16 * KT;
  // this lane's columns of X: the tap's offset on the board and where the channel lies
  int dr[KT], dc[KT];
  uint32_t off[KT];
  bool live[KT];
#pragma unroll
  for (int t = 0; t < KT; t++) {
    const uint32_t k = k0 + 16 * t + r;
    const uint32_t tap = FIRST ? k >> 1 : k / C;
    off[t] = FIRST ? (k & 1) * 42 : k - tap * C;
    live[t] = FIRST ? k < 18 : true;
    dr[t] = (int)(tap / 3) - 1;
    dc[t] = (int)(tap % 3) - 1;
  }
  f32x4 acc[NT][KT];
#pragma unroll
  for (int u = 0; u < NT; u++)
#pragma unroll
    for (int t = 0; t < KT; t++) acc[u][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  float sdb[NT];
#pragma unroll
  for (int u = 0; u < NT; u++) sdb[u] = 0.f;
  float a[4][KT], b[4][NT];
  auto load = [&](uint32_t mb, float (&aa)[4][KT], float (&bb)[4][NT]) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const uint32_t row = mb + 4 * j + h;
      const bool in = row < row1;
      const uint32_t rs = in ? row : row0;   // row0 < m: in bounds
      const uint32_t board = rs / 42, cell = rs - board * 42, rr = cell / 7, cc = cell - rr * 7;
#pragma unroll
      for (int t = 0; t < KT; t++) {
        const int r2 = (int)rr + dr[t], c2 = (int)cc + dc[t];
        const bool ok = in && live[t] && r2 >= 0 && r2 < 6 && c2 >= 0 && c2 < 7;
        const size_t at = FIRST ? (size_t)board * 84 + off[t] + (uint32_t)(r2 * 7 + c2) : ((size_t)board * 42 + (uint32_t)(r2 * 7 + c2)) * C + off[t];
        const float v = x[ok ? at : 0];
        aa[j][t] = ok ? v : 0.f;
      }
#pragma unroll
      for (int u = 0; u < NT; u++) {
        const float v = dz[(size_t)rs * C + 16 * u + r];
        bb[j][u] = in ? v : 0.f;
      }
    }
  };
  load(row0, a, b);
  for (uint32_t mb = row0; mb < row1; mb += 16) {
    // the next block's operands are requested before this block's MFMAs (the last iteration re-reads the first block: in bounds, unused)
    float an[4][KT], bn[4][NT];
    load(mb + 16 < row1 ? mb + 16 : row0, an, bn);
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
  float* pw = part + (size_t)chunk * (C * K + C);
#pragma unroll
  for (int u = 0; u < NT; u++) {
#pragma unroll
    for (int t = 0; t < KT; t++) *reinterpret_cast<f32x4*>(pw + (size_t)(16 * u + r) * K + k0 + 16 * t + 4 * h) = acc[u][t];
    if (kt == 0) {   // uniform over the wavefront
      const float p = sdb[u] + __shfl_xor(sdb[u], 16);
      const float q = p + __shfl_xor(p, 32);
      if (h == 0) pw[C * K + 16 * u + r] = q;
    }
  }
}

// out[e] for four elements a thread: chunk group g adds the chunks g, g + 8, .. in order starting from its first chunk, then the groups'
// sums are added in order g = 0 .. min(8, n_chunks) - 1 (one chunk: its partial result as it is).  part [n_chunks][elems]; elements
// below w_elems go to dw, the others to db.  32 threads per group, 8 groups a workgroup.
__global__ __launch_bounds__(256) void tower_chunk_reduce(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db,
                                                          uint32_t n_chunks, uint32_t elems, uint32_t w_elems) {
  __shared__ f32x4 red[kReduceGroups][32];
  const uint32_t q = threadIdx.x & 31, g = threadIdx.x >> 5;
  const uint32_t e = (blockIdx.x * 32 + q) * 4;
  const bool live = e < elems && g < n_chunks;
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    s = *reinterpret_cast<const f32x4*>(part + (size_t)g * elems + e);
    for (uint32_t c = g + kReduceGroups; c < n_chunks; c += kReduceGroups) s += *reinterpret_cast<const f32x4*>(part + (size_t)c * elems + e);
  }
  red[g][q] = s;
  __syncthreads();
  if (g == 0 && live) {
    f32x4 t = red[0][q];
    const uint32_t groups = min(kReduceGroups, n_chunks);
    for (uint32_t i = 1; i < groups; i++) t += red[i][q];
    *reinterpret_cast<f32x4*>(e < w_elems ? dw + e : db + (e - w_elems)) = t;
  }
}

// ---------------------------------------------------------------------------------------------------------------- batch norm
// A workgroup is CQ = C / 4 column quads x RG = 256 / CQ (rounded down) row groups; thread (cq, rg) owns columns 4 cq .. 4 cq + 3.
// A reduction over the rows [row0, row1) of a matrix: every thread starts from +0 and adds f(row) for its rows row0 + rg, row0 + rg + RG,
// .. in order; then the RG sums G are added as a tree, for half = 32, 16, 8, 4, 2, 1: G[rg] += G[rg + half] for every rg < half with
// rg + half < RG, and the result is G[0] (RG <= 64).  Every thread of a column quad returns the same value.  (The tree, not a chain over
// the groups: 42 rows over 32 groups are otherwise one chain of 42 terms, whose dbeta was 4.5 x less accurate than PyTorch's.)
struct Geom {
  uint32_t cq, rg, CQ, RG;
};

__device__ __forceinline__ Geom geom(uint32_t C) {
  Geom g;
  g.CQ = C / 4;
  g.RG = blockDim.x / g.CQ;
  g.cq = threadIdx.x % g.CQ;
  g.rg = threadIdx.x / g.CQ;
  return g;
}

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

template <typename F>
__device__ __forceinline__ f32x4 column_sum(f32x4* red, const Geom& g, uint32_t row0, uint32_t row1, F f) {
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
  for (uint32_t row = row0 + g.rg; row < row1; row += g.RG) s += f(row);
  __syncthreads();   // the previous use of `red` is over
  red[g.rg * g.CQ + g.cq] = s;
  __syncthreads();
  for (uint32_t half = 32; half > 0; half >>= 1) {
    if (g.rg < half && g.rg + half < g.RG) red[g.rg * g.CQ + g.cq] += red[(g.rg + half) * g.CQ + g.cq];
    __syncthreads();
  }
  return red[g.cq];
}

// the total of the chunks' partial sums part [n_chunks][C]: the same reduction over the chunks
__device__ __forceinline__ f32x4 chunk_total(f32x4* red, const Geom& g, const float* part, uint32_t n_chunks, uint32_t C) {
  return column_sum(red, g, 0, n_chunks, [&](uint32_t c) { return ld4(part + (size_t)c * C + 4 * g.cq); });
}

__device__ __forceinline__ f32x4 rstd_of(f32x4 var, float eps) {
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; e++) o[e] = 1.0f / sqrtf(var[e] + eps);
  return o;
}

#define C4_BN_PROLOGUE                                                                    \
  __shared__ f32x4 red[256];                                                              \
  const Geom g = geom(C);                                                                 \
  const uint32_t chunk = blockIdx.x, row0 = chunk * kChunkRows, row1 = min(m, row0 + kChunkRows); \
  const uint32_t col = 4 * g.cq

// sums[chunk][C] = the chunk's column sums of z
__global__ __launch_bounds__(256) void bn2d_sum(const float* __restrict__ z, float* __restrict__ sums, uint32_t m, uint32_t C) {
  C4_BN_PROLOGUE;
  const f32x4 s = column_sum(red, g, row0, row1, [&](uint32_t row) { return ld4(z + (size_t)row * C + col); });
  if (g.rg == 0) *reinterpret_cast<f32x4*>(sums + (size_t)chunk * C + col) = s;
}

// out[chunk][C] = the chunk's column sums of d (SQUARE: of d d), d = z - mean, mean = total(sums) / m (mean_in: the mean as given)
template <bool SQUARE>
__global__ __launch_bounds__(256) void bn2d_dev(const float* __restrict__ z, const float* __restrict__ sums, const float* __restrict__ mean_in,
                                                float* __restrict__ out, uint32_t m, uint32_t C, uint32_t n_chunks) {
  C4_BN_PROLOGUE;
  const f32x4 mean = mean_in ? ld4(mean_in + col) : chunk_total(red, g, sums, n_chunks, C) / (float)m;
  const f32x4 s = column_sum(red, g, row0, row1, [&](uint32_t row) {
    const f32x4 d = ld4(z + (size_t)row * C + col) - mean;
    return SQUARE ? d * d : d;
  });
  if (g.rg == 0) *reinterpret_cast<f32x4*>(out + (size_t)chunk * C + col) = s;
}

__global__ __launch_bounds__(256) void bn2d_apply(const float* __restrict__ z, const float* __restrict__ a, const float* __restrict__ gamma,
                                                  const float* __restrict__ beta, float eps, const float* __restrict__ sums,
                                                  const float* __restrict__ squares, float* __restrict__ y, float* __restrict__ mean_out,
                                                  float* __restrict__ var_out, uint32_t m, uint32_t C, uint32_t n_chunks) {
  C4_BN_PROLOGUE;
  const f32x4 mean = chunk_total(red, g, sums, n_chunks, C) / (float)m;
  const f32x4 var = chunk_total(red, g, squares, n_chunks, C) / (float)m;
  const f32x4 rstd = rstd_of(var, eps), gm = ld4(gamma + col), bt = ld4(beta + col);
  for (uint32_t row = row0 + g.rg; row < row1; row += g.RG) {
    const size_t at = (size_t)row * C + col;
    const f32x4 pre = (ld4(z + at) - mean) * rstd * gm + bt, av = ld4(a + at);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; e++) o[e] = av[e] + (!(pre[e] <= 0.f) ? pre[e] : 0.f);   // a NaN passes
    *reinterpret_cast<f32x4*>(y + at) = o;
  }
  if (chunk == 0 && g.rg == 0) {
    *reinterpret_cast<f32x4*>(mean_out + col) = mean;
    *reinterpret_cast<f32x4*>(var_out + col) = var;
  }
}

// sb[chunk][C], sg[chunk][C] = the chunk's column sums of gr and of gr xh: gr = dy where the forward's pre-activation passes ReLU,
// xh = ((z - mean) - corr) rstd, corr = total(devs) / m (c4_train.hip's train_bn_relu_bwd says why)
__global__ __launch_bounds__(256) void bn2d_bwd_sums(const float* __restrict__ dy, const float* __restrict__ z, const float* __restrict__ mean_in,
                                                     const float* __restrict__ var_in, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float eps, const float* __restrict__ devs,
                                                     float* __restrict__ sb, float* __restrict__ sg, uint32_t m, uint32_t C, uint32_t n_chunks) {
  C4_BN_PROLOGUE;
  const f32x4 mean = ld4(mean_in + col), rstd = rstd_of(ld4(var_in + col), eps), gm = ld4(gamma + col), bt = ld4(beta + col);
  const f32x4 corr = chunk_total(red, g, devs, n_chunks, C) / (float)m;
  auto grad = [&](uint32_t row, f32x4& d) {
    const size_t at = (size_t)row * C + col;
    d = ld4(z + at) - mean;
    const f32x4 pre = d * rstd * gm + bt, dv = ld4(dy + at);   // the forward's operations in the forward's order
    f32x4 gr;
#pragma unroll
    for (int e = 0; e < 4; e++) gr[e] = !(pre[e] <= 0.f) ? dv[e] : 0.f;   // ReLU'(0) = 0; the forward's predicate
    return gr;
  };
  const f32x4 b = column_sum(red, g, row0, row1, [&](uint32_t row) {
    f32x4 d;
    return grad(row, d);
  });
  const f32x4 s = column_sum(red, g, row0, row1, [&](uint32_t row) {
    f32x4 d;
    const f32x4 gr = grad(row, d);
    return gr * ((d - corr) * rstd);
  });
  if (g.rg == 0) {
    *reinterpret_cast<f32x4*>(sb + (size_t)chunk * C + col) = b;
    *reinterpret_cast<f32x4*>(sg + (size_t)chunk * C + col) = s;
  }
}

__global__ __launch_bounds__(256) void bn2d_bwd_apply(const float* __restrict__ dy, const float* __restrict__ z, const float* __restrict__ mean_in,
                                                      const float* __restrict__ var_in, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float eps, const float* __restrict__ devs,
                                                      const float* __restrict__ sb, const float* __restrict__ sg, float* __restrict__ dz,
                                                      float* __restrict__ dgamma, float* __restrict__ dbeta, uint32_t m, uint32_t C,
                                                      uint32_t n_chunks) {
  C4_BN_PROLOGUE;
  const f32x4 mean = ld4(mean_in + col), rstd = rstd_of(ld4(var_in + col), eps), gm = ld4(gamma + col), bt = ld4(beta + col);
  const f32x4 corr = chunk_total(red, g, devs, n_chunks, C) / (float)m;
  const f32x4 db = chunk_total(red, g, sb, n_chunks, C);
  const f32x4 dg = chunk_total(red, g, sg, n_chunks, C);
  const f32x4 c1 = db / (float)m, c2 = dg / (float)m, scale = gm * rstd;
  for (uint32_t row = row0 + g.rg; row < row1; row += g.RG) {
    const size_t at = (size_t)row * C + col;
    const f32x4 d = ld4(z + at) - mean;
    const f32x4 pre = d * rstd * gm + bt, dv = ld4(dy + at);
    f32x4 gr;
#pragma unroll
    for (int e = 0; e < 4; e++) gr[e] = !(pre[e] <= 0.f) ? dv[e] : 0.f;
    *reinterpret_cast<f32x4*>(dz + at) = scale * ((gr - c1) - ((d - corr) * rstd) * c2);
  }
  if (chunk == 0 && g.rg == 0) {
    *reinterpret_cast<f32x4*>(dgamma + col) = dg;
    *reinterpret_cast<f32x4*>(dbeta + col) = db;
  }
}

// ---------------------------------------------------------------------------------------------------------------- host
using c4host::aligned16;
using c4host::launched;

bool channels_ok(uint32_t c) { return c >= 16 && c <= 64 && c % 16 == 0; }

uint32_t chunks_of(uint32_t n_boards) { return (n_boards + kChunkBoards - 1) / kChunkBoards; }

// what every entry point refuses: 0 on success (a message is set otherwise)
int shape_refusal(const char* me, uint32_t n_boards, uint32_t channels) {
  if (!channels_ok(channels)) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": channels must be 16, 32, 48 or 64");
  if (n_boards == 0) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": n_boards >= 1");
  if ((uint64_t)n_boards * 42 * channels >= (1ull << 31)) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": n_boards too large (42 B C must stay below 2^31)");
  return C4_OK;
}

template <bool FIRST>
hipError_t launch_wgrad(const float* dz, const float* x, float* part, uint32_t m, uint32_t c, uint32_t n_chunks, hipStream_t s) {
  const uint32_t k = FIRST ? 32 : 9 * c;
  // two column tiles a wavefront where the tile count is even (the first convolution: always); both shapes compute the same bits
  const uint32_t kt = FIRST || c % 32 == 0 ? 2 : 1;
  const uint64_t waves = (uint64_t)n_chunks * (k / (16 * kt));
  const dim3 grid((uint32_t)((waves + 3) / 4)), block(256);
  switch (c) {
    case 16:
      if constexpr (FIRST) tower_wgrad_partial<FIRST, 1, 2><<<grid, block, 0, s>>>(dz, x, part, m, n_chunks);
      else tower_wgrad_partial<FIRST, 1, 1><<<grid, block, 0, s>>>(dz, x, part, m, n_chunks);
      break;
    case 32: tower_wgrad_partial<FIRST, 2, 2><<<grid, block, 0, s>>>(dz, x, part, m, n_chunks); break;
    case 48:
      if constexpr (FIRST) tower_wgrad_partial<FIRST, 3, 2><<<grid, block, 0, s>>>(dz, x, part, m, n_chunks);
      else tower_wgrad_partial<FIRST, 3, 1><<<grid, block, 0, s>>>(dz, x, part, m, n_chunks);
      break;
    default: tower_wgrad_partial<FIRST, 4, 2><<<grid, block, 0, s>>>(dz, x, part, m, n_chunks); break;
  }
  return hipGetLastError();
}

template <bool FIRST>
int wgrad(const char* me, const float* dz, const float* x, float* dw, float* db, uint32_t n_boards, uint32_t c, float* work, void* stream) {
  if (!dz || !x || !dw || !db || !work) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": null argument");
  if (const int rc = shape_refusal(me, n_boards, c)) return rc;
  if (!aligned16(dz) || !aligned16(x) || !aligned16(dw) || !aligned16(db) || !aligned16(work))
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": arrays must be 16-byte aligned");
  C4_ON_STREAM_DEVICE(stream);
  const hipStream_t s = (hipStream_t)stream;
  const uint32_t n_chunks = chunks_of(n_boards), w_elems = c * (FIRST ? 32 : 9 * c), elems = w_elems + c;
  if (const int rc = launched(me, launch_wgrad<FIRST>(dz, x, work, 42 * n_boards, c, n_chunks, s))) return rc;
  tower_chunk_reduce<<<dim3((elems / 4 + 31) / 32), dim3(256), 0, s>>>(work, dw, db, n_chunks, elems, w_elems);
  return launched(me, hipGetLastError());
}

dim3 bn_block(uint32_t c) { return dim3((256 / (c / 4)) * (c / 4)); }

}  // namespace

extern "C" int c4_train_tower_work_bytes(uint32_t n_boards, uint32_t channels, uint64_t* bytes_out) {
  const char* me = "c4_train_tower_work_bytes";
  if (!bytes_out) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": null argument");
  if (const int rc = shape_refusal(me, n_boards, channels)) return rc;
  *bytes_out = (uint64_t)chunks_of(n_boards) * (9ull * channels * channels + channels) * sizeof(float);
  return C4_OK;
}

extern "C" int c4_train_conv0_f32(const float* planes_dev, const float* w0_dev, const float* bias_dev, float* z_dev, uint32_t n_boards,
                                  uint32_t channels, void* stream) {
  const char* me = "c4_train_conv0_f32";
  if (!planes_dev || !w0_dev || !bias_dev || !z_dev) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": null argument");
  if (const int rc = shape_refusal(me, n_boards, channels)) return rc;
  if (!aligned16(w0_dev) || !aligned16(bias_dev) || !aligned16(z_dev)) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": w0, bias and z must be 16-byte aligned");
  C4_ON_STREAM_DEVICE(stream);
  return launched(me, c4f32::launch_train_conv(true, planes_dev, w0_dev, bias_dev, z_dev, 42 * n_boards, channels, (hipStream_t)stream));
}

extern "C" int c4_train_conv3x3_f32(const float* x_dev, const float* w_dev, const float* bias_dev, float* z_dev, uint32_t n_boards, uint32_t channels,
                                    void* stream) {
  const char* me = "c4_train_conv3x3_f32";
  if (!x_dev || !w_dev || !bias_dev || !z_dev) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": null argument");
  if (x_dev == z_dev) return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": z must not be x (a cell reads its neighbours)");
  if (const int rc = shape_refusal(me, n_boards, channels)) return rc;
  if (!aligned16(x_dev) || !aligned16(w_dev) || !aligned16(bias_dev) || !aligned16(z_dev))
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": arrays must be 16-byte aligned");
  C4_ON_STREAM_DEVICE(stream);
  return launched(me, c4f32::launch_train_conv(false, x_dev, w_dev, bias_dev, z_dev, 42 * n_boards, channels, (hipStream_t)stream));
}

extern "C" int c4_train_conv0_wgrad_f32(const float* dz_dev, const float* planes_dev, float* dw0_dev, float* db_dev, uint32_t n_boards,
                                        uint32_t channels, float* work_dev, void* stream) {
  return wgrad<true>("c4_train_conv0_wgrad_f32", dz_dev, planes_dev, dw0_dev, db_dev, n_boards, channels, work_dev, stream);
}

extern "C" int c4_train_conv3x3_wgrad_f32(const float* dz_dev, const float* x_dev, float* dw_dev, float* db_dev, uint32_t n_boards, uint32_t channels,
                                          float* work_dev, void* stream) {
  return wgrad<false>("c4_train_conv3x3_wgrad_f32", dz_dev, x_dev, dw_dev, db_dev, n_boards, channels, work_dev, stream);
}

extern "C" int c4_train_bn2d_relu_res_fwd_f32(const float* z_dev, const float* a_dev, const float* gamma_dev, const float* beta_dev, float eps,
                                              uint32_t n_boards, uint32_t channels, float* y_dev, float* mean_dev, float* var_dev, float* work_dev,
                                              void* stream) {
  const char* me = "c4_train_bn2d_relu_res_fwd_f32";
  if (!z_dev || !a_dev || !gamma_dev || !beta_dev || !y_dev || !mean_dev || !var_dev || !work_dev)
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": null argument");
  if (const int rc = shape_refusal(me, n_boards, channels)) return rc;
  if (!aligned16(z_dev) || !aligned16(a_dev) || !aligned16(gamma_dev) || !aligned16(beta_dev) || !aligned16(y_dev) || !aligned16(mean_dev) ||
      !aligned16(var_dev) || !aligned16(work_dev))
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": arrays must be 16-byte aligned");
  C4_ON_STREAM_DEVICE(stream);
  const hipStream_t s = (hipStream_t)stream;
  const uint32_t m = 42 * n_boards, c = channels, n_chunks = chunks_of(n_boards);
  float* sums = work_dev;
  float* squares = work_dev + (size_t)n_chunks * c;
  const dim3 grid(n_chunks), block = bn_block(c);
  bn2d_sum<<<grid, block, 0, s>>>(z_dev, sums, m, c);
  if (const int rc = launched(me, hipGetLastError())) return rc;
  bn2d_dev<true><<<grid, block, 0, s>>>(z_dev, sums, nullptr, squares, m, c, n_chunks);
  if (const int rc = launched(me, hipGetLastError())) return rc;
  bn2d_apply<<<grid, block, 0, s>>>(z_dev, a_dev, gamma_dev, beta_dev, eps, sums, squares, y_dev, mean_dev, var_dev, m, c, n_chunks);
  return launched(me, hipGetLastError());
}

extern "C" int c4_train_bn2d_relu_res_bwd_f32(const float* dy_dev, const float* z_dev, const float* mean_dev, const float* var_dev,
                                              const float* gamma_dev, const float* beta_dev, float eps, uint32_t n_boards, uint32_t channels,
                                              float* dz_dev, float* dgamma_dev, float* dbeta_dev, float* work_dev, void* stream) {
  const char* me = "c4_train_bn2d_relu_res_bwd_f32";
  if (!dy_dev || !z_dev || !mean_dev || !var_dev || !gamma_dev || !beta_dev || !dz_dev || !dgamma_dev || !dbeta_dev || !work_dev)
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": null argument");
  if (const int rc = shape_refusal(me, n_boards, channels)) return rc;
  if (!aligned16(dy_dev) || !aligned16(z_dev) || !aligned16(mean_dev) || !aligned16(var_dev) || !aligned16(gamma_dev) || !aligned16(beta_dev) ||
      !aligned16(dz_dev) || !aligned16(dgamma_dev) || !aligned16(dbeta_dev) || !aligned16(work_dev))
    return c4host::fail(C4_ERR_BAD_ARG, std::string(me) + ": arrays must be 16-byte aligned");
  C4_ON_STREAM_DEVICE(stream);
  const hipStream_t s = (hipStream_t)stream;
  const uint32_t m = 42 * n_boards, c = channels, n_chunks = chunks_of(n_boards);
  float* devs = work_dev;
  float* sb = work_dev + (size_t)n_chunks * c;
  float* sg = sb + (size_t)n_chunks * c;
  const dim3 grid(n_chunks), block = bn_block(c);
  bn2d_dev<false><<<grid, block, 0, s>>>(z_dev, nullptr, mean_dev, devs, m, c, n_chunks);
  if (const int rc = launched(me, hipGetLastError())) return rc;
  bn2d_bwd_sums<<<grid, block, 0, s>>>(dy_dev, z_dev, mean_dev, var_dev, gamma_dev, beta_dev, eps, devs, sb, sg, m, c, n_chunks);
  if (const int rc = launched(me, hipGetLastError())) return rc;
  bn2d_bwd_apply<<<grid, block, 0, s>>>(dy_dev, z_dev, mean_dev, var_dev, gamma_dev, beta_dev, eps, devs, sb, sg, dz_dev, dgamma_dev, dbeta_dev, m, c,
                                        n_chunks);
  return launched(me, hipGetLastError());
}
