// c4_elementwise.hip -- the element-wise kernels behind the parity tests and their entry points (no session: positions, planes,
// the glibc expf / logf ports, softmax, temperature and move sampling for n independent elements; store_plane is all they share with the session.
// k_dirichlet / c4_dirichlet stay in c4_session.hip, see there).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/c4a0_hip.h"
#include "c4_device.hpp"
#include "c4_host.hpp"
#include "c4_tree.hpp"

#pragma clang fp contract(off)

namespace {

using c4host::fail;
using c4host::grid_for;
using c4host::with_planes;

// ------------------------------------------------------------------------------------------
// Element-wise kernels (SURVEY 8a K1 and the arithmetic pieces) for the parity tests
// ------------------------------------------------------------------------------------------
__global__ void k_pos_ops(const uint64_t* mask, const uint64_t* value, const int32_t* col, uint64_t n, float c_ply,
                          uint64_t* om, uint64_t* ov, uint32_t* olegal, uint32_t* oterm, float* oq) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t m = mask[i], v = value[i];
  const uint32_t legal = c4::legal_mask(m);
  const uint32_t t = c4::terminal_state(m, v);
  float a = 0.0f, b = 0.0f;
  if (t) c4::terminal_value(t, m, c_ply, a, b);
  olegal[i] = legal;
  oterm[i] = t;
  oq[2 * i] = a;
  oq[2 * i + 1] = b;
  const int32_t c = col[i];
  if (c >= 0 && c < 7 && ((legal >> c) & 1u)) {
    c4::make_move(m, v, (uint32_t)c);
    om[i] = m; ov[i] = v;
  } else {
    om[i] = 0; ov[i] = 0;  // make_move returns None (c4r.rs:71)
  }
}

template <typename PlaneT>
__global__ void k_encode(const uint64_t* mask, const uint64_t* value, uint64_t n, void* planes) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * C4_PLANES_LEN) return;
  const uint64_t g = i / C4_PLANES_LEN;
  const uint32_t e = (uint32_t)(i % C4_PLANES_LEN);
  store_plane<PlaneT>(planes, i, c4::plane_bit(mask[g], value[g], e));
}

__global__ void k_expf_logf(const float* x, uint64_t n, int which, float* y) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  y[i] = which ? c4::c4_logf(x[i]) : c4::c4_expf(x[i]);
}

__global__ void k_softmax7(const float* logits, const uint32_t* legal, uint64_t n, float* out, uint32_t* err) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float l[7], o[7];
  for (int c = 0; c < 7; c++) {
    l[c] = logits[7 * i + c];
    if (legal && !((legal[i] >> c) & 1u)) l[c] = __uint_as_float(0xff800000u);
  }
  const bool ok = c4::softmax7(l, o);
  err[i] = ok ? 0u : (uint32_t)C4_ERR_DEGENERATE_POLICY;
  for (int c = 0; c < 7; c++) out[7 * i + c] = ok ? o[c] : 0.0f;
}

__global__ void k_temperature(const float* policy, const float* t, uint64_t n, float* out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float p[7], o[7];
  for (int c = 0; c < 7; c++) p[c] = policy[7 * i + c];
  c4::apply_temperature(p, t[i], o);
  for (int c = 0; c < 7; c++) out[7 * i + c] = o[c];
}

__global__ void k_sample_move(const uint64_t* game_id, const uint32_t* n_moves, const float* policy, const float* t,
                              uint64_t n, int32_t* out_col, uint32_t* out_u32) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float p[7], o[7];
  for (int c = 0; c < 7; c++) p[c] = policy[7 * i + c];
  c4::apply_temperature(p, t[i], o);
  const uint32_t u = c4::rng_first_u32(game_id[i] * (uint64_t)(42 + n_moves[i]));
  out_col[i] = c4::weighted_index(o, u);
  if (out_u32) out_u32[i] = u;
}

}  // namespace

// ---- element-wise entry points ----
// They run on the device their stream belongs to (the caller's current device for the null stream) and
// leave the caller's current device as they found it, like the session entry points (C4_ON_STREAM_DEVICE, c4_host.hpp).

extern "C" {

int c4_pos_ops(const uint64_t* mask_dev, const uint64_t* value_dev, const int32_t* col_dev, uint64_t n, float c_ply_penalty,
               uint64_t* out_mask_dev, uint64_t* out_value_dev, uint32_t* out_legal_dev, uint32_t* out_terminal_dev,
               float* out_q_dev, void* stream) {
  if (n == 0) return C4_OK;
  C4_ON_STREAM_DEVICE(stream);
  hipLaunchKernelGGL(k_pos_ops, grid_for(n), dim3(256), 0, (hipStream_t)stream, mask_dev, value_dev, col_dev, n, c_ply_penalty,
                     out_mask_dev, out_value_dev, out_legal_dev, out_terminal_dev, out_q_dev);
  HIP_TRY(hipGetLastError());
  return C4_OK;
}

int c4_encode_planes(const uint64_t* mask_dev, const uint64_t* value_dev, uint64_t n, uint32_t planes_dtype, void* planes_dev, void* stream) {
  if (n == 0) return C4_OK;
  C4_ON_STREAM_DEVICE(stream);
  if (planes_dtype > 1) return fail(C4_ERR_BAD_ARG, "planes_dtype must be 0 or 1");
  with_planes(planes_dtype, [&](auto planes) {
    hipLaunchKernelGGL(k_encode<decltype(planes)>, grid_for(n * C4_PLANES_LEN), dim3(256), 0, (hipStream_t)stream, mask_dev, value_dev, n, planes_dev);
  });
  HIP_TRY(hipGetLastError());
  return C4_OK;
}

int c4_expf_logf(const float* x_dev, uint64_t n, int which, float* y_dev, void* stream) {
  if (n == 0) return C4_OK;
  C4_ON_STREAM_DEVICE(stream);
  hipLaunchKernelGGL(k_expf_logf, grid_for(n), dim3(256), 0, (hipStream_t)stream, x_dev, n, which, y_dev);
  HIP_TRY(hipGetLastError());
  return C4_OK;
}

int c4_softmax7(const float* logits_dev, const uint32_t* legal_dev, uint64_t n, float* out_dev, uint32_t* out_err_dev, void* stream) {
  if (n == 0) return C4_OK;
  C4_ON_STREAM_DEVICE(stream);
  hipLaunchKernelGGL(k_softmax7, grid_for(n), dim3(256), 0, (hipStream_t)stream, logits_dev, legal_dev, n, out_dev, out_err_dev);
  HIP_TRY(hipGetLastError());
  return C4_OK;
}

int c4_apply_temperature(const float* policy_dev, const float* temperature_dev, uint64_t n, float* out_dev, void* stream) {
  if (n == 0) return C4_OK;
  C4_ON_STREAM_DEVICE(stream);
  hipLaunchKernelGGL(k_temperature, grid_for(n), dim3(256), 0, (hipStream_t)stream, policy_dev, temperature_dev, n, out_dev);
  HIP_TRY(hipGetLastError());
  return C4_OK;
}

int c4_sample_move(const uint64_t* game_id_dev, const uint32_t* n_moves_dev, const float* policy_dev, const float* temperature_dev,
                   uint64_t n, int32_t* out_col_dev, uint32_t* out_u32_dev, void* stream) {
  if (n == 0) return C4_OK;
  C4_ON_STREAM_DEVICE(stream);
  hipLaunchKernelGGL(k_sample_move, grid_for(n), dim3(256), 0, (hipStream_t)stream, game_id_dev, n_moves_dev, policy_dev,
                     temperature_dev, n, out_col_dev, out_u32_dev);
  HIP_TRY(hipGetLastError());
  return C4_OK;
}

}  // extern "C"
