// c4_session_readout.hip -- what a session hands back: the finished games' records (counts, packed records, the store itself), one
// slot's root statistics, a hold session's snapshot and probe, and the diagnostic build's phase stamps.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <string>

#include "../../include/c4a0_hip.h"
#include "c4_device.hpp"
#include "c4_host.hpp"
#include "c4_session_impl.hpp"
#include "c4_tree.hpp"

#pragma clang fp contract(off)

namespace {

using c4host::fail;

// Exclusive prefix sum of the per-game sample counts = where each game's records start in the packed
// array.  One 1024-thread workgroup walks the list with a running carry (n_games is a few 10^4..10^6).
__global__ __launch_bounds__(1024) void k_sample_offsets(const uint32_t* counts, unsigned long long n_games,
                                                         unsigned long long* offsets, unsigned long long* total) {
  __shared__ unsigned long long wave_sum[16];
  __shared__ unsigned long long carry;
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) carry = 0;
  __syncthreads();
  for (unsigned long long base = 0; base < n_games; base += 1024) {
    const unsigned long long i = base + tid;
    const unsigned long long v = i < n_games ? counts[i] : 0ull;
    unsigned long long x = v;                                   // inclusive scan inside the wavefront
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned long long y = ((unsigned long long)__shfl_up((int)(x >> 32), off, 64) << 32) | (uint32_t)__shfl_up((int)(uint32_t)x, off, 64);
      if ((int)lane >= off) x += y;
    }
    if (lane == 63) wave_sum[wave] = x;
    __syncthreads();
    unsigned long long before = carry;                           // sums of the wavefronts before this one
    for (uint32_t w = 0; w < wave; w++) before += wave_sum[w];
    if (i < n_games) offsets[i] = before + x - v;
    __syncthreads();
    if (tid == 1023) carry = before + x;
    __syncthreads();
  }
  if (tid == 0) *total = carry;
}

// K6: pack finished games' records contiguously (one wavefront per game, 4 records per pass)
__global__ __launch_bounds__(64) void k_pack_samples(const c4_sample_rec* src, const uint32_t* counts,
                                                     const unsigned long long* offsets, uint64_t n_games, c4_sample_rec* dst) {
  const uint64_t game = blockIdx.x;
  if (game >= n_games) return;
  const uint32_t n = counts[game];
  const uint4* s4 = (const uint4*)(src + game * C4_MAX_SAMPLES_PER_GAME);
  uint4* d4 = (uint4*)(dst + offsets[game]);
  for (uint32_t i = threadIdx.x; i < n * 4u; i += 64) d4[i] = s4[i];  // 64-byte record = 4 x 16 bytes
}

// c4_session_snapshot: InteractivePlay::snapshot (interactive_play.rs:57, 145-166) of every slot with a game, in ONE launch -- the
// root position, root_policy (mcts.rs:396-412), the root's q as q_sum / (visits + 1) (mcts.rs:359-367: the arithmetic of
// c4_session_root_stats and of a search record), the root's visit count and the slot's status.  8 lanes per slot.
__global__ __launch_bounds__(64) void k_hold_snapshot(Params p, c4_sample_rec* dst, uint32_t* visits, uint32_t* status) {
  const uint32_t lane = threadIdx.x & 63, sub = lane & 7;
  const int gbase = (int)(lane & ~7u);
  const uint32_t g = blockIdx.x * 8 + (lane >> 3);
  const uint32_t gs = g < p.n_slots ? g : 0;
  const Slot* st = p.slots + gs;
  const Block* blocks = p.blocks + (size_t)gs * p.blocks_per_slot;
  const uint32_t state = st->state, root_block = st->arena >> 16, root_ref = st->root_ref;
  const bool game = slot_status(state) != kIdle;
  const uint4 re = load_block_lane(blocks, game ? root_block : 0u, sub);
  const float cnt = (game && sub < 7 && root_block != 0) ? (float)re.x : 0.0f;
  float w[7];
  float csum = 0.0f;
  for (int i = 0; i < 7; i++) { w[i] = shfl_f32(cnt, gbase + i); csum = csum + w[i]; }
  if (g >= p.n_slots) return;
  c4_sample_rec* rec = dst + g;
  if (!game) {
    reinterpret_cast<uint2*>(rec)[sub] = make_uint2(0u, 0u);
    if (sub == 7) { visits[g] = 0; status[g] = kIdle; }
    return;
  }
  if (sub < 7) rec->policy[sub] = (csum == 0.0f) ? (1.0f / 7.0f) : (w[sub] / csum);
  if (sub == 7) {
    const Entry* re0 = &blocks[root_ref >> 3].e[root_ref & 7];
    const float nf = (float)re0->n + 1.0f;
    rec->game_id = st->game_id; rec->mask = st->root_mask; rec->value = st->root_value;
    rec->q_penalty = re0->q_pen / nf; rec->q_no_penalty = re0->q_nopen / nf;
    rec->meta = ((state >> 16) & 0xFFu) | (3u << 16);
    visits[g] = re0->n;
    status[g] = slot_status(state);
  }
}

}  // namespace

extern "C" {

int c4_session_sample_counts(c4_session* s, uint32_t* counts_host, uint64_t n_games) {
  if (!s || !counts_host) return fail(C4_ERR_BAD_ARG, "null argument");
  if (n_games != s->n_games) return fail(C4_ERR_BAD_ARG, "n_games does not match set_games");
  C4_ON_DEVICE(s->cfg.device);
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (n_games) HIP_TRY(hipMemcpy(counts_host, s->p.sample_counts, n_games * sizeof(uint32_t), hipMemcpyDeviceToHost));
  return C4_OK;
}

int c4_session_drain_samples(c4_session* s, c4_sample_rec* dst_host, uint64_t cap, uint64_t* n_written) {
  if (!s || !n_written) return fail(C4_ERR_BAD_ARG, "null argument");
  if (!s->have_games) return fail(C4_ERR_NOT_BOUND, "set_games must precede drain_samples");
  // The records are packed ON THE DEVICE (prefix sum + K6, as for the collective) and come back in ONE
  // transfer straight into the caller's buffer: no host-side staging of the 43-record-per-game store.
  uint64_t total = 0;
  int rc = c4_session_pack_samples(s, nullptr, 0, &total);   // size query: offsets + total (synchronises the stream)
  if (rc != C4_OK) return rc;
  *n_written = total;
  if (!dst_host || total == 0) return C4_OK;
  if (cap < total) return fail(C4_ERR_BAD_ARG, "destination too small");
  C4_ON_DEVICE(s->cfg.device);
  c4_sample_rec* tmp = nullptr;
  HIP_TRY(hipMalloc(&tmp, total * sizeof(c4_sample_rec)));
  rc = c4_session_pack_samples(s, tmp, total, &total);
  if (rc == C4_OK) {
    const hipError_t e = hipMemcpy(dst_host, tmp, total * sizeof(c4_sample_rec), hipMemcpyDeviceToHost);
    if (e != hipSuccess) rc = fail(C4_ERR_HIP, std::string("drain_samples: copying the packed records: ") + hipGetErrorString(e));
  }
  (void)hipFree(tmp);
  return rc;
}

int c4_session_pack_samples(c4_session* s, c4_sample_rec* dst_dev, uint64_t cap, uint64_t* n_written) {
  if (!s || !n_written) return fail(C4_ERR_BAD_ARG, "null argument");
  if (!s->have_games) return fail(C4_ERR_NOT_BOUND, "set_games must precede pack_samples");
  C4_ON_DEVICE(s->cfg.device);
  // record offsets by a device prefix sum into the session's persistent buffer; only the total comes back
  unsigned long long* total_dev = s->offsets_dev + (s->n_games ? s->n_games : 1);
  hipLaunchKernelGGL(k_sample_offsets, dim3(1), dim3(1024), 0, s->stream, s->p.sample_counts, (unsigned long long)s->n_games,
                     s->offsets_dev, total_dev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s->total_host, total_dev, sizeof(unsigned long long), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  const uint64_t total = *s->total_host;
  *n_written = total;
  if (!dst_dev || total == 0) return C4_OK;  // size query
  if (cap < total) return fail(C4_ERR_BAD_ARG, "destination too small");
  hipLaunchKernelGGL(k_pack_samples, dim3((unsigned)s->n_games), dim3(64), 0, s->stream, s->p.samples, s->p.sample_counts,
                     s->offsets_dev, s->n_games, dst_dev);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(s->stream));
  return C4_OK;
}

// diagnostic builds only: raw phase stamps [n_waves][16] of the last launch (zeros otherwise)
int c4_session_debug_phase_stamps(c4_session* s, uint64_t* out_host, uint64_t cap_words, uint64_t* n_words) {
  if (!s || !n_words) return fail(C4_ERR_BAD_ARG, "null argument");
  *n_words = (uint64_t)s->n_waves * 16;
  if (!out_host) return C4_OK;
  if (cap_words < *n_words) return fail(C4_ERR_BAD_ARG, "destination too small");
  HIP_TRY(hipStreamSynchronize(s->stream));
  HIP_TRY(hipMemcpy(out_host, s->p.phase, *n_words * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return C4_OK;
}

int c4_session_sample_store(c4_session* s, const c4_sample_rec** recs_dev, const uint32_t** counts_dev, uint64_t* n_games) {
  if (!s) return fail(C4_ERR_BAD_ARG, "null session");
  if (recs_dev) *recs_dev = s->p.samples;
  if (counts_dev) *counts_dev = s->p.sample_counts;
  if (n_games) *n_games = s->n_games;
  return C4_OK;
}

int c4_session_root_stats(c4_session* s, uint32_t slot, float policy[7], float* q_penalty, float* q_no_penalty,
                          uint64_t* visit_count, uint64_t* root_mask, uint64_t* root_value) {
  if (!s || slot >= s->cfg.n_slots) return fail(C4_ERR_BAD_ARG, "bad slot");
  C4_ON_DEVICE(s->cfg.device);
  HIP_TRY(hipStreamSynchronize(s->stream));
  Slot st;
  HIP_TRY(hipMemcpy(&st, s->p.slots + slot, sizeof st, hipMemcpyDeviceToHost));
  const size_t base = (size_t)slot * s->cfg.blocks_per_slot;
  Block rb;
  HIP_TRY(hipMemcpy(&rb, s->p.blocks + base + (st.root_ref >> 3), sizeof rb, hipMemcpyDeviceToHost));
  const Entry& re = rb.e[st.root_ref & 7];
  // mcts.rs:359-367: q_sum / (visit_count as f32 + 1.0)
  const float nf = (float)re.n + 1.0f;
  if (q_penalty) *q_penalty = re.q_pen / nf;
  if (q_no_penalty) *q_no_penalty = re.q_nopen / nf;
  if (visit_count) *visit_count = re.n;
  if (root_mask) *root_mask = st.root_mask;
  if (root_value) *root_value = st.root_value;
  if (policy) {
    // mcts.rs:396-412
    float cnt[7] = {0, 0, 0, 0, 0, 0, 0}, sum = 0.0f;
    const uint32_t root_block = st.arena >> 16;
    if (root_block) {
      Block cb;
      HIP_TRY(hipMemcpy(&cb, s->p.blocks + base + root_block, sizeof cb, hipMemcpyDeviceToHost));
      for (int c = 0; c < 7; c++) cnt[c] = (float)cb.e[c].n;
    }
    for (int c = 0; c < 7; c++) sum = sum + cnt[c];
    for (int c = 0; c < 7; c++) policy[c] = (sum == 0.0f) ? (1.0f / 7.0f) : cnt[c] / sum;
  }
  return C4_OK;
}

int c4_session_snapshot(c4_session* s, c4_sample_rec* dst_host, uint32_t* visits_host, uint32_t* status_host, uint64_t cap) {
  if (!s) return fail(C4_ERR_BAD_ARG, "null session");
  if (!hold_mode(s)) return fail(C4_ERR_BAD_ARG, "c4_session_snapshot: not a hold session (C4_FLAG_HOLD)");
  if (!s->have_games) return fail(C4_ERR_NOT_BOUND, "set_games must precede c4_session_snapshot");
  const size_t n = s->cfg.n_slots;
  if (cap < n) return fail(C4_ERR_BAD_ARG, "c4_session_snapshot: the arrays hold one entry per slot (" + std::to_string(n) + ")");
  C4_ON_DEVICE(s->cfg.device);
  const size_t bytes = n * (sizeof(c4_sample_rec) + 8);   // [n] records, [n] visit counts, [n] status words
  if (!s->snap_dev) {
    HIP_TRY(hipMalloc(&s->snap_dev, bytes));
    HIP_TRY(hipHostMalloc(&s->snap_host, bytes));
  }
  c4_sample_rec* recs = (c4_sample_rec*)s->snap_dev;
  uint32_t* visits = (uint32_t*)(s->snap_dev + n * sizeof(c4_sample_rec));
  hipLaunchKernelGGL(k_hold_snapshot, dim3((unsigned)((n + 7) / 8)), dim3(64), 0, s->stream, s->p, recs, visits, visits + n);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s->snap_host, s->snap_dev, bytes, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  if (dst_host) memcpy(dst_host, s->snap_host, n * sizeof(c4_sample_rec));
  if (visits_host) memcpy(visits_host, s->snap_host + n * sizeof(c4_sample_rec), n * 4);
  if (status_host) memcpy(status_host, s->snap_host + n * sizeof(c4_sample_rec) + n * 4, n * 4);
  return C4_OK;
}

int c4_session_hold_poll(c4_session* s, uint32_t* n_active, uint32_t* max_need, uint32_t* error) {
  if (!s) return fail(C4_ERR_BAD_ARG, "null session");
  if (!hold_mode(s)) return fail(C4_ERR_BAD_ARG, "c4_session_hold_poll: not a hold session (C4_FLAG_HOLD)");
  const int rc = c4_session_poll(s, nullptr, error);
  if (rc != C4_OK) return rc;
  if (n_active) *n_active = s->hold_probe_valid ? s->hold_probe_active : C4_HOLD_POLL_UNKNOWN;
  if (max_need) *max_need = s->hold_probe_valid ? s->hold_probe_need : C4_HOLD_POLL_UNKNOWN;
  return C4_OK;
}

}  // extern "C"
