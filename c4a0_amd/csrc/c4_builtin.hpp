// c4_builtin.hpp -- the two evaluators that need no weights, written once for the device (c4_builtin_players.hip: one lane per
// row of a batch) and for the host (c4_builtin_eval_host: the same functions in a loop).  The tournament's anchors (reference
// src/c4a0/tournament.py:54-77): `uniform` answers seven equal logits and q = 0, `random` logits in [0, 1) and one q in [-1, 1).
//
// Both are PURE functions of (kind, seed, model id, position): a position's answer never depends on the batch it arrives in,
// and a game can be replayed from outside.  (The reference's RandomPlayer draws from torch's global generator -- another answer
// at every call; here the draw is keyed by the position.)  The definition is in include/c4a0_hip.h ("built-in players"); every
// output is a dyadic rational that f32 holds exactly, so host and device agree bit for bit.
//
// The position is read from the two planes as the batch holds them: cell i = 7 * row + col of plane 0 sets bit i of `value`
// where it is != 0, of plane 1 bit i of `mask & ~value`.  A row's 84 values arrive as 8-byte words (four bf16 or two f32 each)
// that a Cells accumulator folds into an 84-bit string; no HIP type is needed here.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define C4B_HD __host__ __device__ __forceinline__
#else
#define C4B_HD inline
#endif

namespace c4b {

constexpr uint32_t kUniform = 0, kRandom = 1;        // == C4_BUILTIN_UNIFORM, C4_BUILTIN_RANDOM
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kCells42 = (1ull << 42) - 1;
constexpr uint32_t kBf16Words = 21, kF32Words = 42;  // 8-byte words of a row: 84 bf16 / 84 f32 values

C4B_HD bool valid_kind(uint32_t kind) { return kind == kUniform || kind == kRandom; }

// the 84 "!= 0" bits of a row, in the planes' own order: bits 0..41 plane 0, bits 42..83 plane 1
struct Cells {
  uint64_t lo = 0, hi = 0;
  C4B_HD void set(uint32_t e, bool on) {
    if (e < 64) lo |= (uint64_t)on << e; else hi |= (uint64_t)on << (e - 64);
  }
  // word w of a bf16 row: values 4 w .. 4 w + 3, little endian (x != 0 for every bit pattern but +-0; a NaN counts, as in numpy)
  C4B_HD void add_bf16x4(uint32_t w, uint64_t word) {
    for (uint32_t j = 0; j < 4; j++) set(4 * w + j, ((word >> (16 * j)) & 0x7FFFull) != 0);
  }
  // word w of an f32 row: values 2 w, 2 w + 1
  C4B_HD void add_f32x2(uint32_t w, uint64_t word) {
    for (uint32_t j = 0; j < 2; j++) set(2 * w + j, ((word >> (32 * j)) & 0x7FFFFFFFull) != 0);
  }
  C4B_HD uint64_t value() const { return lo & kCells42; }
  C4B_HD uint64_t mask() const { return value() | (((lo >> 42) | (hi << 22)) & kCells42); }
};

C4B_HD uint64_t mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// out[0..6] the logits, out[7] q_penalty, out[8] q_no_penalty (the row format of c4_head_out_bf16_grouped's answers)
C4B_HD void answer(uint32_t kind, uint64_t seed, uint64_t model_id, uint64_t mask, uint64_t value, float out[9]) {
  if (kind != kRandom) {
    for (int j = 0; j < 7; j++) out[j] = 1.0f;
    out[7] = out[8] = 0.0f;
    return;
  }
  uint64_t k = mix(seed + kGolden);
  k = mix(k ^ model_id);
  k = mix(k ^ mask);
  k = mix(k ^ value);
  for (int j = 0; j < 7; j++) out[j] = (float)(uint32_t)(mix(k + (uint64_t)(j + 1) * kGolden) >> 40) * (1.0f / 16777216.0f);   // 24 bits: exact
  const int32_t u7 = (int32_t)(mix(k + 8 * kGolden) >> 40);
  out[7] = out[8] = (float)(u7 - (1 << 23)) * (1.0f / 8388608.0f);
}

}  // namespace c4b
