// actmask.h — action masks (invalid-action masking: Huang & Ontañón 2020, "A Closer Look at Invalid Action Masking in Policy
// Gradient Algorithms") as wave-level device functions, written the way ordinal.h is: one wave per row, lane = bin.
//
// A row of a head carries one 64-bit word: bit k set means bin k may be chosen.  The mask acts in BIN space, after the
// ordinal transform where the head is ordinal: with on = lane < K and x the (unnormalised) logit of bin `lane`,
//   on_m = on && bit(lane)        x = on_m ? x : -inf
// and everything behind it (the two softmax passes, the entropy, the probabilities, d total / d logit) uses on_m where the
// unmasked row body uses on.  The statements are selects: with every bit of the K bins set, on_m == on on every lane and the
// row runs the arithmetic of the unmasked body bit for bit.
//
// A word with no bit set among the K bins means "unmasked": there is no NaN path and a captured graph needs no host check.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// the K low bits
__device__ __forceinline__ uint64_t am_all(int K) { return K >= 64 ? ~0ull : ((1ull << K) - 1ull); }

// the row's word as stored (int64 tensors, read as uint64)
__device__ __forceinline__ uint64_t am_word(const int64_t* allowed, int64_t row) { return (uint64_t)allowed[row]; }

// the bits of the head's K bins, "empty means all"
__device__ __forceinline__ uint64_t am_effective(uint64_t w, int K) {
  const uint64_t all = am_all(K);
  const uint64_t m = w & all;
  return m ? m : all;
}

// a proper mask: at least one of the K bins is forbidden
__device__ __forceinline__ bool am_proper(uint64_t m, int K) { return m != am_all(K); }

// on_m of this lane (m: an effective word, so bits >= K are clear)
__device__ __forceinline__ bool am_on(uint64_t m, int lane) { return ((m >> lane) & 1ull) != 0ull; }

// the number of allowed bins
__device__ __forceinline__ int am_count(uint64_t m) { return __popcll(m); }

// The pressure of a row: 1 - exp(lse_masked - lse_unmasked), the probability mass the unmasked head would have put on the
// forbidden bins.  x: the unmasked logit of bin `lane` (-inf on lanes >= K), on = lane < K, lse_m: the masked row's
// log-sum-exp.  Exactly 0 for a row without a proper mask (the caller passes proper = false and nothing is computed).
__device__ __forceinline__ float am_pressure(float x, bool on, float lse_m, bool proper) {
  if (!proper) return 0.f;
  float mx = x;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float se = on ? expf(x - mx) : 0.f;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o, 64);
  const float lse = mx + logf(se);
  return fminf(fmaxf(1.f - expf(lse_m - lse), 0.f), 1.f);
}
