// The Gumbel noise of a device-sampled token draw (lap_amd/sampling.py is the host restatement and the specification):
// Philox4x32-10 with key = the 64-bit seed and counter (j >> 1, row, step, 0); vocabulary index j takes output word j & 1;
// u = ((word >> 9) + 0.5) 2^-23 (exact in f32, strictly inside (0, 1)); g = -log(-log(u)) with the accurate logf (the host
// has to reproduce it to a few ulp, which the hardware-log fast form does not allow).  score = logit * inv_t + g with the
// product and the sum rounded separately (no fma contraction), as numpy does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lap_sampling {

// One block: words 0 and 1 (words 2 and 3 are unused; the compiler drops what only they need of the last round).
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t& w0, uint32_t& w1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w0 = c0; w1 = c1;
}

__device__ __forceinline__ float gumbel_from_word(uint32_t w) {
  const float u = ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-07f;    // 2^-23
  return -logf(-logf(u));
}

// scores of vocabulary rows 2 unit and 2 unit + 1 of `row` at decode step `step`
__device__ __forceinline__ void gumbel_scores(float v0, float v1, float inv_t, uint32_t seed_lo, uint32_t seed_hi, uint32_t step,
                                              uint32_t row, uint32_t unit, float& s0, float& s1) {
  uint32_t w0, w1;
  philox4x32_10(unit, row, step, 0u, seed_lo, seed_hi, w0, w1);
  s0 = __fadd_rn(__fmul_rn(v0, inv_t), gumbel_from_word(w0));
  s1 = __fadd_rn(__fmul_rn(v1, inv_t), gumbel_from_word(w1));
}

// scores of vocabulary rows j0 and j1 of `row` (any two rows; j1 == j0: s1 is s0): row j takes word j & 1 of block j >> 1, and
// one block serves both rows when they share it
__device__ __forceinline__ void gumbel_scores_at(float v0, float v1, float inv_t, uint32_t seed_lo, uint32_t seed_hi, uint32_t step,
                                                 uint32_t row, uint32_t j0, uint32_t j1, float& s0, float& s1) {
  uint32_t a0, a1, b0, b1;
  philox4x32_10(j0 >> 1, row, step, 0u, seed_lo, seed_hi, a0, a1);
  b0 = a0; b1 = a1;
  if ((j1 >> 1) != (j0 >> 1)) philox4x32_10(j1 >> 1, row, step, 0u, seed_lo, seed_hi, b0, b1);
  s0 = __fadd_rn(__fmul_rn(v0, inv_t), gumbel_from_word((j0 & 1u) ? a1 : a0));
  s1 = __fadd_rn(__fmul_rn(v1, inv_t), gumbel_from_word((j1 & 1u) ? b1 : b0));
}

}  // namespace lap_sampling
