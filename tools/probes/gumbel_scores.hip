// Debug build of the device sampler's score (lap_amd/csrc/sampling.hpp): the production kernels keep only the argmax, this one
// writes every score = logit * inv_t + g so that the host restatement (lap_amd/sampling.py) can be differenced against it
// (tools/probes/gumbel_score_error.py; the TIE allowance of tests/test_ar_sampling_gpu.py comes from that figure).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize -shared tools/probes/gumbel_scores.hip -o tools/probes/gumbel_scores.so
#include "../../lap_amd/csrc/sampling.hpp"

__global__ __launch_bounds__(256) void gumbel_scores_kernel(const float* __restrict__ x, int n, float inv_t, uint32_t seed_lo,
                                                            uint32_t seed_hi, uint32_t step, float* __restrict__ out) {
  const int units = (n + 1) / 2;
  const long long base = (long long)blockIdx.y * n;
  for (int u = blockIdx.x * 256 + threadIdx.x; u < units; u += gridDim.x * 256) {
    const int c0 = 2 * u, c1 = min(2 * u + 1, n - 1);
    float s0, s1;
    lap_sampling::gumbel_scores(x[base + c0], x[base + c1], inv_t, seed_lo, seed_hi, step, blockIdx.y, (uint32_t)u, s0, s1);
    out[base + c0] = s0;
    if (c1 != c0) out[base + c1] = s1;
  }
}

// x, out: f32 [rows][n] contiguous
extern "C" int probe_gumbel_scores(const float* x, int rows, int n, float inv_t, unsigned int seed_lo, unsigned int seed_hi, int step,
                                   float* out, void* stream) {
  if (!x || !out || rows < 1 || n < 1) return 1;
  hipLaunchKernelGGL(gumbel_scores_kernel, dim3(256, rows), dim3(256), 0, (hipStream_t)stream, x, n, inv_t, (uint32_t)seed_lo,
                     (uint32_t)seed_hi, (uint32_t)step, out);
  return hipGetLastError() == hipSuccess ? 0 : 2;
}
