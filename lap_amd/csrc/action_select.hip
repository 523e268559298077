// Candidate selection of best-of-N flow sampling (lap_amd/action_select.py is the specification): the scores of N candidate action
// chunks, the argmin (lowest index on ties) and a bit copy of the chosen chunk, in ONE launch of one block — no host read-back, no
// allocation, safe to capture.  The whole input is N x S x action_dim <= 64 x 4096 floats: a second block would only wait.
#include "common.hpp"
#include "../../include/lap_hip.h"

namespace {

constexpr int SEL_MAX_N = 64;

// mode 0 (medoid):    score[n] = sum_m sum_e (cand[n][e] - cand[m][e])^2
// mode 1 (coherence): score[n] = sum_s weights[s] sum_a (cand[n][s][a] - known[s][a])^2
// f32 throughout: a thread sums its elements serially (<= ceil(E / 256) x N terms), the 256 partial sums meet in a tree.
__global__ __launch_bounds__(256) void action_select_kernel(const float* __restrict__ cand, const float* __restrict__ known,
                                                            const float* __restrict__ weights, float* __restrict__ scores,
                                                            int* __restrict__ index, float* __restrict__ best, int N, int S, int ad, int mode) {
  __shared__ float red[256];
  __shared__ float sc[SEL_MAX_N];
  __shared__ int sel;
  const int tid = threadIdx.x, E = S * ad;
  for (int n = 0; n < N; ++n) {
    float a = 0.f;
    for (int e = tid; e < E; e += 256) {
      const float c = cand[n * E + e];
      if (mode == 0) {
        for (int m = 0; m < N; ++m) {
          const float d = c - cand[m * E + e];
          a += d * d;
        }
      } else {
        const float d = c - known[e];
        a += weights[e / ad] * (d * d);
      }
    }
    red[tid] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) red[tid] += red[tid + s];
      __syncthreads();
    }
    if (tid == 0) sc[n] = red[0];
    __syncthreads();
  }
  if (tid == 0) {
    int bi = 0;
    for (int n = 1; n < N; ++n)
      if (sc[n] < sc[bi]) bi = n;      // strict: the lowest index wins a tie
    sel = bi;
    index[0] = bi;
  }
  __syncthreads();
  if (tid < N) scores[tid] = sc[tid];
  const float* src = cand + sel * E;
  for (int e = tid; e < E; e += 256) best[e] = src[e];
}

}  // namespace

extern "C" int lap_action_select(const float* cand, const float* known, const float* weights, float* scores, int* index, float* best,
                                 int N, int S, int action_dim, int mode, void* stream) {
  if (!cand || !scores || !index || !best || N < 1 || N > SEL_MAX_N || S < 1 || action_dim < 1 || (mode != 0 && mode != 1)) return LAP_ERR_ARG;
  if ((long long)S * action_dim > 4096 || best == cand) return LAP_ERR_ARG;
  if (mode == 1 && (!known || !weights)) return LAP_ERR_ARG;
  hipLaunchKernelGGL(action_select_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, cand, known, weights, scores, index, best, N, S, action_dim, mode);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}
