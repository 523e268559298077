// Teacher-forced scoring of ONE given sequence on multi-row steps (lap_amd/score.py restates the quantity in numpy and is its
// specification).  The candidate lives in one device buffer cand = {length, ids[cap]} (the layout of the speculative decoder's
// reference sequence).  A score step runs the fused decode kernels of csrc/decode.hip on S rows (1 <= S <= 8) that are the
// consecutive positions t-1 .. t-1+S-1 of the sequence: row r feeds ids[t-1+r] at position plen + t-1+r and scores ids[t+r].  It is
// the speculative decoder's verify step with a draft that is always right, so every given token is scored and an answer of L
// tokens costs about L / S passes over the weights.
//   embed    x[r] = bf16(table[ids[t-1+r]] * sqrt(D)) (dec_embed_kernel's arithmetic); an id outside the table, or a row at or past
//            the candidate's end, gives a zero row
//   finish   one block.  n = min(S, length - t); for r < n: logp[t+r] = z_tgt - (M + logf(S_sum)) from the TARGET LM head's plp
//            partials {m, s, z of the target} (dec_finish_kernel<LOGP>'s reduction: the maximum in any order, the terms added in
//            block-index order), greedy[t+r] = the argmax over pval / pidx (lowest index among ties); then t += n, done = t >=
//            length, and the two counters state[24] (steps), state[25] (tokens scored beyond the first of a step).  No EOS logic.
// The layers are lap_decode_spec_qkv / lap_decode_spec_attention and the other projections at B = S (S = 1: the plain B = 1
// kernels), the head is lap_decode_lm_head_score (decode.hip's TARGET instances).  Token 0 is scored from the prefill's last row
// with the same head at B = 1 and this finish at S = 1.  All kernels read t = state[0], done = state[1] and return at once when
// done is set.  Device state is written with plain per-lane stores.
#include "common.hpp"
#include "../../include/lap_hip.h"

#define S_ ((hipStream_t)stream)

namespace {

constexpr int SCORE_MAXS = 8;              // rows of a score step (the decode kernels' DEC_MAXB)
constexpr int SCORE_D = 2048;
constexpr int SCORE_MAXBLK = 1024;         // the LM head's partials per row (lap_decode_lm_blocks()) that the finish has room for

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// grid = S: row r embeds ids[t-1+r] while t-1+r < min(length, cap), else a zero row
__global__ __launch_bounds__(256) void score_embed_kernel(const int* state, const float* table, int row_lo, int row_hi, const int* cand,
                                                          int cap, bf16* x, int D, float scale) {
  if (state[1]) return;
  const int r = blockIdx.x, t = state[0];
  if (t < 1 || t > cap) return;
  const int len = min(cand[0], cap), j = t - 1 + r;
  const int tok = j < len ? cand[1 + j] : -1;
  for (int c = threadIdx.x * 8; c < D; c += 2048) {
    bf16x8 o;
    if (tok >= row_lo && tok < row_hi) {
      const float* src = table + (long long)(tok - row_lo) * D + c;
      const f32x4 a = *reinterpret_cast<const f32x4*>(src), e4 = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { o[e] = f2bf(a[e] * scale); o[4 + e] = f2bf(e4[e] * scale); }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2bf(0.f);
    }
    *reinterpret_cast<bf16x8*>(x + (long long)r * D + c) = o;
  }
}

// one block; partials [nblk][S] (pval, pidx) and [nblk][S][3] (plp), nblk <= SCORE_MAXBLK.  Per row: the best partial (lowest index
// among ties), M = max of the blocks' m and z_tgt = max of the blocks' third words (exact in any order: the block that owns the
// target holds its z, every other -inf), the terms s_k expf(m_k - M) (an empty block's is 0) formed by all threads and added by
// lane r for row r in block index order.  A row without a target (z_tgt = -inf) scores -inf.  Thread 0 then writes rows r < n at
// t + r < length <= cap and moves the state; t >= length on entry sets done and writes nothing.
__global__ __launch_bounds__(256) void score_finish_kernel(int* state, const float* pval, const int* pidx, const float* plp, int nblk,
                                                           const int* cand, float* logp, int* greedy, int cap, int S) {
  __shared__ float sv[4], sm[4], sz[4];
  __shared__ int si[4];
  __shared__ int tok[SCORE_MAXS];
  __shared__ float term[SCORE_MAXS][SCORE_MAXBLK + 1], lpv[SCORE_MAXS][2];
  if (state[1]) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int r = 0; r < S; ++r) {
    float v = -INFINITY, M = -INFINITY, z = -INFINITY;
    int i = 0x7fffffff;
    for (int k = threadIdx.x; k < nblk; k += 256) {
      const float pv = pval[(long long)k * S + r];
      const int pi = pidx[(long long)k * S + r];
      if (better(pv, pi, v, i)) { v = pv; i = pi; }
      const float* q = plp + ((long long)k * S + r) * 3;
      M = fmaxf(M, q[0]);
      z = fmaxf(z, q[2]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(i, o, 64);
      if (better(ov, oi, v, i)) { v = ov; i = oi; }
      M = fmaxf(M, __shfl_xor(M, o, 64));
      z = fmaxf(z, __shfl_xor(z, o, 64));
    }
    if (lane == 0) { sv[w] = v; si[w] = i; sm[w] = M; sz[w] = z; }
    __syncthreads();
    M = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    for (int k = threadIdx.x; k < nblk; k += 256) {
      const float* q = plp + ((long long)k * S + r) * 3;
      term[r][k] = q[0] == -INFINITY ? 0.f : __fmul_rn(q[1], expf(q[0] - M));
    }
    if (threadIdx.x == 0) {
      for (int k = 1; k < 4; ++k)
        if (better(sv[k], si[k], v, i)) { v = sv[k]; i = si[k]; }
      tok[r] = i;
      lpv[r][0] = M;
      lpv[r][1] = fmaxf(fmaxf(sz[0], sz[1]), fmaxf(sz[2], sz[3]));
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < S) {
    const int r = threadIdx.x;
    float sum = 0.f;
    for (int k = 0; k < nblk; ++k) sum = __fadd_rn(sum, term[r][k]);
    const float z = lpv[r][1];
    lpv[r][1] = z == -INFINITY ? -INFINITY : z - (lpv[r][0] + logf(sum));
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = state[0];
    if (t < 0) return;
    const int len = max(0, min(cand[0], cap));
    if (t >= len) { state[1] = 1; return; }
    const int n = min(S, len - t);
    for (int r = 0; r < n; ++r) {
      logp[t + r] = lpv[r][1];
      greedy[t + r] = tok[r];
    }
    state[0] = t + n;
    state[1] = t + n >= len ? 1 : 0;
    state[24] = state[24] + 1;
    state[25] = state[25] + n - 1;
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int lap_decode_score_embed(const int* state, const float* table, int row_lo, int row_hi, const int* cand, int cap, void* x,
                                      int S, int D, float scale, void* stream) {
  if (!state || !table || !cand || !x || S < 1 || S > SCORE_MAXS || D != SCORE_D || cap < 1 || !aligned16(table) || !aligned16(x))
    return LAP_ERR_ARG;
  hipLaunchKernelGGL(score_embed_kernel, dim3(S), dim3(256), 0, S_, state, table, row_lo, row_hi, cand, cap, (bf16*)x, D, scale);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

extern "C" int lap_decode_score_finish(int* state, const float* pval, const int* pidx, const float* plp, const int* cand, float* logp,
                                       int* greedy, int S, int cap, void* stream) {
  if (!state || !pval || !pidx || !plp || !cand || !logp || !greedy || S < 1 || S > SCORE_MAXS || cap < 1 ||
      lap_decode_lm_blocks() > SCORE_MAXBLK) return LAP_ERR_ARG;
  hipLaunchKernelGGL(score_finish_kernel, dim3(1), dim3(256), 0, S_, state, pval, pidx, plp, lap_decode_lm_blocks(), cand, logp, greedy,
                     cap, S);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}
