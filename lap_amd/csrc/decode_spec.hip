// Greedy speculative decoding of ONE LAP_AR sequence on a multi-row verify step (lap_amd/speculate.py restates the draft and the
// accept rule in numpy and is their specification).  A verify step runs the fused decode kernels of csrc/decode.hip on S rows
// (2 <= S <= 8) that are the consecutive positions t-1 .. t-1+S-1 of the sequence: row 0 feeds the real last token out[t-1],
// row r the drafted token draft[r-1].  Every row of those kernels is accumulated independently of the batch width, so row r
// computes what the single-token step at t + r computes provided the drafts before it were right; the accept kernel emits tok[0]
// and then tok[r] while draft[r-1] == tok[r-1], which reproduces the greedy decode token for token.
//   draft    one block: the next S-1 tokens after the best anchor of (out[t-2], out[t-1]) in the reference sequence `ref`
//   embed    x[0] = bf16(table[out[t-1]] * sqrt(D)), x[r] = bf16(table[draft[r-1]] * sqrt(D)); an id outside the table (the -1 of
//            a missing draft included) gives a zero row, as in lap_decode_embed
//   accept   one block: the per-row argmax over the LM head's partials (dec_finish_kernel's reduction, lowest index among ties),
//            the accept rule, out[t ..], EOS, t += n, done, and the two counters state[24] (verify steps), state[25] (accepted)
// The QKV and attention variants are instances of decode.hip's templates (lap_decode_spec_qkv, lap_decode_spec_attention); the
// other projections and the greedy LM heads run unchanged at B = S.  All kernels read t = state[0], done = state[1] and return at
// once when done is set.  Device state is written with plain per-lane stores.
#include "common.hpp"
#include "../../include/lap_hip.h"

#define S_ ((hipStream_t)stream)

namespace {

constexpr int SPEC_MAXS = 8;               // rows of a verify step (the decode kernels' DEC_MAXB)
constexpr int SPEC_D = 2048;
constexpr long long NO_ANCHOR = 0x7fffffffffffffffLL;

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// An anchor is an index a < n with ref[a] == out[t-1]; a 2-gram anchor also has a >= 1 and ref[a-1] == out[t-2] (t >= 2).  The
// 2-gram anchor nearest to t-1 wins (the lower a on a tie), else the nearest 1-gram anchor, else a = t-1.  Candidates are ordered
// by the key (|a - (t-1)| << 32) | a, so the choice is a minimum and does not depend on the order of the reduction.
// draft[r] = ref[a+1+r] while a+1+r < n, else -1 (never a token, so never accepted).  n is clamped to [0, cap]: every read of
// ref is below cap.
__global__ __launch_bounds__(256) void spec_draft_kernel(const int* state, const int* ref, const int* nref, const int* out, int cap,
                                                         int* draft, int S) {
  __shared__ long long k2[256], k1[256];
  if (state[1]) return;
  const int t = state[0];
  if (t < 1 || t > cap) return;
  const int n = max(0, min(nref[0], cap));
  const int last = out[t - 1];
  const bool has_prev = t >= 2;
  const int prev = has_prev ? out[t - 2] : 0;
  long long b2 = NO_ANCHOR, b1 = NO_ANCHOR;
  for (int a = threadIdx.x; a < n; a += 256) {
    if (ref[a] != last) continue;
    const int d = a > t - 1 ? a - (t - 1) : (t - 1) - a;
    const long long key = ((long long)d << 32) | (long long)a;
    b1 = min(b1, key);
    if (has_prev && a >= 1 && ref[a - 1] == prev) b2 = min(b2, key);
  }
  k2[threadIdx.x] = b2;
  k1[threadIdx.x] = b1;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      k2[threadIdx.x] = min(k2[threadIdx.x], k2[threadIdx.x + s]);
      k1[threadIdx.x] = min(k1[threadIdx.x], k1[threadIdx.x + s]);
    }
    __syncthreads();
  }
  if ((int)threadIdx.x < S - 1) {
    const long long k = k2[0] != NO_ANCHOR ? k2[0] : k1[0];
    const int a = k != NO_ANCHOR ? (int)(k & 0xffffffffLL) : t - 1;
    const int j = a + 1 + (int)threadIdx.x;
    draft[threadIdx.x] = j < n ? ref[j] : -1;
  }
}

// grid = S: row 0 embeds out[t-1], row r embeds draft[r-1] (dec_embed_kernel's arithmetic)
__global__ __launch_bounds__(256) void spec_embed_kernel(const int* state, const float* table, int row_lo, int row_hi, const int* out,
                                                         const int* draft, int cap, bf16* x, int D, float scale) {
  if (state[1]) return;
  const int r = blockIdx.x, t = state[0];
  if (t < 1 || t > cap) return;
  const int tok = r == 0 ? out[t - 1] : draft[r - 1];
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

// one block.  tok[r] = the best of row r's partials [nblk][S] (lowest index among ties), then thread 0: emit tok[0]; for r = 1 ..
// S-1 go on only while tok[r-1] != eos and draft[r-1] == tok[r-1] and t + r < cap, and emit tok[r].  With n emitted: out[t + i] =
// tok[i], EOS mask, t += n, done, state[24] += 1, state[25] += n - 1.  t >= cap on entry sets done and writes nothing; nothing is
// written past an EOS.  Every store to out is at t + r < cap.
__global__ __launch_bounds__(256) void spec_accept_kernel(int* state, const float* pval, const int* pidx, int nblk, const int* draft,
                                                          int* out, int cap, int S, int eos_token) {
  __shared__ float sv[4];
  __shared__ int si[4];
  __shared__ int tok[SPEC_MAXS];
  if (state[1]) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int r = 0; r < S; ++r) {
    float v = -INFINITY;
    int i = 0x7fffffff;
    for (int k = threadIdx.x; k < nblk; k += 256) {
      const float pv = pval[(long long)k * S + r];
      const int pi = pidx[(long long)k * S + r];
      if (better(pv, pi, v, i)) { v = pv; i = pi; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(i, o, 64);
      if (better(ov, oi, v, i)) { v = ov; i = oi; }
    }
    if (lane == 0) { sv[w] = v; si[w] = i; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int k = 1; k < 4; ++k)
        if (better(sv[k], si[k], v, i)) { v = sv[k]; i = si[k]; }
      tok[r] = i;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int t = state[0];
    if (t < 0) return;
    if (t >= cap) { state[1] = 1; return; }
    int n = 0, e = state[8];
    for (int r = 0; r < S; ++r) {
      if (r > 0 && !(tok[r - 1] != eos_token && draft[r - 1] == tok[r - 1] && t + r < cap)) break;
      out[t + r] = tok[r];
      e |= tok[r] == eos_token ? 1 : 0;
      n = r + 1;
    }
    state[8] = e;
    state[0] = t + n;
    state[1] = (t + n >= cap || e) ? 1 : 0;
    state[24] = state[24] + 1;
    state[25] = state[25] + n - 1;
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int lap_decode_spec_draft(const int* state, const int* ref, const int* nref, const int* out, int cap, int* draft, int S,
                                     void* stream) {
  if (!state || !ref || !nref || !out || !draft || cap < 1 || S < 2 || S > SPEC_MAXS) return LAP_ERR_ARG;
  hipLaunchKernelGGL(spec_draft_kernel, dim3(1), dim3(256), 0, S_, state, ref, nref, out, cap, draft, S);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

extern "C" int lap_decode_spec_embed(const int* state, const float* table, int row_lo, int row_hi, const int* out, const int* draft,
                                     int cap, void* x, int S, int D, float scale, void* stream) {
  if (!state || !table || !out || !draft || !x || S < 2 || S > SPEC_MAXS || D != SPEC_D || cap < 1 || !aligned16(table) || !aligned16(x))
    return LAP_ERR_ARG;
  hipLaunchKernelGGL(spec_embed_kernel, dim3(S), dim3(256), 0, S_, state, table, row_lo, row_hi, out, draft, cap, (bf16*)x, D, scale);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

extern "C" int lap_decode_spec_accept(int* state, const float* pval, const int* pidx, const int* draft, int* out, int S, int cap,
                                      int eos_token, void* stream) {
  if (!state || !pval || !pidx || !draft || !out || S < 2 || S > SPEC_MAXS || cap < 1) return LAP_ERR_ARG;
  hipLaunchKernelGGL(spec_accept_kernel, dim3(1), dim3(256), 0, S_, state, pval, pidx, lap_decode_lm_blocks(), draft, out, cap, S,
                     eos_token);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}
