// Grammar-constrained token draw of the fused LAP_AR decode (lap_amd/grammar.py `decode_reference` is the host restatement and
// the specification).  A deterministic automaton over token ids lives on the device in CSR form: state q allows the ids
// ids[offsets[q] .. offsets[q+1]) (strictly ascending) and edge e leads to state next[e]; gstate[b] is the state of row b.
// ONE kernel, one block of 256 threads per row of stored f32 logits [B][V] (the SUBSET LM head over the union of all edges wrote
// them; -inf elsewhere):
//   the threads stride over the segment of q = gstate[b]; an entry gathers logits[b][id] and forms the sampler's score
//   float(logit * inv_t) + g(seed, t, b, id) (lap_sampling::gumbel_scores_at: the noise of the VOCABULARY index, as everywhere;
//   inv_t == 0 or no sampling words: the plain logit); the block reduces with better() (value, then lowest id; the ids of a
//   segment ascend, so that is also the lowest edge) and carries the winning edge; thread 0 writes out[b][t], the EOS bit,
//   logp[b][t] and gstate[b] = next[edge].
// logp (optional): z_tok - (M + logf(S)) over the segment, z = float(logit * inv_t) (the raw logit when greedy), with the running
// pair (m, s) of csrc/decode.hip's lse_push / lse_merge, restated here.  The order of the additions is fixed: a thread's entries
// in order, the lanes of a wave by a shfl_down tree (lane 0 holds the wave's pair), the four waves in order, so a replay
// reproduces the bits.
// Bookkeeping: that of lap_decode_filter_finish.  Nothing is written when done is set; t >= cap sets done and writes nothing; a
// block writes its row, fences and adds one to state[2]; the block that finds B - 1 there is the last, and it alone advances t,
// sets done and puts the counter back to zero, so every block has read t before it moves.  No block waits for another.
// Addresses: q outside [0, Q), a segment outside [0, E], an id outside [0, V) or an edge whose logits are all NaN are never used
// as an address: such a row emits eos_token and keeps its gstate.
// Jump-forward decoding (`jump_forward=S`: ONE sequence on steps of S rows, the arrangement of csrc/decode_spec.hip) adds two
// kernels: lap_decode_grammar_draft, which drafts the token of every state that has a single edge, and
// lap_decode_grammar_spec_finish, which draws the S rows in sequence with the row body of the kernel above and accepts the
// longest verified run.  They are described where they stand.
#include "common.hpp"
#include "sampling.hpp"
#include "../../include/lap_hip.h"

#define S_ ((hipStream_t)stream)

namespace {

constexpr int GT = 256, GW = GT / 64;       // threads, waves per block
constexpr int GRAM_MAXB = 8;                // rows of a fused decode

struct GramP {
  int* state; const int* samp;               // the decode state, the sampling words (NULL: greedy)
  int* gstate;                               // [B] the automaton state of every row
  const int* offsets; const int* ids; const int* next; int Q, E;
  const float* x; int V;                     // logits [B][V]
  int* out; float* logp; int cap, eos, B;    // out [B][cap], logp [B][cap] or NULL
};

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// (csrc/decode.hip's pair, to the letter: every expf argument is <= 0, and m == -inf is tested before a difference is formed)
__device__ __forceinline__ void lse_push(float z, float& m, float& s) {
  const float e = (m == -INFINITY || z == -INFINITY) ? 0.f : expf(-fabsf(z - m));
  if (z > m) { s = __fadd_rn(__fmul_rn(s, e), 1.0f); m = z; }
  else s = __fadd_rn(s, e);
}
__device__ __forceinline__ void lse_merge(float m2, float s2, float& m, float& s) {
  const float M = fmaxf(m, m2);
  if (M == -INFINITY) return;          // both empty: (m, s) stays (-inf, 0)
  s = __fadd_rn(__fmul_rn(s, expf(m - M)), __fmul_rn(s2, expf(m2 - M)));
  m = M;
}

// What one row draws, valid on thread 0 of the block: the token (eos_token for a bad row), the state after it (q itself for a bad
// row), and the token's log-probability over the segment of q (want_lp).
struct GramDraw { int tok, next; float logp; };

// The draw of ONE row by the whole block: `x` its f32 logits [V], q its automaton state, (t, row) the step and row index of the
// noise.  Every thread of the block calls it (it holds a __syncthreads); the result is valid on thread 0.  Both kernels below
// call this body, so a row of the multi-row finish has the bits of lap_decode_grammar_finish on the same state and logits.  A
// caller that calls it again must put a __syncthreads between the calls (the shared partials are read by thread 0 after the
// barrier inside).
__device__ __forceinline__ GramDraw grammar_draw_row(const GramP& p, const float* x, int q, int t, int row, bool want_lp) {
  __shared__ float redv[GW], redz[GW], redm[GW], reds[GW];
  __shared__ int redi[GW], rede[GW], redbad[GW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  float inv_t = 0.f;
  uint32_t seed_lo = 0, seed_hi = 0;
  if (p.samp) { seed_lo = (uint32_t)p.samp[0]; seed_hi = (uint32_t)p.samp[1]; inv_t = __int_as_float(p.samp[2]); }
  const bool greedy = inv_t == 0.f;
  const int V = p.V;

  int lo = 0, hi = 0, bad = 0;
  if (q >= 0 && q < p.Q) { lo = p.offsets[q]; hi = p.offsets[q + 1]; }
  if (lo < 0 || hi > p.E || hi <= lo) { bad = 1; lo = hi = 0; }      // (also q out of range: the empty segment)

  float best = -INFINITY, bz = -INFINITY, lm = -INFINITY, ls = 0.f;
  int bi = 0x7fffffff, be = -1;
  for (int e = lo + tid; e < hi; e += GT) {
    const int id = p.ids[e];
    if (id < 0 || id >= V) { bad = 1; continue; }
    const float v = x[id];
    const float z = greedy ? v : __fmul_rn(v, inv_t);
    float s = v, s1;
    if (!greedy) lap_sampling::gumbel_scores_at(v, v, inv_t, seed_lo, seed_hi, (uint32_t)t, (uint32_t)row, (uint32_t)id, (uint32_t)id, s, s1);
    if (better(s, id, best, bi)) { best = s; bi = id; be = e; bz = z; }
    if (want_lp) lse_push(z, lm, ls);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_down(best, o, 64), oz = __shfl_down(bz, o, 64);
    const int oi = __shfl_down(bi, o, 64), oe = __shfl_down(be, o, 64);
    if (better(ov, oi, best, bi)) { best = ov; bi = oi; be = oe; bz = oz; }
    bad |= __shfl_down(bad, o, 64);
    if (want_lp) {                      // (block-uniform)
      const float om = __shfl_down(lm, o, 64), os = __shfl_down(ls, o, 64);
      lse_merge(om, os, lm, ls);
    }
  }
  if (lane == 0) { redv[w] = best; redi[w] = bi; rede[w] = be; redz[w] = bz; redm[w] = lm; reds[w] = ls; redbad[w] = bad; }
  __syncthreads();
  GramDraw d{p.eos, q, -INFINITY};
  if (tid != 0) return d;
  for (int k = 1; k < GW; ++k) {
    if (better(redv[k], redi[k], best, bi)) { best = redv[k]; bi = redi[k]; be = rede[k]; bz = redz[k]; }
    bad |= redbad[k];
    if (want_lp) lse_merge(redm[k], reds[k], lm, ls);
  }
  const bool ok = !bad && be >= 0;      // (be < 0 with a clean segment: every score was NaN)
  if (ok) { d.tok = bi; d.next = p.next[be]; }
  if (want_lp) d.logp = (ok && lm > -INFINITY) ? bz - (lm + logf(ls)) : -INFINITY;
  return d;
}

__global__ __launch_bounds__(GT) void grammar_finish_kernel(GramP p) {
  const int tid = threadIdx.x, row = blockIdx.x;
  if (p.state[1]) return;
  const int t = p.state[0];
  if (t >= p.cap || t < 0) {            // (the budget is spent: nothing is written but the flag, as in lap_decode_finish)
    if (row == 0 && tid == 0) p.state[1] = 1;
    return;
  }
  const bool want_lp = p.logp != nullptr;
  const int q = p.gstate[row];
  const GramDraw d = grammar_draw_row(p, p.x + (long long)row * p.V, q, t, row, want_lp);
  if (tid != 0) return;
  const int tok = d.tok;
  p.out[(long long)row * p.cap + t] = tok;
  if (want_lp) p.logp[(long long)row * p.cap + t] = d.logp;
  p.gstate[row] = d.next;          // (a bad row: q itself)
  const int eb = p.state[8 + row] | (tok == p.eos ? 1 : 0);
  p.state[8 + row] = eb;
  __threadfence();
  if (atomicAdd(&p.state[2], 1) == p.B - 1) {        // the last block to arrive: t + 1, done
    __threadfence();
    int all = 1;
    for (int b = 0; b < p.B; ++b) all &= __hip_atomic_load(&p.state[8 + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    p.state[2] = 0;
    p.state[0] = t + 1;
    p.state[1] = (t + 1 >= p.cap || all) ? 1 : 0;
  }
}

// ---- jump-forward decoding (lap_amd/speculate.py `grammar_drafts` / `grammar_verify` restate the two kernels below)
// One block; thread 0 walks.  lap_decode_spec_draft has written the raw reference drafts to draft[0 .. S-2].  From q = gstate[0], for
// r = 0 .. S-2: a state with one edge drafts that id (the token is known before the model runs); otherwise the raw draft[r] is kept
// when it is an edge of q (binary search in the segment); otherwise this draft and every later one is -1.  After a drafted token q
// moves along its edge; drafts after a drafted EOS are -1.  A q outside [0, Q), a segment outside [0, E] and an id outside [0, V)
// are never used as an address: the remaining drafts are -1.  gstate is not written.
__global__ __launch_bounds__(64) void grammar_draft_kernel(const int* state, const int* gstate, const int* offsets, const int* ids,
                                                           const int* next, int Q, int E, int V, int cap, int eos, int* draft, int S) {
  if (threadIdx.x != 0 || state[1]) return;
  const int t = state[0];
  if (t < 1 || t > cap) return;         // (lap_decode_spec_draft's own condition: it wrote nothing either)
  int q = gstate[0];
  bool live = true;
  for (int r = 0; r < S - 1; ++r) {
    int d = -1;
    if (live) {
      live = false;
      if (q >= 0 && q < Q) {
        const int lo = offsets[q], hi = offsets[q + 1];
        if (lo >= 0 && hi <= E && hi > lo) {
          int e = -1;
          if (hi - lo == 1) {
            e = lo;
          } else {
            const int want = draft[r];
            int a = lo, b = hi;           // the first entry >= want in [lo, hi)
            while (a < b) {
              const int m = a + ((b - a) >> 1);
              if (ids[m] < want) a = m + 1; else b = m;
            }
            if (a < hi && ids[a] == want) e = a;
          }
          if (e >= 0) {
            const int id = ids[e];
            if (id >= 0 && id < V) {
              d = id;
              q = next[e];
              live = id != eos;
            }
          }
        }
      }
    }
    draft[r] = d;
  }
}

// One block of 256 threads; the S rows of stored logits [S][V] in sequence, because row r's state is the edge row r-1 took.  Row r
// draws with grammar_draw_row at step t + r and row index 0: the bits of lap_decode_grammar_finish of a B = 1 decode at that step.
// The accept rule is lap_decode_spec_accept's: row 0 is emitted; row r only while tok[r-1] != eos, draft[r-1] == tok[r-1] and
// t + r < cap.  With n emitted: out[t + i], logp[t + i], the EOS bit, gstate[0] = the state after the last emitted token, t += n,
// done, state[24] += 1, state[25] += n - 1.  t >= cap on entry sets done and writes nothing; every store is at t + r < cap.
__global__ __launch_bounds__(GT) void grammar_spec_finish_kernel(GramP p, const int* draft, int S) {
  __shared__ int s_go, s_q;
  const int tid = threadIdx.x;
  if (p.state[1]) return;
  const int t = p.state[0];
  if (t >= p.cap || t < 0) {
    if (tid == 0) p.state[1] = 1;
    return;
  }
  const bool want_lp = p.logp != nullptr;
  int q = p.gstate[0];
  int n = 0, eb = 0;
  for (int r = 0; r < S; ++r) {         // (block-uniform: every thread leaves the loop at the same r)
    const GramDraw d = grammar_draw_row(p, p.x + (long long)r * p.V, q, t + r, 0, want_lp);
    if (tid == 0) {
      p.out[t + r] = d.tok;             // t + r < cap: r == 0 by the test above, r > 0 by the accept rule below
      if (want_lp) p.logp[t + r] = d.logp;
      eb |= d.tok == p.eos ? 1 : 0;
      n = r + 1;
      s_q = d.next;
      s_go = (r + 1 < S && d.tok != p.eos && draft[r] == d.tok && t + r + 1 < p.cap) ? 1 : 0;
    }
    __syncthreads();                    // (also: thread 0 has read the shared partials of this row before the next row writes them)
    if (!s_go) break;
    q = s_q;
  }
  if (tid != 0) return;
  p.gstate[0] = s_q;
  const int e = p.state[8] | eb;
  p.state[8] = e;
  p.state[0] = t + n;
  p.state[1] = (t + n >= p.cap || e) ? 1 : 0;
  p.state[24] = p.state[24] + 1;
  p.state[25] = p.state[25] + n - 1;
}

}  // namespace

extern "C" int lap_decode_grammar_finish(int* state, const int* sampling, int* gstate, const int* offsets, const int* ids,
                                         const int* next, int Q, int E, const float* logits, int* out, float* logp, int B, int V,
                                         int cap, int eos_token, void* stream) {
  if (!state || !gstate || !offsets || !ids || !next || !logits || !out || Q < 1 || E < 1 || B < 1 || B > GRAM_MAXB || V < 2 || cap < 1)
    return LAP_ERR_ARG;
  GramP p{};
  p.state = state; p.samp = sampling; p.gstate = gstate; p.offsets = offsets; p.ids = ids; p.next = next; p.Q = Q; p.E = E;
  p.x = logits; p.V = V; p.out = out; p.logp = logp; p.cap = cap; p.eos = eos_token; p.B = B;
  hipLaunchKernelGGL(grammar_finish_kernel, dim3(B), dim3(GT), 0, S_, p);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

extern "C" int lap_decode_grammar_draft(const int* state, const int* gstate, const int* offsets, const int* ids, const int* next, int Q,
                                        int E, int V, int cap, int eos_token, int* draft, int S, void* stream) {
  if (!state || !gstate || !offsets || !ids || !next || !draft || Q < 1 || E < 1 || V < 2 || cap < 1 || S < 2 || S > GRAM_MAXB)
    return LAP_ERR_ARG;
  hipLaunchKernelGGL(grammar_draft_kernel, dim3(1), dim3(64), 0, S_, state, gstate, offsets, ids, next, Q, E, V, cap, eos_token, draft, S);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

extern "C" int lap_decode_grammar_spec_finish(int* state, const int* sampling, int* gstate, const int* offsets, const int* ids,
                                              const int* next, int Q, int E, const float* logits, const int* draft, int* out,
                                              float* logp, int S, int V, int cap, int eos_token, void* stream) {
  if (!state || !gstate || !offsets || !ids || !next || !logits || !draft || !out || Q < 1 || E < 1 || S < 2 || S > GRAM_MAXB || V < 2 ||
      cap < 1)
    return LAP_ERR_ARG;
  GramP p{};
  p.state = state; p.samp = sampling; p.gstate = gstate; p.offsets = offsets; p.ids = ids; p.next = next; p.Q = Q; p.E = E;
  p.x = logits; p.V = V; p.out = out; p.logp = logp; p.cap = cap; p.eos = eos_token; p.B = 1;
  hipLaunchKernelGGL(grammar_spec_finish_kernel, dim3(1), dim3(GT), 0, S_, p, draft, S);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}
