// Beam search over the rows of one fused LAP_AR decode batch (lap_amd/beam.py is the host restatement and the specification).
// The N <= 8 beams are the rows of a B = N decode; they advance in lockstep on the step counter state[0].  Beside the decode
// state lives the beam buffer, int32 [32]:
//   beam[0 + b]   bits of the f32 score of beam b (the sum of its token log-probabilities; -inf: the beam contributes nothing)
//   beam[8 + b]   beam b has finished (it emitted EOS, or it is padding)
//   beam[16 + b]  the parent of beam b at the last step (the row whose history and K / V it continues)
//   beam[24]      early_stop: done is also set when the rank-0 beam has finished
//   beam[25]      steps whose parent permutation was not the identity (a counter for tools)
// A decode starts from {0, -inf, ...}, nothing finished (`hip.decode_beam_init_words`; a device copy inside the prefill part).
// Three kernels (and, under a grammar, the two described where they stand: a topn over the edges of every row's automaton state and
// the select that also moves that state); each reads t = state[0] and done = state[1], returns at once when done is set, writes device state with plain
// per-lane stores, and never uses an id, a parent or a position outside its range as an address.
//   topn     grid N, 1024 threads per row of stored f32 logits [N][V]: one pass forms the log-sum-exp over the entries > -inf
//            (the pair (m, s) of csrc/decode.hip; a thread's entries in order, the lanes by a shfl_down tree, the waves in order)
//            and every thread's 8 best (logit, id); N rounds of a block argmax (value, then lowest id) then emit the row's N best
//            as cand_logp[b][r] = logit - lse, cand_id[b][r]; missing candidates get id -1.  A row of score -inf writes none, a
//            finished row writes the one candidate (logp 0, id 0).
//   select   one block: lane j < N * N holds candidate j = (score[j / N] + logp, parent j / N, id) and counts the candidates
//            that beat it (score descending, then lower parent, then lower id); rank r < N becomes beam r, ranks nobody takes are
//            finished beams of score -inf, parent = own index, token 0.  Then the histories out[b][0..t) and logp[b][0..t) are
//            permuted by parent: a thread owns column p, loads the N values it will store into registers, then stores them, so no
//            row reads what is already overwritten.  Then out[b][t], logp[b][t], the beam buffer, the EOS words state[8 + b],
//            t + 1 and done = every beam finished, or t + 1 >= cap, or early_stop and beam 0 finished.  t >= cap on entry sets
//            done and writes nothing else, as lap_decode_finish.
//   reorder  gen[l][kv][b][p] <- gen[l][kv][parent[b]][p] for p < min(t, cap): a thread owns one 16-byte slice of (p, dim),
//            loads it from the parent row of every row that moves, then stores.  Nothing is read or written when the permutation
//            is the identity, when a parent is outside [0, N), or at positions >= t.  The step calls it before its layers, when
//            position t - 1 is not yet written: that one stale position moves too and is overwritten later in the same step.
#include "common.hpp"
#include "../../include/lap_hip.h"

#define S_ ((hipStream_t)stream)

namespace {

constexpr int BT = 256;                     // threads of the select and reorder blocks
constexpr int GT = 256, GW = GT / 64;       // threads, waves of a grammar topn block
constexpr int TT = 1024, TW = TT / 64;      // threads, waves of a topn block
constexpr int TU = 8;                       // logits a topn thread loads before it works on them (independent loads in flight)
constexpr int BEAM_MAX = 8;                 // rows of a fused decode
constexpr int BEAM_WORDS = 32;
constexpr int NO_ID = 0x7fffffff;

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

__global__ __launch_bounds__(TT) void beam_topn_kernel(const int* state, const int* beam, const float* logits, int V, int N, int cap,
                                                       float* cand_logp, int* cand_id) {
  __shared__ float redv[TW], redm[TW], reds[TW], s_lse;
  __shared__ int redi[TW];
  if (state[1]) return;
  const int t = state[0];
  if (t < 0 || t >= cap) return;        // (the select kernel sets done)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, row = blockIdx.x;
  float* cl = cand_logp + row * N;
  int* ci = cand_id + row * N;
  const float score = __int_as_float(beam[row]);
  if (!(score > -INFINITY) || beam[8 + row]) {      // (block-uniform) nothing, or the one candidate of a finished row
    if (tid < N) {
      const bool one = score > -INFINITY && tid == 0;
      cl[tid] = one ? 0.f : -INFINITY;
      ci[tid] = one ? 0 : -1;
    }
    return;
  }
  const float* x = logits + (long long)row * V;
  float tv[BEAM_MAX];
  int ti[BEAM_MAX];
#pragma unroll
  for (int k = 0; k < BEAM_MAX; ++k) { tv[k] = -INFINITY; ti[k] = NO_ID; }
  float m = -INFINITY, s = 0.f;
  for (int j0 = tid; j0 < V; j0 += TT * TU) {       // a thread's ids ascend: j0, j0 + TT, ...
    float ld[TU];
#pragma unroll
    for (int u = 0; u < TU; ++u) {
      const int j = j0 + u * TT;
      ld[u] = j < V ? __builtin_nontemporal_load(x + j) : -INFINITY;
    }
#pragma unroll
    for (int u = 0; u < TU; ++u) {
      const float v = ld[u];
      const int j = j0 + u * TT;
      if (!(v > -INFINITY)) continue;   // (-inf, NaN and past the row: outside the sum, no candidate)
      lse_push(v, m, s);
      if (better(v, j, tv[BEAM_MAX - 1], ti[BEAM_MAX - 1])) {
        tv[BEAM_MAX - 1] = v; ti[BEAM_MAX - 1] = j;
#pragma unroll
        for (int k = BEAM_MAX - 1; k > 0; --k) {
          if (better(tv[k], ti[k], tv[k - 1], ti[k - 1])) {
            const float fv = tv[k]; tv[k] = tv[k - 1]; tv[k - 1] = fv;
            const int fi = ti[k]; ti[k] = ti[k - 1]; ti[k - 1] = fi;
          }
        }
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_down(m, o, 64), os = __shfl_down(s, o, 64);
    lse_merge(om, os, m, s);
  }
  if (lane == 0) { redm[w] = m; reds[w] = s; }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < TW; ++k) lse_merge(redm[k], reds[k], m, s);
    s_lse = m > -INFINITY ? __fadd_rn(m, logf(s)) : -INFINITY;
  }
  __syncthreads();
  const float lse = s_lse;
  const bool usable = lse > -INFINITY && lse < INFINITY;        // (a NaN fails both)
  for (int r = 0; r < N; ++r) {         // (block-uniform) round r: the best head of all threads' lists
    float v = tv[0];
    int i = ti[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(i, o, 64);
      if (better(ov, oi, v, i)) { v = ov; i = oi; }
    }
    if (lane == 0) { redv[w] = v; redi[w] = i; }
    __syncthreads();
    v = redv[0]; i = redi[0];
    for (int k = 1; k < TW; ++k)
      if (better(redv[k], redi[k], v, i)) { v = redv[k]; i = redi[k]; }
    if (i != NO_ID && ti[0] == i) {     // the one thread that owns id i drops it
#pragma unroll
      for (int k = 0; k < BEAM_MAX - 1; ++k) { tv[k] = tv[k + 1]; ti[k] = ti[k + 1]; }
      tv[BEAM_MAX - 1] = -INFINITY; ti[BEAM_MAX - 1] = NO_ID;
    }
    if (tid == 0) {
      const bool ok = usable && i != NO_ID;
      cl[r] = ok ? __fsub_rn(v, lse) : -INFINITY;
      ci[r] = ok ? i : -1;
    }
    __syncthreads();                    // (the partials are read before the next round writes them)
  }
}

// One block of 256 threads per row, under a grammar: the row's candidates are the edges of the automaton state q = gstate[row] (the
// CSR automaton of csrc/decode_grammar.hip), so the threads stride over that segment alone, gather logits[row][id] and form the
// log-sum-exp over the segment in grammar_draw_row's order (a thread's entries in order, the lanes by a shfl_down tree, the four
// waves in order).  A thread keeps its 8 best (logit, id, edge); N block-argmax rounds emit cand_logp, cand_id and cand_next =
// next[edge].  q outside [0, Q), a segment outside [0, E] and an id outside [0, V) are never used as an address: such a row writes no
// candidates (every id -1).  A finished row writes the one candidate (logp 0, id 0, next = its own state, which the select keeps).
__global__ __launch_bounds__(GT) void beam_grammar_topn_kernel(const int* state, const int* beam, const int* gstate, const int* offsets,
                                                               const int* ids, const int* next, int Q, int E, const float* logits, int V,
                                                               int N, int cap, float* cand_logp, int* cand_id, int* cand_next) {
  __shared__ float redv[GW], redm[GW], reds[GW], s_lse;
  __shared__ int redi[GW], rede[GW];
  if (state[1]) return;
  const int t = state[0];
  if (t < 0 || t >= cap) return;        // (the select kernel sets done)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, row = blockIdx.x;
  float* cl = cand_logp + row * N;
  int* ci = cand_id + row * N;
  int* cn = cand_next + row * N;
  const float score = __int_as_float(beam[row]);
  const int q = gstate[row];
  if (!(score > -INFINITY) || beam[8 + row]) {      // (block-uniform) nothing, or the one candidate of a finished row
    if (tid < N) {
      const bool one = score > -INFINITY && tid == 0;
      cl[tid] = one ? 0.f : -INFINITY;
      ci[tid] = one ? 0 : -1;
      cn[tid] = one ? q : -1;
    }
    return;
  }
  int lo = 0, hi = 0, bad = 0;
  if (q >= 0 && q < Q) { lo = offsets[q]; hi = offsets[q + 1]; }
  if (lo < 0 || hi > E || hi < lo) { bad = 1; lo = hi = 0; }
  const float* x = logits + (long long)row * V;
  float tv[BEAM_MAX];
  int ti[BEAM_MAX], te[BEAM_MAX];
#pragma unroll
  for (int k = 0; k < BEAM_MAX; ++k) { tv[k] = -INFINITY; ti[k] = NO_ID; te[k] = -1; }
  float m = -INFINITY, s = 0.f;
  for (int e = lo + tid; e < hi; e += GT) {         // a thread's edges, hence its ids, ascend
    const int id = ids[e];
    if (id < 0 || id >= V) { bad = 1; continue; }
    const float v = x[id];
    if (!(v > -INFINITY)) continue;     // (-inf and NaN: outside the sum, no candidate)
    lse_push(v, m, s);
    if (better(v, id, tv[BEAM_MAX - 1], ti[BEAM_MAX - 1])) {
      tv[BEAM_MAX - 1] = v; ti[BEAM_MAX - 1] = id; te[BEAM_MAX - 1] = e;
#pragma unroll
      for (int k = BEAM_MAX - 1; k > 0; --k) {
        if (better(tv[k], ti[k], tv[k - 1], ti[k - 1])) {
          const float fv = tv[k]; tv[k] = tv[k - 1]; tv[k - 1] = fv;
          const int fi = ti[k]; ti[k] = ti[k - 1]; ti[k - 1] = fi;
          const int fe = te[k]; te[k] = te[k - 1]; te[k - 1] = fe;
        }
      }
    }
  }
  if (__syncthreads_or(bad)) {          // (block-uniform) a state, segment or id out of range: the row offers nothing
    if (tid < N) { cl[tid] = -INFINITY; ci[tid] = -1; cn[tid] = -1; }
    return;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_down(m, o, 64), os = __shfl_down(s, o, 64);
    lse_merge(om, os, m, s);
  }
  if (lane == 0) { redm[w] = m; reds[w] = s; }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < GW; ++k) lse_merge(redm[k], reds[k], m, s);
    s_lse = m > -INFINITY ? __fadd_rn(m, logf(s)) : -INFINITY;
  }
  __syncthreads();
  const float lse = s_lse;
  const bool usable = lse > -INFINITY && lse < INFINITY;        // (a NaN fails both)
  for (int r = 0; r < N; ++r) {         // (block-uniform) round r: the best head of all threads' lists
    float v = tv[0];
    int i = ti[0], e = te[0];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(i, o, 64), oe = __shfl_xor(e, o, 64);
      if (better(ov, oi, v, i)) { v = ov; i = oi; e = oe; }
    }
    if (lane == 0) { redv[w] = v; redi[w] = i; rede[w] = e; }
    __syncthreads();
    v = redv[0]; i = redi[0]; e = rede[0];
    for (int k = 1; k < GW; ++k)
      if (better(redv[k], redi[k], v, i)) { v = redv[k]; i = redi[k]; e = rede[k]; }
    if (e >= 0 && te[0] == e) {         // the one thread that owns edge e drops it
#pragma unroll
      for (int k = 0; k < BEAM_MAX - 1; ++k) { tv[k] = tv[k + 1]; ti[k] = ti[k + 1]; te[k] = te[k + 1]; }
      tv[BEAM_MAX - 1] = -INFINITY; ti[BEAM_MAX - 1] = NO_ID; te[BEAM_MAX - 1] = -1;
    }
    if (tid == 0) {
      const bool ok = usable && e >= 0;             // (e in [lo, hi), inside [0, E))
      cl[r] = ok ? __fsub_rn(v, lse) : -INFINITY;
      ci[r] = ok ? i : -1;
      cn[r] = ok ? next[e] : -1;
    }
    __syncthreads();                    // (the partials are read before the next round writes them)
  }
}

// GRAMMAR: the select of a grammar beam step.  cand_next[j] is the automaton state after candidate j; gstate[r] becomes the state of
// beam r's parent when that parent had finished or beam r is padding (its parent is its own index), else the candidate's next
// state.  The N old states are loaded before the barrier and stored after it.
template <bool GRAMMAR>
__global__ __launch_bounds__(BT) void beam_select_kernel(int* state, int* beam, const float* cand_logp, const int* cand_id, int N,
                                                         int V, int* out, float* logp, int cap, int eos, int* gstate,
                                                         const int* cand_next) {
  __shared__ float c_s[BEAM_MAX * BEAM_MAX], c_lp[BEAM_MAX * BEAM_MAX], n_lp[BEAM_MAX], n_sc[BEAM_MAX];
  __shared__ int c_id[BEAM_MAX * BEAM_MAX], c_ok[BEAM_MAX * BEAM_MAX], n_par[BEAM_MAX], n_tok[BEAM_MAX], n_fin[BEAM_MAX];
  __shared__ int n_nx[BEAM_MAX], n_keep[BEAM_MAX];
  const int tid = threadIdx.x;
  if (state[1]) return;
  const int t = state[0];
  if (t >= cap || t < 0) {              // (the budget is spent: nothing is written but the flag, as in lap_decode_finish)
    if (tid == 0) state[1] = 1;
    return;
  }
  const int NN = N * N;
  if (tid < BEAM_MAX * BEAM_MAX) {
    float sc = -INFINITY, lp = 0.f;
    int id = -1, ok = 0;
    if (tid < NN) {
      id = cand_id[tid];
      lp = cand_logp[tid];
      sc = __fadd_rn(__int_as_float(beam[tid / N]), lp);
      ok = (id >= 0 && id < V && sc > -INFINITY) ? 1 : 0;       // (a NaN score is no candidate)
    }
    c_s[tid] = sc; c_lp[tid] = lp; c_id[tid] = id; c_ok[tid] = ok;
  }
  if (tid < BEAM_MAX) { n_par[tid] = tid; n_tok[tid] = 0; n_lp[tid] = 0.f; n_sc[tid] = -INFINITY; n_fin[tid] = 1; }
  if constexpr (GRAMMAR) {
    if (tid < BEAM_MAX) { n_nx[tid] = 0; n_keep[tid] = 1; }
  }
  __syncthreads();
  if (tid < NN && c_ok[tid]) {
    const int b = tid / N, id = c_id[tid];
    const float sc = c_s[tid];
    int rank = 0;
    for (int k = 0; k < NN; ++k) {
      if (k == tid || !c_ok[k]) continue;
      const int kb = k / N;
      rank += (c_s[k] > sc || (c_s[k] == sc && (kb < b || (kb == b && c_id[k] < id)))) ? 1 : 0;
    }
    if (rank < N) {
      n_par[rank] = b; n_tok[rank] = id; n_lp[rank] = c_lp[tid]; n_sc[rank] = sc;
      n_fin[rank] = (beam[8 + b] || id == eos) ? 1 : 0;
      if constexpr (GRAMMAR) { n_nx[rank] = cand_next[tid]; n_keep[rank] = beam[8 + b] ? 1 : 0; }
    }
  }
  __syncthreads();
  int old_q = 0;
  if constexpr (GRAMMAR) {
    if (tid < N) old_q = gstate[n_par[tid]];        // (n_par in [0, N)) every old state is in a register ...
    __syncthreads();                                // ... before the first is overwritten below
  }
  int par[BEAM_MAX];
  bool ident = true;
#pragma unroll
  for (int k = 0; k < BEAM_MAX; ++k) {
    par[k] = k < N ? n_par[k] : k;      // (in [0, N): written above from b = tid / N < N, or k itself)
    ident = ident && par[k] == k;
  }
  if (!ident) {
    for (int p = tid; p < t; p += BT) {     // column p of both histories: all loads, then all stores
      int vo[BEAM_MAX];
      float vl[BEAM_MAX];
#pragma unroll
      for (int k = 0; k < BEAM_MAX; ++k)
        if (k < N) { vo[k] = out[(long long)par[k] * cap + p]; vl[k] = logp[(long long)par[k] * cap + p]; }
#pragma unroll
      for (int k = 0; k < BEAM_MAX; ++k)
        if (k < N) { out[(long long)k * cap + p] = vo[k]; logp[(long long)k * cap + p] = vl[k]; }
    }
  }
  if (tid < N) {
    out[(long long)tid * cap + t] = n_tok[tid];
    logp[(long long)tid * cap + t] = n_lp[tid];
    beam[tid] = __float_as_int(n_sc[tid]);
    beam[8 + tid] = n_fin[tid];
    beam[16 + tid] = n_par[tid];
    state[8 + tid] = n_fin[tid];
    if constexpr (GRAMMAR) gstate[tid] = n_keep[tid] ? old_q : n_nx[tid];
  }
  if (tid == 0) {
    int all = 1;
    for (int k = 0; k < N; ++k) all &= n_fin[k];
    if (!ident) beam[25] = beam[25] + 1;
    state[0] = t + 1;
    state[1] = (t + 1 >= cap || all || (beam[24] && n_fin[0])) ? 1 : 0;
  }
}

// gen viewed as uint4 [L2][N][cap * spp], spp = the 16-byte slices of one position (head_dim / 8)
template <int N>
__global__ __launch_bounds__(BT) void beam_reorder_kernel(const int* state, const int* beam, uint4* gen, int cap, int spp) {
  if (state[1]) return;
  const int t = min(state[0], cap);
  if (t <= 0) return;
  int par[N];
  bool ident = true, bad = false;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    par[k] = beam[16 + k];
    bad = bad || par[k] < 0 || par[k] >= N;
    ident = ident && par[k] == k;
  }
  if (ident || bad) return;
  const long long idx = (long long)blockIdx.x * BT + threadIdx.x;
  if (idx >= (long long)t * spp) return;
  const long long rowstride = (long long)cap * spp;
  uint4* base = gen + (long long)blockIdx.y * N * rowstride + idx;
  // (eight named registers, not an array: all loads stand before the first store)
  uint4 n0, n1, n2, n3, n4, n5, n6, n7;
#define BEAM_LD(k) if constexpr (N > k) n##k = base[par[k] * rowstride];
#define BEAM_ST(k) if constexpr (N > k) { if (par[k] != k) base[k * rowstride] = n##k; }
  BEAM_LD(0) BEAM_LD(1) BEAM_LD(2) BEAM_LD(3) BEAM_LD(4) BEAM_LD(5) BEAM_LD(6) BEAM_LD(7)
  BEAM_ST(0) BEAM_ST(1) BEAM_ST(2) BEAM_ST(3) BEAM_ST(4) BEAM_ST(5) BEAM_ST(6) BEAM_ST(7)
#undef BEAM_LD
#undef BEAM_ST
}

}  // namespace

extern "C" int lap_decode_beam_words(void) { return BEAM_WORDS; }

extern "C" int lap_decode_beam_topn(const int* state, const int* beam, const float* logits, float* cand_logp, int* cand_id, int N,
                                    int V, int cap, void* stream) {
  if (!state || !beam || !logits || !cand_logp || !cand_id || N < 1 || N > BEAM_MAX || V < 1 || V > (1 << 30) || cap < 1) return LAP_ERR_ARG;
  hipLaunchKernelGGL(beam_topn_kernel, dim3(N), dim3(TT), 0, S_, state, beam, logits, V, N, cap, cand_logp, cand_id);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

extern "C" int lap_decode_beam_select(int* state, int* beam, const float* cand_logp, const int* cand_id, int* out, float* logp, int N,
                                      int V, int cap, int eos_token, void* stream) {
  if (!state || !beam || !cand_logp || !cand_id || !out || !logp || N < 1 || N > BEAM_MAX || V < 1 || cap < 1) return LAP_ERR_ARG;
  hipLaunchKernelGGL(beam_select_kernel<false>, dim3(1), dim3(BT), 0, S_, state, beam, cand_logp, cand_id, N, V, out, logp, cap, eos_token,
                     (int*)nullptr, (const int*)nullptr);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

extern "C" int lap_decode_beam_grammar_topn(const int* state, const int* beam, const int* gstate, const int* offsets, const int* ids,
                                            const int* next, int Q, int E, const float* logits, float* cand_logp, int* cand_id,
                                            int* cand_next, int N, int V, int cap, void* stream) {
  if (!state || !beam || !gstate || !offsets || !ids || !next || !logits || !cand_logp || !cand_id || !cand_next || Q < 1 || E < 1 ||
      E > (1 << 30) || N < 1 || N > BEAM_MAX || V < 1 || V > (1 << 30) || cap < 1)
    return LAP_ERR_ARG;
  hipLaunchKernelGGL(beam_grammar_topn_kernel, dim3(N), dim3(GT), 0, S_, state, beam, gstate, offsets, ids, next, Q, E, logits, V, N, cap,
                     cand_logp, cand_id, cand_next);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

extern "C" int lap_decode_beam_grammar_select(int* state, int* beam, int* gstate, const float* cand_logp, const int* cand_id,
                                              const int* cand_next, int* out, float* logp, int N, int V, int cap, int eos_token,
                                              void* stream) {
  if (!state || !beam || !gstate || !cand_logp || !cand_id || !cand_next || !out || !logp || N < 1 || N > BEAM_MAX || V < 1 || cap < 1)
    return LAP_ERR_ARG;
  hipLaunchKernelGGL(beam_select_kernel<true>, dim3(1), dim3(BT), 0, S_, state, beam, cand_logp, cand_id, N, V, out, logp, cap, eos_token,
                     gstate, cand_next);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

extern "C" int lap_decode_beam_reorder(const int* state, const int* beam, void* gen, int N, int L2, int cap, int head_dim, void* stream) {
  if (!state || !beam || !gen || N < 1 || N > BEAM_MAX || L2 < 1 || L2 > 65535 || cap < 1 || head_dim < 8 || head_dim % 8 ||
      ((uintptr_t)gen & 15))
    return LAP_ERR_ARG;
  const int spp = head_dim / 8;
  const long long slices = (long long)cap * spp;
  const long long blocks = (slices + BT - 1) / BT;
  if (blocks > 0x7fffffffLL) return LAP_ERR_ARG;
  const dim3 grid((unsigned)blocks, L2);
  switch (N) {      // (one beam: its parent is itself)
    case 1: return LAP_OK;
#define BEAM_REORDER_CASE(N_) \
    case N_: hipLaunchKernelGGL(beam_reorder_kernel<N_>, grid, dim3(BT), 0, S_, state, beam, (uint4*)gen, cap, spp); break;
    BEAM_REORDER_CASE(2) BEAM_REORDER_CASE(3) BEAM_REORDER_CASE(4) BEAM_REORDER_CASE(5)
    BEAM_REORDER_CASE(6) BEAM_REORDER_CASE(7) BEAM_REORDER_CASE(8)
#undef BEAM_REORDER_CASE
  }
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}
