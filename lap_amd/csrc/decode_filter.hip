// Top-k and nucleus (top-p) filtering of a device-sampled LAP_AR token draw (lap_amd/sampling.py `filter_keep` is the host
// restatement and the specification).  ONE kernel body, one block of 1024 threads per row of stored f32 logits [rows][V]:
//   z[j] = float(logit[j] * inv_t), the product the sampler forms; the candidates are the entries with z > -inf (a constrained
//   decode leaves -inf outside its set), ordered by z descending, then index ascending (the tie rule of better());
//   top_k keeps the first k of that order; top_p keeps, of those, rank r while c_{r-1} < p W (w = exp(z - max z), W the mass of
//   what top_k kept, c the cumulative mass in order; rank 0 always); the token is the argmax over the kept entries of the score
//   lap_sampling::gumbel_scores_at gives vocabulary index j, so a neutral filter draws the unfiltered sampler's token.
//
// The cut is found by a radix select over the order-preserving 32-bit key of z, four passes of 8 bits over the row; a bucket
// keeps an integer count and its mass as a 64-bit fixed-point integer, q = floor(exp(z - M) 2^40) (q <= 2^40, so a row of up to
// 2^22 entries sums below 2^63).  Integer sums do not depend on the order of the additions: the cut is the same in every replay
// and for every schedule of the LDS atomics.  A thread adds a run of entries of one bucket with one atomic (the top digit of a
// float key is its sign and seven exponent bits, which a row fills very unevenly).
//   select by count (top_k):  T with #(key > T) < k <= #(key >= T); of the entries equal to T the first m = k - #(key > T) by
//                             index are kept; W = mass(key > T) + m q(T)
//   select by mass (top_p):   tau = ceil(p W); T with mass(key > T) < tau <= mass(key >= T); m = ceil((tau - mass(key > T)) / q(T))
//                             (the ties all have q(T)).  The cumulative masses of the whole order are those of top_k's prefix, and
//                             tau <= W = c_{k-1}, so this select needs no knowledge of k and keeps at most k entries.
// The stricter of the two cuts holds.  The last pass gives every wave a contiguous range of the row, so that the index order of
// the entries equal to T is a running ballot count (with the earlier waves' counts as its base, from a counting pass that runs
// only when a select ran), and takes the argmax of the score over the kept entries.
// q: d = z - M is formed exactly as hi + lo (two-sum), q = expf(hi) (1 + lo) 2^40 truncated: relative error 1.5 2^-23 (expf is
// within 1 ulp), absolute 2^-40; FILTER_MARGIN of lap_amd/sampling.py is derived from these two.
// No block waits for another.  The fused entry (grid = B) counts arrivals in state[2]: a block writes its token, EOS bit and
// log-probability, fences and adds one; the block that finds B - 1 there is the last, and it alone advances t, sets done and puts
// the counter back to zero, so every block has read t before it moves.  k and p are clamped before use; every address comes from
// a loop index below V or from the row index.
#include "common.hpp"
#include "sampling.hpp"
#include "../../include/lap_hip.h"

#define S_ ((hipStream_t)stream)

namespace {

constexpr int FT = 1024, FW = FT / 64;      // threads, waves per block
constexpr int FILT_MAXB = 8;                // rows of a fused decode
constexpr int FILT_MAXV = 1 << 22;          // q <= 2^40 each: the row's mass stays below 2^63
typedef unsigned long long u64;

struct FiltP {
  const float* x; int ld, V;                 // logits [rows][ld]
  int* state; const int* samp; const int* filt;      // FUSED: the decode state, the sampling words, the filter words
  float inv_t; uint32_t seed_lo, seed_hi, step; int top_k; float top_p;     // host step: the same by value
  int* out; int cap, eos, B; float* logp;    // FUSED: out [B][cap], logp [B][cap] or NULL; host step: out [rows]
  int* kept; float* cut;                     // debug, NULL in production: the size of the kept set, the smallest kept z
};

struct Cut { uint32_t T, m, kept; u64 mass; };      // kept = #(key > T) + m; mass: of the kept entries

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

__device__ __forceinline__ float zof(float v, float inv_t) { return inv_t != 0.f ? __fmul_rn(v, inv_t) : v; }

// order-preserving key: z1 > z2 <=> key(z1) > key(z2); -0 and +0 share a key, as they compare equal
__device__ __forceinline__ uint32_t zkey(float z) {
  const uint32_t u = z == 0.f ? 0u : __float_as_uint(z);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_z(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ u64 zmass(float z, float M) {
  const float hi = __fsub_rn(z, M), bb = __fsub_rn(hi, z);
  const float lo = __fsub_rn(__fsub_rn(z, __fsub_rn(hi, bb)), __fadd_rn(M, bb));      // z - M == hi + lo exactly
  if (!(hi > -64.f) || !(hi <= 0.f)) return 0;                                        // below 2^-40 (and NaN from infinite logits)
  const float e = expf(hi);
  return (u64)(__builtin_fmaf(e, lo, e) * 1099511627776.0f);                          // 2^40; truncated
}

// f(logit, j) for j = start, start + stride, ... below V, with FU loads in flight per thread (one block streams the row: a loop
// that waits for every load runs at one memory latency per entry)
constexpr int FU = 8;
template <class F>
__device__ __forceinline__ void for_row(const float* x, int V, int start, int stride, F f) {
  for (int j = start; j < V; j += FU * stride) {
    float v[FU];
#pragma unroll
    for (int u = 0; u < FU; ++u) { const int jj = j + u * stride; v[u] = jj < V ? x[jj] : -INFINITY; }
#pragma unroll
    for (int u = 0; u < FU; ++u) { const int jj = j + u * stride; if (jj < V) f(v[u], jj); }
  }
}

struct SelRes { uint32_t sel, ecnt, n; u64 emass, nmass; };

// One radix select over the candidates of row x (see the head of the file).  target_c / target_m: k, or tau.
template <bool BY_MASS>
__device__ Cut radix_select(const float* x, int V, float inv_t, float M, uint32_t target_c, u64 target_m, uint32_t* cnt, u64* mass,
                            SelRes* res) {
  const int tid = threadIdx.x, lane = tid & 63;
  uint32_t prefix = 0, cnt_above = 0;
  u64 mass_above = 0;
  for (int level = 0; level < 4; ++level) {
    const int shift = 24 - 8 * level;
    if (tid < 256) { cnt[tid] = 0; mass[tid] = 0; }
    __syncthreads();
    int cb = -1;
    uint32_t cc = 0;
    u64 cm = 0;
    for_row(x, V, tid, FT, [&](float v, int) {
      const float z = zof(v, inv_t);
      if (!(z > -INFINITY)) return;
      const uint32_t key = zkey(z);
      if (level && ((key ^ prefix) >> (shift + 8))) return;
      const u64 q = zmass(z, M);
      if (BY_MASS && q == 0) return;            // (never at or above the cut of a mass select)
      const int b = (int)((key >> shift) & 255u);
      if (b != cb) {
        if (cc) { atomicAdd(&cnt[cb], cc); if (cm) atomicAdd(&mass[cb], cm); }
        cb = b; cc = 0; cm = 0;
      }
      ++cc; cm += q;
    });
    if (cc) { atomicAdd(&cnt[cb], cc); if (cm) atomicAdd(&mass[cb], cm); }
    __syncthreads();
    if (tid < 64) {       // wave 0: buckets in descending order, four per lane
      if (lane == 0) { res->sel = 0; res->ecnt = 0; res->emass = 0; res->n = 0; res->nmass = 0; }
      uint32_t c[4], cs = 0;
      u64 ms[4], mss = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int b = 255 - (4 * lane + i);
        c[i] = cnt[b]; ms[i] = mass[b];
        cs += c[i]; mss += ms[i];
      }
      uint32_t ic = cs;
      u64 im = mss;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t tc = __shfl_up(ic, o, 64);
        const u64 tm = __shfl_up(im, o, 64);
        if (lane >= o) { ic += tc; im += tm; }
      }
      uint32_t ec = ic - cs;
      u64 em = im - mss;
      const uint32_t tc = target_c - cnt_above;
      const u64 tm = target_m - mass_above;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool hit = BY_MASS ? (em < tm && tm <= em + ms[i]) : (ec < tc && tc <= ec + c[i]);
        if (hit) { res->sel = 255u - (uint32_t)(4 * lane + i); res->ecnt = ec; res->emass = em; res->n = c[i]; res->nmass = ms[i]; }
        ec += c[i]; em += ms[i];
      }
    }
    __syncthreads();
    prefix |= res->sel << shift;
    cnt_above += res->ecnt;
    mass_above += res->emass;
  }
  // the bucket of the last level is one key: n ties of the same q
  const uint32_t n = res->n;
  const u64 qT = zmass(key_z(prefix), M);
  Cut c;
  c.T = prefix;
  if (BY_MASS) {
    const u64 rem = target_m - mass_above;
    u64 m = qT ? (rem + qT - 1) / qT : (u64)n;
    if (m > n) m = n;
    if (m < 1) m = 1;
    c.m = (uint32_t)m;
  } else {
    uint32_t m = target_c - cnt_above;
    if (m > n) m = n;
    if (m < 1) m = 1;
    c.m = m;
  }
  c.kept = cnt_above + c.m;
  c.mass = mass_above + (u64)c.m * qT;
  __syncthreads();        // (res is rewritten by the next select)
  return c;
}

template <bool FUSED>
__global__ __launch_bounds__(FT) void filter_draw_kernel(FiltP p) {
  __shared__ uint32_t cnt[256];
  __shared__ u64 mass[256];
  __shared__ SelRes res;
  __shared__ float redf[FW], redz[FW];
  __shared__ int redi[FW];
  __shared__ uint32_t redc[FW];
  __shared__ u64 redm[FW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, row = blockIdx.x;
  float inv_t = p.inv_t, top_p = p.top_p;
  uint32_t seed_lo = p.seed_lo, seed_hi = p.seed_hi, step = p.step;
  int top_k = p.top_k, t = 0;
  if (FUSED) {
    if (p.state[1]) return;
    t = p.state[0];
    if (t >= p.cap || t < 0) {          // (the budget is spent: nothing is written but the flag, as in lap_decode_finish)
      if (row == 0 && tid == 0) p.state[1] = 1;
      return;
    }
    seed_lo = (uint32_t)p.samp[0]; seed_hi = (uint32_t)p.samp[1]; inv_t = __int_as_float(p.samp[2]);
    step = (uint32_t)t;
    top_k = p.filt[0]; top_p = __int_as_float(p.filt[1]);
  }
  const int V = p.V;
  const float* x = p.x + (long long)row * p.ld;
  const bool greedy = inv_t == 0.f;       // the argmax is always kept: no filter

  // pass 0: M = max z, the smallest z, the number of candidates
  float M = -INFINITY, zmin = INFINITY;
  uint32_t nc = 0;
  for_row(x, V, tid, FT, [&](float v, int) {
    const float z = zof(v, inv_t);
    if (z > -INFINITY) { M = fmaxf(M, z); zmin = fminf(zmin, z); ++nc; }
  });
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    M = fmaxf(M, __shfl_xor(M, o, 64)); zmin = fminf(zmin, __shfl_xor(zmin, o, 64)); nc += __shfl_xor(nc, o, 64);
  }
  if (lane == 0) { redf[w] = M; redz[w] = zmin; redc[w] = nc; }
  __syncthreads();
  M = redf[0]; zmin = redz[0]; nc = redc[0];
  for (int k = 1; k < FW; ++k) { M = fmaxf(M, redf[k]); zmin = fminf(zmin, redz[k]); nc += redc[k]; }
  __syncthreads();

  const bool k_on = !greedy && top_k >= 1 && (uint32_t)top_k < nc;
  const bool p_on = !greedy && nc > 0 && !(top_p >= 1.0f) && top_p == top_p;
  const bool want_lp = FUSED && p.logp != nullptr;

  // the mass of all candidates: the S of the log-probability, and the W of top_p when top_k keeps everything
  u64 Sall = 0;
  if (want_lp || (p_on && !k_on)) {
    u64 s = 0;
    for_row(x, V, tid, FT, [&](float v, int) {
      const float z = zof(v, inv_t);
      if (z > -INFINITY) s += zmass(z, M);
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) redm[w] = s;
    __syncthreads();
    for (int k = 0; k < FW; ++k) Sall += redm[k];
    __syncthreads();
  }

  // the cut: every candidate with key > T, and the first m by index of those with key == T
  uint32_t T = 0, m = 0xffffffffu, nkept = nc;
  bool ties = false;          // a select ran: m may be less than the number of entries equal to T
  u64 Wk = Sall;              // the mass of what top_k keeps
  if (k_on) {
    const Cut ck = radix_select<false>(x, V, inv_t, M, (uint32_t)top_k, 0, cnt, mass, &res);
    T = ck.T; m = ck.m; nkept = ck.kept; ties = true;
    Wk = ck.mass;
  }
  if (p_on) {
    u64 tau = top_p > 0.f ? __double2ull_ru((double)Wk * (double)top_p) : 1;
    if (tau > Wk) tau = Wk;
    if (tau < 1) tau = 1;
    const Cut cp = radix_select<true>(x, V, inv_t, M, 0, tau, cnt, mass, &res);
    if (!k_on || cp.kept < nkept) { T = cp.T; m = cp.m; nkept = cp.kept; ties = true; }
  }

  // last pass: wave w takes the contiguous range [j0, j1)
  const int L = (((V + FW - 1) / FW) + 63) & ~63;
  const int j0 = min(V, w * L), j1 = min(V, j0 + L);
  uint32_t run = 0;
  if (ties) {                 // the entries equal to T in the waves before this one (block-uniform branch)
    uint32_t c = 0;
    for_row(x, j1, j0 + lane, 64, [&](float v, int) {
      const float z = zof(v, inv_t);
      c += (z > -INFINITY && zkey(z) == T) ? 1u : 0u;
    });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) redc[w] = c;
    __syncthreads();
    for (int k = 0; k < w; ++k) run += redc[k];
  }
  float best = -INFINITY, bz = -INFINITY;
  int bi = 0x7fffffff;
  for (int base0 = j0; base0 < j1; base0 += 64 * FU) {
    float vv[FU];
#pragma unroll
    for (int u = 0; u < FU; ++u) { const int jj = base0 + 64 * u + lane; vv[u] = jj < j1 ? x[jj] : -INFINITY; }
#pragma unroll
    for (int u = 0; u < FU; ++u) {
    const int base = base0 + 64 * u;
    if (base >= j1) continue;           // (wave-uniform)
    const int j = base + lane;
    const bool in = j < j1;
    const float v = vv[u];
    const float z = zof(v, inv_t);
    const bool cand = in && z > -INFINITY;
    const uint32_t key = zkey(z);
    bool keep = cand && (greedy || nkept == nc || key > T);
    const bool tie = cand && !keep && key == T;
    if (ties) {
      const u64 bal = __ballot(tie);
      const uint32_t r = run + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
      keep = keep || (tie && r < m);
      run += (uint32_t)__popcll(bal);
    }
    if (keep) {
      float s = z, s1;
      if (!greedy) lap_sampling::gumbel_scores_at(v, v, inv_t, seed_lo, seed_hi, step, (uint32_t)row, (uint32_t)j, (uint32_t)j, s, s1);
      if (better(s, j, best, bi)) { best = s; bi = j; bz = z; }
    }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64), oz = __shfl_xor(bz, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (better(ov, oi, best, bi)) { best = ov; bi = oi; bz = oz; }
  }
  __syncthreads();
  if (lane == 0) { redf[w] = best; redi[w] = bi; redz[w] = bz; }
  __syncthreads();
  if (tid != 0) return;
  for (int k = 1; k < FW; ++k)
    if (better(redf[k], redi[k], best, bi)) { best = redf[k]; bi = redi[k]; bz = redz[k]; }
  const int tok = nc ? bi : 0;            // (a row without a candidate: index 0, as the argmax of a row of -inf)
  if (p.kept) p.kept[row] = (int)nkept;
  if (p.cut) p.cut[row] = nc == 0 ? -INFINITY : ties ? key_z(T) : zmin;
  if (!FUSED) { p.out[row] = tok; return; }
  p.out[(long long)row * p.cap + t] = tok;
  if (want_lp) p.logp[(long long)row * p.cap + t] = nc ? bz - (M + logf((float)Sall * 9.094947017729282e-13f)) : -INFINITY;    // 2^-40
  const int e = p.state[8 + row] | (tok == p.eos ? 1 : 0);
  p.state[8 + row] = e;
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

}  // namespace

extern "C" int lap_filter_gumbel_argmax_rows_f32(const float* logits, int rows, int n, int ld, float inv_t, unsigned int seed_lo,
                                                 unsigned int seed_hi, int step, int top_k, float top_p, int* out, int* kept,
                                                 float* cut, void* stream) {
  if (!logits || !out || rows < 1 || n < 1 || n > FILT_MAXV || ld < n || step < 0 || !(inv_t >= 0.f) || !(inv_t < INFINITY))
    return LAP_ERR_ARG;
  FiltP p{};
  p.x = logits; p.ld = ld; p.V = n; p.inv_t = inv_t; p.seed_lo = seed_lo; p.seed_hi = seed_hi; p.step = (uint32_t)step;
  p.top_k = top_k; p.top_p = top_p; p.out = out; p.kept = kept; p.cut = cut;
  hipLaunchKernelGGL(filter_draw_kernel<false>, dim3(rows), dim3(FT), 0, S_, p);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

extern "C" int lap_decode_filter_words(void) { return 4; }

extern "C" int lap_decode_filter_finish(int* state, const int* sampling, const int* filter, const float* logits, int* out, float* logp,
                                        int B, int V, int cap, int eos_token, int* kept, float* cut, void* stream) {
  if (!state || !sampling || !filter || !logits || !out || B < 1 || B > FILT_MAXB || V < 2 || V > FILT_MAXV || cap < 1) return LAP_ERR_ARG;
  FiltP p{};
  p.x = logits; p.ld = V; p.V = V; p.state = state; p.samp = sampling; p.filt = filter; p.out = out; p.cap = cap; p.eos = eos_token;
  p.B = B; p.logp = logp; p.kept = kept; p.cut = cut;
  hipLaunchKernelGGL(filter_draw_kernel<true>, dim3(B), dim3(FT), 0, S_, p);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}
