// Fused single-token decode of the VLM stream (expert 0) for LAP.sample_tokens (lap.py:678-766, the LAP_AR serving mode) at
// the Gemma-2B widths: D 2048, 8 query heads / 1 kv head of 256, MLP 16384, B <= 8 rows.
//
// Every kernel of a decode step reads where it is from a small device state instead of host arguments, so one captured step
// replays unchanged for every token (the reference's lax.while_loop body):
//   state[0] = t       tokens written to out[:, .] so far; a decode step feeds token out[:, t-1] at position plen[b] + t-1,
//                      appends its K / V at generated-cache row t-1 and attends to t generated keys
//   state[1] = done    t >= max_steps or every sample has emitted EOS: every kernel returns at once, nothing more is written
//   state[8 + b]       EOS seen by sample b
//   state[16 + b]      plen[b] (the prefill length of sample b)
//
// Kernels (one launch each; weights [N][K] bf16, streamed once straight into VGPRs with nontemporal loads, f32 accumulation):
//   embed       x[b] = bf16(table[out[b][t-1]] * sqrt(D))                                   (lap_embed_gather)
//   qkv         h = RMSNorm(x)(1 + n_attn) -> bf16(h Wqkv^T) -> RoPE, q scale, head split;  (lap_rmsnorm_fwd, linear_fwd,
//               K / V go to row t-1 of the generated cache, q to a small buffer              lap_rope_split_fwd)
//   attention   8 query heads against [prefix keys gated by kinfo | t generated keys], keys split over waves of 16, then a
//               combine pass                                                                 (lap_attention_serve)
//   proj_res    y = bf16(a W^T + x)  (out projection, down projection)                     (linear_fwd + residual)
//   gate_up     h = RMSNorm(x)(1 + n_ffw) -> act = bf16(bf16(gelu_tanh(bf16 g)) * bf16 u)  (linear_fwd, lap_geglu_fwd_ld)
//   lm_head     h = RMSNorm(x)(1 + final_norm) -> logit = f32(hi h) + f32(lo h) per vocabulary row, never stored (except
//               the debug `logits` output); per block (max, lowest index) partials          (_lm_logits)
//   lm_head_sample   lm_head whose partials are over score = logit * inv_t + Gumbel noise of (seed, t, b, vocabulary row)
//               (sampling.hpp) when the sampling words {seed low, seed high, bits of inv_t, 0} hold inv_t != 0, and lm_head's
//               partials bit for bit when inv_t == 0                                        (lap_gumbel_argmax_rows_f32)
//   lm_head_subset*  the same heads over an allowed set of vocabulary rows (constrained decoding)
//               All LM heads are ONE kernel template, dec_lm_head_kernel<B, SAMPLE, SUBSET, P>, over ONE statement of the row
//               dot product (lm_row_pair) and of the block partials (lm_block_partials): full or subset, greedy or sampling, a
//               head differs only in which two rows a unit is, which wave takes it and which noise call it makes.  So the
//               logit of vocabulary row j is the same bits in every head by construction, and tests/test_decode_bits_gpu.py
//               pins those bits (and the projections') to a recorded fixture: a change to the arithmetic shows there.
//   lm_head_lp / finish_lp   any of the LM heads above with the LOGP parameter: the log-sum-exp of z = logit * tau rides along in
//               the same pass (per block {m, s, z of the best candidate}), and the finish also writes logp[:, t] = z_tok - lse
//   finish      one block: argmax over the partials with the lowest index among ties, out[:, t] = token, EOS mask, t += 1,
//               done                                                                         (lap_argmax_rows_f32)
//   spec_qkv / spec_attention   the qkv and attention kernels on S rows that are consecutive positions of ONE sequence (exact
//               speculative decoding: EPI_QKV_SPEC and dec_attn_kernel<true> below; csrc/decode_spec.hip holds the draft, embed
//               and accept kernels of a verify step).  The plain instances' code paths are unchanged.
// Rounding points are those of the eager step; only the summation order of the dot products differs.
// Device state is written with plain per-lane stores.
//
// fp8 weight-only decoding (the *_fp8 entry points; format: lap_amd/fp8.py): the weight stream is OCP e4m3 codes [N][K], one
// byte per weight, with one power-of-two scale 2^e per output row n, e the largest integer with amax_n 2^e <= 448.  The same
// kernels stream the codes (8 per lane per load: lane l owns the k it owns in the bf16 stream), widen them with
// v_cvt_pk_f32_fp8, accumulate the CODES in f32 and multiply the finished row sum by 2^-e once, ahead of the epilogue's first
// rounding point.  A power-of-two scale commutes with f32 accumulation and every code 2^-e is a bf16 number, so with the same
// k-to-lane map and the same order of additions this computes, bit for bit, what the bf16 kernel computes on the dequantised
// weights (LAP_DEC_F8_LANE = 16 is the 1 KiB-per-wave-instruction variant, equal up to the summation order only).  lap_quantize_fp8_rows makes codes and scales from bf16 or f32 rows into caller-owned buffers.
#include "common.hpp"
#include "sampling.hpp"
#include "../../include/lap_hip.h"
#include <type_traits>

#define S_ ((hipStream_t)stream)

namespace {

constexpr int DEC_D = 2048, DEC_NH = 8, DEC_NKV = 1, DEC_HD = 256, DEC_H = 16384, DEC_MAXB = 8;
constexpr int KC = 16;                     // keys per attention wave
constexpr int LM_BLOCKS = 1024;            // LM-head grid (partials per sample)
constexpr float NEG_BIG = -1.0e30f;
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
constexpr int QWORD = (1 << 24) | 0xFFFFFF;    // the decode query's info word (class 1, index past every key)

__device__ __forceinline__ bool mask_ok(int qi, int ki) {
  return (((qi >> 24) & (ki >> 24)) != 0) && ((ki & 0xffffff) <= (qi & 0xffffff));
}

__device__ __forceinline__ void ld8f(const bf16* p, float (&v)[8]) {
  const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
}
__device__ __forceinline__ bf16x8 ldw(const bf16* p) {      // the weight stream: read once by one wave
  return __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(p));
}
__device__ __forceinline__ float dot8(const bf16x8 w, const float (&x)[8], float acc) {
#pragma unroll
  for (int e = 0; e < 8; ++e) acc = __builtin_fmaf((float)w[e], x[e], acc);
  return acc;
}
// ---- the e4m3 weight stream
#ifndef LAP_DEC_F8_LANE
#define LAP_DEC_F8_LANE 8                  // codes per lane per load: 8 (the bf16 stream's k-to-lane map: bit-equal results) or 16 (1 KiB per wave instruction)
#endif
constexpr int F8L = LAP_DEC_F8_LANE;
static_assert(F8L == 8 || F8L == 16, "LAP_DEC_F8_LANE: 8 or 16");
typedef __attribute__((ext_vector_type(F8L / 4))) unsigned f8w;
__device__ __forceinline__ f8w ldw8(const uint8_t* p) {     // read once by one wave, like ldw
  return __builtin_nontemporal_load(reinterpret_cast<const f8w*>(p));
}
__device__ __forceinline__ void widen8(const f8w w, float (&c)[F8L]) {
#pragma unroll
  for (int i = 0; i < F8L / 4; ++i) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    c[4 * i] = lo[0]; c[4 * i + 1] = lo[1]; c[4 * i + 2] = hi[0]; c[4 * i + 3] = hi[1];
  }
}
__device__ __forceinline__ void ldxf(const bf16* p, float (&v)[F8L]) {
#pragma unroll
  for (int c = 0; c < F8L / 8; ++c) {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(p + 8 * c);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[8 * c + e] = (float)t[e];
  }
}
__device__ __forceinline__ float dotf8(const float (&c)[F8L], const float (&x)[F8L], float acc) {
#pragma unroll
  for (int e = 0; e < F8L; ++e) acc = __builtin_fmaf(c[e], x[e], acc);
  return acc;
}
__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// RMSNorm prologue (lap_rmsnorm_fwd's plain form: h = bf16(x r (1 + gamma)), r = 1 / sqrt(mean(x^2) + eps)) of B rows of
// width D into LDS.  256 threads, D % 8 == 0, D <= 2048.
template <int B>
__device__ __forceinline__ void norm_rows_to_lds(const bf16* x, const float* gamma, int D, float eps, bf16* sx, float* red) {
  for (int b = 0; b < B; ++b) {
    float ss = 0.f;
    for (int c = threadIdx.x * 8; c < D; c += 2048) {
      float v[8];
      ld8f(x + (long long)b * D + c, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) ss += v[e] * v[e];
    }
    ss = block_sum<4>(ss, red);
    const float r = 1.0f / sqrtf(ss / (float)D + eps);
    for (int c = threadIdx.x * 8; c < D; c += 2048) {
      float v[8];
      ld8f(x + (long long)b * D + c, v);
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2bf(v[e] * r * (1.0f + gamma[c + e]));
      *reinterpret_cast<bf16x8*>(sx + b * D + c) = o;
    }
  }
  __syncthreads();
}

enum { EPI_QKV = 0, EPI_GEGLU = 1, EPI_RES = 2, EPI_QKV_SPEC = 3 };
// EPI_QKV_SPEC (speculative decoding, lap_decode_spec_qkv): the B rows are the consecutive positions t-1 .. t-1+B-1 of ONE
// sequence (sample 0), not B samples.  Row r rotates at plen[0] + t-1+r and writes K / V to generated-cache row t-1+r of sample 0
// and q to row r; a row with t-1+r >= cap writes nothing.  The accumulation is EPI_QKV's, so row r holds the bits the plain
// kernel writes at state[0] = t + r for the same input row.  K / V rows written for drafts that the accept kernel then rejects
// lie at or beyond the next step's row t'-1; that step overwrites them before a query may see them, because the key count of a
// query (min(t' + r, cap)) reaches only rows this same step has written.

struct ProjP {
  const int* state;
  const bf16* x;          // block input [B][K] (normalised in the prologue when gamma != NULL)
  const float* gamma;
  const bf16* w;          // [N][K]
  int K, units;
  float eps;
  bf16* out;              // GEGLU: act [B][H]; RES: y [B][N]
  const bf16* res;        // RES: residual [B][N]
  int N, H;               // RES: N; GEGLU: H
  bf16* q; bf16* ck; bf16* cv;   // QKV: q [B][NH*HD], generated caches [B][cap][HD]
  int cap, NH, HD;
  float q_scale;
};

struct ProjP8 : ProjP {     // w: e4m3 codes [N][K]
  const float* wscale;      // [N] 2^e per output row
};

// One "unit" = the two output features an epilogue needs together: QKV the rotation pair (d, d + HD/2) of one head; GeGLU a
// gate column and its up column; RES two neighbouring columns.  KW waves of a block split K for one unit (KW = 4) or each
// wave owns a unit (KW = 1); blocks walk the units with a grid stride.
template <int EPI>
__device__ __forceinline__ void unit_features(const ProjP& p, int u, int& f0, int& f1) {
  if (EPI == EPI_QKV || EPI == EPI_QKV_SPEC) { const int half = p.HD / 2; f0 = (u / half) * p.HD + u % half; f1 = f0 + half; }
  else if (EPI == EPI_GEGLU) { f0 = u; f1 = u + p.H; }
  else { f0 = 2 * u; f1 = 2 * u + 1; }
}

// P = ProjP8: the fp8 weight stream (the ProjP instances are the bf16 kernels unchanged).
template <int EPI, int B, bool NORM, int KW, class P = ProjP>
__global__ __launch_bounds__(256) void dec_proj_kernel(P p) {
  constexpr bool F8 = std::is_same<P, ProjP8>::value;
  __shared__ __attribute__((aligned(16))) bf16 sx[NORM ? B * DEC_D : 8];
  __shared__ float red[4];
  __shared__ float sacc[KW > 1 ? 4 * 2 * B : 1];
  if (p.state[1]) return;
  const int t = p.state[0];
  if ((EPI == EPI_QKV || EPI == EPI_QKV_SPEC) && (t < 1 || t > p.cap)) return;      // (cache row t - 1)
  if (NORM) norm_rows_to_lds<B>(p.x, p.gamma, p.K, p.eps, sx, red);
  const bf16* xs = NORM ? sx : p.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  constexpr int NU = 4 / KW;                      // units per block iteration
  const int wu = w / KW, wk = w % KW;
  const int Ks = p.K / KW;
  for (int u0 = blockIdx.x * NU; u0 < p.units; u0 += gridDim.x * NU) {
    const int u = u0 + wu;
    const bool valid = u < p.units;
    int f0 = 0, f1 = 0;
    unit_features<EPI>(p, valid ? u : 0, f0, f1);
    float a0[B], a1[B];
#pragma unroll
    for (int b = 0; b < B; ++b) { a0[b] = 0.f; a1[b] = 0.f; }
    if constexpr (F8) {
      if (valid) {
        const uint8_t* w0 = reinterpret_cast<const uint8_t*>(p.w) + (long long)f0 * p.K;
        const uint8_t* w1 = reinterpret_cast<const uint8_t*>(p.w) + (long long)f1 * p.K;
#pragma unroll 4
        for (int k = wk * Ks + lane * F8L; k < (wk + 1) * Ks; k += 64 * F8L) {
          const f8w v0 = ldw8(w0 + k), v1 = ldw8(w1 + k);
          float c0[F8L], c1[F8L];
          widen8(v0, c0);
          widen8(v1, c1);
#pragma unroll
          for (int b = 0; b < B; ++b) {
            float xv[F8L];
            ldxf(xs + (long long)b * p.K + k, xv);
            a0[b] = dotf8(c0, xv, a0[b]);
            a1[b] = dotf8(c1, xv, a1[b]);
          }
        }
      }
    } else if (valid) {
      const bf16* w0 = p.w + (long long)f0 * p.K;
      const bf16* w1 = p.w + (long long)f1 * p.K;
#pragma unroll 4
      for (int k = wk * Ks + lane * 8; k < (wk + 1) * Ks; k += 512) {
        const bf16x8 v0 = ldw(w0 + k), v1 = ldw(w1 + k);
#pragma unroll
        for (int b = 0; b < B; ++b) {
          float xv[8];
          ld8f(xs + (long long)b * p.K + k, xv);
          a0[b] = dot8(v0, xv, a0[b]);
          a1[b] = dot8(v1, xv, a1[b]);
        }
      }
    }
#pragma unroll
    for (int b = 0; b < B; ++b) { a0[b] = wave_sum(a0[b]); a1[b] = wave_sum(a1[b]); }
    if (KW > 1) {        // the K slices of the block's waves, summed in wave order
      if (lane == 0) {
#pragma unroll
        for (int b = 0; b < B; ++b) { sacc[(w * 2 + 0) * B + b] = a0[b]; sacc[(w * 2 + 1) * B + b] = a1[b]; }
      }
      __syncthreads();
#pragma unroll
      for (int b = 0; b < B; ++b) {
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int i = 0; i < KW; ++i) { s0 += sacc[(i * 2 + 0) * B + b]; s1 += sacc[(i * 2 + 1) * B + b]; }
        a0[b] = s0; a1[b] = s1;
      }
      __syncthreads();
    }
    if (!valid || wk != 0 || lane >= B) continue;
    // epilogue: lane b writes sample b
    float y0 = 0.f, y1 = 0.f;
#pragma unroll
    for (int b = 0; b < B; ++b) if (b == lane) { y0 = a0[b]; y1 = a1[b]; }
    const int b = lane;
    if constexpr (F8) { y0 *= 1.0f / p.wscale[f0]; y1 *= 1.0f / p.wscale[f1]; }     // 2^-e: exact
    if (EPI == EPI_RES) {
      const bf16* r = p.res + (long long)b * p.N + f0;
      bf16x2 o;
      o[0] = f2bf(y0 + (float)r[0]);
      o[1] = f2bf(y1 + (float)r[1]);
      *reinterpret_cast<bf16x2*>(p.out + (long long)b * p.N + f0) = o;
    } else if (EPI == EPI_GEGLU) {
      const float g = round_bf16(y0), up = round_bf16(y1);
      p.out[(long long)b * p.H + f0] = f2bf(round_bf16(gelu_tanh_f(g)) * up);
    } else if (EPI == EPI_QKV_SPEC) {      // row b is position t-1+b of sample 0 (EPI_QKV's arithmetic)
      const int half = p.HD / 2, head = u / half, i = u % half;
      const int s = t - 1 + b;
      if (s >= p.cap) continue;
      float x1 = round_bf16(y0), x2 = round_bf16(y1);
      if (head <= p.NH) {
        float sn, cs, r1, r2;
        rope_sincos((float)(p.state[16] + s), i, p.HD, sn, cs);
        rope_rotate(x1, x2, sn, cs, r1, r2);
        x1 = round_bf16(r1); x2 = round_bf16(r2);
        if (head < p.NH) { x1 *= p.q_scale; x2 *= p.q_scale; }
      }
      bf16* dst;
      if (head < p.NH) dst = p.q + (long long)b * p.NH * p.HD + head * p.HD;
      else dst = (head == p.NH ? p.ck : p.cv) + (long long)s * p.HD;
      dst[i] = f2bf(x1);
      dst[i + half] = f2bf(x2);
    } else {
      const int half = p.HD / 2, head = u / half, i = u % half;
      const int s = t - 1;
      float x1 = round_bf16(y0), x2 = round_bf16(y1);
      if (head <= p.NH) {          // q heads and the k head are rotated
        float sn, cs, r1, r2;
        rope_sincos((float)(p.state[16 + b] + s), i, p.HD, sn, cs);
        rope_rotate(x1, x2, sn, cs, r1, r2);
        x1 = round_bf16(r1); x2 = round_bf16(r2);
        if (head < p.NH) { x1 *= p.q_scale; x2 *= p.q_scale; }
      }
      bf16* dst;
      if (head < p.NH) dst = p.q + (long long)b * p.NH * p.HD + head * p.HD;
      else dst = (head == p.NH ? p.ck : p.cv) + ((long long)b * p.cap + s) * p.HD;
      dst[i] = f2bf(x1);
      dst[i + half] = f2bf(x2);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------- embed
__global__ __launch_bounds__(256) void dec_embed_kernel(const int* state, const float* table, int row_lo, int row_hi,
                                                        const int* out, int cap, bf16* x, int D, float scale) {
  if (state[1]) return;
  const int b = blockIdx.x, t = state[0];
  if (t < 1 || t > cap) return;
  const int tok = out[(long long)b * cap + t - 1];
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
    *reinterpret_cast<bf16x8*>(x + (long long)b * D + c) = o;
  }
}

// --------------------------------------------------------------------------------------------------------- attention
// grid (ceil(chunks / 4), B), 4 waves; wave c owns keys [16 c, 16 c + 16) of [prefix (Pn) | generated (cap)].  Lane l holds
// dims 4 l .. 4 l + 3 of the 8 query heads.  Per chunk: scores s (f32), m = max over the chunk's allowed keys, e = exp2(s
// log2e - m log2e), p = bf16(e) (lap_attention_serve's rounding point), l = sum e, o = sum p v; written as o / l and
// lse = (m + log2 l) ln 2, or lse = NEG_BIG for a chunk with no allowed key.
struct AttnDecP {
  const int* state;
  const bf16* q;                       // [B][NH * HD]
  const bf16* pk; const bf16* pv;      // prefix caches [B * Pn][HD]
  const int* kinfo;                    // [B][Pn]
  const bf16* gk; const bf16* gv;      // generated caches [B][cap][HD]
  int Pn, cap, nchunk, npre;
  float* lpart;                        // [B][nchunk][NH]
  float* opart;                        // [B][nchunk][NH][HD]
  bf16* o;                             // [B][NH * HD]
};

// SPEC (speculative decoding, lap_decode_spec_attention): grid y = r, the query is q row r of ONE sequence; the prefix K / V,
// kinfo and the generated cache are sample 0's, and the generated segment has min(t + r, cap) keys.  The chunk partition is
// unchanged, so row r's partials are the plain kernel's at state[0] = t + r with B = 1.
template <bool SPEC>
__global__ __launch_bounds__(256) void dec_attn_kernel(AttnDecP p) {
  constexpr int NH = DEC_NH, HD = DEC_HD;
  if (p.state[1]) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, b = blockIdx.y;
  const int sb = SPEC ? 0 : b;                 // the sample whose keys row b reads
  const int c = blockIdx.x * 4 + w;
  if (c >= p.nchunk) return;
  const int t = min(SPEC ? p.state[0] + b : p.state[0], p.cap);
  const bf16* kb; const bf16* vb;
  int nkeys, j0;
  if (c < p.npre) {
    j0 = c * KC;
    nkeys = min(KC, p.Pn - j0);
    kb = p.pk + ((long long)sb * p.Pn + j0) * HD;
    vb = p.pv + ((long long)sb * p.Pn + j0) * HD;
  } else {
    j0 = (c - p.npre) * KC;
    nkeys = max(0, min(KC, t - j0));          // t generated keys (this step's included)
    kb = p.gk + ((long long)sb * p.cap + j0) * HD;
    vb = p.gv + ((long long)sb * p.cap + j0) * HD;
  }
  float qf[NH][4];
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    const bf16x4 v = *reinterpret_cast<const bf16x4*>(p.q + (long long)b * NH * HD + h * HD + lane * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) qf[h][e] = (float)v[e];
  }
  // every K / V row and mask word of the chunk is loaded up front (one round trip), then the scores: lane j < KC keeps those of key j
  bf16x4 kr[KC], vr[KC];
#pragma unroll
  for (int j = 0; j < KC; ++j) {
    kr[j] = bf16x4{};
    vr[j] = bf16x4{};
    if (j < nkeys) {
      kr[j] = *reinterpret_cast<const bf16x4*>(kb + (long long)j * HD + lane * 4);
      vr[j] = *reinterpret_cast<const bf16x4*>(vb + (long long)j * HD + lane * 4);
    }
  }
  const bool okl = lane < nkeys && (c < p.npre ? mask_ok(QWORD, p.kinfo[(long long)sb * p.Pn + j0 + lane]) : true);
  const unsigned long long okmask = __ballot(okl);
  float sj[NH];
  const bool okj = okl;
#pragma unroll
  for (int h = 0; h < NH; ++h) sj[h] = NEG_BIG;
#pragma unroll
  for (int j = 0; j < KC; ++j) {
    if (!((okmask >> j) & 1ull)) continue;    // (uniform over the wave)
    float kf[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) kf[e] = (float)kr[j][e];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) s = __builtin_fmaf(qf[h][e], kf[e], s);
      s = wave_sum(s);
      if (lane == j) sj[h] = s;
    }
  }
  float m[NH], l[NH], pj[NH];
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    m[h] = wave_max(okj ? sj[h] : NEG_BIG) * LOG2E;
    const float e = okj ? __builtin_amdgcn_exp2f(sj[h] * LOG2E - m[h]) : 0.f;
    l[h] = wave_sum(e);
    pj[h] = round_bf16(e);
  }
  float acc[NH][4];
#pragma unroll
  for (int h = 0; h < NH; ++h)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[h][e] = 0.f;
#pragma unroll
  for (int j = 0; j < KC; ++j) {
    if (!((okmask >> j) & 1ull)) continue;    // (p = 0 for a masked key)
    float vf[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) vf[e] = (float)vr[j][e];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
      const float pp = __shfl(pj[h], j, 64);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[h][e] = __builtin_fmaf(pp, vf[e], acc[h][e]);
    }
  }
  const long long pr = (long long)b * p.nchunk + c;
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    const float inv = l[h] > 0.f ? 1.0f / l[h] : 0.f;
    f32x4 o4;
#pragma unroll
    for (int e = 0; e < 4; ++e) o4[e] = acc[h][e] * inv;
    *reinterpret_cast<f32x4*>(p.opart + (pr * NH + h) * HD + lane * 4) = o4;
    if (lane == 0) p.lpart[pr * NH + h] = l[h] > 0.f ? (m[h] + __builtin_amdgcn_logf(l[h])) * LN2 : NEG_BIG;
  }
}

// grid (NH, B), 64 threads: thread = 4 dims of one head.  O = sum_c exp(lse_c - max) o_c / sum_c exp(lse_c - max) (the
// combine of lap_attention_serve; chunks without an allowed key have weight 0).
__global__ __launch_bounds__(64) void dec_attn_combine_kernel(AttnDecP p) {
  constexpr int NH = DEC_NH, HD = DEC_HD;
  if (p.state[1]) return;
  const int h = blockIdx.x, b = blockIdx.y, d0 = threadIdx.x * 4;
  const float* lp = p.lpart + (long long)b * p.nchunk * NH + h;
  const float* op = p.opart + ((long long)b * p.nchunk * NH + h) * HD + d0;
  float mx = NEG_BIG;
#pragma unroll 8
  for (int c = 0; c < p.nchunk; ++c) mx = fmaxf(mx, lp[(long long)c * NH]);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float den = 0.f;
#pragma unroll 8
  for (int c = 0; c < p.nchunk; ++c) {
    const float li = lp[(long long)c * NH];
    const float wgt = li > NEG_BIG * 0.5f ? __expf(li - mx) : 0.f;
    den += wgt;
    acc += *reinterpret_cast<const f32x4*>(op + (long long)c * NH * HD) * wgt;
  }
  const float sc = den > 0.f ? 1.0f / den : 0.f;
  bf16x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = f2bf(acc[e] * sc);
  *reinterpret_cast<bf16x4*>(p.o + (long long)b * NH * HD + h * HD + d0) = o;
}

// ------------------------------------------------------------------------------------------------------------ LM head
struct LmP {
  const int* state;
  const bf16* x; const float* gamma; float eps;
  const bf16* hi; const bf16* lo;      // [V][D] planes (lo may be NULL)
  int V, D;
  float* logits;                       // debug: f32 [B][V] or NULL
  float* pval; int* pidx;              // partials [gridDim.x][B]
  const int* samp;                     // SAMPLE: {seed low, seed high, bits of inv_t (0 = greedy), reserved}
  const int* ids; int n;               // SUBSET: the allowed vocabulary rows, sorted ascending, unique, inside [0, V)
};

// P = LmP8: `hi` is ONE plane of e4m3 codes with a scale per vocabulary row instead of the hi / lo bf16 planes; partials,
// sampling epilogue and the debug logits are those of the LmP instances.
struct LmP8 : LmP {
  const float* wscale;                 // [V] 2^e per vocabulary row
};

// P = LmLogP<LmP> / LmLogP<LmP8>: the LOGP instances' arguments (the instances without LOGP keep theirs as they are)
template <class Base>
struct LmLogP : Base {
  float* plp;                          // partials [gridDim.x][B][3] = {m, s, z of the block's best candidate}
};

// P = LmScoreP<LmP> / LmScoreP<LmP8>: the TARGET instances' arguments (teacher-forced scoring, csrc/decode_score.hip).  A TARGET
// instance is the LOGP instance of the same rows whose third plp word is the z of a GIVEN id, row b's target cand[1 + t + b] of the
// candidate buffer {length, ids[cap]}, instead of the z of the row's best candidate.
template <class Base>
struct LmScoreP : LmLogP<Base> {
  const int* cand; int cap;            // the candidate {length, ids[cap]}; length is clamped to [0, cap]
};
template <class P> struct lm_is_target : std::false_type {};
template <class Base> struct lm_is_target<LmScoreP<Base>> : std::true_type {};

// The row dot product of the LM head.  Every head (full or subset, greedy or sampling, bf16 or fp8) runs this one statement of
// it, so the logit of vocabulary row j is the same bits in all of them by construction; tests/test_decode_bits_gpu.py pins
// those bits to a recorded fixture.  The logits of rows f0 and f1 (f1 == f0: one row) for all B rows of `sx` are wave-uniform
// after the wave_sums: the debug store, and either lane b's pair (SAMPLE: y0 / y1 of lane b = row b) or the running best of
// every row (greedy).
// SAMPLE: the sampler is the epilogue of a unit.  Lane b keeps row b's pair, runs row b's Philox block and its four logarithms
// (B <= 8 lanes carry data, the instruction count is that of one row) and folds the two scores into ITS running best, so the
// B-fold compare chain of the greedy form becomes one.
template <int B, bool SAMPLE, class P>
__device__ __forceinline__ void lm_row_pair(const P& p, const bf16* sx, int lane, int f0, int f1, float (&bv)[B], int (&bi)[B],
                                            float& y0, float& y1) {
  constexpr bool F8 = std::is_base_of<LmP8, P>::value;
  float h0[B], h1[B], l0[B], l1[B];
#pragma unroll
  for (int b = 0; b < B; ++b) { h0[b] = 0.f; h1[b] = 0.f; l0[b] = 0.f; l1[b] = 0.f; }
  if constexpr (F8) {
    const uint8_t* c0p = reinterpret_cast<const uint8_t*>(p.hi) + (long long)f0 * p.D;
    const uint8_t* c1p = reinterpret_cast<const uint8_t*>(p.hi) + (long long)f1 * p.D;
#pragma unroll 2
    for (int k = lane * F8L; k < p.D; k += 64 * F8L) {
      const f8w w0 = ldw8(c0p + k), w1 = ldw8(c1p + k);
      float c0[F8L], c1[F8L];
      widen8(w0, c0);
      widen8(w1, c1);
#pragma unroll
      for (int b = 0; b < B; ++b) {
        float xv[F8L];
        ldxf(sx + b * p.D + k, xv);
        h0[b] = dotf8(c0, xv, h0[b]);
        h1[b] = dotf8(c1, xv, h1[b]);
      }
    }
  } else {
#pragma unroll (B > 4 ? 2 : 4)            // (4 at B = 7 spills)
    for (int k = lane * 8; k < p.D; k += 512) {
      const bf16x8 w0 = ldw(p.hi + (long long)f0 * p.D + k), w1 = ldw(p.hi + (long long)f1 * p.D + k);
      bf16x8 z0 = w0, z1 = w1;
      if (p.lo) { z0 = ldw(p.lo + (long long)f0 * p.D + k); z1 = ldw(p.lo + (long long)f1 * p.D + k); }
#pragma unroll
      for (int b = 0; b < B; ++b) {
        float xv[8];
        ld8f(sx + b * p.D + k, xv);
        h0[b] = dot8(w0, xv, h0[b]);
        h1[b] = dot8(w1, xv, h1[b]);
        if (p.lo) { l0[b] = dot8(z0, xv, l0[b]); l1[b] = dot8(z1, xv, l1[b]); }
      }
    }
  }
  float r0 = 1.f, r1 = 1.f;
  if constexpr (F8) { r0 = 1.0f / p.wscale[f0]; r1 = 1.0f / p.wscale[f1]; }     // 2^-e: exact
#pragma unroll
  for (int b = 0; b < B; ++b) {
    float v0 = wave_sum(h0[b]), v1 = wave_sum(h1[b]);
    if constexpr (F8) { v0 *= r0; v1 *= r1; }
    else if (p.lo) { v0 += wave_sum(l0[b]); v1 += wave_sum(l1[b]); }   // the eager path: C = hi.h, then C += lo.h
    if (p.logits && lane == 0) {
      p.logits[(long long)b * p.V + f0] = v0;
      if (f1 != f0) p.logits[(long long)b * p.V + f1] = v1;
    }
    if (SAMPLE) {
      if (b == lane) { y0 = v0; y1 = v1; }
    } else {
      if (better(v0, f0, bv[b], bi[b])) { bv[b] = v0; bi[b] = f0; }
      if (f1 != f0 && better(v1, f1, bv[b], bi[b])) { bv[b] = v1; bi[b] = f1; }
    }
  }
}

// The block's partial of every row from its four waves' bests (greedy: bv / bi of lane 0; SAMPLE: lbv / lbi of lane b).
template <int B, bool SAMPLE, class P>
__device__ __forceinline__ void lm_block_partials(const P& p, int lane, int w, const float (&bv)[B], const int (&bi)[B], float lbv,
                                                  int lbi, float (*sv)[B], int (*si)[B]) {
  if (SAMPLE) {
    if (lane < B) { sv[w][lane] = lbv; si[w][lane] = lbi; }
  } else if (lane == 0) {
#pragma unroll
    for (int b = 0; b < B; ++b) { sv[w][b] = bv[b]; si[w][b] = bi[b]; }
  }
  __syncthreads();
  if (threadIdx.x < B) {
    const int b = threadIdx.x;
    float v = sv[0][b];
    int i = si[0][b];
    for (int k = 1; k < 4; ++k)
      if (better(sv[k][b], si[k][b], v, i)) { v = sv[k][b]; i = si[k][b]; }
    p.pval[(long long)blockIdx.x * B + b] = v;
    p.pidx[(long long)blockIdx.x * B + b] = i;
  }
}

// LOGP: the log-sum-exp of z = float32(logit * tau) (tau = inv_t under sampling, else 1) rides along as a running pair (m, s),
// m = max z so far, s = sum exp(z - m); the pair of nothing is (-inf, 0).  Every expf argument is <= 0, and m == -inf is tested
// before a difference is formed, so neither a large logit nor two empty pairs make an inf - inf.  Accurate expf, like the
// sampler's logarithms.  The order of the additions is fixed: a lane's units in its wave's order (row f0, then f1), the four waves
// in order (lm_block_logp), the blocks in index order (dec_finish_kernel<true>), so a replay reproduces the bits.
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

// LOGP, after lm_block_partials (which leaves the waves' bests in sv / si): the block's (m, s) of every row from its four
// waves' pairs in wave order, and the noise-free z of the candidate that lm_block_partials chose.  TARGET: the z of the row's
// target instead, from the wave that met it (the others hold -inf; a maximum, so the order does not matter).
template <int B, class P>
__device__ __forceinline__ void lm_block_logp(const P& p, int lane, int w, float lm, float ls, float lz, const float (*sv)[B],
                                              const int (*si)[B]) {
  __shared__ float slp[4][B][3];
  if (lane < B) { slp[w][lane][0] = lm; slp[w][lane][1] = ls; slp[w][lane][2] = lz; }
  __syncthreads();
  if (threadIdx.x < B) {
    const int b = threadIdx.x;
    float v = sv[0][b], m = slp[0][b][0], s = slp[0][b][1], z = slp[0][b][2];
    int i = si[0][b];
    for (int k = 1; k < 4; ++k) {
      if constexpr (lm_is_target<P>::value) z = fmaxf(z, slp[k][b][2]);
      else if (better(sv[k][b], si[k][b], v, i)) { v = sv[k][b]; i = si[k][b]; z = slp[k][b][2]; }
      lse_merge(slp[k][b][0], slp[k][b][1], m, s);
    }
    float* o = p.plp + ((long long)blockIdx.x * B + b) * 3;
    o[0] = m; o[1] = s; o[2] = z;
  }
}

// The LM heads.  A unit is two vocabulary rows run through lm_row_pair by one wave; the heads differ only in which rows a unit
// is and which wave takes it.
// Full: unit u is rows 2u, 2u + 1 (the last unit of an odd V is one row), unit u = 4 blockIdx.x + w.  SAMPLE: the rows share the
// Philox block (u, b, t, 0).
// SUBSET (the head over an allowed set p.ids[0 .. n)): unit u is the pair ids[2u], ids[2u + 1] (the last unit of an odd n is one
// row); partials and the debug logits carry the vocabulary index, and the partial count stays lap_decode_lm_blocks().  Units go
// to blocks first and to a block's waves second, so that a set of a few hundred rows is streamed by as many CUs; a block
// without a unit writes the neutral partial and skips the norm.  An id outside [0, V) (a broken caller) is never used as an
// address: its row is left out.  SAMPLE: row j takes word j & 1 of the Philox block (j >> 1, b, t, 0), as everywhere; the two
// rows of a unit share a block only when they are 2m and 2m + 1.
// LOGP (SAMPLE instances only; p.samp may then be NULL: greedy): lane b also keeps row b's running (m, s) over z and the z of
// its best candidate, and the block writes them to p.plp (lm_block_logp); pval / pidx / logits are those of the instance without
// it, bit for bit.  A row whose id is outside [0, V) enters neither; the single row of an odd last unit enters once.
// TARGET (P = LmScoreP<.>, a LOGP instance): lane b keeps the z of row b's target tg = cand[1 + t + b] instead of the z of its best
// candidate, and no noise is drawn: pval / pidx are the greedy head's, (m, s) the LOGP head's at the same inv_t.  The target is
// only ever compared with the rows a unit runs, never used as an address: one outside [0, V), outside the subset or at t + b >=
// length meets no row and leaves -inf.  The block that owns the target's unit writes its z, every other block -inf.
template <int B, bool SAMPLE, bool SUBSET, class P, bool LOGP = false>
__global__ __launch_bounds__(256) void dec_lm_head_kernel(P p) {
  static_assert(SAMPLE || !LOGP, "LOGP: the lane-b-owns-row-b form only");
  constexpr bool TARGET = lm_is_target<P>::value;
  static_assert(LOGP || !TARGET, "TARGET: a LOGP instance");
  __shared__ __attribute__((aligned(16))) bf16 sx[B * DEC_D];
  __shared__ float red[4];
  __shared__ float sv[4][B];
  __shared__ int si[4][B];
  if (p.state[1]) return;
  const int units = ((SUBSET ? p.n : p.V) + 1) / 2;
  if (SUBSET && (int)blockIdx.x >= units) {
    if (threadIdx.x < B) {
      p.pval[(long long)blockIdx.x * B + threadIdx.x] = -INFINITY;
      p.pidx[(long long)blockIdx.x * B + threadIdx.x] = 0x7fffffff;
      if constexpr (LOGP) {
        float* o = p.plp + ((long long)blockIdx.x * B + threadIdx.x) * 3;
        o[0] = -INFINITY; o[1] = 0.f; o[2] = -INFINITY;
      }
    }
    return;
  }
  norm_rows_to_lds<B>(p.x, p.gamma, p.D, p.eps, sx, red);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  float bv[B];
  int bi[B];
#pragma unroll
  for (int b = 0; b < B; ++b) { bv[b] = -INFINITY; bi[b] = 0x7fffffff; }
  float lbv = -INFINITY;               // SAMPLE: lane b's running best of row b
  int lbi = 0x7fffffff;
  uint32_t seed_lo = 0, seed_hi = 0, step = 0;
  float inv_t = 0.f;
  if (SAMPLE && (!LOGP || p.samp)) {
    seed_lo = (uint32_t)p.samp[0]; seed_hi = (uint32_t)p.samp[1]; inv_t = __int_as_float(p.samp[2]);
    step = (uint32_t)p.state[0];
  }
  float lm = -INFINITY, ls = 0.f, lz = -INFINITY;      // LOGP: lane b's (m, s) of row b and the z of its best candidate
  int tg = -1;                         // TARGET: lane b's target id, -1 when row b has none
  if constexpr (TARGET) {
    const int j = p.state[0] + lane, len = min(p.cand[0], p.cap);
    if (lane < B && j >= 0 && j < len) tg = p.cand[1 + j];
  }
  for (int u = SUBSET ? blockIdx.x + w * gridDim.x : blockIdx.x * 4 + w; u < units; u += gridDim.x * 4) {
    int f0, f1;
    if (SUBSET) {
      f0 = p.ids[2 * u]; f1 = p.ids[min(2 * u + 1, p.n - 1)];
      const bool ok0 = (unsigned)f0 < (unsigned)p.V, ok1 = (unsigned)f1 < (unsigned)p.V;
      if (!ok0 && !ok1) continue;
      if (!ok0) f0 = f1;
      if (!ok1) f1 = f0;
    } else {
      f0 = 2 * u; f1 = min(2 * u + 1, p.V - 1);
    }
    float y0 = 0.f, y1 = 0.f;
    lm_row_pair<B, SAMPLE>(p, sx, lane, f0, f1, bv, bi, y0, y1);
    if (SAMPLE) {
      float z0 = y0, z1 = y1;
      if constexpr (LOGP) {
        // z = float(logit * inv_t): fmaf(., ., 0) rounds once, like the product.  It is not written as the product the sampler
        // forms, so that the sampler's product keeps its single use and the score compiles to what it compiles to in the
        // instances without LOGP (there the compiler contracts product and sum into one fma): pval stays theirs bit for bit.
        if (inv_t != 0.f) { z0 = __builtin_fmaf(y0, inv_t, 0.0f); z1 = __builtin_fmaf(y1, inv_t, 0.0f); }
        lse_push(z0, lm, ls);
        if (f1 != f0) lse_push(z1, lm, ls);
        if constexpr (TARGET) {
          if (f0 == tg) lz = z0;
          if (f1 != f0 && f1 == tg) lz = z1;
        }
      }
      if (!TARGET && inv_t != 0.f) {
        if (SUBSET) lap_sampling::gumbel_scores_at(y0, y1, inv_t, seed_lo, seed_hi, step, (uint32_t)lane, (uint32_t)f0, (uint32_t)f1, y0, y1);
        else lap_sampling::gumbel_scores(y0, y1, inv_t, seed_lo, seed_hi, step, (uint32_t)lane, (uint32_t)u, y0, y1);
      }
      if (better(y0, f0, lbv, lbi)) { lbv = y0; lbi = f0; if constexpr (LOGP && !TARGET) lz = z0; }
      if (f1 != f0 && better(y1, f1, lbv, lbi)) { lbv = y1; lbi = f1; if constexpr (LOGP && !TARGET) lz = z1; }
    }
  }
  lm_block_partials<B, SAMPLE>(p, lane, w, bv, bi, lbv, lbi, sv, si);
  if constexpr (LOGP) lm_block_logp<B>(p, lane, w, lm, ls, lz, sv, si);
}

// one block: per sample, the best of the partials (lowest index among ties); then out[:, t], EOS mask, t + 1, done.
// LOGP (nblk <= LM_BLOCKS): also logp[b][t] = z_tok - (M + logf(S)) from the LM head's plp partials {m, s, z of the block's best}.
// The reduction carries the block index k of the best partial (a payload: the choice is unchanged), z_tok is that block's z.  M =
// max of the blocks' m (exact in any order); the terms s_k expf(m_k - M) (an empty block's is 0) are formed by all threads and
// added by lane b for row b in block index order.
template <bool LOGP>
__global__ __launch_bounds__(256) void dec_finish_kernel(int* state, const float* pval, const int* pidx, int nblk, int* out, int cap,
                                                         int B, int eos_token, const float* plp, float* logp) {
  __shared__ float sv[4];
  __shared__ int si[4];
  __shared__ int tok[DEC_MAXB];
  __shared__ float sm[LOGP ? 4 : 1], term[LOGP ? DEC_MAXB : 1][LOGP ? LM_BLOCKS + 1 : 1], lpv[LOGP ? DEC_MAXB : 1][2];
  __shared__ int sk[LOGP ? 4 : 1];
  if (state[1]) return;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int b = 0; b < B; ++b) {
    float v = -INFINITY;
    int i = 0x7fffffff;
    int kb = 0;
    float M = -INFINITY;
    for (int k = threadIdx.x; k < nblk; k += 256) {
      const float pv = pval[(long long)k * B + b];
      const int pi = pidx[(long long)k * B + b];
      if (better(pv, pi, v, i)) { v = pv; i = pi; if constexpr (LOGP) kb = k; }
      if constexpr (LOGP) M = fmaxf(M, plp[((long long)k * B + b) * 3]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(i, o, 64);
      if constexpr (LOGP) {
        const int ok = __shfl_xor(kb, o, 64);
        if (better(ov, oi, v, i)) kb = ok;
        M = fmaxf(M, __shfl_xor(M, o, 64));
      }
      if (better(ov, oi, v, i)) { v = ov; i = oi; }
    }
    if (lane == 0) {
      sv[w] = v; si[w] = i;
      if constexpr (LOGP) { sk[w] = kb; sm[w] = M; }
    }
    __syncthreads();
    if constexpr (LOGP) {
      M = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
      for (int k = threadIdx.x; k < nblk; k += 256) {
        const float* q = plp + ((long long)k * B + b) * 3;
        term[b][k] = q[0] == -INFINITY ? 0.f : __fmul_rn(q[1], expf(q[0] - M));
      }
    }
    if (threadIdx.x == 0) {
      for (int k = 1; k < 4; ++k)
        if (better(sv[k], si[k], v, i)) { v = sv[k]; i = si[k]; if constexpr (LOGP) kb = sk[k]; }
      tok[b] = i;
      if constexpr (LOGP) { lpv[b][0] = M; lpv[b][1] = plp[((long long)kb * B + b) * 3 + 2]; }
    }
    __syncthreads();
  }
  if constexpr (LOGP) {
    if (threadIdx.x < B) {
      const int b = threadIdx.x;
      float S = 0.f;
      for (int k = 0; k < nblk; ++k) S = __fadd_rn(S, term[b][k]);
      lpv[b][1] = lpv[b][1] - (lpv[b][0] + logf(S));
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int t = state[0];
    if (t >= cap) { state[1] = 1; return; }
    int all = 1;
    for (int b = 0; b < B; ++b) {
      if constexpr (LOGP) logp[(long long)b * cap + t] = lpv[b][1];
      out[(long long)b * cap + t] = tok[b];
      const int e = state[8 + b] | (tok[b] == eos_token ? 1 : 0);
      state[8 + b] = e;
      all &= e;
    }
    state[0] = t + 1;
    state[1] = (t + 1 >= cap || all) ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void dec_init_kernel(int* state, const int* plen, int* out, int B, int cap) {
  for (long long i = threadIdx.x; i < (long long)B * cap; i += 256) out[i] = 0;
  if (threadIdx.x < 32) {
    const int i = threadIdx.x;
    state[i] = (i >= 16 && i < 16 + B) ? plen[i - 16] : 0;
  }
}

#define DISPATCH_B(B_, ...)                                                        \
  switch (B_) {                                                                    \
    case 1: { constexpr int BB = 1; __VA_ARGS__; } break;                          \
    case 2: { constexpr int BB = 2; __VA_ARGS__; } break;                          \
    case 3: { constexpr int BB = 3; __VA_ARGS__; } break;                          \
    case 4: { constexpr int BB = 4; __VA_ARGS__; } break;                          \
    case 5: { constexpr int BB = 5; __VA_ARGS__; } break;                          \
    case 6: { constexpr int BB = 6; __VA_ARGS__; } break;                          \
    case 7: { constexpr int BB = 7; __VA_ARGS__; } break;                          \
    case 8: { constexpr int BB = 8; __VA_ARGS__; } break;                          \
    default: return LAP_ERR_ARG;                                                   \
  }

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ------------------------------------------------------------------------------------------------- e4m3 row quantiser
// One block per row (grid stride): amax, e = the largest integer with amax 2^e <= 448 (0 for an all-zero row; kept inside
// [-126, 126] so that 2^e and 2^-e are normal f32 numbers), scale[n] = 2^e, codes = e4m3(w 2^e) to nearest even.  w 2^e is
// exact and never above 448, so the conversion needs no clamp.  Runs once per parameter version.
template <class T>
__global__ __launch_bounds__(256) void quant_fp8_rows_kernel(const T* src, uint8_t* codes, float* scales, long long N, int K) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (long long n = blockIdx.x; n < N; n += gridDim.x) {
    const T* s = src + n * K;
    float am = 0.f;
    for (int c = threadIdx.x * 4; c < K; c += 1024) {
#pragma unroll
      for (int e = 0; e < 4; ++e) am = fmaxf(am, fabsf((float)s[c + e]));
    }
    am = wave_max(am);
    __syncthreads();
    if (lane == 0) red[w] = am;
    __syncthreads();
    am = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    int e = 0;
    if (am > 0.f) {
      int x;
      const float m = frexpf(am, &x);                 // am = m 2^x, 0.5 <= m < 1; 448 = 0.875 2^9
      e = min(max((m <= 0.875f ? 9 : 8) - x, -126), 126);
    }
    const float sc = ldexpf(1.0f, e);
    if (threadIdx.x == 0) scales[n] = sc;
    for (int c = threadIdx.x * 4; c < K; c += 1024) {
      int q = 0;
      q = __builtin_amdgcn_cvt_pk_fp8_f32((float)s[c] * sc, (float)s[c + 1] * sc, q, false);
      q = __builtin_amdgcn_cvt_pk_fp8_f32((float)s[c + 2] * sc, (float)s[c + 3] * sc, q, true);
      *reinterpret_cast<int*>(codes + n * K + c) = q;
    }
  }
}

// a wave's K slice is whole lane loads of the code stream (a slice of 512 codes keeps half the lanes of a 16-byte load busy)
inline bool f8_k_ok(int K, int kwaves) { return K % 16 == 0 && K % kwaves == 0 && (K / kwaves) % F8L == 0; }

// the launch of one projection (EPI, NORM, KW) on the bf16 or the fp8 weight stream, at the batch B
template <int EPI, bool NORM, int KW, class P>
int launch_proj_p(const P& p, int B, dim3 grid, void* stream) {
  DISPATCH_B(B, hipLaunchKernelGGL((dec_proj_kernel<EPI, BB, NORM, KW, P>), grid, dim3(256), 0, S_, p));
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}
template <int EPI, bool NORM, int KW>
int launch_proj(const ProjP8& p, bool f8, int B, dim3 grid, void* stream) {
  return f8 ? launch_proj_p<EPI, NORM, KW, ProjP8>(p, B, grid, stream) : launch_proj_p<EPI, NORM, KW, ProjP>(p, B, grid, stream);
}

int qkv_impl(const int* state, const void* x, const float* gamma, const void* wqkv, const float* wscale, bool f8, void* q,
             void* cache_k, void* cache_v, int B, int D, int NH, int HD, int cap, float q_scale, float eps, void* stream,
             bool spec = false) {
  if (!lap_decode_ok(B, D, NH, 1, HD, DEC_H, 2) || !state || !gamma || !q || !cache_k || !cache_v || cap < 1 ||
      !aligned16(x) || !aligned16(wqkv) || (f8 && (!wscale || !f8_k_ok(D, 1)))) return LAP_ERR_ARG;
  ProjP8 p{};
  p.state = state; p.x = (const bf16*)x; p.gamma = gamma; p.w = (const bf16*)wqkv; p.K = D; p.units = (NH + 2) * HD / 2;
  p.eps = eps; p.q = (bf16*)q; p.ck = (bf16*)cache_k; p.cv = (bf16*)cache_v; p.cap = cap; p.NH = NH; p.HD = HD; p.q_scale = q_scale;
  p.wscale = wscale;
  if (spec) return launch_proj<EPI_QKV_SPEC, true, 1>(p, f8, B, dim3((p.units + 3) / 4), stream);
  return launch_proj<EPI_QKV, true, 1>(p, f8, B, dim3((p.units + 3) / 4), stream);
}

int gate_up_impl(const int* state, const void* x, const float* gamma, const void* wgu, const float* wscale, bool f8, void* act,
                 int B, int D, int H, float eps, void* stream) {
  if (!lap_decode_ok(B, D, DEC_NH, 1, DEC_HD, H, 2) || !state || !gamma || !act || !aligned16(x) || !aligned16(wgu) ||
      (f8 && (!wscale || !f8_k_ok(D, 1)))) return LAP_ERR_ARG;
  ProjP8 p{};
  p.state = state; p.x = (const bf16*)x; p.gamma = gamma; p.w = (const bf16*)wgu; p.K = D; p.units = H; p.H = H; p.eps = eps;
  p.out = (bf16*)act;
  p.wscale = wscale;
  return launch_proj<EPI_GEGLU, true, 1>(p, f8, B, dim3(min(H / 4, 1024)), stream);
}

int proj_residual_impl(const int* state, const void* a, const void* w, const float* wscale, bool f8, const void* x, void* y, int B,
                       int N, int K, int kwaves, void* stream) {
  if (!state || !a || !w || !x || !y || B < 1 || B > DEC_MAXB || N < 2 || (N & 1) || K < 512 || (K % 2048) ||
      (kwaves != 1 && kwaves != 4) || !aligned16(a) || !aligned16(w) || ((uintptr_t)y & 3) || ((uintptr_t)x & 3) ||
      (f8 && (!wscale || !f8_k_ok(K, kwaves)))) return LAP_ERR_ARG;
  ProjP8 p{};
  p.state = state; p.x = (const bf16*)a; p.w = (const bf16*)w; p.K = K; p.units = N / 2; p.N = N; p.res = (const bf16*)x;
  p.out = (bf16*)y;
  p.wscale = wscale;
  const int nu = 4 / kwaves;
  const dim3 grid(min((p.units + nu - 1) / nu, 2048));
  return kwaves == 4 ? launch_proj<EPI_RES, false, 4>(p, f8, B, grid, stream) : launch_proj<EPI_RES, false, 1>(p, f8, B, grid, stream);
}

template <bool SAMPLE, bool SUBSET, class P, bool LOGP = false>
int launch_lm_head(const P& p, int B, void* stream) {
  DISPATCH_B(B, hipLaunchKernelGGL((dec_lm_head_kernel<BB, SAMPLE, SUBSET, P, LOGP>), dim3(LM_BLOCKS), dim3(256), 0, S_, p));
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

// sampling == NULL: the greedy head.  f8: `hi` holds the code plane, `lo` is not used.  subset: the head over ids[0 .. n).
// plp != NULL: the LOGP instances (the sampling form of the kernel, which is the greedy head while sampling is NULL or inv_t == 0).
int lm_head_impl(const int* state, const int* sampling, bool sample, const void* x, const float* gamma, const void* hi, const void* lo,
                 const float* wscale, bool f8, int B, int D, int V, float eps, float* logits, float* pval, int* pidx, void* stream,
                 bool subset = false, const int* ids = nullptr, int n = 0, float* plp = nullptr, const int* cand = nullptr,
                 int cand_cap = 0) {
  if (!state || (sample && !sampling) || !gamma || !hi || !pval || !pidx || B < 1 || B > DEC_MAXB || D != DEC_D || V < 2 ||
      !aligned16(x) || !aligned16(hi) || (lo && !aligned16(lo)) || (f8 && (!wscale || !f8_k_ok(D, 1))) ||
      (subset && (!ids || n < 1 || n > V))) return LAP_ERR_ARG;
  LmP8 p{};
  p.state = state; p.x = (const bf16*)x; p.gamma = gamma; p.eps = eps; p.hi = (const bf16*)hi; p.lo = f8 ? nullptr : (const bf16*)lo;
  p.V = V; p.D = D; p.logits = logits; p.pval = pval; p.pidx = pidx; p.samp = sampling; p.ids = ids; p.n = n;
  p.wscale = wscale;
  if (cand) {      // the TARGET instances (plp is theirs too)
    if (!plp || cand_cap < 1) return LAP_ERR_ARG;
    LmScoreP<LmP> q{};
    LmScoreP<LmP8> q8{};
    static_cast<LmP&>(q) = p; static_cast<LmP8&>(q8) = p;
    q.plp = q8.plp = plp; q.cand = q8.cand = cand; q.cap = q8.cap = cand_cap;
    switch ((f8 ? 2 : 0) | (subset ? 1 : 0)) {
      case 0: return launch_lm_head<true, false, LmScoreP<LmP>, true>(q, B, stream);
      case 1: return launch_lm_head<true, true, LmScoreP<LmP>, true>(q, B, stream);
      case 2: return launch_lm_head<true, false, LmScoreP<LmP8>, true>(q8, B, stream);
      default: return launch_lm_head<true, true, LmScoreP<LmP8>, true>(q8, B, stream);
    }
  }
  if (plp) {
    LmLogP<LmP> q{};
    LmLogP<LmP8> q8{};
    static_cast<LmP&>(q) = p; static_cast<LmP8&>(q8) = p;
    q.plp = q8.plp = plp;
    switch ((f8 ? 2 : 0) | (subset ? 1 : 0)) {
      case 0: return launch_lm_head<true, false, LmLogP<LmP>, true>(q, B, stream);
      case 1: return launch_lm_head<true, true, LmLogP<LmP>, true>(q, B, stream);
      case 2: return launch_lm_head<true, false, LmLogP<LmP8>, true>(q8, B, stream);
      default: return launch_lm_head<true, true, LmLogP<LmP8>, true>(q8, B, stream);
    }
  }
  switch ((sample ? 4 : 0) | (f8 ? 2 : 0) | (subset ? 1 : 0)) {
    case 0: return launch_lm_head<false, false, LmP>(p, B, stream);
    case 1: return launch_lm_head<false, true, LmP>(p, B, stream);
    case 2: return launch_lm_head<false, false, LmP8>(p, B, stream);
    case 3: return launch_lm_head<false, true, LmP8>(p, B, stream);
    case 4: return launch_lm_head<true, false, LmP>(p, B, stream);
    case 5: return launch_lm_head<true, true, LmP>(p, B, stream);
    case 6: return launch_lm_head<true, false, LmP8>(p, B, stream);
    default: return launch_lm_head<true, true, LmP8>(p, B, stream);
  }
}

}  // namespace

extern "C" int lap_decode_ok(int B, int D, int NH, int NKV, int HD, int H, int V) {
  return B >= 1 && B <= DEC_MAXB && D == DEC_D && NH == DEC_NH && NKV == DEC_NKV && HD == DEC_HD && H == DEC_H && V >= 2 ? 1 : 0;
}

extern "C" int lap_decode_state_words(void) { return 32; }

extern "C" int lap_decode_lm_blocks(void) { return LM_BLOCKS; }

extern "C" int lap_decode_init(int* state, const int* plen, int* out, int B, int cap, void* stream) {
  if (!state || !plen || !out || B < 1 || B > DEC_MAXB || cap < 1) return LAP_ERR_ARG;
  hipLaunchKernelGGL(dec_init_kernel, dim3(1), dim3(256), 0, S_, state, plen, out, B, cap);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

extern "C" int lap_decode_embed(const int* state, const float* table, int row_lo, int row_hi, const int* out, int cap, void* x,
                                int B, int D, float scale, void* stream) {
  if (!state || !table || !out || !x || B < 1 || B > DEC_MAXB || D != DEC_D || cap < 1 || !aligned16(table) || !aligned16(x)) return LAP_ERR_ARG;
  hipLaunchKernelGGL(dec_embed_kernel, dim3(B), dim3(256), 0, S_, state, table, row_lo, row_hi, out, cap, (bf16*)x, D, scale);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

extern "C" int lap_decode_qkv(const int* state, const void* x, const float* gamma, const void* wqkv, void* q, void* cache_k,
                              void* cache_v, int B, int D, int NH, int HD, int cap, float q_scale, float eps, void* stream) {
  return qkv_impl(state, x, gamma, wqkv, nullptr, false, q, cache_k, cache_v, B, D, NH, HD, cap, q_scale, eps, stream);
}

extern "C" int lap_decode_gate_up(const int* state, const void* x, const float* gamma, const void* wgu, void* act, int B, int D,
                                  int H, float eps, void* stream) {
  return gate_up_impl(state, x, gamma, wgu, nullptr, false, act, B, D, H, eps, stream);
}

extern "C" int lap_decode_proj_residual(const int* state, const void* a, const void* w, const void* x, void* y, int B, int N, int K,
                                        int kwaves, void* stream) {
  return proj_residual_impl(state, a, w, nullptr, false, x, y, B, N, K, kwaves, stream);
}

extern "C" int lap_decode_attn_scratch_floats(int B, int Pn, int cap) {
  if (B < 1 || B > DEC_MAXB || Pn < 1 || cap < 1 || Pn > (1 << 20) || cap > (1 << 20)) return -1;
  const int nchunk = (Pn + KC - 1) / KC + (cap + KC - 1) / KC;
  return B * nchunk * DEC_NH * (DEC_HD + 1);
}

namespace {
int attention_impl(const int* state, const void* q, const void* prefix_k, const void* prefix_v, const int* kinfo, int Pn,
                   const void* cache_k, const void* cache_v, int cap, void* o, float* scratch, long long scratch_floats, int B, int NH,
                   int NKV, int HD, bool spec, void* stream) {
  if (!state || !q || !prefix_k || !prefix_v || !kinfo || !cache_k || !cache_v || !o || !scratch || Pn < 1 || cap < 1 ||
      !lap_decode_ok(B, DEC_D, NH, NKV, HD, DEC_H, 2) || scratch_floats < lap_decode_attn_scratch_floats(B, Pn, cap) ||
      !aligned16(scratch)) return LAP_ERR_ARG;
  AttnDecP p{};
  p.state = state; p.q = (const bf16*)q; p.pk = (const bf16*)prefix_k; p.pv = (const bf16*)prefix_v; p.kinfo = kinfo;
  p.gk = (const bf16*)cache_k; p.gv = (const bf16*)cache_v; p.Pn = Pn; p.cap = cap;
  p.npre = (Pn + KC - 1) / KC;
  p.nchunk = p.npre + (cap + KC - 1) / KC;
  p.opart = scratch;
  p.lpart = scratch + (long long)B * p.nchunk * DEC_NH * DEC_HD;
  p.o = (bf16*)o;
  if (spec) hipLaunchKernelGGL(dec_attn_kernel<true>, dim3((p.nchunk + 3) / 4, B), dim3(256), 0, S_, p);
  else hipLaunchKernelGGL(dec_attn_kernel<false>, dim3((p.nchunk + 3) / 4, B), dim3(256), 0, S_, p);
  LAP_CHECK_LAUNCH();
  hipLaunchKernelGGL(dec_attn_combine_kernel, dim3(DEC_NH, B), dim3(64), 0, S_, p);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}
}  // namespace

extern "C" int lap_decode_attention(const int* state, const void* q, const void* prefix_k, const void* prefix_v, const int* kinfo,
                                    int Pn, const void* cache_k, const void* cache_v, int cap, void* o, float* scratch,
                                    long long scratch_floats, int B, int NH, int NKV, int HD, void* stream) {
  return attention_impl(state, q, prefix_k, prefix_v, kinfo, Pn, cache_k, cache_v, cap, o, scratch, scratch_floats, B, NH, NKV, HD,
                        false, stream);
}

extern "C" int lap_decode_lm_head(const int* state, const void* x, const float* gamma, const void* hi, const void* lo, int B, int D,
                                  int V, float eps, float* logits, float* pval, int* pidx, void* stream) {
  return lm_head_impl(state, nullptr, false, x, gamma, hi, lo, nullptr, false, B, D, V, eps, logits, pval, pidx, stream);
}

extern "C" int lap_decode_sampling_words(void) { return 4; }

extern "C" int lap_decode_lm_head_sample(const int* state, const int* sampling, const void* x, const float* gamma, const void* hi,
                                         const void* lo, int B, int D, int V, float eps, float* logits, float* pval, int* pidx,
                                         void* stream) {
  return lm_head_impl(state, sampling, true, x, gamma, hi, lo, nullptr, false, B, D, V, eps, logits, pval, pidx, stream);
}

extern "C" int lap_decode_finish(int* state, const float* pval, const int* pidx, int* out, int B, int cap, int eos_token,
                                 void* stream) {
  if (!state || !pval || !pidx || !out || B < 1 || B > DEC_MAXB || cap < 1) return LAP_ERR_ARG;
  hipLaunchKernelGGL(dec_finish_kernel<false>, dim3(1), dim3(256), 0, S_, state, pval, pidx, LM_BLOCKS, out, cap, B, eos_token,
                     (const float*)nullptr, (float*)nullptr);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

// ---- fp8 weight-only decoding: the entry points above on e4m3 codes [N][K] + f32 row scales [N] (2^e)
extern "C" int lap_quantize_fp8_rows(const void* src, int src_f32, void* codes, float* scales, long long N, int K, void* stream) {
  if (!src || !codes || !scales || N < 1 || N > 0x7fffffffLL || K < 4 || (K & 3) || ((uintptr_t)codes & 3)) return LAP_ERR_ARG;
  const dim3 grid((unsigned)min(N, 1LL << 20));
  if (src_f32) hipLaunchKernelGGL(quant_fp8_rows_kernel<float>, grid, dim3(256), 0, S_, (const float*)src, (uint8_t*)codes, scales, N, K);
  else hipLaunchKernelGGL(quant_fp8_rows_kernel<bf16>, grid, dim3(256), 0, S_, (const bf16*)src, (uint8_t*)codes, scales, N, K);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

extern "C" int lap_decode_qkv_fp8(const int* state, const void* x, const float* gamma, const void* wqkv8, const float* wscale, void* q,
                                  void* cache_k, void* cache_v, int B, int D, int NH, int HD, int cap, float q_scale, float eps,
                                  void* stream) {
  return qkv_impl(state, x, gamma, wqkv8, wscale, true, q, cache_k, cache_v, B, D, NH, HD, cap, q_scale, eps, stream);
}

extern "C" int lap_decode_gate_up_fp8(const int* state, const void* x, const float* gamma, const void* wgu8, const float* wscale,
                                      void* act, int B, int D, int H, float eps, void* stream) {
  return gate_up_impl(state, x, gamma, wgu8, wscale, true, act, B, D, H, eps, stream);
}

extern "C" int lap_decode_proj_residual_fp8(const int* state, const void* a, const void* w8, const float* wscale, const void* x, void* y,
                                            int B, int N, int K, int kwaves, void* stream) {
  return proj_residual_impl(state, a, w8, wscale, true, x, y, B, N, K, kwaves, stream);
}

extern "C" int lap_decode_lm_head_fp8(const int* state, const void* x, const float* gamma, const void* w8, const float* wscale, int B,
                                      int D, int V, float eps, float* logits, float* pval, int* pidx, void* stream) {
  return lm_head_impl(state, nullptr, false, x, gamma, w8, nullptr, wscale, true, B, D, V, eps, logits, pval, pidx, stream);
}

extern "C" int lap_decode_lm_head_sample_fp8(const int* state, const int* sampling, const void* x, const float* gamma, const void* w8,
                                             const float* wscale, int B, int D, int V, float eps, float* logits, float* pval, int* pidx,
                                             void* stream) {
  return lm_head_impl(state, sampling, true, x, gamma, w8, nullptr, wscale, true, B, D, V, eps, logits, pval, pidx, stream);
}

// ---- constrained decoding: the four LM heads over an allowed set of vocabulary rows (ids: int32 [n], sorted, unique, in [0, V))
extern "C" int lap_decode_lm_head_subset(const int* state, const void* x, const float* gamma, const void* hi, const void* lo,
                                         const int* ids, int n, int B, int D, int V, float eps, float* logits, float* pval, int* pidx,
                                         void* stream) {
  return lm_head_impl(state, nullptr, false, x, gamma, hi, lo, nullptr, false, B, D, V, eps, logits, pval, pidx, stream, true, ids, n);
}

extern "C" int lap_decode_lm_head_subset_sample(const int* state, const int* sampling, const void* x, const float* gamma, const void* hi,
                                                const void* lo, const int* ids, int n, int B, int D, int V, float eps, float* logits,
                                                float* pval, int* pidx, void* stream) {
  return lm_head_impl(state, sampling, true, x, gamma, hi, lo, nullptr, false, B, D, V, eps, logits, pval, pidx, stream, true, ids, n);
}

extern "C" int lap_decode_lm_head_subset_fp8(const int* state, const void* x, const float* gamma, const void* w8, const float* wscale,
                                             const int* ids, int n, int B, int D, int V, float eps, float* logits, float* pval,
                                             int* pidx, void* stream) {
  return lm_head_impl(state, nullptr, false, x, gamma, w8, nullptr, wscale, true, B, D, V, eps, logits, pval, pidx, stream, true, ids, n);
}

extern "C" int lap_decode_lm_head_subset_sample_fp8(const int* state, const int* sampling, const void* x, const float* gamma,
                                                    const void* w8, const float* wscale, const int* ids, int n, int B, int D, int V,
                                                    float eps, float* logits, float* pval, int* pidx, void* stream) {
  return lm_head_impl(state, sampling, true, x, gamma, w8, nullptr, wscale, true, B, D, V, eps, logits, pval, pidx, stream, true, ids, n);
}

// ---- token log-probabilities: one LM head for every form that also leaves the log-sum-exp partials, and the finish that reads them
extern "C" int lap_decode_lm_head_lp(const int* state, const int* sampling, const void* x, const float* gamma, const void* hi,
                                     const void* lo, const float* wscale, const int* ids, int n, int B, int D, int V, float eps,
                                     float* logits, float* pval, int* pidx, float* plp, void* stream) {
  if (!plp || (wscale && lo)) return LAP_ERR_ARG;
  return lm_head_impl(state, sampling, false, x, gamma, hi, lo, wscale, wscale != nullptr, B, D, V, eps, logits, pval, pidx, stream,
                      ids != nullptr, ids, n, plp);
}

extern "C" int lap_decode_finish_lp(int* state, const float* pval, const int* pidx, const float* plp, int* out, float* logp, int B,
                                    int cap, int eos_token, void* stream) {
  if (!state || !pval || !pidx || !plp || !out || !logp || B < 1 || B > DEC_MAXB || cap < 1) return LAP_ERR_ARG;
  hipLaunchKernelGGL(dec_finish_kernel<true>, dim3(1), dim3(256), 0, S_, state, pval, pidx, LM_BLOCKS, out, cap, B, eos_token, plp, logp);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

// ---- teacher-forced scoring (lap_amd/score.py; the embed and finish kernels are csrc/decode_score.hip): the LOGP heads whose third
// plp word is the z of the target cand[1 + t + b] of row b.  sampling NULL or inv_t == 0: z = logit; ids != NULL: the SUBSET form.
extern "C" int lap_decode_lm_head_score(const int* state, const int* sampling, const int* cand, int cap, const void* x,
                                        const float* gamma, const void* hi, const void* lo, const int* ids, int n, int B, int D, int V,
                                        float eps, float* logits, float* pval, int* pidx, float* plp, void* stream) {
  if (!plp || !cand) return LAP_ERR_ARG;
  return lm_head_impl(state, sampling, false, x, gamma, hi, lo, nullptr, false, B, D, V, eps, logits, pval, pidx, stream, ids != nullptr,
                      ids, n, plp, cand, cap);
}

extern "C" int lap_decode_lm_head_score_fp8(const int* state, const int* sampling, const int* cand, int cap, const void* x,
                                            const float* gamma, const void* w8, const float* wscale, const int* ids, int n, int B, int D,
                                            int V, float eps, float* logits, float* pval, int* pidx, float* plp, void* stream) {
  if (!plp || !cand || !wscale) return LAP_ERR_ARG;
  return lm_head_impl(state, sampling, false, x, gamma, w8, nullptr, wscale, true, B, D, V, eps, logits, pval, pidx, stream,
                      ids != nullptr, ids, n, plp, cand, cap);
}

// ---- speculative decoding (lap_amd/speculate.py; the draft, embed and accept kernels are csrc/decode_spec.hip): the QKV and
// attention variants whose S rows are consecutive positions of one sequence.  wscale != NULL: wqkv holds e4m3 codes.
extern "C" int lap_decode_spec_qkv(const int* state, const void* x, const float* gamma, const void* wqkv, const float* wscale, void* q,
                                   void* cache_k, void* cache_v, int S, int D, int NH, int HD, int cap, float q_scale, float eps,
                                   void* stream) {
  if (S < 2) return LAP_ERR_ARG;
  return qkv_impl(state, x, gamma, wqkv, wscale, wscale != nullptr, q, cache_k, cache_v, S, D, NH, HD, cap, q_scale, eps, stream, true);
}

extern "C" int lap_decode_spec_attention(const int* state, const void* q, const void* prefix_k, const void* prefix_v, const int* kinfo,
                                         int Pn, const void* cache_k, const void* cache_v, int cap, void* o, float* scratch,
                                         long long scratch_floats, int S, int NH, int NKV, int HD, void* stream) {
  if (S < 2) return LAP_ERR_ARG;
  return attention_impl(state, q, prefix_k, prefix_v, kinfo, Pn, cache_k, cache_v, cap, o, scratch, scratch_floats, S, NH, NKV, HD,
                        true, stream);
}
