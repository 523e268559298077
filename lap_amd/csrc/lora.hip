// Low-rank adapter (LoRA) arithmetic of the Gemma projections (lora.Einsum / lora.FeedForward of openpi, gemma.py:180-200,
// 279-285,366-372 of the reference), gfx950.
//
// Every LoRA'd projection y = x W (+ s (x A) B) is described by G groups of rank R: the down matrix A has G*R rows
// ([G*R][K], k contiguous, like the engine's Wt) and the up matrix B has nsum stacked copies of G*R rows ([nsum*G*R][Ng],
// n contiguous); group g adds columns [g*Ng, (g+1)*Ng) of y from columns [g*R, (g+1)*R) of t = x A^T.  q|k|v: one group per
// head (R = r, Ng = head_dim); gate|up: two groups; out / down projections: one group, and the out projection sums its
// nsum = num_heads copies of B (attn_vec_einsum's `BTL,NLD->BTD`: N is summed out of lora_b).
//
//   lap_lora_down     t[m][g*R + c] = bf16(sum_n sum_k xs[m][g*xg + k] * W[(n*G + g)*R + c][k])      v_mfma_f32_16x16x32_bf16
//                     the forward down projection (xg = 0, G = 1, W = A) and the data gradient of t (X = dy, xg = Ng, W = B);
//                     xs = X, or bf16(s * X) when s != 1 (the cotangent of the reference's bf16(p) * s)
//   lap_lora_up_add   y[m][g*Ng + c] = bf16(y + bf16(s * bf16(sum_n sum_j t[m][g*R + j] * B[(n*G + g)*R + j][c])))  in place,
//                     f32 FMA (the contraction is R <= 320 long); also the data-gradient add dx += bf16(dt A) (G = 1, s = 1)
//   lap_lora_wgrad    out[(n*G + g)*R + i][c] = sum_m a[m][g*R + i] * bs[m][g*bg + c] for every copy n < ncopy: dA = dt^T x,
//                     dB = t^T dy (bs = bf16(s * dy) when s != 1); f32 MFMA accumulation over M in a fixed order, split over
//                     M into f32 partials that a second pass sums in order (deterministic), bf16 or f32 output
//   lap_lora_merge    Weff[g*Ng + c][i] = bf16(W[g*Ng + c][i] + s * sum_n sum_j B[(n*G + g)*R + j][c] * A[g*R + j][i]), f32 in
//                     (the serving paths' merged weights)
//
// Stores are plain vector / per-lane global stores.
#include "common.hpp"
#include "../../include/lap_hip.h"

#define S_ ((hipStream_t)stream)

namespace {

__device__ __forceinline__ bf16x8 zero8() {
  u32x4 z = {0u, 0u, 0u, 0u};
  return __builtin_bit_cast(bf16x8, z);
}

__device__ __forceinline__ bf16x8 scale8(bf16x8 v, float s) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = f2bf(bf2f(v[j]) * s);
  return v;
}

// One wave = 16 rows x up to 4 column tiles of 16; a block = 4 waves (64 rows); blockIdx.y = group * nchunk + column chunk.
__global__ __launch_bounds__(256) void lora_down_kernel(const bf16* __restrict__ X, int ldx, int xg, const bf16* __restrict__ W, int ldw,
                                                        int nsum, bf16* __restrict__ T, int ldt, int M, int K, int G, int R, float s,
                                                        int nchunk) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = blockIdx.y / nchunk, c0 = (blockIdx.y % nchunk) * 64;
  const int nt = min(4, (R - c0) >> 4);
  const int m0 = blockIdx.x * 64 + wave * 16;
  const int row = m0 + (lane & 15);
  const bool row_ok = row < M;
  const int kq = 8 * (lane >> 4);
  const bf16* xr = X + (long long)(row_ok ? row : 0) * ldx + (long long)g * xg;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int n = 0; n < nsum; ++n) {
    const bf16* wb = W + ((long long)(n * G + g) * R + c0 + (lane & 15)) * ldw;
    for (int k0 = 0; k0 < K; k0 += 32) {
      const int k = k0 + kq;
      const bool k_ok = k < K;
      bf16x8 a = zero8();
      if (row_ok && k_ok) a = *(const bf16x8*)(xr + k);
      if (s != 1.0f) a = scale8(a, s);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (t < nt) {
          bf16x8 b = zero8();
          if (k_ok) b = *(const bf16x8*)(wb + (long long)t * 16 * ldw + k);
          acc[t] = mfma16(a, b, acc[t]);
        }
      }
    }
  }
  // C/D of 16x16x32: column = lane & 15, row = 4 (lane >> 4) + i
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (t < nt) {
      const int col = g * R + c0 + t * 16 + (lane & 15);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = m0 + 4 * (lane >> 4) + i;
        if (r < M) T[(long long)r * ldt + col] = f2bf(acc[t][i]);
      }
    }
  }
}

// A thread: 8 consecutive columns (one 16-byte load / store of y) x 4 rows; a block: 512 columns x 16 rows.
__global__ __launch_bounds__(256) void lora_up_add_kernel(const bf16* __restrict__ T, int ldt, const bf16* __restrict__ Bm, int ldb,
                                                          int nsum, bf16* __restrict__ Y, int ldy, int M, int Ng, int G, int R, float s) {
  const int col = (blockIdx.x * 64 + (threadIdx.x & 63)) * 8;
  if (col >= G * Ng) return;
  const int g = col / Ng, c = col - g * Ng;
  const int r0 = blockIdx.y * 16 + (threadIdx.x >> 6) * 4;
  const bf16* tb = T + (long long)g * R;
  long long trow[4];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) trow[rr] = (long long)min(r0 + rr, M - 1) * ldt;
  float acc[4][8];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[rr][e] = 0.f;
  for (int n = 0; n < nsum; ++n) {
    const bf16* bb = Bm + (long long)(n * G + g) * R * ldb + c;
    for (int j = 0; j < R; ++j) {
      const bf16x8 bv = *(const bf16x8*)(bb + (long long)j * ldb);
      float b[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) b[e] = bf2f(bv[e]);
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const float tv = bf2f(tb[trow[rr] + j]);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[rr][e] = __builtin_fmaf(tv, b[e], acc[rr][e]);
      }
    }
  }
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int r = r0 + rr;
    if (r >= M) break;
    bf16x8* yp = (bf16x8*)(Y + (long long)r * ldy + col);
    bf16x8 yv = *yp;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float p = round_bf16(acc[rr][e]);
      if (s != 1.0f) p = round_bf16(p * s);
      yv[e] = f2bf(bf2f(yv[e]) + p);
    }
    *yp = yv;
  }
}

// Output tile 16 rows (of one group) x 64 columns; 4 waves of 16 x 16.  M advances in steps of 32 (one MFMA k-step) through LDS.
__global__ __launch_bounds__(256) void lora_wgrad_kernel(const bf16* __restrict__ A, int lda, const bf16* __restrict__ Bm, int ldb, int bg,
                                                         void* __restrict__ out, int ldo, int ncopy, int out_f32, float* __restrict__ part,
                                                         int M, int Ng, int G, int R, float s, int mchunk) {
  __shared__ __attribute__((aligned(16))) bf16 sa[32][16];
  __shared__ __attribute__((aligned(16))) bf16 sb[32][64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = blockIdx.x * 64;
  const int orow0 = blockIdx.y * 16;            // first output row (of G * R)
  const int g = orow0 / R;
  const int m_begin = blockIdx.z * mchunk, m_end = min(M, m_begin + mchunk);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int m0 = m_begin; m0 < m_end; m0 += 32) {
    if (tid < 64) {
      const int r = tid >> 1, h = tid & 1;
      bf16x8 v = zero8();
      if (m0 + r < m_end) v = *(const bf16x8*)(A + (long long)(m0 + r) * lda + orow0 + 8 * h);
      *(bf16x8*)&sa[r][8 * h] = v;
    }
    {
      const int r = tid >> 3, q = tid & 7, c = c0 + 8 * q;
      bf16x8 v = zero8();
      if (m0 + r < m_end && c < Ng) {
        v = *(const bf16x8*)(Bm + (long long)(m0 + r) * ldb + (long long)g * bg + c);
        if (s != 1.0f) v = scale8(v, s);
      }
      *(bf16x8*)&sb[r][8 * q] = v;
    }
    __syncthreads();
    bf16x8 af, bfr;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      af[j] = sa[8 * (lane >> 4) + j][lane & 15];
      bfr[j] = sb[8 * (lane >> 4) + j][16 * wave + (lane & 15)];
    }
    acc = mfma16(af, bfr, acc);
    __syncthreads();
  }
  const int c = c0 + 16 * wave + (lane & 15);
  if (c >= Ng) return;
  const int GR = G * R;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int orow = orow0 + 4 * (lane >> 4) + i;
    if (part != nullptr) {
      part[((long long)blockIdx.z * GR + orow) * Ng + c] = acc[i];
    } else {
      for (int n = 0; n < ncopy; ++n) {
        const long long o = ((long long)n * GR + orow) * ldo + c;
        if (out_f32) ((float*)out)[o] = acc[i];
        else ((bf16*)out)[o] = f2bf(acc[i]);
      }
    }
  }
}

__global__ __launch_bounds__(256) void lora_wgrad_reduce_kernel(const float* __restrict__ part, int S, void* __restrict__ out, int ldo,
                                                                int ncopy, int out_f32, int rows, int Ng) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long n_el = (long long)rows * Ng;
  if (idx >= n_el) return;
  float v = 0.f;
  for (int z = 0; z < S; ++z) v += part[(long long)z * n_el + idx];
  const int r = (int)(idx / Ng), c = (int)(idx - (long long)r * Ng);
  for (int n = 0; n < ncopy; ++n) {
    const long long o = ((long long)n * rows + r) * ldo + c;
    if (out_f32) ((float*)out)[o] = v;
    else ((bf16*)out)[o] = f2bf(v);
  }
}

// A thread: 4 consecutive input columns of one output row; blockIdx.y = output row.
__global__ __launch_bounds__(256) void lora_merge_kernel(const float* __restrict__ W, int ldw, const float* __restrict__ A, int lda,
                                                         const float* __restrict__ Bm, int ldb, int nsum, bf16* __restrict__ out, int ldo,
                                                         int I, int Ng, int G, int R, float s) {
  const int o = blockIdx.y;
  const int i = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= I) return;
  const int g = o / Ng, c = o - g * Ng;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int n = 0; n < nsum; ++n) {
    for (int j = 0; j < R; ++j) {
      const float b = Bm[((long long)(n * G + g) * R + j) * ldb + c];
      const f32x4 a = *(const f32x4*)(A + (long long)(g * R + j) * lda + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(b, a[e], acc[e]);
    }
  }
  const f32x4 w = *(const f32x4*)(W + (long long)o * ldw + i);
  bf16x4 y;
#pragma unroll
  for (int e = 0; e < 4; ++e) y[e] = f2bf(w[e] + s * acc[e]);
  *(bf16x4*)(out + (long long)o * ldo + i) = y;
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool al8(const void* p) { return ((uintptr_t)p & 7) == 0; }

}  // namespace

extern "C" int lap_lora_down(const void* X, int ldx, int xg, const void* W, int ldw, int nsum, void* T, int ldt, int M, int K, int G,
                             int R, float s, void* stream) {
  if (!X || !W || !T || M <= 0 || K <= 0 || G <= 0 || R <= 0 || nsum <= 0 || (R & 15) || (K & 7) || (ldx & 7) || (xg & 7) ||
      (ldw & 7) || ldx < (long long)(G - 1) * xg + K || ldw < K || ldt < G * R || !al16(X) || !al16(W))
    return LAP_ERR_ARG;
  const int nchunk = (R + 63) / 64;
  hipLaunchKernelGGL(lora_down_kernel, dim3((M + 63) / 64, G * nchunk), dim3(256), 0, S_, (const bf16*)X, ldx, xg, (const bf16*)W, ldw,
                     nsum, (bf16*)T, ldt, M, K, G, R, s, nchunk);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

extern "C" int lap_lora_up_add(const void* T, int ldt, const void* B, int ldb, int nsum, void* Y, int ldy, int M, int Ng, int G, int R,
                               float s, void* stream) {
  if (!T || !B || !Y || M <= 0 || Ng <= 0 || G <= 0 || R <= 0 || nsum <= 0 || (Ng & 7) || (ldb & 7) || (ldy & 7) || ldb < Ng ||
      ldy < G * Ng || ldt < G * R || !al16(B) || !al16(Y))
    return LAP_ERR_ARG;
  const long long chunks = (long long)G * Ng / 8;
  hipLaunchKernelGGL(lora_up_add_kernel, dim3((unsigned)((chunks + 63) / 64), (M + 15) / 16), dim3(256), 0, S_, (const bf16*)T, ldt,
                     (const bf16*)B, ldb, nsum, (bf16*)Y, ldy, M, Ng, G, R, s);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

extern "C" int lap_lora_wgrad(const void* A, int lda, const void* B, int ldb, int bg, void* out, int ldo, int ncopy, int out_f32,
                              int M, int Ng, int G, int R, float s, int msplit, float* scratch, long long scratch_floats, void* stream) {
  if (!A || !B || !out || M <= 0 || Ng <= 0 || G <= 0 || R <= 0 || ncopy <= 0 || msplit <= 0 || (R & 15) || (Ng & 7) || (lda & 7) ||
      (ldb & 7) || (bg & 7) || lda < G * R || ldb < (long long)(G - 1) * bg + Ng || ldo < Ng || !al16(A) || !al16(B))
    return LAP_ERR_ARG;
  const int GR = G * R;
  int mchunk = (M + msplit - 1) / msplit;
  mchunk = (mchunk + 31) & ~31;
  const int S = (M + mchunk - 1) / mchunk;
  float* part = nullptr;
  if (S > 1) {
    if (!scratch || scratch_floats < (long long)S * GR * Ng) return LAP_ERR_ARG;
    part = scratch;
  }
  hipLaunchKernelGGL(lora_wgrad_kernel, dim3((Ng + 63) / 64, GR / 16, S), dim3(256), 0, S_, (const bf16*)A, lda, (const bf16*)B, ldb, bg,
                     out, ldo, ncopy, out_f32, part, M, Ng, G, R, s, mchunk);
  LAP_CHECK_LAUNCH();
  if (S > 1) {
    const long long n_el = (long long)GR * Ng;
    hipLaunchKernelGGL(lora_wgrad_reduce_kernel, dim3((unsigned)((n_el + 255) / 256)), dim3(256), 0, S_, (const float*)part, S, out, ldo,
                       ncopy, out_f32, GR, Ng);
    LAP_CHECK_LAUNCH();
  }
  return LAP_OK;
}

extern "C" int lap_lora_merge(const float* W, int ldw, const float* A, int lda, const float* B, int ldb, int nsum, void* out, int ldo, int I,
                              int Ng, int G, int R, float s, void* stream) {
  if (!W || !A || !B || !out || I <= 0 || Ng <= 0 || G <= 0 || R <= 0 || nsum <= 0 || (I & 3) || (ldw & 3) || (lda & 3) || (ldo & 3) ||
      ldw < I || lda < I || ldo < I || ldb < Ng || !al16(W) || !al16(A) || !al8(out))
    return LAP_ERR_ARG;
  hipLaunchKernelGGL(lora_merge_kernel, dim3((I / 4 + 255) / 256, G * Ng), dim3(256), 0, S_, W, ldw, A, lda, B, ldb, nsum, (bf16*)out,
                     ldo, I, Ng, G, R, s);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}
