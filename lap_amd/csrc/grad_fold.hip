// Gradient accumulation (TrainConfig.grad_accum_steps > 1): the weight gradient of one micro-step, as its backward left it
// (bf16 for the GEMM-weight units, f32 for the embedding table: ParamStore.grad_dtype), folded into the unit's f32 accumulator.
// The last fold of an optimizer step also adds the sum of squares of the values it stores to the global gradient norm, so the
// accumulated gradient is not read a second time.  HBM-bound: 2 (or 4) bytes read, 4 read (not on the first fold), 4 written
// per parameter.
#include <cstdint>
#include "common.hpp"
#include "../../include/lap_hip.h"

namespace {

// One 16-byte gradient load per lane and iteration (8 bf16 / 4 f32 values) against 32 / 16 bytes of the accumulator; a wave
// sweeps 1 KiB of the gradient and 2 KiB / 1 KiB of the accumulator contiguously.  Like the optimizer pass (loss_optim.hip:
// adamw_ema_kernel) it runs on the side stream beside the assembly GEMM: at most one 256-thread block per CU, 32 VGPRs, a
// grid-stride loop, nontemporal accesses (every byte is touched once per micro-step), no LDS but the block reduction's.
//
// Ranges are cut anywhere by a freeze filter, so only the element alignment of the two pointers is assumed.  The host picks `head`
// (lap_grad_fold): the elements in front of the GRADIENT's first 16-byte boundary (0 .. 7 bf16, 0 .. 3 f32) where the accumulator is
// 16-byte aligned behind them too — always, where both buffers are 16-byte aligned at one element offset — and the body then takes
// vector loads on both (GAL); else the 0 .. 3 elements that align the accumulator alone, and the gradient's values are loaded one by
// one.  `tail` (< E) is what is left behind the last whole group.  Block 0 handles head and tail, one element per lane.
template <bool G16, bool GAL>
__global__ __launch_bounds__(256) void grad_fold_kernel(float* __restrict__ acc, const void* __restrict__ g, long long n, int head_, int first,
                                                        float* __restrict__ sumsq) {
  constexpr int E = G16 ? 8 : 4;
  __shared__ float red[4];
  const bf16* g16 = reinterpret_cast<const bf16*>(g);
  const float* g32 = reinterpret_cast<const float*>(g);
  const long long head = head_;      // <= n (host)
  const bool want_sq = sumsq != nullptr;      // (uniform)
  const long long groups = (n - head) / E;
  const long long tail0 = head + groups * E;
  float sq = 0.f;
  auto one = [&](long long j) {     // element j alone (head / tail)
    const float gv = G16 ? (float)g16[j] : g32[j];
    const float v = first ? gv : acc[j] + gv;
    acc[j] = v;
    if (want_sq) sq += v * v;
  };
  if (blockIdx.x == 0) {
    if ((long long)threadIdx.x < head) one(threadIdx.x);
    const long long t = (long long)threadIdx.x - 32;
    if (t >= 0 && tail0 + t < n) one(tail0 + t);
  }
  const long long stride = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < groups; i += stride) {
    const long long j = head + i * E;
    float gv[E];
    if constexpr (G16) {
      if constexpr (GAL) {
        const bf16x8 q = __builtin_nontemporal_load(reinterpret_cast<const bf16x8*>(g16 + j));
#pragma unroll
        for (int e = 0; e < E; ++e) gv[e] = (float)q[e];
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) gv[e] = (float)g16[j + e];
      }
    } else {
      if constexpr (GAL) {
        const f32x4 q = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g32 + j));
#pragma unroll
        for (int e = 0; e < E; ++e) gv[e] = q[e];
      } else {
#pragma unroll
        for (int e = 0; e < E; ++e) gv[e] = g32[j + e];
      }
    }
    f32x4* a4 = reinterpret_cast<f32x4*>(acc + j);
#pragma unroll
    for (int h = 0; h < E / 4; ++h) {
      f32x4 v;
      if (first) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = gv[4 * h + e];
      } else {
        v = __builtin_nontemporal_load(a4 + h);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += gv[4 * h + e];
      }
      __builtin_nontemporal_store(v, a4 + h);
      if (want_sq) sq += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
  }
  if (want_sq) {     // (the whole block takes the reduction or none of it does)
    const float s = block_sum<4>(sq, red);
    if (threadIdx.x == 0) atomicAdd(sumsq, s);
  }
}

}  // namespace

#define S_ ((hipStream_t)stream)

extern "C" int lap_grad_fold(float* acc, const void* g, int g_is_bf16, long long n, int first, float* sumsq, void* stream) {
  if (n <= 0 || !acc || !g || ((uintptr_t)acc & 3) || ((uintptr_t)g & (g_is_bf16 ? 1 : 3)) || (sumsq && ((uintptr_t)sumsq & 3)))
    return LAP_ERR_ARG;
  // one block per CU at the most (see adamw_launch in loss_optim.hip: a second 32-register wave per SIMD does not fit beside the
  // assembly GEMM's); the count is kept per device
  static long long cap_of[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  long long cap = __atomic_load_n(&cap_of[dev], __ATOMIC_RELAXED);
  if (cap == 0) {
    int cus = 256;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    cap = cus;
    __atomic_store_n(&cap_of[dev], cap, __ATOMIC_RELAXED);
  }
  const int E = g_is_bf16 ? 8 : 4, gsize = g_is_bf16 ? 2 : 4;
  long long head = (long long)(((16u - (unsigned)((uintptr_t)g & 15u)) & 15u) / gsize);      // to the gradient's 16-byte boundary
  bool gal = (((uintptr_t)acc + 4u * (uintptr_t)head) & 15) == 0;
  if (!gal) head = (long long)(((16u - (unsigned)((uintptr_t)acc & 15u)) & 15u) >> 2);       // the accumulator's alone
  if (head > n) head = n;
  const long long groups = (n - head) / E;
  long long blocks = (groups + 255) / 256;
  blocks = blocks < 1 ? 1 : blocks > cap ? cap : blocks;
#define FOLD_GO(G16_, GAL_) hipLaunchKernelGGL((grad_fold_kernel<G16_, GAL_>), dim3((unsigned)blocks), dim3(256), 0, S_, acc, g, n, (int)head, first, sumsq)
  if (g_is_bf16) { if (gal) FOLD_GO(true, true); else FOLD_GO(true, false); }
  else { if (gal) FOLD_GO(false, true); else FOLD_GO(false, false); }
#undef FOLD_GO
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}
