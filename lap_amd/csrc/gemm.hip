// bf16 MFMA GEMM for gfx950 with fused epilogues — the dominant kernel of the
// LAP-3B train step (K8/K11/K12/K13 of SURVEY.md §2.2: QKV / out-proj / GeGLU
// FFN / LM-head projections, their dgrad and wgrad).
//
//   C[M,N] = epilogue( alpha * sum_k opA(m,k) * opB(k,n) )
//
// Operand layouts (chosen per call, no data is ever transposed in HBM):
//   a_kc = 1 : A stored [M][K]  (k contiguous),  element (m,k) = A[m*lda + k]
//   a_kc = 0 : A stored [K][M]  (m contiguous),  element (m,k) = A[k*lda + m]
//   b_kc = 1 : B stored [N][K]  (k contiguous),  element (k,n) = B[n*ldb + k]
//   b_kc = 0 : B stored [K][N]  (n contiguous),  element (k,n) = B[k*ldb + n]
// With weights kept as Wt[out][in]:
//   forward  y = x . Wt^T        -> a_kc=1, b_kc=1
//   dgrad    dx = dy . Wt        -> a_kc=1, b_kc=0
//   wgrad    dWt = dy^T . x      -> a_kc=0, b_kc=0
//
// What is in this file (the tile numbers are lap_gemm_bf16_ex's; csrc/gemm_route.hpp chooses among them):
//   gemm_kernel     the generic BM x BN x BK kernel, WGM x WGN waves, each wave a (BM/WGM) x (BN/WGN) sub-tile of
//                   v_mfma_f32_16x16x32_bf16 fragments, all waves in lockstep, one barrier per k-tile:
//                     tile 5   256x256x64 / 16 waves, one block per CU (128 KiB LDS): ragged K (K % 8 != 0);
//                     tile 2   256x256x64 /  8 waves, direct epilogue: what the bitwise tests compare against;
//                     tile 6   128x128x64 /  8 waves, two blocks per CU: small or awkward shapes, short-K tails, and the quadrants
//                              of a 256x256 grid's last round (sub256); tile 0: the same with 4 waves (a 128x128 tile at the
//                              2.5 PF MFMA peak would need 39 TB/s from L2, more than the ~35 TB/s the XCD L2s deliver);
//                     tiles 15-19  the serving prefill's shapes (forward layout): 320x256 (15: with the GeGLU epilogue), 64x128,
//                              64x64, 128x64, 320x128;
//   gemm_sp_kernel  tile 10: the software-pipelined 8-wave 256x256 kernel, the forward layout's large GEMMs;
//   gemm_pq_kernel  tile 12: the ping-pong 8-wave 256x256 kernel, as soon as an operand is M-contiguous;
//   splitk_reduce_kernel / splitk_tail_reduce_kernel  the second phase of both two-phase split-K forms: slabs [ksplit][M][N] of a
//                   whole product, or compact slabs [ksplit][tiles][256][256] of the tail tiles of a 256x256 grid whose full rounds
//                   ran unsplit.  Without scratch, split-K is f32 atomics onto C (store_tile4).
// The probes (tiles 8, 9, 13) live in gemm_probes.hpp and, like the probe instantiations 1, 3, 4, 7, 11 and the ablation bits of
// lap_gemm_set_debug, are compiled in a LAP_GEMM_EXPERIMENTAL build only.
// HBM -> LDS staging is buffer_load_dwordx4 ... lds (LDS-DMA, no VGPR round trip), at least double buffered.  The LDS image is
// lane-linear per wave instruction, so the bank-conflict swizzle is applied to the per-lane *source* address and again on the
// fragment read (common.hpp).  Out-of-range rows / k-tails use an out-of-bounds buffer
// offset, for which the hardware writes zeros.  Epilogue arithmetic, final store and the 256x256 launcher: gemm_common.hpp.
#include "common.hpp"
#include "gemm_common.hpp"
#include "gemm_route.hpp"

namespace {

// BK: k-depth of one LDS stage (32 or 64); NS: LDS stages.  Loads of tile t+NS-1 are issued while tile t is
// multiplied; the wait before the (single, raw) barrier is a COUNTED vmcnt that leaves NS-2 tiles in flight.
template <int BM, int BN, int WGM, int WGN, int BK, int NS, bool A_KC, bool B_KC, bool OUT_F32>
__global__ __launch_bounds__(WGM* WGN * 64) void gemm_kernel(GemmParams p) {
  constexpr int NW = WGM * WGN;
  constexpr int WTM = BM / WGM, WTN = BN / WGN;   // wave tile
  constexpr int FM = WTM / 16, FN = WTN / 16;     // fragments per wave
  constexpr int KSUB = BK / 32;
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2, STAGE = A_BYTES + B_BYTES;
  constexpr int PA = A_BYTES / 1024 / NW, PB = B_BYTES / 1024 / NW;  // 1 KiB LDS-DMA pieces per wave
  static_assert(A_BYTES % (1024 * NW) == 0 && B_BYTES % (1024 * NW) == 0, "tile / wave mismatch");
  extern __shared__ __attribute__((aligned(16))) char smem[];   // NS stages: [A tile | B tile]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w / WGN, wn = w % WGN;

  // Block -> tile mapping: XCD-aware remap, then groups of GM m-tiles sweep n.
  constexpr int GM = (BM == 256) ? 4 : 8;
  int tm, tn;
  if (BM == 128 && BN == 128 && p.sub256) {
    // last round of a 256x256 grid re-tiled: 4 consecutive blocks (same XCD) are the quadrants of one 256x256 tile
    const int b = xcd_remap(blockIdx.x, gridDim.x);
    tile_coords<4>(p, p.tile_base + (b >> 2), tm, tn);   // (p.tiles_m / tiles_n describe the 256x256 grid here)
    tm = 2 * tm + ((b >> 1) & 1);
    tn = 2 * tn + (b & 1);
    if (tm * BM >= p.M || tn * BN >= p.N) return;   // quadrant outside the matrix (uniform per block)
  } else {
    tile_coords<GM>(p, p.tile_base + xcd_remap(blockIdx.x, gridDim.x), tm, tn);
  }
  const int m0 = tm * BM, n0 = tn * BN;

  auto rsA = operand_rsrc(p.A, A_KC ? p.M : p.K, p.lda);
  auto rsB = operand_rsrc(p.B, B_KC ? p.N : p.K, p.ldb);

  // Staging descriptors.  Piece q covers linear 16-byte chunks [64q, 64q+64) of the tile image;
  // K-contiguous tile: 8 chunks per row (row = m/n index); M-contiguous tile: BM/8 chunks per k-row.
  unsigned offA[PA], offB[PB];
  int kidxA[PA], kidxB[PB];
#pragma unroll
  for (int j = 0; j < PA; ++j) {
    const int ci = (w * PA + j) * 64 + lane;
    if (A_KC) {
      const int row = BK == 64 ? ci >> 3 : ci >> 2, pc = BK == 64 ? ci & 7 : ci & 3;
      const int c = BK == 64 ? pc ^ ((row >> 1) & 7) : pc ^ ((-(row >> 2)) & 3);
      kidxA[j] = c * 8;
      offA[j] = (m0 + row < p.M) ? (unsigned)(((long long)(m0 + row) * p.lda + c * 8) * 2) : OOB;
    } else {
      constexpr int CPR = BM / 8;
      const int kr = ci / CPR, pc = ci % CPR;
      const int c = pc ^ (mc_swz(kr) << 1);
      kidxA[j] = kr;
      offA[j] = (m0 + c * 8 < p.M) ? (unsigned)(((long long)kr * p.lda + m0 + c * 8) * 2) : OOB;
    }
  }
#pragma unroll
  for (int j = 0; j < PB; ++j) {
    const int ci = (w * PB + j) * 64 + lane;
    if (B_KC) {
      const int row = BK == 64 ? ci >> 3 : ci >> 2, pc = BK == 64 ? ci & 7 : ci & 3;
      const int c = BK == 64 ? pc ^ ((row >> 1) & 7) : pc ^ ((-(row >> 2)) & 3);
      kidxB[j] = c * 8;
      int brow = n0 + row;
      if constexpr (BM == 320 && BN == 256 && !OUT_F32) {
        // GeGLU pairing: wave column group wn (64 tile columns) = 32 gate columns + the 32 up columns of the same features
        if (p.geglu) brow = ((row & 63) < 32 ? 0 : p.N / 2) + tn * 128 + (row >> 6) * 32 + (row & 31);
      }
      offB[j] = (brow < p.N) ? (unsigned)(((long long)brow * p.ldb + c * 8) * 2) : OOB;
    } else {
      constexpr int CPR = BN / 8;
      const int kr = ci / CPR, pc = ci % CPR;
      const int c = pc ^ (mc_swz(kr) << 1);
      kidxB[j] = kr;
      offB[j] = (n0 + c * 8 < p.N) ? (unsigned)(((long long)kr * p.ldb + n0 + c * 8) * 2) : OOB;
    }
  }
  const int kt0_probe = blockIdx.y * p.ktiles_per_split + NS - 1;
  unsigned stepA = A_KC ? (unsigned)(BK * 2) : (unsigned)((long long)BK * p.lda * 2);
  unsigned stepB = B_KC ? (unsigned)(BK * 2) : (unsigned)((long long)BK * p.ldb * 2);
#ifdef LAP_GEMM_EXPERIMENTAL
  // timing probe (results wrong): operand tiles fetched as if the operand were stored tile by tile, 1 KiB contiguous per LDS-DMA
  // piece (dbg bit 8: B, bit 16: A) instead of 8 rows x 128 bytes — what a fragment-packed operand image would cost the loop
  {
    const int nkt = (p.K + BK - 1) / BK;
    if (p.dbg & 8) {
#pragma unroll
      for (int j = 0; j < PB; ++j) { offB[j] = (unsigned)(((long long)tn * nkt) * B_BYTES + (w * PB + j) * 1024 + lane * 16); kidxB[j] = 0; }
      stepB = B_BYTES;
    }
    if (p.dbg & 16) {
#pragma unroll
      for (int j = 0; j < PA; ++j) { offA[j] = (unsigned)(((long long)tm * nkt) * A_BYTES + (w * PA + j) * 1024 + lane * 16); kidxA[j] = 0; }
      stepA = A_BYTES;
    }
  }
#endif

  // K a multiple of the k-tile (every production shape): no piece ever reaches past K, so a piece's per-lane offset is the
  // loop-invariant offA / offB (OOB for rows outside the matrix: 0x80000000 is out of range whatever is added) and the k-tile's
  // byte offset travels in the instruction's SCALAR offset — no per-piece compare / select / add in the loop (round 5: the
  // small-tile loops issue ~100 instructions per k-step around 8 - 16 MFMAs; the selects and their exec-mask branches were 40).
  const bool k_even = (p.K % BK) == 0;
#ifdef LAP_GEMM_EXPERIMENTAL
  const bool probe_no_dma = p.dbg & 32, probe_no_mma = p.dbg & 64;   // timing ablations of the k-loop (results wrong)
#else
  constexpr bool probe_no_dma = false, probe_no_mma = false;
#endif
  auto stage = [&](int buf, int kt) {
    const int k0 = kt * BK;
    char* base = smem + buf * STAGE;
    if (probe_no_dma && kt >= kt0_probe) return;
    if (k_even) {
      const unsigned sa = (unsigned)kt * stepA, sb = (unsigned)kt * stepB;
#pragma unroll
      for (int j = 0; j < PA; ++j) {
        const unsigned va = offA[j];
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (LDS_PTR(void))(base + (w * PA + j) * 1024), 16, va, sa, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < PB; ++j) {
        const unsigned vb = offB[j];
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (LDS_PTR(void))(base + A_BYTES + (w * PB + j) * 1024), 16, vb, sb, 0, 0);
      }
    } else {
#pragma unroll
      for (int j = 0; j < PA; ++j) {
        unsigned va = (offA[j] != OOB && k0 + kidxA[j] < p.K) ? offA[j] + (unsigned)kt * stepA : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (LDS_PTR(void))(base + (w * PA + j) * 1024), 16, va, 0, 0, 0);
      }
#pragma unroll
      for (int j = 0; j < PB; ++j) {
        unsigned vb = (offB[j] != OOB && k0 + kidxB[j] < p.K) ? offB[j] + (unsigned)kt * stepB : OOB;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (LDS_PTR(void))(base + A_BYTES + (w * PB + j) * 1024), 16, vb, 0, 0, 0);
      }
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nkt_all = (p.K + BK - 1) / BK;
  const int kt0 = blockIdx.y * p.ktiles_per_split;
  const int kt1 = min(nkt_all, kt0 + p.ktiles_per_split);
#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (kt0 + s < kt1) stage(s, kt0 + s);
  int cur = 0;
  for (int kt = kt0; kt < kt1; ++kt) {
    // my loads of tile kt have landed (NS-2 younger tiles may still be in flight) ...
    if (NS > 2 && kt + NS - 2 < kt1) wait_vmcnt<(NS - 2) * (PA + PB)>(); else wait_vmcnt<0>();
    // ... and so have everybody else's; every wave is also done reading the buffer refilled below.
    __builtin_amdgcn_s_barrier();
    if (kt + NS - 1 < kt1) stage(cur == 0 ? NS - 1 : cur - 1, kt + NS - 1);
    const char* tA = smem + cur * STAGE;
    const char* tB = tA + A_BYTES;
#pragma unroll
    for (int kk = 0; kk < KSUB; ++kk) {
      bf16x8 fa[FM], fb[FN];
      // M-contiguous operands: transposing reads issued raw (the builtin makes the compiler drain the LDS-DMA
      // prefetch of the next tile first, see common.hpp), fenced once per k-step
      bf16x4 ta[A_KC ? 1 : FM][2], tb[B_KC ? 1 : FN][2];
      if (!A_KC) {
#pragma unroll
        for (int i = 0; i < FM; ++i) mc_frag_raw<BM>(tA, wm * WTM + i * 16, kk, lane, ta[i]);
      }
      if (!B_KC) {
#pragma unroll
        for (int j = 0; j < FN; ++j) mc_frag_raw<BN>(tB, wn * WTN + j * 16, kk, lane, tb[j]);
      }
      constexpr bool RAW_KC = BK == 64;   // K-contiguous operands through raw b128 reads as well (+1-3 %)
      if (A_KC) {
#pragma unroll
        for (int i = 0; i < FM; ++i)
          fa[i] = RAW_KC ? kc_frag_raw(tA, wm * WTM + i * 16, kk, lane) : kc32_frag(tA, wm * WTM + i * 16, lane);
      }
      if (B_KC) {
#pragma unroll
        for (int j = 0; j < FN; ++j)
          fb[j] = RAW_KC ? kc_frag_raw(tB, wn * WTN + j * 16, kk, lane) : kc32_frag(tB, wn * WTN + j * 16, lane);
      }
      if (RAW_KC || !A_KC || !B_KC) {
        lds_wait_all();
#pragma unroll
        for (int i = 0; i < FM; ++i) {
          if (!A_KC) { lds_tie(ta[i][0]); lds_tie(ta[i][1]); fa[i] = join8(ta[i][0], ta[i][1]); }
          else if (RAW_KC) lds_tie(fa[i]);
        }
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          if (!B_KC) { lds_tie(tb[j][0]); lds_tie(tb[j][1]); fb[j] = join8(tb[j][0], tb[j][1]); }
          else if (RAW_KC) lds_tie(fb[j]);
        }
      }
      if (!probe_no_mma) {
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          // Operands swapped on purpose: D[row = n][col = m], so each lane ends up
          // with 4 consecutive n of one output row m -> one 8/16-byte store.
          acc[i][j] = mfma16(fb[j], fa[i], acc[i][j]);
      }
    }
    cur = (cur + 1 == NS) ? 0 : cur + 1;
  }

  // Epilogue. Lane holds C[m][n..n+3], m = .. + (lane&15), n = .. + 4*(lane>>4).
  const int li = lane & 15, lg = lane >> 4;
  if constexpr (BM == 256 && BN == 256 && NW == 16) {
    if (p.epi_lds) { staged_epilogue<NW, WTM, WTN, OUT_F32>(p, smem, acc, wm, wn, m0, n0, tid, lane); return; }
  }
  if constexpr (BM == 320 && BN == 256 && !OUT_F32) {
    if (p.geglu) {   // fragments j = 0, 1: gate columns; j = 2, 3: the up columns of the same features (csrc/elementwise.hip geglu_fwd's bits)
      static_assert(FN == 4, "GeGLU pairing assumes 64-column wave tiles");
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const int m = m0 + wm * WTM + i * 16 + li;
        if (m >= p.M) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int gc = tn * 128 + wn * 32 + j * 16 + 4 * lg;
          bf16x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float gt = round_bf16(acc[i][j][e]);
            // geglu 2: the GELU of lap_gemm_asm_geglu_fwd (the training step's kernel: v_exp / v_rcp), 80 of them per lane are 10 us of tanhf otherwise
            o[e] = f2bf(round_bf16(p.geglu == 2 ? gelu_exp2_f(gt) : gelu_tanh_f(gt)) * round_bf16(acc[i][j + 2][e]));
          }
          *reinterpret_cast<bf16x4*>((bf16*)p.C + (long long)m * p.ldc + gc) = o;
        }
      }
      return;
    }
  }
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = m0 + wm * WTM + i * 16 + li;
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = n0 + wn * WTN + j * 16 + 4 * lg;
      if (n >= p.N) continue;
      store_tile4<OUT_F32>(p, m, n, acc[i][j]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Software-pipelined 8-wave kernel (tile 10): 256x256x64 tile, 128x64 per wave, TWO fragment register sets.  Per k-tile
//   A1  set 0 = (kt, k-half 0) is back: 8 MFMAs, issue the raw reads of (kt, k-half 1) into set 1, 8 more MFMAs
//   A2  set 1 landed, my LDS-DMA of tile kt+1 landed, barrier          (every read of tile kt has completed)
//   A3  last 16 MFMAs on set 0, with the 8 LDS-DMA pieces of tile kt+2 threaded between them (into kt's buffer)
//   C   8 MFMAs on set 1 = (kt, k-half 1), issue the raw reads of (kt+1, k-half 0) into set 0, the other 24 MFMAs
// (reads are always issued AFTER a first group of MFMAs has been queued: +1 ms per train step over issuing them first)
// so that after the barrier every wave already holds 48 MFMAs of work whose operands are in registers: the next reads'
// latency, the DMA issue cost and the barrier skew hide under them instead of idling the matrix pipe (the lockstep
// kernel's bubble).  One barrier per k-tile, two LDS buffers, prefetch distance one k-tile.  K % 64 == 0.
template <int OFF>
__device__ __forceinline__ bf16x8 ds_read_b128_raw(unsigned addr) {   // valid after lds_wait_*() + lds_tie(), like kc_frag_raw
  bf16x8 r;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(r) : "v"(addr), "n"(OFF));
  return r;
}

template <int WGM, int WGN, bool A_KC, bool B_KC, bool OUT_F32, bool TWOB = false>
__global__ __launch_bounds__(WGM* WGN * 64) void gemm_sp_kernel(GemmParams p) {
  constexpr int BM = 256, BN = 256, BK = 64, A_BYTES = BM * BK * 2, STAGE = 2 * A_BYTES;
  constexpr int NW = WGM * WGN, WTM = BM / WGM, WTN = BN / WGN, FM = WTM / 16, FN = WTN / 16, PC = 32 / NW;   // PC pieces / operand / wave
  static_assert(FM == 8 && (FN == 4 || FN == 8), "wave tile 128 x 64 or 128 x 128");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w / WGN, wn = w % WGN;
  int tm, tn;
  tile_coords<4>(p, p.tile_base + xcd_remap(blockIdx.x, gridDim.x), tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  auto rsA = operand_rsrc(p.A, A_KC ? p.M : p.K, p.lda);
  auto rsB = operand_rsrc(p.B, B_KC ? p.N : p.K, p.ldb);
  unsigned offA[PC], offB[PC];
  int kcA[PC], kcB[PC];     // K-contiguous operands: first k of the lane's chunk inside a k-tile (K % 64 != 0: chunks past K read as zeros)
#pragma unroll
  for (int j = 0; j < PC; ++j) {
    const int ci = (w * PC + j) * 64 + lane;
    kcA[j] = 0; kcB[j] = 0;
    if (A_KC) {
      const int row = ci >> 3, c = (ci & 7) ^ ((row >> 1) & 7);
      kcA[j] = c * 8;
      offA[j] = (m0 + row < p.M) ? (unsigned)(((long long)(m0 + row) * p.lda + c * 8) * 2) : OOB;
    } else {
      const int kr = ci >> 5, c = (ci & 31) ^ (mc_swz(kr) << 1);
      offA[j] = (m0 + c * 8 < p.M) ? (unsigned)(((long long)kr * p.lda + m0 + c * 8) * 2) : OOB;
    }
    if (B_KC) {
      const int row = ci >> 3, c = (ci & 7) ^ ((row >> 1) & 7);
      kcB[j] = c * 8;
      offB[j] = (n0 + row < p.N) ? (unsigned)(((long long)(n0 + row) * p.ldb + c * 8) * 2) : OOB;
    } else {
      const int kr = ci >> 5, c = (ci & 31) ^ (mc_swz(kr) << 1);
      offB[j] = (n0 + c * 8 < p.N) ? (unsigned)(((long long)kr * p.ldb + n0 + c * 8) * 2) : OOB;
    }
  }
  const unsigned stepA = A_KC ? (unsigned)(BK * 2) : (unsigned)((long long)BK * p.lda * 2);
  const unsigned stepB = B_KC ? (unsigned)(BK * 2) : (unsigned)((long long)BK * p.ldb * 2);
  const int nkt_all = (p.K + BK - 1) / BK;   // (rows of an M- / N-contiguous operand past K lie outside its descriptor: zeros)
  const int kt0 = blockIdx.y * p.ktiles_per_split;
  const int kt1 = min(nkt_all, kt0 + p.ktiles_per_split);
  auto piece = [&](int buf, int kt, int j) {   // j < 4: operand A, else B; past the end: zero fill, keeps the counts uniform
    char* base = smem + buf * STAGE;
    if (j < PC) {
      const unsigned v = (offA[j] != OOB && kt < kt1 && (!A_KC || kt * BK + kcA[j] < p.K)) ? offA[j] + (unsigned)kt * stepA : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (LDS_PTR(void))(base + (w * PC + j) * 1024), 16, v, 0, 0, 0);
    } else {
      const unsigned v = (offB[j - PC] != OOB && kt < kt1 && (!B_KC || kt * BK + kcB[j - PC] < p.K)) ? offB[j - PC] + (unsigned)kt * stepB : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (LDS_PTR(void))(base + A_BYTES + (w * PC + j - PC) * 1024), 16, v, 0, 0, 0);
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 fa[2][FM], fb[2][FN];
  bf16x4 ra[A_KC ? 1 : 2][A_KC ? 1 : FM][2], rb[B_KC ? 1 : 2][B_KC ? 1 : FN][2];
  // K-contiguous fragments of one operand differ by 16 rows = 2048 bytes and share the swizzle ((row >> 1) & 7 does not
  // see multiples of 16): one address register + immediate offsets instead of one register per read
  auto reads = [&](int set, const char* tA, int kk) {
    const char* tB = tA + A_BYTES;
    if (B_KC) {
      const unsigned b0 = lds_addr_of(tB) + kc_tile_off(wn * WTN + (lane & 15), kk * 4 + (lane >> 4));
      fb[set][0] = ds_read_b128_raw<0>(b0); fb[set][1] = ds_read_b128_raw<2048>(b0);
      fb[set][2] = ds_read_b128_raw<4096>(b0); fb[set][3] = ds_read_b128_raw<6144>(b0);
      if constexpr (FN == 8) {
        fb[set][4] = ds_read_b128_raw<8192>(b0); fb[set][5] = ds_read_b128_raw<10240>(b0);
        fb[set][6] = ds_read_b128_raw<12288>(b0); fb[set][7] = ds_read_b128_raw<14336>(b0);
      }
    } else {
#pragma unroll
      for (int j = 0; j < FN; ++j) mc_frag_raw<BN>(tB, wn * WTN + j * 16, kk, lane, rb[B_KC ? 0 : set][B_KC ? 0 : j]);
    }
    if (A_KC) {
      const unsigned a0 = lds_addr_of(tA) + kc_tile_off(wm * WTM + (lane & 15), kk * 4 + (lane >> 4));
      fa[set][0] = ds_read_b128_raw<0>(a0); fa[set][1] = ds_read_b128_raw<2048>(a0);
      fa[set][2] = ds_read_b128_raw<4096>(a0); fa[set][3] = ds_read_b128_raw<6144>(a0);
      fa[set][4] = ds_read_b128_raw<8192>(a0); fa[set][5] = ds_read_b128_raw<10240>(a0);
      fa[set][6] = ds_read_b128_raw<12288>(a0); fa[set][7] = ds_read_b128_raw<14336>(a0);
    } else {
#pragma unroll
      for (int i = 0; i < FM; ++i) mc_frag_raw<BM>(tA, wm * WTM + i * 16, kk, lane, ra[A_KC ? 0 : set][A_KC ? 0 : i]);
    }
  };
  auto tie = [&](int set) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      if (B_KC) lds_tie(fb[set][j]);
      else { lds_tie(rb[B_KC ? 0 : set][B_KC ? 0 : j][0]); lds_tie(rb[B_KC ? 0 : set][B_KC ? 0 : j][1]);
             fb[set][j] = join8(rb[B_KC ? 0 : set][B_KC ? 0 : j][0], rb[B_KC ? 0 : set][B_KC ? 0 : j][1]); }
    }
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      if (A_KC) lds_tie(fa[set][i]);
      else { lds_tie(ra[A_KC ? 0 : set][A_KC ? 0 : i][0]); lds_tie(ra[A_KC ? 0 : set][A_KC ? 0 : i][1]);
             fa[set][i] = join8(ra[A_KC ? 0 : set][A_KC ? 0 : i][0], ra[A_KC ? 0 : set][A_KC ? 0 : i][1]); }
    }
  };
#ifdef LAP_GEMM_EXPERIMENTAL
  const bool no_dma = p.dbg & 1, no_mma = p.dbg & 2;
#define SP_MMA(SET, I0, I1)                                                        \
  if (!no_mma) { _Pragma("unroll") for (int i_ = I0; i_ < I1; ++i_)                \
    _Pragma("unroll") for (int j = 0; j < FN; ++j) acc[i_][j] = mfma16(fb[SET][j], fa[SET][i_], acc[i_][j]); }
#else
  constexpr bool no_dma = false, no_mma = false;
#define SP_MMA(SET, I0, I1)                                                        \
  _Pragma("unroll") for (int i_ = I0; i_ < I1; ++i_)                               \
    _Pragma("unroll") for (int j = 0; j < FN; ++j) acc[i_][j] = mfma16(fb[SET][j], fa[SET][i_], acc[i_][j]);
#endif
#define SP_FENCE() __builtin_amdgcn_sched_barrier(0)

  // prologue: both buffers requested, tile kt0 awaited, its first k-half read
#pragma unroll
  for (int j = 0; j < 2 * PC; ++j) piece(0, kt0, j);
#pragma unroll
  for (int j = 0; j < 2 * PC; ++j) piece(1, kt0 + 1, j);
  wait_vmcnt<2 * PC>();
  __builtin_amdgcn_s_barrier();
  SP_FENCE();
  reads(0, smem, 0);
  for (int kt = kt0; kt < kt1; ++kt) {
    const int cur = (kt - kt0) & 1;
    const char* tA = smem + cur * STAGE;
    // A1
    lds_wait_all();                                          // set 0 (read under the previous tile's last MFMAs) is back
    tie(0);
    SP_MMA(0, 0, 2)
    SP_FENCE();
    reads(1, tA, 1);
    SP_FENCE();
    SP_MMA(0, 2, 4)
    SP_FENCE();
    // A2
    lds_wait_all();
    tie(1);
    if constexpr (!TWOB) wait_vmcnt<0>();   // TWOB: this barrier only says "tile kt is read"; the landing of kt+1 is awaited in C
    SP_FENCE();
    __builtin_amdgcn_s_barrier();
    SP_FENCE();
    // A3: the rest of set 0 with the refill of this tile's buffer (tile kt + 2) threaded through
#pragma unroll
    for (int i = 4; i < 8; ++i) {
      SP_MMA(0, i, i + 1)
      SP_FENCE();
      if (!no_dma) {
#pragma unroll
        for (int q = 0; q < PC / 2; ++q) piece(cur, kt + 2, (PC / 2) * (i - 4) + q);
      }
      SP_FENCE();
    }
    // C
    SP_MMA(1, 0, 2)
    SP_FENCE();
    if constexpr (TWOB) {   // two tiles of LDS-DMA in flight: only the older one (kt + 1) has to have landed here
      wait_vmcnt<2 * PC>();
      SP_FENCE();
      __builtin_amdgcn_s_barrier();
      SP_FENCE();
    }
    reads(0, smem + (cur ^ 1) * STAGE, 0);   // (kt + 1, k-half 0); past the end: harmless reads of a zero-filled buffer
    SP_FENCE();
    SP_MMA(1, 2, 8)
    SP_FENCE();
  }
  wait_vmcnt<0>();
  lds_wait_all();
#undef SP_MMA
#undef SP_FENCE

  if (p.epi_lds) { staged_epilogue<NW, WTM, WTN, OUT_F32>(p, smem, acc, wm, wn, m0, n0, tid, lane); return; }
  const int li = lane & 15, lg = lane >> 4;
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = m0 + wm * WTM + i * 16 + li;
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = n0 + wn * WTN + j * 16 + 4 * lg;
      if (n >= p.N) continue;
      store_tile4<OUT_F32>(p, m, n, acc[i][j]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Ping-pong kernel (tile 12), designed from the round-2 ablation of tile 10: a wave's instruction stream is
// serial (32 MFMAs, then 12 fragment reads + 4 LDS-DMA pieces, per 32-deep k-half), and in tile 10 the two waves of a
// SIMD do the same thing at the same time, so the matrix pipe idles whenever they load.  Here the block's waves form two
// groups (waves 0-3 / 4-7: one wave of each per SIMD) that run every interval in OPPOSITE order:
//     group 0:  barrier | L(j): read k-half j into set j&1, issue the DMA of k-half j+3, wait  | M(j):   32 MFMAs
//     group 1:  barrier | M(j-1): 32 MFMAs on the set read in the previous interval            | L(j)
// so that one wave of each SIMD multiplies while the other loads; ONE barrier per k-half, nothing else synchronises.
// LDS: a ring of FOUR 32 KiB slots, one per k-half (k-half j in slot j & 3; [A 256 x 32 | B 256 x 32], 64-byte rows with
// the kc32 swizzle, or 32 k-rows x 512 B for M-contiguous operands).  Hand-offs: a wave waits for its OWN pieces of k-half
// j (counted vmcnt: the 8 pieces of k-halves j+1, j+2 stay in flight) before barrier j, so after it the k-half is complete;
// both groups have finished reading k-half j-1 before barrier j (group 1's L(j-1) ends interval j-1), so its slot is
// refilled with k-half j+3 during interval j — three intervals (~2 us) ahead of its use instead of tile 10's < 1 k-tile.
template <bool A_KC, bool B_KC, bool OUT_F32>
__global__ __launch_bounds__(512) void gemm_pq_kernel(GemmParams p) {
  constexpr int BM = 256, BN = 256, KH = 32, HALF = BM * KH * 2, SLOT = 2 * HALF, NSLOT = 4;
  constexpr int WGN = 4, NW = 8, WTM = 128, WTN = 64, FM = 8, FN = 4, PC = 2;   // PC: 1 KiB pieces per operand, wave and k-half
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w / WGN, wn = w % WGN;
  const bool g1 = w >= 4;
  int tm, tn;
  tile_coords<4>(p, p.tile_base + xcd_remap(blockIdx.x, gridDim.x), tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  auto rsA = operand_rsrc(p.A, A_KC ? p.M : p.K, p.lda);
  auto rsB = operand_rsrc(p.B, B_KC ? p.N : p.K, p.ldb);
  unsigned offA[PC], offB[PC];
  int kcA[PC], kcB[PC];     // K-contiguous operands: first k of the lane's chunk inside a k-half (chunks past K read as zeros)
#pragma unroll
  for (int j = 0; j < PC; ++j) {
    const int ci = (w * PC + j) * 64 + lane;     // 16-byte chunk of one operand's k-half image (1024 chunks)
    kcA[j] = 0; kcB[j] = 0;
    if (A_KC) {
      const int row = ci >> 2, c = (ci & 3) ^ ((-(row >> 2)) & 3);
      kcA[j] = c * 8;
      offA[j] = (m0 + row < p.M) ? (unsigned)(((long long)(m0 + row) * p.lda + c * 8) * 2) : OOB;
    } else {
      const int kr = ci >> 5, c = (ci & 31) ^ (mc_swz(kr) << 1);
      offA[j] = (m0 + c * 8 < p.M) ? (unsigned)(((long long)kr * p.lda + m0 + c * 8) * 2) : OOB;
    }
    if (B_KC) {
      const int row = ci >> 2, c = (ci & 3) ^ ((-(row >> 2)) & 3);
      kcB[j] = c * 8;
      offB[j] = (n0 + row < p.N) ? (unsigned)(((long long)(n0 + row) * p.ldb + c * 8) * 2) : OOB;
    } else {
      const int kr = ci >> 5, c = (ci & 31) ^ (mc_swz(kr) << 1);
      offB[j] = (n0 + c * 8 < p.N) ? (unsigned)(((long long)kr * p.ldb + n0 + c * 8) * 2) : OOB;
    }
  }
  const unsigned stepA = A_KC ? (unsigned)(KH * 2) : (unsigned)((long long)KH * p.lda * 2);
  const unsigned stepB = B_KC ? (unsigned)(KH * 2) : (unsigned)((long long)KH * p.ldb * 2);
  const int h0 = 2 * blockIdx.y * p.ktiles_per_split;
  const int h1 = min(2 * ((p.K + 2 * KH - 1) / (2 * KH)), h0 + 2 * p.ktiles_per_split);   // k-halves [h0, h1): an even count (past K: zeros)
  auto pieces = [&](int jh) {   // all 4 pieces of this wave for k-half jh -> slot (jh - h0) & 3; past the end: zero fill
    char* base = smem + ((jh - h0) & (NSLOT - 1)) * SLOT;
#pragma unroll
    for (int j = 0; j < PC; ++j) {
      const unsigned v = (offA[j] != OOB && jh < h1 && (!A_KC || jh * KH + kcA[j] < p.K)) ? offA[j] + (unsigned)jh * stepA : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (LDS_PTR(void))(base + (w * PC + j) * 1024), 16, v, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < PC; ++j) {
      const unsigned v = (offB[j] != OOB && jh < h1 && (!B_KC || jh * KH + kcB[j] < p.K)) ? offB[j] + (unsigned)jh * stepB : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (LDS_PTR(void))(base + HALF + (w * PC + j) * 1024), 16, v, 0, 0, 0);
    }
  };
  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // ONE fragment register set: a wave never multiplies and reads at the same time (that is the other wave's job), and a
  // group-1 wave re-reads the registers its MFMAs of k-half j-1 were just issued from (an MFMA takes its A / B operands in
  // its first cycles; the LDS data returns tens of cycles later)
  bf16x8 fa[1][FM], fb[1][FN];
  bf16x4 ra[1][A_KC ? 1 : FM][2], rb[1][B_KC ? 1 : FN][2];
  const int li = lane & 15, lg = lane >> 4;
  auto reads = [&](int set, const char* tA) {
    const char* tB = tA + HALF;
    if (B_KC) {   // fragments are 16 rows = 1024 bytes apart and share the swizzle
      const unsigned b0 = lds_addr_of(tB) + kc32_tile_off(wn * WTN + li, lg);
      fb[set][0] = ds_read_b128_raw<0>(b0); fb[set][1] = ds_read_b128_raw<1024>(b0);
      fb[set][2] = ds_read_b128_raw<2048>(b0); fb[set][3] = ds_read_b128_raw<3072>(b0);
    } else {
#pragma unroll
      for (int j = 0; j < FN; ++j) mc_frag_raw<BN>(tB, wn * WTN + j * 16, 0, lane, rb[0][B_KC ? 0 : j]);
    }
    if (A_KC) {
      const unsigned a0 = lds_addr_of(tA) + kc32_tile_off(wm * WTM + li, lg);
      fa[set][0] = ds_read_b128_raw<0>(a0); fa[set][1] = ds_read_b128_raw<1024>(a0);
      fa[set][2] = ds_read_b128_raw<2048>(a0); fa[set][3] = ds_read_b128_raw<3072>(a0);
      fa[set][4] = ds_read_b128_raw<4096>(a0); fa[set][5] = ds_read_b128_raw<5120>(a0);
      fa[set][6] = ds_read_b128_raw<6144>(a0); fa[set][7] = ds_read_b128_raw<7168>(a0);
    } else {
#pragma unroll
      for (int i = 0; i < FM; ++i) mc_frag_raw<BM>(tA, wm * WTM + i * 16, 0, lane, ra[0][A_KC ? 0 : i]);
    }
  };
  auto tie = [&](int set) {
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      if (B_KC) lds_tie(fb[set][j]);
      else { lds_tie(rb[0][B_KC ? 0 : j][0]); lds_tie(rb[0][B_KC ? 0 : j][1]);
             fb[set][j] = join8(rb[0][B_KC ? 0 : j][0], rb[0][B_KC ? 0 : j][1]); }
    }
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      if (A_KC) lds_tie(fa[set][i]);
      else { lds_tie(ra[0][A_KC ? 0 : i][0]); lds_tie(ra[0][A_KC ? 0 : i][1]);
             fa[set][i] = join8(ra[0][A_KC ? 0 : i][0], ra[0][A_KC ? 0 : i][1]); }
    }
  };
#ifdef LAP_GEMM_EXPERIMENTAL   // ablation / variant bits (lap_gemm_set_debug): 1 no in-loop DMA, 2 no MFMA, 4 no s_setprio
  const bool no_dma = p.dbg & 1, no_mma = p.dbg & 2, no_prio = p.dbg & 4;
#else
  constexpr bool no_dma = false, no_mma = false, no_prio = false;
#endif
#define PQ_FENCE() __builtin_amdgcn_sched_barrier(0)
#define PQ_L(SET, JH)                                                         \
  reads(SET, smem + (((JH) - h0) & (NSLOT - 1)) * SLOT);                      \
  PQ_FENCE();                                                                 \
  if (!no_dma) pieces((JH) + 3);                                              \
  PQ_FENCE();                                                                 \
  lds_wait_all();                                                             \
  tie(SET);                                                                   \
  PQ_FENCE();
#define PQ_M(SET)                                                             \
  if (!no_prio) __builtin_amdgcn_s_setprio(1);                                \
  if (!no_mma) {                                                              \
  _Pragma("unroll") for (int i_ = 0; i_ < FM; ++i_)                           \
    _Pragma("unroll") for (int j_ = 0; j_ < FN; ++j_) acc[i_][j_] = mfma16(fb[SET][j_], fa[SET][i_], acc[i_][j_]); } \
  if (!no_prio) __builtin_amdgcn_s_setprio(0);                                \
  PQ_FENCE();
#define PQ_SYNC()                                                             \
  wait_vmcnt<8>();   /* my 4 pieces of this k-half landed; the next two k-halves may fly */ \
  PQ_FENCE();                                                                 \
  __builtin_amdgcn_s_barrier();                                               \
  PQ_FENCE();

  pieces(h0); pieces(h0 + 1); pieces(h0 + 2);
  if (!g1) {      // two separate loops (same barrier count): one loop with a group branch inside made hipcc spill 450 bytes
    for (int jh = h0; jh < h1; ++jh) {
      PQ_SYNC()
      PQ_L(0, jh)
      PQ_M(0)
    }
  } else {
    PQ_SYNC()
    PQ_L(0, h0)
    for (int jh = h0 + 1; jh < h1; ++jh) {
      PQ_SYNC()
      PQ_M(0)
      PQ_L(0, jh)
    }
    PQ_M(0)
  }
  wait_vmcnt<0>();
  lds_wait_all();
#undef PQ_SYNC
#undef PQ_M
#undef PQ_L
#undef PQ_FENCE

  if (p.epi_lds) { staged_epilogue<NW, WTM, WTN, OUT_F32>(p, smem, acc, wm, wn, m0, n0, tid, lane); return; }
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = m0 + wm * WTM + i * 16 + li;
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = n0 + wn * WTN + j * 16 + 4 * lg;
      if (n >= p.N) continue;
      store_tile4<OUT_F32>(p, m, n, acc[i][j]);
    }
  }
}

#ifdef LAP_GEMM_EXPERIMENTAL
#include "gemm_probes.hpp"   // tiles 8, 9, 13
#endif

template <bool A_KC, bool B_KC, bool OUT_F32>
int launch_pq(const GemmParams& p, hipStream_t s) {   // K % 8 == 0 (a ragged last k-tile is zero-filled by the kernel)
  return launch_256<512, staged_epilogue_lds(OUT_F32), 7, true, OUT_F32>([] { return gemm_pq_kernel<A_KC, B_KC, OUT_F32>; }, p, s);
}

template <int WGM, int WGN, bool A_KC, bool B_KC, bool OUT_F32, bool TWOB = false>
int launch_sp(const GemmParams& p, hipStream_t s) {   // K % 8 == 0, as above
  return launch_256<WGM * WGN * 64, staged_epilogue_lds(OUT_F32), 7, true, OUT_F32>([] { return gemm_sp_kernel<WGM, WGN, A_KC, B_KC, OUT_F32, TWOB>; }, p, s);
}

// Second phase of the two-phase split-K: C[m][n..n+3] = epilogue(alpha * sum_s slab[s * stride ..]), the slabs summed in order.
template <bool OUT_F32>
__device__ __forceinline__ void reduce4(const GemmParams& p, int m, int n, const float* slab, long long stride) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  for (int sp = 0; sp < p.ksplit; ++sp) v += *reinterpret_cast<const f32x4*>(slab + sp * stride);
  store4<OUT_F32>(p, m, n, epilogue4(p, m, n, v * p.alpha));
}

// Slabs [ksplit][M][N] of a whole product: 4 outputs per thread.
template <bool OUT_F32>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(GemmParams p) {
  const long long gid = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (gid >= (long long)p.M * p.N) return;
  reduce4<OUT_F32>(p, (int)(gid / p.N), (int)(gid % p.N), p.part + gid, (long long)p.M * p.N);
}

// The TAIL split of the 256x256 kernels: slabs [ksplit][count][256][256], slot s = logical tile tile_base + s.  64 blocks per tile,
// 4 outputs per thread.
template <bool OUT_F32>
__global__ __launch_bounds__(256) void splitk_tail_reduce_kernel(GemmParams p, int count) {
  const int slot = blockIdx.x >> 6;
  const int within = ((blockIdx.x & 63) * 256 + threadIdx.x) * 4;
  int tm, tn;
  tile_coords<4>(p, p.tile_base + slot, tm, tn);
  const int m = tm * 256 + (within >> 8), n = tn * 256 + (within & 255);
  if (m >= p.M || n >= p.N) return;
  reduce4<OUT_F32>(p, m, n, p.part + ((long long)slot << 16) + within, (long long)count << 16);
}

template <int BM, int BN, int WGM, int WGN, int BK, int NS, bool A_KC, bool B_KC, bool OUT_F32>
int launch(GemmParams p, hipStream_t s) {
  constexpr int EPI = (BM == 256 && BN == 256 && WGM * WGN == 16) ? staged_epilogue_lds(OUT_F32) : 0;   // the 16-wave 256x256 kernel only
  constexpr int LDS = NS * (BM + BN) * BK * 2 > EPI ? NS * (BM + BN) * BK * 2 : EPI;
  auto kern = gemm_kernel<BM, BN, WGM, WGN, BK, NS, A_KC, B_KC, OUT_F32>;
  p.epi_lds = EPI > 0 ? staged_epilogue_mode(p, OUT_F32) : 0;
  if (LDS > 65536) {
    static bool done = false;  // benign race: the attribute is idempotent
    if (!done) {
      hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
      if (e != hipSuccess) return (int)e;
      done = true;
    }
  }
  const bool sub = BM == 128 && BN == 128 && p.sub256;
  p.tiles_m = sub ? (p.M + 255) / 256 : (p.M + BM - 1) / BM;
  p.tiles_n = sub ? (p.N + 255) / 256 : (p.N + BN - 1) / BN;
  const int nkt = (p.K + BK - 1) / BK;
  p.ktiles_per_split = (nkt + p.ksplit - 1) / p.ksplit;
  const int count = sub ? 4 * p.tile_count : (p.tile_count > 0 ? p.tile_count : p.tiles_m * p.tiles_n - p.tile_base);
  dim3 grid(count, p.ksplit);
  hipLaunchKernelGGL(kern, grid, dim3(WGM * WGN * 64), LDS, s, p);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}

template <bool A_KC, bool B_KC, bool OUT_F32>
int dispatch_tile(const GemmParams& p, int tile, hipStream_t s) {
  switch (tile) {
    // production: 10 (software-pipelined 8-wave 256x256, K % 64 == 0), 5 (16-wave 256x256), 6 (128x128); 2 is the
    // direct-epilogue 8-wave kernel the bitwise tests compare against; 0 (default below) the 4-wave 128x128 kernel
    case 12: return launch_pq<A_KC, B_KC, OUT_F32>(p, s);
    case 10: return launch_sp<2, 4, A_KC, B_KC, OUT_F32>(p, s);
    case 6: return launch<128, 128, 2, 4, 64, 2, A_KC, B_KC, OUT_F32>(p, s);
    // serving-prefill shapes (M = 512 / 560 rows, forward layout, bf16 out): see pick_serving_tile
    case 15: if constexpr (A_KC && B_KC) return launch<320, 256, 2, 4, 64, 2, true, true, OUT_F32>(p, s); else return LAP_ERR_ARG;
    case 16: if constexpr (A_KC && B_KC) return launch<64, 128, 2, 4, 64, 3, true, true, OUT_F32>(p, s); else return LAP_ERR_ARG;
    case 17: if constexpr (A_KC && B_KC) return launch<64, 64, 2, 2, 64, 4, true, true, OUT_F32>(p, s); else return LAP_ERR_ARG;
    case 18: if constexpr (A_KC && B_KC) return launch<128, 64, 4, 2, 64, 3, true, true, OUT_F32>(p, s); else return LAP_ERR_ARG;
    case 19: if constexpr (A_KC && B_KC) return launch<320, 128, 2, 4, 64, 2, true, true, OUT_F32>(p, s); else return LAP_ERR_ARG;
    case 5: return launch<256, 256, 4, 4, 64, 2, A_KC, B_KC, OUT_F32>(p, s);
    case 2: return launch<256, 256, 2, 4, 64, 2, A_KC, B_KC, OUT_F32>(p, s);
#ifdef LAP_GEMM_EXPERIMENTAL   // probes kept for the record (13, 9, 8: gemm_probes.hpp): python -m lap_amd.build --variant=exp
    case 13: if constexpr (A_KC && B_KC) return launch_pn<OUT_F32>(p, s); else return LAP_ERR_ARG;
    case 11: return launch_sp<2, 4, A_KC, B_KC, OUT_F32, true>(p, s);   // tile 10 with two barriers per k-tile (probe)
    case 9: return launch_pp16<A_KC, B_KC, OUT_F32>(p, s);
    case 8: return launch_pp<A_KC, B_KC, OUT_F32>(p, s);
    case 7: return launch<256, 128, 4, 4, 64, 2, A_KC, B_KC, OUT_F32>(p, s);
    case 4: return launch<128, 128, 2, 2, 32, 4, A_KC, B_KC, OUT_F32>(p, s);
    case 3: return launch<256, 256, 2, 4, 32, 4, A_KC, B_KC, OUT_F32>(p, s);
    case 1: return launch<256, 128, 4, 2, 64, 3, A_KC, B_KC, OUT_F32>(p, s);
#else
    case 13: case 11: case 9: case 8: case 7: case 4: case 3: case 1: return LAP_ERR_ARG;   // not in this build
#endif
    default: return launch<128, 128, 2, 2, 64, 2, A_KC, B_KC, OUT_F32>(p, s);
  }
}

// run-time (layout, output type) -> the tile launchers' instantiation
int dispatch(const GemmParams& p, int tile, bool a_kc, bool b_kc, bool f32, hipStream_t s) {
  if (f32) {
    if (a_kc && b_kc) return dispatch_tile<true, true, true>(p, tile, s);
    if (a_kc && !b_kc) return dispatch_tile<true, false, true>(p, tile, s);
    if (!a_kc && !b_kc) return dispatch_tile<false, false, true>(p, tile, s);
    return dispatch_tile<false, true, true>(p, tile, s);
  }
  if (a_kc && b_kc) return dispatch_tile<true, true, false>(p, tile, s);
  if (a_kc && !b_kc) return dispatch_tile<true, false, false>(p, tile, s);
  if (!a_kc && !b_kc) return dispatch_tile<false, false, false>(p, tile, s);
  return dispatch_tile<false, true, false>(p, tile, s);
}

int g_gemm_dbg = 0;

// The A/B switches of the routing (LAP_GEMM_NO_ASM=1 ... -> LAP_ROUTE_NO_ASM ...), read once per process.
unsigned route_switches_from_env() {
  static const unsigned sw = [] {
    static const struct { const char* name; unsigned bit; } k[] = {
        {"LAP_GEMM_NO_ASM", LAP_ROUTE_NO_ASM}, {"LAP_GEMM_NO_ASM_NN", LAP_ROUTE_NO_ASM_NN}, {"LAP_GEMM_NO_ASM_RES", LAP_ROUTE_NO_ASM_RES},
        {"LAP_GEMM_NO_MSPLIT", LAP_ROUTE_NO_MSPLIT}, {"LAP_GEMM_NO_MSPLIT_LONGK", LAP_ROUTE_NO_MSPLIT_LONGK}, {"LAP_GEMM_NO_NSPLIT", LAP_ROUTE_NO_NSPLIT},
        {"LAP_GEMM_NO_SERVING_TILES", LAP_ROUTE_NO_SERVING_TILES}, {"LAP_GEMM_NO_PINGPONG", LAP_ROUTE_NO_PINGPONG}, {"LAP_GEMM_NO_KTAIL", LAP_ROUTE_NO_KTAIL}};
    unsigned m = 0;
    for (const auto& e : k)
      if (getenv(e.name) != nullptr) m |= e.bit;
    return m;
  }();
  return sw;
}

// the caller's arguments as the planner takes them
struct GemmCall {
  const void* A; const void* B; void* C; const void* bias; const void* residual;
  int M, N, K, lda, ldb, ldc, ldr;
  float alpha;
  int a_kc, b_kc, flags, tile, ksplit;
  void* scratch;
  long long scratch_bytes;
};

int plan_gemm(const GemmCall& g, unsigned switches, lap_route::Plan& plan) {
  lap_route::Call c = {};
  c.A = (uintptr_t)g.A; c.B = (uintptr_t)g.B; c.C = (uintptr_t)g.C; c.bias = (uintptr_t)g.bias; c.res = (uintptr_t)g.residual;
  c.M = g.M; c.N = g.N; c.K = g.K; c.lda = g.lda; c.ldb = g.ldb; c.ldc = g.ldc; c.ldr = g.ldr; c.alpha = g.alpha;
  c.a_kc = g.a_kc; c.b_kc = g.b_kc; c.flags = g.flags; c.tile = g.tile; c.ksplit = g.ksplit;
  c.scratch = g.scratch != nullptr; c.scratch_bytes = g.scratch_bytes; c.sw = switches;
  return lap_route::plan_call(c, plan);
}

// Launches the legs of a plan in order on the caller's stream; the first failing launch ends the walk with its code.
int run_plan(const lap_route::Plan& plan, const GemmCall& g, float* sumsq, void* stream) {
  const bool f32 = g.flags & LAP_GEMM_OUT_F32;
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i < plan.n; ++i) {
    const lap_gemm_leg& l = plan.legs[i];
    const void* A = (const char*)g.A + l.off_a * 2;
    const void* B = (const char*)g.B + l.off_b * 2;
    void* C = (char*)g.C + l.off_c * (f32 ? 4 : 2);
    const void* bias = g.bias ? (const char*)g.bias + l.off_bias * ((g.flags & LAP_GEMM_BIAS_F32) ? 4 : 2) : nullptr;
    const void* residual = g.residual ? (const char*)g.residual + l.off_res * 2 : nullptr;
    int rc;
    switch (l.engine) {
      case LAP_LEG_ASM: rc = lap_gemm_asm(A, B, C, l.M, l.N, g.K, g.lda, g.ldb, g.ldc, g.a_kc, g.b_kc, f32, stream); break;
      case LAP_LEG_ASM_BIAS: rc = lap_gemm_asm_bias(A, B, C, (const float*)bias, l.M, l.N, g.K, g.lda, g.ldb, g.ldc, stream); break;
      case LAP_LEG_ASM_RES: rc = lap_gemm_asm_res(A, B, C, (const float*)bias, residual, l.M, l.N, g.K, g.lda, g.ldb, g.ldc, stream); break;
      case LAP_LEG_ASM_WGRAD_SUMSQ:
        rc = f32 ? lap_gemm_asm_wgrad(A, B, C, l.M, l.N, g.K, g.lda, g.ldb, g.ldc, sumsq, stream)
                 : lap_gemm_asm_wgrad_b16(A, B, C, l.M, l.N, g.K, g.lda, g.ldb, g.ldc, sumsq, stream);
        break;
      default: {
        GemmParams p = {};
        p.A = (const bf16*)A; p.B = (const bf16*)B; p.C = C; p.bias = bias; p.R = (const bf16*)residual;
        p.M = l.M; p.N = l.N; p.K = g.K; p.lda = g.lda; p.ldb = g.ldb; p.ldc = g.ldc; p.ldr = g.ldr; p.alpha = g.alpha;
        p.bias_kind = bias ? ((g.flags & LAP_GEMM_BIAS_F32) ? 2 : 1) : 0;
        p.gelu = (g.flags & LAP_GEMM_GELU) ? ((g.flags & LAP_GEMM_GELU_BF16) ? 2 : 1) : 0;
        p.accum = (g.flags & LAP_GEMM_ACCUM) ? 1 : 0;
        p.geglu = (g.flags & LAP_GEMM_GEGLU) ? ((g.flags & LAP_GEMM_GELU_EXP2) ? 2 : 1) : 0;
        p.ksplit = l.ksplit;
        p.dbg = g_gemm_dbg;
        p.part = l.part ? (float*)g.scratch : nullptr;
        p.tile_base = l.tile_base; p.tile_count = l.tile_count; p.sub256 = l.sub256; p.part_compact = l.part_compact;
        rc = dispatch(p, l.engine, g.a_kc, g.b_kc, l.f32_tile, s);
        if (rc || l.reduce == LAP_LEG_REDUCE_NONE) break;
        if (l.reduce == LAP_LEG_REDUCE_TAIL) {
          p.tiles_m = (l.M + 255) / 256; p.tiles_n = (l.N + 255) / 256;
          if (f32) hipLaunchKernelGGL(splitk_tail_reduce_kernel<true>, dim3(l.tile_count * 64), dim3(256), 0, s, p, l.tile_count);
          else hipLaunchKernelGGL(splitk_tail_reduce_kernel<false>, dim3(l.tile_count * 64), dim3(256), 0, s, p, l.tile_count);
        } else {
          const long long n4 = (long long)l.M * l.N / 4;
          if (f32) hipLaunchKernelGGL(splitk_reduce_kernel<true>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, p);
          else hipLaunchKernelGGL(splitk_reduce_kernel<false>, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, p);
        }
        LAP_CHECK_LAUNCH();
      }
    }
    if (rc) return rc;
  }
  return LAP_OK;
}

int gemm_planned(const GemmCall& g, unsigned switches, float* sumsq, int* folded, void* stream) {
  lap_route::Plan plan;
  if (int rc = plan_gemm(g, switches, plan)) return rc;
  if (folded) *folded = plan.legs[0].engine == LAP_LEG_ASM_WGRAD_SUMSQ;
  return run_plan(plan, g, sumsq, stream);
}

// Weight gradient dW [M][N] (f32 or bf16) = A^T B over K rows (A [K][M], B [K][N]) with its sum of squares folded in where the
// assembly kernel takes the product (*folded = 1: *sumsq has received sum(dW^2)); every other shape runs as lap_gemm_bf16_ex would
// run it and leaves the norm to the caller (*folded = 0).  The routing rule is the plain-product rule of lap_gemm_bf16_ex.
int gemm_wgrad(bool f32, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, float* sumsq, int* folded,
               void* scratch, long long scratch_bytes, void* stream) {
  if (!folded) return LAP_ERR_ARG;
  *folded = 0;
  const GemmCall g = {A, B, C, nullptr, nullptr, M, N, K, lda, ldb, ldc, 0, 1.0f, 0, 0, f32 ? LAP_GEMM_OUT_F32 : 0, -1, 0, scratch, scratch_bytes};
  return gemm_planned(g, route_switches_from_env() | (sumsq ? LAP_ROUTE_WGRAD_SUMSQ : 0), sumsq, folded, stream);
}

}  // namespace

extern "C" int lap_gemm_set_debug(int bits) {   // ablation knob; has an effect in LAP_GEMM_EXPERIMENTAL builds only
#ifdef LAP_GEMM_EXPERIMENTAL
  g_gemm_dbg = bits;
  return LAP_OK;
#else
  return bits ? LAP_ERR_ARG : LAP_OK;
#endif
}

extern "C" int lap_gemm_wgrad_f32(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, float* sumsq,
                                  int* folded, void* scratch, long long scratch_bytes, void* stream) {
  return gemm_wgrad(true, A, B, C, M, N, K, lda, ldb, ldc, sumsq, folded, scratch, scratch_bytes, stream);
}

// The same for a weight gradient stored as bf16 (dW [M][N] bf16; ParamStore.grad_dtype): the bf16 assembly kernels fold the squares of
// their f32 accumulators.
extern "C" int lap_gemm_wgrad_bf16(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, float* sumsq,
                                   int* folded, void* scratch, long long scratch_bytes, void* stream) {
  return gemm_wgrad(false, A, B, C, M, N, K, lda, ldb, ldc, sumsq, folded, scratch, scratch_bytes, stream);
}

// Plan (csrc/gemm_route.hpp: every routing rule lives there), then launch the legs.
extern "C" int lap_gemm_bf16_ex(const void* A, const void* B, void* C, const void* bias, const void* residual,
                                int M, int N, int K, int lda, int ldb, int ldc, int ldr, float alpha,
                                int a_kc, int b_kc, int flags, int tile, int ksplit, void* scratch,
                                long long scratch_bytes, void* stream) {
  const GemmCall g = {A, B, C, bias, residual, M, N, K, lda, ldb, ldc, ldr, alpha, a_kc, b_kc, flags, tile, ksplit, scratch, scratch_bytes};
  return gemm_planned(g, route_switches_from_env(), nullptr, nullptr, stream);
}

extern "C" int lap_gemm_plan(const void* A, const void* B, const void* C, const void* bias, const void* residual,
                             int M, int N, int K, int lda, int ldb, int ldc, int ldr, float alpha,
                             int a_kc, int b_kc, int flags, int tile, int ksplit, const void* scratch, long long scratch_bytes,
                             unsigned switches, lap_gemm_leg* legs, int max_legs, int* n_legs) {
  if (!legs || !n_legs || max_legs < 0) return LAP_ERR_ARG;
  *n_legs = 0;
  const GemmCall g = {A, B, (void*)C, bias, residual, M, N, K, lda, ldb, ldc, ldr, alpha, a_kc, b_kc, flags, tile, ksplit, (void*)scratch, scratch_bytes};
  lap_route::Plan plan;
  if (int rc = plan_gemm(g, switches, plan)) return rc;
  if (plan.n > max_legs) return LAP_ERR_ARG;
  for (int i = 0; i < plan.n; ++i) legs[i] = plan.legs[i];
  *n_legs = plan.n;
  return LAP_OK;
}

extern "C" int lap_gemm_bf16(const void* A, const void* B, void* C, const void* bias, const void* residual,
                             int M, int N, int K, int lda, int ldb, int ldc, int ldr, float alpha,
                             int a_kc, int b_kc, int flags, void* stream) {
  return lap_gemm_bf16_ex(A, B, C, bias, residual, M, N, K, lda, ldb, ldc, ldr, alpha, a_kc, b_kc, flags, -1, 0, nullptr, 0,
                          stream);
}
