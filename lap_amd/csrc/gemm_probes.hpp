// Probe kernels of the bf16 GEMM: measured, documented in DESIGN.md §4, not production.  gemm.hip includes this file inside its
// anonymous namespace, and only in a LAP_GEMM_EXPERIMENTAL build (python -m lap_amd.build --variant=exp); dispatch_tile reaches the
// kernels as tiles 8 (gemm_pp_kernel), 9 (gemm_pp16_kernel) and 13 (gemm_pn_kernel).  The other probe tiles are instantiations of
// the production kernels (1, 3, 4, 7: gemm_kernel shapes; 11: gemm_sp_kernel with TWOB), and the ablation bits of
// lap_gemm_set_debug live in those kernels, in gemm.hip.  Uses gemm_common.hpp and gemm.hip's ds_read_b128_raw.
#pragma once

// ---------------------------------------------------------------------------------------------------------------
// Ping-pong 256x256x64 kernel: 8 waves (2 x 4), 128x64 per wave, one block per CU.  Each k-tile is cut into four
// phases (one 64x32 quadrant of the wave's output x K = 64 = 16 MFMAs); a phase is
//     [ds_read the fragments this quadrant needs | issue ONE half-tile of LDS-DMA | counted vmcnt]  barrier
//     [16 MFMAs]  barrier
// and the second wave row runs one barrier behind the first, so on every SIMD one wave is in its MFMA segment while
// its partner is in its LDS segment: the matrix pipe and the LDS port work concurrently by construction instead of
// by luck of the wave scheduler.  Quadrant order (0,0) (0,1) (1,1) (1,0) reuses the A half for two phases and keeps
// both B halves in registers: 12 / 4 / 8 / 0 ds_read_b128 per phase.
// Staging granularity is the HALF tile (the 128 rows of A, or 128 columns of B, that one quadrant row / column
// reads: a 16 KiB image, 2 LDS-DMA pieces per wave), 8 slots = 2 k-tiles.  A half is dead as soon as its quadrant
// has been read, so it is refilled with the k-tile after next: phase 1 issues B1(kt+1), phase 2 A1(kt+1), phase 3
// A0(kt+2), phase 4 B0(kt+2) - every half is requested five phases (1.25 k-tiles) before its first reader and four
// halves (64 KiB per block) are in flight at every wait, which is always the same `s_waitcnt vmcnt(8)` (never 0
// inside the loop; past the end of K the pieces are out-of-range buffer loads, i.e. zero fills without traffic).
// Ordering: a wait in the LDS segment of phase p makes the half visible to readers from phase p + 1 on (one barrier
// more than usual because the two groups are a barrier apart); a half is refilled at the earliest two phases after
// its last read.  All fragment reads are raw (common.hpp), fenced by the lgkmcnt(0) that opens the MFMA segment.
template <bool A_KC, bool B_KC, bool OUT_F32>
__global__ __launch_bounds__(512) void gemm_pp_kernel(GemmParams p) {
  constexpr int BM = 256, BN = 256, BK = 64, HALF = 128 * BK * 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // slot (buf, h): h = 0 A0, 1 A1, 2 B0, 3 B1
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 2, wn = w & 3;   // waves 0-3: row 0 (leading group), waves 4-7: row 1 (one barrier behind)

  const int t = p.tile_base + xcd_remap(blockIdx.x, gridDim.x);
  int tm, tn;
  tile_coords<4>(p, t, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;

  auto rsA = operand_rsrc(p.A, A_KC ? p.M : p.K, p.lda);
  auto rsB = operand_rsrc(p.B, B_KC ? p.N : p.K, p.ldb);
  // Half images.  A half mh holds the rows {wm' * 128 + mh * 64 + r} at local index wm' * 64 + r; B half nh holds the
  // columns {wn' * 64 + nh * 32 + c} at local index wn' * 32 + c.  K-contiguous: [128 rows][64 k]; M-contiguous:
  // [64 k][128 m].  Piece q = 2 w + j covers linear 16-byte chunks [64 q, 64 q + 64) of the image.
  unsigned off[4][2];
  int kidxA[2], kidxB[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int ci = (w * 2 + j) * 64 + lane;
    int la, ca, lb, cb;   // local row / column index, logical 16-byte chunk
    if (A_KC) { la = ci >> 3; ca = (ci & 7) ^ ((la >> 1) & 7); kidxA[j] = ca * 8; }
    else { const int kr = ci >> 4; ca = (ci & 15) ^ (mc_swz(kr) << 1); la = ca * 8; kidxA[j] = kr; }
    if (B_KC) { lb = ci >> 3; cb = (ci & 7) ^ ((lb >> 1) & 7); kidxB[j] = cb * 8; }
    else { const int kr = ci >> 4; cb = (ci & 15) ^ (mc_swz(kr) << 1); lb = cb * 8; kidxB[j] = kr; }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int gm = m0 + (la >> 6) * 128 + h * 64 + (la & 63);
      const int gn = n0 + (lb >> 5) * 64 + h * 32 + (lb & 31);
      off[h][j] = gm < p.M ? (unsigned)((A_KC ? (long long)gm * p.lda + ca * 8 : (long long)kidxA[j] * p.lda + gm) * 2) : OOB;
      off[2 + h][j] = gn < p.N ? (unsigned)((B_KC ? (long long)gn * p.ldb + cb * 8 : (long long)kidxB[j] * p.ldb + gn) * 2) : OOB;
    }
  }
  const unsigned stepA = A_KC ? (unsigned)(BK * 2) : (unsigned)((long long)BK * p.lda * 2);
  const unsigned stepB = B_KC ? (unsigned)(BK * 2) : (unsigned)((long long)BK * p.ldb * 2);

  const int nkt_all = (p.K + BK - 1) / BK;
  const int kt0 = blockIdx.y * p.ktiles_per_split;
  const int kt1 = min(nkt_all, kt0 + p.ktiles_per_split);
  const int kend = min(p.K, kt1 * BK);
  auto issue = [&](int buf, int h, int kt) {
    char* base = smem + (buf * 4 + h) * HALF + w * 2048;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kidx = h < 2 ? kidxA[j] : kidxB[j];
      const unsigned v = (off[h][j] != OOB && kt * BK + kidx < kend) ? off[h][j] + (unsigned)kt * (h < 2 ? stepA : stepB) : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(h < 2 ? rsA : rsB, (LDS_PTR(void))(base + j * 1024), 16, v, 0, 0, 0);
    }
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  bf16x8 fa[4][2], fb[2][2][2];                               // A half: [m-frag][kk]; B: [n-half][n-frag][kk]
  bf16x4 ra[A_KC ? 1 : 4][2][2], rb[B_KC ? 1 : 2][2][2][2];   // transposing reads arrive as two 64-bit halves
  auto read_a = [&](const char* img) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        if (A_KC) fa[i][kk] = kc_frag_raw(img, wm * 64 + i * 16, kk, lane);
        else mc_frag_raw<128>(img, wm * 64 + i * 16, kk, lane, ra[A_KC ? 0 : i][kk]);
      }
  };
  auto read_b = [&](const char* img, int nh) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        if (B_KC) fb[nh][j][kk] = kc_frag_raw(img, wn * 32 + j * 16, kk, lane);
        else mc_frag_raw<128>(img, wn * 32 + j * 16, kk, lane, rb[B_KC ? 0 : nh][j][kk]);
      }
  };
  auto tie_a = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        if (A_KC) lds_tie(fa[i][kk]);
        else { lds_tie(ra[A_KC ? 0 : i][kk][0]); lds_tie(ra[A_KC ? 0 : i][kk][1]); fa[i][kk] = join8(ra[A_KC ? 0 : i][kk][0], ra[A_KC ? 0 : i][kk][1]); }
      }
  };
  auto tie_b = [&](int nh) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        if (B_KC) lds_tie(fb[nh][j][kk]);
        else {
          lds_tie(rb[B_KC ? 0 : nh][j][kk][0]); lds_tie(rb[B_KC ? 0 : nh][j][kk][1]);
          fb[nh][j][kk] = join8(rb[B_KC ? 0 : nh][j][kk][0], rb[B_KC ? 0 : nh][j][kk][1]);
        }
      }
  };
#define PP_BAR() { __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_barrier(); __builtin_amdgcn_sched_barrier(0); }
#define PP_MMA(MH, NH)                                                                         \
  {                                                                                            \
    __builtin_amdgcn_s_setprio(1);                                                             \
    _Pragma("unroll") for (int kk = 0; kk < 2; ++kk)                                           \
      _Pragma("unroll") for (int i = 0; i < 4; ++i)                                            \
        _Pragma("unroll") for (int j = 0; j < 2; ++j)                                          \
          acc[MH * 4 + i][NH * 2 + j] = mfma16(fb[NH][j][kk], fa[i][kk], acc[MH * 4 + i][NH * 2 + j]); \
    __builtin_amdgcn_s_setprio(0);                                                             \
  }

  // prologue: the six halves the steady state would already have requested, in its order
  issue(0, 0, kt0); issue(0, 2, kt0); issue(0, 3, kt0); issue(0, 1, kt0); issue(1, 0, kt0 + 1); issue(1, 2, kt0 + 1);
  wait_vmcnt<8>();                            // A0, B0 of the first k-tile
  PP_BAR()
  if (wm == 1) __builtin_amdgcn_s_barrier();  // second wave row drops one barrier behind
  __builtin_amdgcn_sched_barrier(0);
  for (int kt = kt0; kt < kt1; ++kt) {
    const int buf = (kt - kt0) & 1;
    const char* img = smem + buf * 4 * HALF;
    // phase 1: quadrant (0,0)
    read_a(img);
    read_b(img + 2 * HALF, 0);
    issue(buf ^ 1, 3, kt + 1);
    wait_vmcnt<8>();                          // B1(kt) for phase 2
    PP_BAR()
    lds_wait_all();
    tie_a(); tie_b(0);
    PP_MMA(0, 0)
    PP_BAR()
    // phase 2: quadrant (0,1)
    read_b(img + 3 * HALF, 1);
    issue(buf ^ 1, 1, kt + 1);
    wait_vmcnt<8>();                          // A1(kt) for phase 3
    PP_BAR()
    lds_wait_all();
    tie_b(1);
    PP_MMA(0, 1)
    PP_BAR()
    // phase 3: quadrant (1,1)
    read_a(img + HALF);
    issue(buf, 0, kt + 2);
    PP_BAR()
    lds_wait_all();
    tie_a();
    PP_MMA(1, 1)
    PP_BAR()
    // phase 4: quadrant (1,0): nothing to read
    issue(buf, 2, kt + 2);
    wait_vmcnt<8>();                          // A0, B0 of the next k-tile
    PP_BAR()
    PP_MMA(1, 0)
    PP_BAR()
  }
  wait_vmcnt<0>();
  if (wm == 0) __builtin_amdgcn_s_barrier();  // balance the stagger
#undef PP_MMA
#undef PP_BAR

  const int li = lane & 15, lg = lane >> 4;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int m = m0 + wm * 128 + i * 16 + li;
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wn * 64 + j * 16 + 4 * lg;
      if (n >= p.N) continue;
      store_tile4<OUT_F32>(p, m, n, acc[i][j]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// 16-wave ping-pong (tile 9): the 256x256 / 64x64-per-wave geometry of the production kernel, but the k-loop advances in
// 32-deep SUB-TILES (one MFMA k-step: 8 fragment reads, 16 MFMAs per wave) and the wave rows alternate between two
// groups one barrier apart (rows 0, 2 lead; rows 1, 3 trail), so that each SIMD always has two waves in their MFMA
// segment (512 pipe cycles) while its other two are in their LDS segment (reads of the next sub-tile, 2 LDS-DMA pieces,
// counted wait).  The lockstep kernel pays a matrix-pipe bubble after every barrier (all 16 waves issue DMA + reads and
// wait for LDS at the same time); here that segment of one group hides under the other group's MFMAs.
// Ring of 4 sub-tile slots (32 KiB each: A [256][32] | B [256][32], the BK = 32 images of common.hpp / kc32_*): phase st
// reads slot st, issues sub-tile st + 2 into the slot last read two phases ago, and `s_waitcnt vmcnt(2)` makes sub-tile
// st + 1 visible for the next phase (wait in phase p -> read in phase p + 1, as for tile 8).
__device__ __forceinline__ bf16x8 kc32_frag_raw(const char* tile, int row0, int lane) {
  const int i = lane & 15, g = lane >> 4;
  bf16x8 r;
  asm volatile("ds_read_b128 %0, %1" : "=v"(r) : "v"(lds_addr_of(tile) + kc32_tile_off(row0 + i, g)));
  return r;
}

template <bool A_KC, bool B_KC, bool OUT_F32>
__global__ __launch_bounds__(1024) void gemm_pp16_kernel(GemmParams p) {
  constexpr int BM = 256, BN = 256, SK = 32, OPB = 256 * SK * 2, SLOT = 2 * OPB;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // 4 slots: [A sub-tile | B sub-tile]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 2, wn = w & 3;
  const int trailing = wm & 1;

  const int t = p.tile_base + xcd_remap(blockIdx.x, gridDim.x);
  int tm, tn;
  tile_coords<4>(p, t, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  auto rsA = operand_rsrc(p.A, A_KC ? p.M : p.K, p.lda);
  auto rsB = operand_rsrc(p.B, B_KC ? p.N : p.K, p.ldb);
  // one 1 KiB piece per wave and operand: linear 16-byte chunks [64 w, 64 w + 64) of the sub-tile image
  unsigned offA, offB;
  int kidxA, kidxB;
  {
    const int ci = w * 64 + lane;
    if (A_KC) {
      const int row = ci >> 2, c = (ci & 3) ^ ((-(row >> 2)) & 3);
      kidxA = c * 8;
      offA = (m0 + row < p.M) ? (unsigned)(((long long)(m0 + row) * p.lda + c * 8) * 2) : OOB;
    } else {
      const int kr = ci >> 5, c = (ci & 31) ^ (mc_swz(kr) << 1);
      kidxA = kr;
      offA = (m0 + c * 8 < p.M) ? (unsigned)(((long long)kr * p.lda + m0 + c * 8) * 2) : OOB;
    }
    if (B_KC) {
      const int row = ci >> 2, c = (ci & 3) ^ ((-(row >> 2)) & 3);
      kidxB = c * 8;
      offB = (n0 + row < p.N) ? (unsigned)(((long long)(n0 + row) * p.ldb + c * 8) * 2) : OOB;
    } else {
      const int kr = ci >> 5, c = (ci & 31) ^ (mc_swz(kr) << 1);
      kidxB = kr;
      offB = (n0 + c * 8 < p.N) ? (unsigned)(((long long)kr * p.ldb + n0 + c * 8) * 2) : OOB;
    }
  }
  const unsigned stepA = A_KC ? (unsigned)(SK * 2) : (unsigned)((long long)SK * p.lda * 2);
  const unsigned stepB = B_KC ? (unsigned)(SK * 2) : (unsigned)((long long)SK * p.ldb * 2);
  const int st0 = blockIdx.y * p.ktiles_per_split * 2;
  const int st1 = min((p.K + SK - 1) / SK, st0 + p.ktiles_per_split * 2);
  const int kend = min(p.K, st1 * SK);
  auto issue = [&](int st) {   // past the end: out-of-range pieces (zero fill, no traffic) keep the wait counts uniform
    char* base = smem + (st & 3) * SLOT + w * 1024;
    const unsigned va = (offA != OOB && st * SK + kidxA < kend) ? offA + (unsigned)st * stepA : OOB;
    const unsigned vb = (offB != OOB && st * SK + kidxB < kend) ? offB + (unsigned)st * stepB : OOB;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (LDS_PTR(void))(base), 16, va, 0, 0, 0);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (LDS_PTR(void))(base + OPB), 16, vb, 0, 0, 0);
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 fa[4], fb[4];
  bf16x4 ra[A_KC ? 1 : 4][2], rb[B_KC ? 1 : 4][2];

#define P16_BAR() { __builtin_amdgcn_sched_barrier(0); __builtin_amdgcn_s_barrier(); __builtin_amdgcn_sched_barrier(0); }
  issue(st0); issue(st0 + 1);
  wait_vmcnt<2>();                                // sub-tile st0 landed
  P16_BAR()
  if (trailing) __builtin_amdgcn_s_barrier();     // rows 1, 3 drop one barrier behind
  __builtin_amdgcn_sched_barrier(0);
  for (int st = st0; st < st1; ++st) {
    const char* tA = smem + (st & 3) * SLOT;
    const char* tB = tA + OPB;
    // ---- LDS segment
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (A_KC) fa[i] = kc32_frag_raw(tA, wm * 64 + i * 16, lane);
      else mc_frag_raw<BM>(tA, wm * 64 + i * 16, 0, lane, ra[A_KC ? 0 : i]);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (B_KC) fb[j] = kc32_frag_raw(tB, wn * 64 + j * 16, lane);
      else mc_frag_raw<BN>(tB, wn * 64 + j * 16, 0, lane, rb[B_KC ? 0 : j]);
    }
    issue(st + 2);
    wait_vmcnt<2>();                              // sub-tile st + 1 (read in the next phase)
    P16_BAR()
    // ---- MFMA segment
    lds_wait_all();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (A_KC) lds_tie(fa[i]);
      else { lds_tie(ra[A_KC ? 0 : i][0]); lds_tie(ra[A_KC ? 0 : i][1]); fa[i] = join8(ra[A_KC ? 0 : i][0], ra[A_KC ? 0 : i][1]); }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (B_KC) lds_tie(fb[j]);
      else { lds_tie(rb[B_KC ? 0 : j][0]); lds_tie(rb[B_KC ? 0 : j][1]); fb[j] = join8(rb[B_KC ? 0 : j][0], rb[B_KC ? 0 : j][1]); }
    }
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = mfma16(fb[j], fa[i], acc[i][j]);
    __builtin_amdgcn_s_setprio(0);
    P16_BAR()
  }
  wait_vmcnt<0>();
  if (!trailing) __builtin_amdgcn_s_barrier();    // balance the stagger
#undef P16_BAR

  const int li = lane & 15, lg = lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + wm * 64 + i * 16 + li;
    if (m >= p.M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wn * 64 + j * 16 + 4 * lg;
      if (n >= p.N) continue;
      store_tile4<OUT_F32>(p, m, n, acc[i][j]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Ping-pong kernel for the forward layout (tile 13: both operands K-contiguous).  Tile 12's 32-deep k-half slots would
// cut every 128-byte operand row into two 64-byte LDS-DMA requests; here the two intervals of a 64-deep k-tile split the
// wave's A FRAGMENTS instead of K, so every piece still moves full lines:
//     interval 2t   : A_lo(t) x B(t)   (A fragments 0-3, both k-steps, 32 MFMAs)      reads: 8 B + 8 A_lo fragments
//     interval 2t+1 : A_hi(t) x B(t)   (A fragments 4-7; B stays in registers)        reads: 8 A_hi fragments
// with the two wave groups in opposite order inside every interval (group 0: read, multiply; group 1: multiply what it read
// in the previous interval, read) and one barrier per interval, as in tile 12.  LDS: rings of two for each of
// A_lo (16 KiB: tile rows 0-63 and 128-191), A_hi (16 KiB: rows 64-127, 192-255) and B (32 KiB) = 128 KiB.  A_hi(t+1) is
// requested in interval 2t (its slot held A_hi(t-1), read in interval 2t-1), A_lo / B(t+2) in interval 2t+1 — three
// intervals ahead of their first use; a wave's own pieces are awaited with vmcnt(8) in both kinds of interval.
template <bool OUT_F32>
__global__ __launch_bounds__(512) void gemm_pn_kernel(GemmParams p) {
  constexpr int BM = 256, BN = 256, BK = 64, HALF_A = 128 * BK * 2, B_BYTES = BN * BK * 2;   // 16 KiB, 32 KiB
  constexpr int OFF_ALO = 0, OFF_AHI = 2 * HALF_A, OFF_B = 4 * HALF_A;                         // rings of two
  constexpr int WGN = 4, NW = 8, WTM = 128, WTN = 64, FM = 8, FN = 4;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w / WGN, wn = w % WGN;
  const bool g1 = w >= 4;
  int tm, tn;
  tile_coords<4>(p, p.tile_base + xcd_remap(blockIdx.x, gridDim.x), tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  auto rsA = operand_rsrc(p.A, p.M, p.lda);
  auto rsB = operand_rsrc(p.B, p.N, p.ldb);
  // per-lane source offsets: A halves 2 pieces per wave each, B 4 pieces; image row r of an A half <-> tile row
  // (r & 63) + 128 (r >> 6) (+ 64 for the hi half); 8 chunks of 16 bytes per 128-byte row, XOR-swizzled on the source side
  unsigned offAlo[2], offAhi[2], offB[4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int ci = (w * 2 + j) * 64 + lane;
    const int r = ci >> 3, c = (ci & 7) ^ ((r >> 1) & 7);
    const int trow = (r & 63) + 128 * (r >> 6);
    offAlo[j] = (m0 + trow < p.M) ? (unsigned)(((long long)(m0 + trow) * p.lda + c * 8) * 2) : OOB;
    offAhi[j] = (m0 + trow + 64 < p.M) ? (unsigned)(((long long)(m0 + trow + 64) * p.lda + c * 8) * 2) : OOB;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ci = (w * 4 + j) * 64 + lane;
    const int r = ci >> 3, c = (ci & 7) ^ ((r >> 1) & 7);
    offB[j] = (n0 + r < p.N) ? (unsigned)(((long long)(n0 + r) * p.ldb + c * 8) * 2) : OOB;
  }
  const int kt0 = blockIdx.y * p.ktiles_per_split;
  const int kt1 = min(p.K / BK, kt0 + p.ktiles_per_split);
  auto dma_alo_b = [&](int kt) {     // A_lo(kt) + B(kt): 6 pieces
    const int sl = (kt - kt0) & 1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const unsigned v = (offAlo[j] != OOB && kt < kt1) ? offAlo[j] + (unsigned)kt * (BK * 2) : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (LDS_PTR(void))(smem + OFF_ALO + sl * HALF_A + (w * 2 + j) * 1024), 16, v, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned v = (offB[j] != OOB && kt < kt1) ? offB[j] + (unsigned)kt * (BK * 2) : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsB, (LDS_PTR(void))(smem + OFF_B + sl * B_BYTES + (w * 4 + j) * 1024), 16, v, 0, 0, 0);
    }
  };
  auto dma_ahi = [&](int kt) {       // A_hi(kt): 2 pieces
    const int sl = (kt - kt0) & 1;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const unsigned v = (offAhi[j] != OOB && kt < kt1) ? offAhi[j] + (unsigned)kt * (BK * 2) : OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (LDS_PTR(void))(smem + OFF_AHI + sl * HALF_A + (w * 2 + j) * 1024), 16, v, 0, 0, 0);
    }
  };
  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  bf16x8 fa[2][4], fb[2][FN];    // [k-step][fragment]: ONE set (see tile 12)
  const int li = lane & 15, lg = lane >> 4;
  auto read_b = [&](int sl) {
    const char* tB = smem + OFF_B + sl * B_BYTES;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const unsigned b0 = lds_addr_of(tB) + kc_tile_off(wn * WTN + li, kk * 4 + lg);
      fb[kk][0] = ds_read_b128_raw<0>(b0); fb[kk][1] = ds_read_b128_raw<2048>(b0);
      fb[kk][2] = ds_read_b128_raw<4096>(b0); fb[kk][3] = ds_read_b128_raw<6144>(b0);
    }
  };
  auto read_a = [&](const char* tA) {   // the wave's four fragments of an A half: image rows wm * 64 + 16 f + li
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const unsigned a0 = lds_addr_of(tA) + kc_tile_off(wm * 64 + li, kk * 4 + lg);
      fa[kk][0] = ds_read_b128_raw<0>(a0); fa[kk][1] = ds_read_b128_raw<2048>(a0);
      fa[kk][2] = ds_read_b128_raw<4096>(a0); fa[kk][3] = ds_read_b128_raw<6144>(a0);
    }
  };
  auto tie_a = [&]() {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int i = 0; i < 4; ++i) lds_tie(fa[kk][i]);
  };
  auto tie_b = [&]() {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int j = 0; j < FN; ++j) lds_tie(fb[kk][j]);
  };
#define PN_FENCE() __builtin_amdgcn_sched_barrier(0)
#define PN_SYNC()                                                             \
  wait_vmcnt<8>();                                                            \
  PN_FENCE();                                                                 \
  __builtin_amdgcn_s_barrier();                                               \
  PN_FENCE();
#define PN_L_EVEN(KT)   /* B(KT) and A_lo(KT) into registers; request A_hi(KT + 1) */ \
  read_b(((KT) - kt0) & 1);                                                   \
  read_a(smem + OFF_ALO + (((KT) - kt0) & 1) * HALF_A);                       \
  PN_FENCE();                                                                 \
  dma_ahi((KT) + 1);                                                          \
  PN_FENCE();                                                                 \
  lds_wait_all();                                                             \
  tie_b(); tie_a();                                                           \
  PN_FENCE();
#define PN_L_ODD(KT)    /* A_hi(KT) into registers; request A_lo / B(KT + 2) */ \
  read_a(smem + OFF_AHI + (((KT) - kt0) & 1) * HALF_A);                       \
  PN_FENCE();                                                                 \
  dma_alo_b((KT) + 2);                                                        \
  PN_FENCE();                                                                 \
  lds_wait_all();                                                             \
  tie_a();                                                                    \
  PN_FENCE();
#define PN_M(I0)                                                              \
  __builtin_amdgcn_s_setprio(1);                                              \
  _Pragma("unroll") for (int kk_ = 0; kk_ < 2; ++kk_)                         \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                          \
      _Pragma("unroll") for (int j_ = 0; j_ < FN; ++j_)                       \
        acc[(I0) + i_][j_] = mfma16(fb[kk_][j_], fa[kk_][i_], acc[(I0) + i_][j_]); \
  __builtin_amdgcn_s_setprio(0);                                              \
  PN_FENCE();

  // prologue: the steady-state request order from its start — A_lo/B(0), A_hi(0), A_lo/B(1); interval 0 then asks for A_hi(1)
  dma_alo_b(kt0); dma_ahi(kt0); dma_alo_b(kt0 + 1);
  if (!g1) {
    for (int kt = kt0; kt < kt1; ++kt) {
      PN_SYNC()
      PN_L_EVEN(kt)
      PN_M(0)
      PN_SYNC()
      PN_L_ODD(kt)
      PN_M(4)
    }
  } else {
    PN_SYNC()
    PN_L_EVEN(kt0)
    for (int kt = kt0; kt < kt1; ++kt) {
      PN_SYNC()
      PN_M(0)
      PN_L_ODD(kt)
      if (kt + 1 < kt1) {
        PN_SYNC()
        PN_M(4)
        PN_L_EVEN(kt + 1)
      }
    }
    PN_M(4)
  }
  wait_vmcnt<0>();
  lds_wait_all();
#undef PN_M
#undef PN_L_ODD
#undef PN_L_EVEN
#undef PN_SYNC
#undef PN_FENCE

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

template <bool OUT_F32>
int launch_pn(const GemmParams& p, hipStream_t s) {
  return launch_256<512, staged_epilogue_lds(OUT_F32), 63, true, OUT_F32>([] { return gemm_pn_kernel<OUT_F32>; }, p, s);
}

template <bool A_KC, bool B_KC, bool OUT_F32>
int launch_pp16(const GemmParams& p, hipStream_t s) {   // four 32 KiB sub-tile slots
  return launch_256<1024, 4 * 2 * 256 * 32 * 2, 0, false, OUT_F32>([] { return gemm_pp16_kernel<A_KC, B_KC, OUT_F32>; }, p, s);
}

template <bool A_KC, bool B_KC, bool OUT_F32>
int launch_pp(const GemmParams& p, hipStream_t s) {     // eight 16 KiB half-tile slots
  return launch_256<512, 2 * (256 + 256) * 64 * 2, 0, false, OUT_F32>([] { return gemm_pp_kernel<A_KC, B_KC, OUT_F32>; }, p, s);
}
