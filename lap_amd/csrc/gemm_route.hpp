// Route planner of lap_gemm_bf16_ex: which kernels a call launches, on which sub-products, decided on the host before anything is
// launched.  Plain C++17 with no HIP dependency (tests drive it through lap_gemm_plan on a machine without a GPU); pointers are looked
// at for null and alignment only, the environment is never read here (the switches arrive as a mask: route_switches_from_env in
// gemm.hip reads them once).  csrc/gemm.hip walks the legs of a plan and launches them in order on the caller's stream.
//
// A new routing rule is a clause of plan_call below; tests/test_gemm_route_cpu.py shows its effect on every recorded shape.
#pragma once
#include <stdint.h>

#include "../../include/lap_hip.h"

#ifndef LAP_ERR_ARG
#define LAP_OK 0
#define LAP_ERR_ARG 1001
#endif

namespace lap_route {

// Leg capacity of a plan.  The deepest composition the rules allow: the N cut makes two sub-products; each is at most an M cut
// (assembly leg + remainder) whose remainder is at most a tail split (full rounds + tail): 3 legs per sub-product, 6 in all.  (Today's
// thresholds stay below that: a remainder has fewer than 256 tiles and is never tail split, the 128-column part never reaches the
// assembly kernels; the longest recorded plan has 2 legs.)  A plan that would need more is rejected, never written.
constexpr int kMaxLegs = LAP_GEMM_MAX_LEGS;

struct Plan {
  int n = 0;
  lap_gemm_leg legs[kMaxLegs];
};

// One (sub-)product: the arguments of lap_gemm_bf16_ex with pointers as integers, and the element offsets of the sub-product inside
// the caller's buffers (what a leg records).
struct Call {
  uintptr_t A, B, C, bias, res;
  long long oa, ob, oc, obias, ores;
  int M, N, K, lda, ldb, ldc, ldr;
  float alpha;
  int a_kc, b_kc, flags, tile, ksplit;
  bool scratch;
  long long scratch_bytes;
  unsigned sw;   // LAP_ROUTE_* switches
};

// share of the last round's tile slots that hold a tile, when `tiles` tiles run in rounds of `per_round`
inline double round_fill(long long tiles, long long per_round = 256) {
  return (double)tiles / ((double)per_round * (double)((tiles + per_round - 1) / per_round));
}

// ---- eligibility of the assembly kernels (exported as lap_gemm_asm*_ok by csrc/gemm_asm.hip) ----
// kernel index of a (layout, output type) pair, or -1
inline int asm_variant(int a_kc, int b_kc, int out_f32) {
  if (a_kc && b_kc && !out_f32) return 0;
  if (a_kc && !b_kc && !out_f32) return 1;
  if (!a_kc && !b_kc && out_f32) return 2;
  if (!a_kc && !b_kc && !out_f32) return 11;      // weight gradient stored as bf16 (round 5)
  return -1;
}

inline int asm_ok(int a_kc, int b_kc, int out_f32, int M, int N, int K, int lda, int ldb, int ldc) {
  if (asm_variant(a_kc, b_kc, out_f32) < 0) return 0;
  if (M <= 0 || N <= 0 || K < 512 || (M & 255) || (N & 255) || (K & 127) || (lda & 7) || (ldb & 7) || (ldc & 7)) return 0;
  const long long ra = a_kc ? 255LL * lda * 2 + K * 2LL : (K - 1LL) * lda * 2 + 512;     // byte range of an operand panel
  const long long rb = b_kc ? 255LL * ldb * 2 + K * 2LL : (K - 1LL) * ldb * 2 + 512;
  const long long rc = 255LL * ldc * (out_f32 ? 4 : 2) + (out_f32 ? 1024 : 512);
  return ra < 0x7fffffffLL && rb < 0x7fffffffLL && rc < 0x7fffffffLL && (long long)(M / 256) * (N / 256) < (1 << 20);
}

// forward layout + f32 bias per output column, bf16 output; N any multiple of 16
inline int asm_bias_ok(int M, int N, int K, int lda, int ldb, int ldc) {
  if (M <= 0 || N < 512 || K < 512 || (M & 255) || (N & 15) || (K & 127) || (lda & 7) || (ldb & 7) || (ldc & 7)) return 0;
  return 255LL * lda * 2 + K * 2LL < 0x7fffffffLL && 255LL * ldb * 2 + K * 2LL < 0x7fffffffLL && 255LL * ldc * 2 + 512 < 0x7fffffffLL &&
         (long long)(M / 256) * ((N + 255) / 256) < (1 << 20);
}

inline int asm_res_ok(int biased, int M, int N, int K, int lda, int ldb, int ldc) {
  return biased ? asm_bias_ok(M, N, K, lda, ldb, ldc) : asm_ok(1, 1, 0, M, N, K, lda, ldb, ldc);
}

// Tile heuristic between the two production shapes (measured on MI355X, tools/bench_kernels.py):
//   tile 5 = 256x256, 16 waves, 1 block/CU  — 1.0-1.3 PF when its rounds over the 256 CUs are well filled;
//   tile 6 = 128x128,  8 waves, 2 blocks/CU — 0.9-1.0 PF, finer quantisation, better for short K / few tiles.
// score = round-fill efficiency x relative kernel efficiency (which grows with K for the big tile).
inline int pick_tile(int M, int N, int K) {
  const long long t5 = (long long)((M + 255) / 256) * ((N + 255) / 256);
  const long long t6 = (long long)((M + 127) / 128) * ((N + 127) / 128);
  const double fill5 = round_fill(t5);
  const double fill6 = round_fill(t6, 512);
  const double eff5 = 1.15 + 0.13 * (K >= 8192 ? 1.0 : K / 8192.0);
  if (t6 <= 256) return 6;  // not even one round of small tiles: finest granularity (+ split-K) wins
  return (fill5 * eff5 > fill6) ? 5 : 6;
}

// Automatic two-phase split-K (only when the caller lends scratch): fills the last round of a poorly filled
// 256x256 grid, or spreads a GEMM with a handful of output tiles (skinny-M serving, small weights) over the chip.
inline int pick_ksplit(int tile, int M, int N, int K, long long scratch_bytes, bool fwd_layout) {
  const long long cap = scratch_bytes / ((long long)M * N * 4);
  if (cap < 2) return 1;
  if (tile == 5 || tile == 8) {
    const long long t5 = (long long)((M + 255) / 256) * ((N + 255) / 256);
    const double fill1 = round_fill(t5);
    if (fill1 >= 0.8 || K < 4096) return 1;
    int best = 1;
    double score = fill1;
    for (int sp = 2; sp <= 4 && sp <= cap; ++sp) {
      const double sc = round_fill(t5 * sp) - 0.02 * sp;
      if (sc > score) { score = sc; best = sp; }
    }
    return best;
  }
  if (tile == 6 || tile == 0) {
    const long long t6 = (long long)((M + 127) / 128) * ((N + 127) / 128);
    // windows tuned per regime (tools/gemm_sweep.py): the serving prefill (forward layout, M <= 1024) splits up to 256
    // tiles; the train step's action-expert GEMMs (M = 1600: 104 tiles walking K = 2048 .. 8192) up to 128
    const bool serving = fwd_layout && M <= 1024;
    if (t6 > (serving ? 256 : 128) || K < 1024) return 1;
    // Few tiles (serving prefill at M ~ 512, small weights): a 128x128 block that walks all of K loads 512 * K bytes through
    // ONE CU's vector-memory path (~45 GB/s, tools/bench_skinny.py) — 22 us at K = 2048 whatever the MFMA rate.  Splitting K
    // until the chip holds two blocks per CU shortens that chain; the reduce pass costs ~5 us + the slab traffic.
    long long sp = (t6 > 96 ? 512 : 256) / t6;
    if (sp > K / 256) sp = K / 256;
    if (!serving && t6 > 96 && sp > K / 1024) sp = K / 1024;
    if (sp > 16) sp = 16;
    if (sp > cap) sp = cap;
    return sp < 2 ? 1 : (int)sp;
  }
  return 1;
}

// Serving prefill (batch-1 action chunk: 512 SigLIP rows, 560 Gemma rows; forward layout, bf16 out).  Every block of such
// a GEMM is bound by what it pulls through its CU's vector-memory path (~45 GB/s), so the tile is the one with the fewest
// operand bytes per block that still covers the chip WITHOUT a split-K reduce pass behind it (tools/bench_prefill_gemm.py,
// hipGraph-timed, automatic choice -> here): SigLIP qkv 22.8 -> 12.5 us, out 14.7 -> 10.1, fc1 24.5 -> 16.8, head 19.3 ->
// 10.1; Gemma qkv 22.2 -> 17.1, out 18.2 -> 17.4, gate|up 90.8 -> 74.2 (a 320-row tile: 560 rows are 2 x 280, not 3 x 256).
// Long contractions (SigLIP fc2, Gemma down: K >= 4096) keep their K split.  LAP_ROUTE_NO_SERVING_TILES: off (A/B).
// Returns the tile, or -1 where the generic choice stands.
inline int pick_serving_tile(int M, int N, int K, bool f32) {
  if (K <= 1536 && N >= 1024) return N >= 3072 ? 16 : 17;     // (also the f32 hi / lo stem products)
  if (f32) return -1;
  if (K <= 2560 && N >= 8192 && M > 512 && M <= 640) return 15;
  if (K <= 2560 && N >= 2048 && N < 8192) return 16;
  return -1;
}

// Tail split (256x256 kernel, automatic split only): the full rounds of 256 tiles run unsplit; only the tiles of
// the last, poorly filled round are split along K so that they fill the chip for 1/sp of a round.
// Returns the tail's tiles (0: no tail split) and in *tail_sp its K split (1: the tail as quadrants on the 128x128 kernel).
inline int pick_tail_split(int M, int N, int K, long long scratch_bytes, int* tail_sp) {
  const long long t5 = (long long)((M + 255) / 256) * ((N + 255) / 256);
  const int tail = (int)(t5 % 256), nkt = (K + 63) / 64;
  *tail_sp = 0;
  if (!(t5 > 256 && tail > 0 && tail < 200)) return 0;
  // Cost model (microseconds, calibrated on in-situ traces): a tile costs ~6 + 1.9 per 64-deep k-tile; splitting the
  // tail sp ways shortens that to nkt / sp k-tiles but adds a reduce pass over sp f32 slabs + the output
  // (~25 us of launch + latency + bytes at ~2.5 TB/s).  Short contractions (K <= 2048) are cheaper unsplit
  // (measured: tools/bench_tail.py).
  int smax = 256 / tail;
  if (smax > 8) smax = 8;
  const long long cap = scratch_bytes / ((long long)tail * 65536 * 4);
  if (smax > cap) smax = (int)cap;
  const double whole = 6.0 + 1.9 * nkt;
  double best = whole;
  int sp = 1;
  for (int c = 2; c <= smax; ++c) {
    const double cost = 6.0 + 1.9 * ((nkt + c - 1) / c) + 25.0 + (double)tail * 65536.0 * (4.0 * c + 2.0) / 2.5e6;
    if (cost < best - 4.0) { best = cost; sp = c; }   // (a split has to pay for its extra launch clearly)
  }
  // third option, for short contractions: the tail as 4 x tail quadrants on the 128x128 kernel (one round of it when
  // tail <= 128), modelled as 0.64 of a 256x256 tile time + its launch.  Measured gain is small: 4-9 us per GEMM
  // isolated (tools/bench_tail.py), 345.0 -> 344.1 ms per train step in an interleaved A/B (within noise)
  if (tail <= 128 && 0.64 * whole + 6.0 < best - 4.0) { *tail_sp = 1; return tail; }
  if (sp >= 2) { *tail_sp = sp; return tail; }
  return 0;
}

// the sub-product of `c` that starts m0 rows and n0 columns in (tile and split chosen afresh, as for a call of its own)
inline Call sub_call(const Call& c, int m0, int n0, int M, int N) {
  Call s = c;
  const long long esz = (c.flags & LAP_GEMM_OUT_F32) ? 4 : 2, bsz = (c.flags & LAP_GEMM_BIAS_F32) ? 4 : 2;
  const long long da = c.a_kc ? (long long)m0 * c.lda : m0, db = c.b_kc ? (long long)n0 * c.ldb : n0;
  const long long dc = (long long)m0 * c.ldc + n0, dr = (long long)m0 * c.ldr + n0;
  s.A += da * 2; s.oa += da;
  s.B += db * 2; s.ob += db;
  s.C += dc * esz; s.oc += dc;
  if (c.bias) { s.bias += n0 * bsz; s.obias += n0; }
  if (c.res) { s.res += dr * 2; s.ores += dr; }
  s.M = M; s.N = N; s.tile = -1; s.ksplit = 0;
  s.sw &= ~(unsigned)LAP_ROUTE_WGRAD_SUMSQ;
  return s;
}

inline int push_leg(Plan& plan, const Call& c, int engine, lap_gemm_leg** out = nullptr) {
  if (plan.n >= kMaxLegs) return LAP_ERR_ARG;
  lap_gemm_leg& l = plan.legs[plan.n++];
  l = lap_gemm_leg{};
  l.off_a = c.oa; l.off_b = c.ob; l.off_c = c.oc; l.off_bias = c.obias; l.off_res = c.ores;
  l.engine = engine; l.M = c.M; l.N = c.N; l.ksplit = 1;
  if (out) *out = &l;
  return LAP_OK;
}

// Appends the legs of one (sub-)product to `plan`, or returns the code lap_gemm_bf16_ex rejects it with.
inline int plan_call(const Call& c, Plan& plan) {
  const int M = c.M, N = c.N, K = c.K, lda = c.lda, ldb = c.ldb, ldc = c.ldc, ldr = c.ldr, a_kc = c.a_kc, b_kc = c.b_kc, flags = c.flags;
  const uintptr_t bias = c.bias, residual = c.res;
  const float alpha = c.alpha;
  const bool scratch = c.scratch;
  const long long scratch_bytes = c.scratch_bytes;
  const auto off = [&](unsigned bit) { return (c.sw & bit) != 0; };
  int tile = c.tile, ksplit = c.ksplit;
  const bool f32 = flags & LAP_GEMM_OUT_F32;
  const bool no_asm = off(LAP_ROUTE_NO_ASM);
  // A weight gradient whose caller wants its sum of squares (lap_gemm_wgrad_*): folded into the assembly kernel's epilogue where
  // that kernel takes the product by the plain-product rule below; every other shape is planned like any call.
  if (off(LAP_ROUTE_WGRAD_SUMSQ) && !no_asm && M > 0 && N > 0 && asm_ok(0, 0, f32, M, N, K, lda, ldb, ldc)) {
    const long long t5 = (long long)(M / 256) * (N / 256);
    if (t5 >= 128 && round_fill(t5) >= 0.8) return push_leg(plan, c, LAP_LEG_ASM_WGRAD_SUMSQ);
  }
  if (M <= 0 || N <= 0 || K <= 0) return LAP_ERR_ARG;
  // 16-byte chunk granularity along each contiguous axis; 4-wide epilogue stores.
  if ((N & 3) || (ldc & 3) || (lda & 7) || (ldb & 7)) return LAP_ERR_ARG;
  if (a_kc ? (K & 7) : (M & 7)) return LAP_ERR_ARG;
  if (b_kc ? (K & 7) : (N & 7)) return LAP_ERR_ARG;
  if (residual && (ldr & 3)) return LAP_ERR_ARG;
  if ((c.A | c.B | c.C) & 15) return LAP_ERR_ARG;
  // 31-bit byte offsets inside one buffer descriptor.
  if ((long long)(a_kc ? M : K) * lda * 2 >= 0x7fffffffLL) return LAP_ERR_ARG;
  if ((long long)(b_kc ? N : K) * ldb * 2 >= 0x7fffffffLL) return LAP_ERR_ARG;
  if ((flags & LAP_GEMM_ACCUM) && !f32) return LAP_ERR_ARG;
  if ((flags & LAP_GEMM_GELU) && f32) return LAP_ERR_ARG;
  if (tile < -1 || tile > 19 || ksplit < 0) return LAP_ERR_ARG;
  if (flags & LAP_GEMM_GEGLU) {   // gate|up projection + GeGLU in one launch (serving prefill): the 320-row tile only
    if (!a_kc || !b_kc || f32 || bias || residual || (flags & ~(LAP_GEMM_GEGLU | LAP_GEMM_GELU_EXP2)) || (N & 255) || M > 640 || alpha != 1.0f || ksplit > 1 || (tile >= 0 && tile != 15))
      return LAP_ERR_ARG;
    tile = 15; ksplit = 1;
  }
  // Few output tiles but a very long contraction (LM-head dgrad: 1504 x 2048 over K = 257152; prefill down
  // projection): the big tile with enough K splits to cover the chip beats the small tile walking all of K.
  if (tile < 0 && ksplit == 0 && scratch && K >= 16384 && !(flags & LAP_GEMM_PARTIALS)) {
    const long long t5 = (long long)((M + 255) / 256) * ((N + 255) / 256);
    if (t5 <= 128) {
      long long sp = 256 / t5;
      const long long cap = scratch_bytes / ((long long)M * N * 4);
      if (sp > 8) sp = 8;
      if (sp > (K + 63) / 64 / 16) sp = (K + 63) / 64 / 16;
      if (sp > cap) sp = cap;
      if (sp >= 2) { tile = 5; ksplit = (int)sp; }
    }
  }
  // Plain products over whole 256-tiles (no bias / residual / GELU / accumulate / split): the hand-scheduled assembly main
  // loop (csrc/gemm_asm_kernels.s: forward bf16, data-gradient bf16, weight-gradient f32 layouts; same accumulation order,
  // bitwise equal) whenever its persistent rounds are well filled, or the contraction is too short for the tail split
  // below to pay.  tile 14 forces it (tests); LAP_ROUTE_NO_ASM disables it (A/B runs).
  {
    const bool no_extras = !(flags & (LAP_GEMM_GELU | LAP_GEMM_ACCUM | LAP_GEMM_PARTIALS)) && alpha == 1.0f;
    const bool plain = !bias && !residual && no_extras && ksplit <= 1 && asm_ok(a_kc, b_kc, f32, M, N, K, lda, ldb, ldc);
    // forward + f32 bias per column (Flax Dense of SigLIP: qkv, fc1), N any multiple of 16
    const bool biased = a_kc && b_kc && !f32 && bias && (flags & LAP_GEMM_BIAS_F32) && !residual && no_extras && ksplit <= 1 &&
                        asm_bias_ok(M, N, K, lda, ldb, ldc) && !(bias & 15);
    // forward + bf16 residual with C's leading dimension (+ optional f32 bias): out / down projections of a block
    const bool resid = a_kc && b_kc && !f32 && residual && ldr == ldc && !(residual & 15) &&
                       (!bias || ((flags & LAP_GEMM_BIAS_F32) && !(bias & 15))) && no_extras && ksplit <= 1 &&
                       asm_res_ok(bias != 0, M, N, K, lda, ldb, ldc);
    if (tile == 14 && resid) return push_leg(plan, c, LAP_LEG_ASM_RES);
    if (tile < 0 && resid && !no_asm) {
      const bool no_res = off(LAP_ROUTE_NO_ASM_RES);      // A/B switch
      const long long tm = M / 256, tn = (N + 255) / 256, t5 = tm * tn, rounds = t5 / 256;
      const double fill = round_fill(t5);
      if (!no_res && t5 >= 128 && (fill >= 0.8 || (bias && K <= 2048))) return push_leg(plan, c, LAP_LEG_ASM_RES);
      // (the M cut of the plain products below, with the residual rows following the cut; LAP_ROUTE_NO_MSPLIT_LONGK: A/B switch,
      // see the plain products below)
      if (!no_res && !off(LAP_ROUTE_NO_MSPLIT) && !bias && ksplit == 0 && scratch && (K <= 4096 || !off(LAP_ROUTE_NO_MSPLIT_LONGK)) && rounds >= 1 &&
          fill < 0.8 && (rounds * 256) % tn == 0) {
        const int M0 = (int)(rounds * 256 / tn) * 256;
        if (int rc = push_leg(plan, sub_call(c, 0, 0, M0, N), LAP_LEG_ASM_RES)) return rc;
        return plan_call(sub_call(c, M0, 0, M - M0, N), plan);
      }
    }
    if (tile == 14 && biased) return push_leg(plan, c, LAP_LEG_ASM_BIAS);
    if (tile < 0 && biased && !no_asm) {
      const long long t5 = (long long)(M / 256) * ((N + 255) / 256);
      if (t5 >= 128 && round_fill(t5) >= 0.8) return push_leg(plan, c, LAP_LEG_ASM_BIAS);
    }
    if (tile == 14) return plain ? push_leg(plan, c, LAP_LEG_ASM) : LAP_ERR_ARG;
    // M = 17,920 rows x N = 2,048 columns are 70 x 8 = 560 tiles: 2.19 rounds of the chip.  The persistent kernel would run a
    // third round for 48 tiles; the HIP tile splits those 48 along K.  Same cut here, made along M: rows [0, 64 x 256) are
    // exactly two rounds for the assembly kernel, the last 1,536 rows a product of their own on the automatic route (its
    // K split covers the chip).  tools/bench_msplit.py (isolated, us): qkv data gradient K = 2560 195 -> 152, out data gradient
    // K = 2048 161 -> 124, plain forward K = 2048 129 -> 121.  LAP_ROUTE_NO_MSPLIT: off (A/B).
    // Long contractions with a K-contiguous A (gate|up data gradient K = 32768, down forward + residual K = 16384; the engine pads
    // A's rows off the 16 KiB stride): isolated the cut is a wash (1726 vs 1762 us, 922 vs 949 us: the last 1536 rows cost 181 /
    // 100 us on the HIP tile's K split either way), in the train step it is worth 2.8 ms (302.0 -> 299.2 ms, interleaved on
    // one box) — the assembly kernel's two rounds leave the optimizer stream more of the chip than the HIP tile's.
    // LAP_ROUTE_NO_MSPLIT_LONGK: off (A/B).
    if (tile < 0 && plain && !no_asm && ksplit == 0 && scratch && (K <= 4096 || (!off(LAP_ROUTE_NO_MSPLIT_LONGK) && a_kc))) {
      const long long tm = M / 256, tn = N / 256, t5 = tm * tn, rounds = t5 / 256;
      if (!off(LAP_ROUTE_NO_MSPLIT) && rounds >= 1 && round_fill(t5) < 0.8 && (rounds * 256) % tn == 0) {
        const int M0 = (int)(rounds * 256 / tn) * 256;
        if (int rc = push_leg(plan, sub_call(c, 0, 0, M0, N), LAP_LEG_ASM)) return rc;
        return plan_call(sub_call(c, M0, 0, M - M0, N), plan);
      }
    }
    // Ragged M with very many rows (the embedding table's weight gradient: 257,152 = 1004.5 x 256 rows): the whole m-tiles on the
    // assembly kernel, the last M % 256 rows as a product of their own (weight-gradient layout only: A's tail is a column offset)
    if (tile < 0 && !no_asm && !a_kc && !b_kc && f32 && (M & 255) && M >= 65536 && !bias && !residual && no_extras && ksplit == 0) {
      const int M0 = M & ~255;
      if (asm_ok(0, 0, 1, M0, N, K, lda, ldb, ldc)) {
        if (int rc = push_leg(plan, sub_call(c, 0, 0, M0, N), LAP_LEG_ASM)) return rc;
        return plan_call(sub_call(c, M0, 0, M - M0, N), plan);
      }
    }
    if (tile < 0 && plain && !no_asm) {
      const long long t5 = (long long)(M / 256) * (N / 256);
      const double fill = round_fill(t5);
      // measured against the HIP tiles (tools/bench_asm_gemm.py bench): forward +10-17 % whenever the rounds are filled or the
      // contraction is short; weight gradient +10 % (tall outputs run as the wide product of the swapped operands with
      // transposed stores, see lap_gemm_asm); data gradient: 0 .. +14 % on short contractions with filled rounds (the
      // ping-pong tile's rate on a weight with 32 KiB rows varies from box to box), long ones keep the tail split
      const bool win = (a_kc && b_kc) ? (fill >= 0.8 || K <= 4096) : (!a_kc && !b_kc) ? fill >= 0.8 : (fill >= 0.8 && K <= 4096 && !off(LAP_ROUTE_NO_ASM_NN));
      if (t5 >= 128 && win) return push_leg(plan, c, LAP_LEG_ASM);
    }
  }
  // N = 256 j + 128 with many rows (SigLIP's width 1152 at B x 512 rows: out / fc2 forward, qkv / fc1 data gradients): the 256-wide
  // tiling needs j + 1 column tiles of which the last is half empty, e.g. 64 x 4.5 -> 320 tile slots = two rounds of the chip for
  // 1.13 rounds of work.  Cut the product along N instead: columns [0, 256 j) are whole tiles (64 x 4 = exactly one round at
  // B = 32, and a plain / bias-only product of that shape is eligible for the assembly kernels), the last 128 columns a second,
  // small product on the 128 x 128 tile (with its automatic K split: those 128 columns see another f32 summation order,
  // everything else keeps its bits).
  // tools/bench_nsplit.py (isolated, us): fc2 forward K = 4304 240 -> 200, qkv data gradient K = 3456 141 -> 122, fc1 data gradient
  // K = 4304 172 -> 159; K = 1152 (out projection) loses 4 us to the second launch, so short contractions stay whole.  The tail
  // product re-reads all of A for 128 columns, which is what keeps the gain below the 1.5 / 2 rounds it removes.
  // LAP_ROUTE_NO_NSPLIT: off (A/B).
  if (tile < 0 && ksplit == 0 && (N & 255) == 128 && N >= 640 && N <= 2048 + 128 && M >= 4096 && K >= 2048 && !(flags & LAP_GEMM_PARTIALS)) {
    const long long tm = (M + 255) / 256, t_all = tm * (N / 256 + 1), t_whole = tm * (N / 256);
    if (!off(LAP_ROUTE_NO_NSPLIT) && round_fill(t_all) < 0.8 && round_fill(t_whole) >= 0.9) {
      if (int rc = plan_call(sub_call(c, 0, 0, M, N - 128), plan)) return rc;
      return plan_call(sub_call(c, 0, N - 128, M, 128), plan);
    }
  }
  if (tile < 0 && ksplit == 0 && a_kc && b_kc && M > 256 && M <= 768 && !(flags & LAP_GEMM_PARTIALS) && (f32 || !(flags & LAP_GEMM_ACCUM)) &&
      !off(LAP_ROUTE_NO_SERVING_TILES)) {
    const int t = pick_serving_tile(M, N, K, f32);
    if (t >= 0) { tile = t; ksplit = 1; }
  }
  if (tile < 0) tile = pick_tile(M, N, K);
  int tail_tiles = 0, tail_sp = 0;
  if (ksplit == 0 && scratch && tile == 5 && !(flags & LAP_GEMM_PARTIALS)) tail_tiles = pick_tail_split(M, N, K, scratch_bytes, &tail_sp);
  if (ksplit == 0 && scratch && !tail_tiles) ksplit = pick_ksplit(tile, M, N, K, scratch_bytes, a_kc && b_kc);
  // K % 8 == 0: the software-pipelined 8-wave kernel (tile 10) for the forward layout, the ping-pong kernel (tile 12) as
  // soon as an operand is M-contiguous (data / weight gradients: +5-11 % measured, tools/bench_kernels.py; on the forward
  // layout its 64-byte k-half rows cost more in LDS-DMA requests than the ping-pong gains); else the 16-wave kernel.
  // LAP_ROUTE_NO_PINGPONG: A/B switch for benchmarks; LAP_ROUTE_NO_KTAIL: A/B switch, ragged K back on the lockstep tile
  const int big = (!(K & 7) && (!(K & 63) || !off(LAP_ROUTE_NO_KTAIL))) ? ((a_kc && b_kc) || off(LAP_ROUTE_NO_PINGPONG) ? 10 : 12) : 5;
  if (tile == 5) tile = big;
  const bool two_phase = ksplit > 1 && scratch;
  if (two_phase && scratch_bytes < (long long)ksplit * M * N * 4) return LAP_ERR_ARG;
  if (ksplit > 1 && !two_phase && (!f32 || !(flags & LAP_GEMM_ACCUM) || bias || residual)) return LAP_ERR_ARG;
  if ((flags & LAP_GEMM_PARTIALS) && (!scratch || ksplit < 1 || scratch_bytes < (long long)(ksplit > 1 ? ksplit : 1) * M * N * 4)) return LAP_ERR_ARG;
  // what the tile launchers reject (csrc/gemm.hip dispatch_tile, launch_sp / launch_pq)
  if (tile >= 15 && !(a_kc && b_kc)) return LAP_ERR_ARG;
  if ((tile >= 10 && tile <= 13) && (K & 7)) return LAP_ERR_ARG;
#ifndef LAP_GEMM_EXPERIMENTAL
  if (tile == 13 || tile == 11 || tile == 9 || tile == 8 || tile == 7 || tile == 4 || tile == 3 || tile == 1) return LAP_ERR_ARG;   // not in this build
#endif
  lap_gemm_leg* l;
  if (tail_tiles) {
    const int t5 = ((M + 255) / 256) * ((N + 255) / 256);
    // (a) the full rounds, straight to C
    if (int rc = push_leg(plan, c, big, &l)) return rc;
    l->f32_tile = f32; l->tile_count = t5 - tail_tiles;
    if (int rc = push_leg(plan, c, tail_sp == 1 ? 6 : big, &l)) return rc;
    l->tile_base = t5 - tail_tiles; l->tile_count = tail_tiles;
    if (tail_sp == 1) {   // (b') the tail tiles as quadrants on the 128x128 kernel, straight to C with the caller's epilogue
      l->f32_tile = f32; l->sub256 = 1;
    } else {              // (b) the tail tiles, split along K into compact f32 slabs, then reduce + epilogue
      l->f32_tile = 1; l->ksplit = tail_sp; l->part = 1; l->part_compact = 1; l->reduce = LAP_LEG_REDUCE_TAIL;
    }
    return LAP_OK;
  }
  if (int rc = push_leg(plan, c, tile, &l)) return rc;
  l->ksplit = ksplit > 1 ? ksplit : 1;
  l->part = two_phase || (flags & LAP_GEMM_PARTIALS);
  l->f32_tile = l->part ? 1 : (int)f32;
  l->reduce = (two_phase && !(flags & LAP_GEMM_PARTIALS)) ? LAP_LEG_REDUCE_SPLITK : LAP_LEG_REDUCE_NONE;
  return LAP_OK;
}

}  // namespace lap_route
