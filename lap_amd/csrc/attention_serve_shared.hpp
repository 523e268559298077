// Shared-prefix few-query attention: the denoise step of N candidate action chunks of ONE observation (best-of-N flow sampling).
// The N candidates differ in their queries and fresh keys only; the cached prefix K / V exists ONCE ([Pn][kv_rs], no batch
// stride).  Included by attention.hip after attention_serve.hpp (shares its LDS layout, serve_runs and the combine kernels).
//
// The keys are cut into runs exactly as lap_attention_serve cuts them for batch N, and a (run, query tile, head, candidate) UNIT
// is computed with the arithmetic of attn_run_body<false> — same MFMA order, same softmax statistics, same scratch layout — so
// that attn_serve_combine_kernel merges the runs and the result is bit-equal to lap_attention_serve on a cache replicated N
// times.  What differs is who holds the K / V image of a run:
//   block   a prefix run's image (<= 128 rows x 512 B of K and of V, the ring's swizzle) is fetched ONCE by a block, which then
//           walks `upb` consecutive units of that run and kv head — unit u = (candidate, query tile, head of the kv head),
//           head fastest — instead of once per unit; a fresh-key run belongs to one candidate and its blocks walk that
//           candidate's (query tile, head) units.  `upb` is the smallest count with which the whole launch is <= 256 blocks
//           (shared_plan): LAP-3B at N = 8 (5 prefix runs of 112 keys + 1 fresh run, 4 query tiles, 8 heads) is 5 x 37 + 8 x 5 =
//           225 blocks of 7 units against 1536 blocks that fetch 1536 images.
//   loads   the DMA pieces of the image, the keys' info words of all N candidates and the query fragments of the block's first
//           two units are issued back to back before the one wait; the fragments of unit u + 2 are issued before unit u + 1 is
//           computed (one unit ahead: 8 KB that the L2 holds), so no later unit waits on HBM either.
//   LDS     SV_LDS (K image | V image | statistics | probabilities) + (N - 1) x 512 B of info words: <= 140,800 B.
// upb = 1 is the "simple form" (one unit per block, the grid of lap_attention_serve with a zero batch stride on the prefix): kept
// behind `form` for A/B measurements.
constexpr int SS_MAX_N = 8;
constexpr int SS_LDS = SV_LDS + (SS_MAX_N - 1) * SV_KEYS * 4;      // info words of candidates 1 .. N-1 behind the probabilities

struct SharedPlan { int upb, nb0, nb1, blocks; };      // units per block; blocks per (prefix run, kv head) / (fresh run, candidate, kv head)
// U0 = N x query tiles x heads per kv head units share a prefix run's image, U1 = query tiles x heads per kv head a fresh run's.
inline SharedPlan shared_plan(const ServeRuns& sr, int N, int QT, int HPK, int NKV, int form) {
  const int U0 = N * QT * HPK, U1 = QT * HPK;
  SharedPlan pl = {1, U0, U1, 0};
  for (int upb = 1;; ++upb) {
    pl.upb = upb;
    pl.nb0 = (U0 + upb - 1) / upb;
    pl.nb1 = (U1 + upb - 1) / upb;
    pl.blocks = NKV * (sr.nr0 * pl.nb0 + sr.nr1 * N * pl.nb1);
    if (form == 1 || pl.blocks <= 256 || upb >= U0) return pl;
  }
}

struct SharedQ { bf16x8 f[8]; int info; };

// The query fragments and the info word of lane's row of unit (n, qt, h); issued, not waited for.
__device__ __forceinline__ void shared_load_q(const AttnP& p, int n, int qt, int h, int lane, SharedQ& q) {
  const int Sq = p.qlen[1], myq = qt * 16 + (lane & 15);
  const bool vq = myq < Sq;
  load_row_frags<256>(p.q[1] + (n * (long long)Sq + myq) * p.q_rs[1] + h * 256, vq, lane, q.f);
  q.info = !vq ? 0 : (p.qinfo ? p.qinfo[(long long)n * Sq + myq] : 0x7fffffff);
}

// grid = (plan.blocks); p.B = N, p.k[0] / p.v[0] = the single prefix copy.
__global__ __launch_bounds__(512) void attn_serve_shared_kernel(AttnP p, ServeRuns sr, SharedPlan pl) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using C = DmaCfg<256>;
  constexpr int HD = 256, PITCH = C::PITCH, KS = C::KS;
  constexpr int KOFF = 0, VOFF = SV_KEYS * PITCH;
  int* sKw = reinterpret_cast<int*>(smem + 2 * SV_KEYS * PITCH);        // candidate 0's (or the fresh run's own) info words
  int* sKwN = reinterpret_cast<int*>(smem + SV_LDS) - SV_KEYS;          // candidate n >= 1 of a prefix run: sKwN + n * SV_KEYS
  const int tid = threadIdx.x;
  const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = lane & 15, g = lane >> 4;
  const int N = p.B, HPK = p.NH / p.NKV;
  const int Sq = p.qlen[1], Pn = p.klen[0], Sk = p.klen[1], Tk = Pn + Sk;
  const int QT = (Sq + 15) >> 4;

  // ---- which run, which kv head, which units (block uniform)
  int bid = blockIdx.x;
  const int per_hk = sr.nr0 * pl.nb0 + sr.nr1 * N * pl.nb1;
  const int hk = bid / per_hk;
  bid -= hk * per_hk;
  const bool fresh = bid >= sr.nr0 * pl.nb0;
  int run, cand = 0, chunk;
  if (!fresh) {
    run = bid / pl.nb0;
    chunk = bid - run * pl.nb0;
  } else {
    int r = bid - sr.nr0 * pl.nb0;
    chunk = r % pl.nb1; r /= pl.nb1;
    cand = r % N;
    run = sr.nr0 + r / N;
  }
  const int U = (fresh ? 1 : N) * QT * HPK;
  const int u0 = chunk * pl.upb, u1 = min(u0 + pl.upb, U);
  if (u0 >= u1) return;
  // unit u -> (candidate, query tile, head)
  auto unit = [&](int u, int& n, int& qt, int& h) {
    h = hk * HPK + u % HPK;
    qt = (u / HPK) % QT;
    n = fresh ? cand : u / (HPK * QT);
  };

  const int base = fresh ? (run - sr.nr0) * sr.rl1 : run * sr.rl0;           // the run's first row inside its segment
  const int nrows = min(fresh ? sr.rl1 : sr.rl0, (fresh ? Sk : Pn) - base);
  const int nt = (nrows + 15) >> 4, nt2 = (nt + 1) & ~1;

  // ---- the image: every DMA piece back to back (attn_run_body's; the prefix has NO batch stride)
  const int seg = fresh ? 1 : 0;
  const long long kvoff = (fresh ? (long long)cand * p.klen[1] * p.kv_rs[1] : 0ll) + hk * HD;
  const auto rsK = __builtin_amdgcn_make_buffer_rsrc((void*)(p.k[seg] + kvoff), 0, seg_records(p.klen[seg], p.kv_rs[seg], HD), 0x00020000);
  const auto rsV = __builtin_amdgcn_make_buffer_rsrc((void*)(p.v[seg] + kvoff), 0, seg_records(p.klen[seg], p.kv_rs[seg], HD), 0x00020000);
  const int rb = p.kv_rs[seg] * 2;
#pragma unroll
  for (int kv = 0; kv < 2; ++kv) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int pc = w * 8 + j;                       // wave uniform
      if (2 * pc >= nt2 * 16) continue;
      const int row = 2 * pc + (lane >> 5);
      const int col = ((lane & 31) ^ C::swz(row)) << 4;
      char* dst = smem + pc * 1024 + (kv ? VOFF : KOFF);
      const unsigned off = row < nrows ? (unsigned)((base + row) * rb + col) : DMA_OOB;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(kv ? rsV : rsK, (LDS_PTR(void))dst, 16, off, 0, 0, 0);
    }
  }
  // ---- the first two units' queries and the keys' info words of every candidate this block serves
  SharedQ qa, qb = {};
  int n, qt, h;
  unit(u0, n, qt, h);
  shared_load_q(p, n, qt, h, lane, qa);
  if (u0 + 1 < u1) {
    unit(u0 + 1, n, qt, h);
    shared_load_q(p, n, qt, h, lane, qb);
  }
  if (tid < SV_KEYS) {
    const int joint = tid < nrows ? (fresh ? Pn : 0) + base + tid : -1;       // index into a candidate's [prefix | fresh] key list
    const int c0 = fresh ? cand : 0;
    sKw[tid] = joint < 0 ? 0 : (p.kinfo ? p.kinfo[(long long)c0 * Tk + joint] : 0x7f000000);
    if (!fresh)
      for (int c = 1; c < N; ++c) sKwN[c * SV_KEYS + tid] = joint < 0 ? 0 : (p.kinfo ? p.kinfo[(long long)c * Tk + joint] : 0x7f000000);
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");

  float* sMax = reinterpret_cast<float*>(smem + SV_STAT);          // [8 waves][16 queries]
  float* sSum = sMax + 8 * 16;
  bf16x4* sP = reinterpret_cast<bf16x4*>(smem + SV_PROB);          // [8 key tiles][64 lanes]
  const char* kp[C::KREGS];
  unsigned va_unused[C::VREGS];
  dma_frag_bases<HD>(smem, lane, kp, va_unused);
  const float c2 = p.scale * LOG2E;
  const int tr_row = 4 * g + (i >> 2);
  const unsigned lane_swz = (unsigned)(C::swz(tr_row) ^ ((i & 3) >> 1));
  const unsigned lane_off = lds_addr_of(smem) + (unsigned)(VOFF + tr_row * PITCH + ((i & 1) << 3));

  for (int u = u0; u < u1; ++u) {
    unit(u, n, qt, h);
    const SharedQ qc = qa;
    qa = qb;
    if (u + 2 < u1) {           // one unit ahead (the compiler's own vmcnt waits cover it)
      int n2, qt2, h2;
      unit(u + 2, n2, qt2, h2);
      shared_load_q(p, n2, qt2, h2, lane, qb);
    }
    const int myq = qt * 16 + i;
    const bool vq = myq < Sq;
    const int qcls = qc.info >> 24, qidx = qc.info & 0xffffff;
    const int* kwp = (fresh || n == 0) ? sKw : sKwN + n * SV_KEYS;
    // ---- S^T = K Q^T: wave t owns key tile t of the run (attn_run_body, expression for expression)
    f32x4 sc = f32x4{0.f, 0.f, 0.f, 0.f};
    bool ok[4] = {false, false, false, false};
    float mx = NEG_BIG;
    if (w < nt) {
#pragma unroll
      for (int kk = 0; kk < KS; ++kk)
        sc = mfma16(*reinterpret_cast<const bf16x8*>(kp[kreg<HD>(kk)] + KOFF + w * 16 * PITCH + kimm<HD>(kk)), qc.f[kk], sc);
      const i32x4 kw = *reinterpret_cast<const i32x4*>(kwp + w * 16 + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        ok[r] = (qcls & (kw[r] >> 24)) != 0 && (kw[r] & 0xffffff) <= qidx;
        if (ok[r]) mx = fmaxf(mx, sc[r]);
      }
    }
    mx = max_over_groups(mx);
    if (g == 0) sMax[w * 16 + i] = mx;
    __syncthreads();
    float m = NEG_BIG;
#pragma unroll
    for (int t = 0; t < 8; ++t) m = fmaxf(m, sMax[t * 16 + i]);
    m *= c2;
    float lw = 0.f;
    bf16x4 pr;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e = ok[r] ? __builtin_amdgcn_exp2f(sc[r] * c2 - m) : 0.f;
      lw += e;
      pr[r] = f2bf(e);
    }
    lw = sum_over_groups(lw);
    if (g == 0) sSum[w * 16 + i] = lw;
    sP[w * 64 + lane] = pr;
    __syncthreads();
    float l = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) l += sSum[t * 16 + i];
    // ---- O^T = V^T P^T for this wave's two column fragments (columns 32 w .. 32 w + 31)
    f32x4 acc[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) acc[d] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (2 * c < nt) {
        const bf16x8 pb = join8(sP[(2 * c) * 64 + lane], sP[(2 * c + 1) * 64 + lane]);
#pragma unroll
        for (int d = 0; d < 2; ++d) {
          const unsigned a0 = lane_off + (((unsigned)(2 * (2 * w + d)) ^ lane_swz) << 4) + (unsigned)(c * 32 * PITCH);     // (LDS byte addresses)
          acc[d] = mfma16(join8(ds_read_tr_at(a0), ds_read_tr_at(a0 + 16 * PITCH)), pb, acc[d]);
        }
      }
    }
    if (vq) {
      const float inv = l > 0.f ? 1.0f / l : 0.f;
      const long long row = ((long long)run * p.B + n) * Sq + myq;
      float* op = p.part + (row * p.NH + h) * HD + w * 32;
#pragma unroll
      for (int d = 0; d < 2; ++d) *reinterpret_cast<f32x4*>(op + d * 16 + 4 * g) = acc[d] * inv;
      if (w == 0 && g == 0) p.lpart[(((long long)run * p.B + n) * p.NH + h) * Sq + myq] = l > 0.f ? (m + __builtin_amdgcn_logf(l)) * LN2 : NEG_BIG;
    }
    // (the next unit's sMax is written behind this unit's second barrier, its sSum / sP behind its own first one, which every
    //  wave reaches only after this unit's P.V reads: no third barrier)
  }
}

// form: 0 = resident image (<= 256 blocks), 1 = one unit per block.
int launch_serve_shared(const AttnP& p, int form, hipStream_t s) {
  const ServeRuns sr = serve_runs(p.klen[0], p.klen[1], p.nsplit);
  if (sr.nruns < 1 || sr.nruns > SV_MAX_RUNS || p.klen[1] < 0) return LAP_ERR_ARG;
  AttnP q = p;
  q.nsplit = sr.nruns;
  const SharedPlan pl = shared_plan(sr, p.B, (p.qlen[1] + 15) / 16, p.NH / p.NKV, p.NKV, form);
  static bool attr = false;
  if (!attr) {
    if (int e = set_lds(attn_serve_shared_kernel, SS_LDS)) return e;
    attr = true;
  }
  hipLaunchKernelGGL(attn_serve_shared_kernel, dim3(pl.blocks), dim3(512), SS_LDS, s, q, sr, pl);
  LAP_CHECK_LAUNCH();
  const long long n4 = (long long)p.B * p.qlen[1] * p.NH * 256 / 4;
  const dim3 grid((unsigned)((n4 + 255) / 256));
  if (sr.nruns <= 4) hipLaunchKernelGGL(attn_serve_combine_kernel<4>, grid, dim3(256), 0, s, q);
  else if (sr.nruns <= 8) hipLaunchKernelGGL(attn_serve_combine_kernel<8>, grid, dim3(256), 0, s, q);
  else hipLaunchKernelGGL(attn_serve_combine_kernel<16>, grid, dim3(256), 0, s, q);
  LAP_CHECK_LAUNCH();
  return LAP_OK;
}
