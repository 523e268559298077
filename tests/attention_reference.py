"""Float64 references, element bounds, float32 restatements and seeded inputs for the training attention kernels
(csrc/attention.hip, csrc/attention_dma.hpp), shared by tests/test_attention_reference_gpu.py (device against reference) and
tests/test_attention_reference_cpu.py (the criteria against float32 restatements and corrupted references).  Plain torch on the
CPU; nothing here calls lap_amd.hip.

Tensors are joint over the two segments: q / o / dO [B, Tq, NH, HD], k / v [B, Tk, NKV, HD], lse [B, NH, Tq], allowed [B, Tq, Tk].

Bounds (u = 2^-24; every term is a rounding of a stated format carried to the output through its gain, as decode_reference._rnd):
 * logit.  s = scale q.k is a float32 MFMA chain: |s_dev - s| <= DEPTH u L, L = scale sum_d |q||k|.  The exponent's argument
   (s - m, s c2 - lse2: one multiply or fma each) adds 4 u (|s| + |m| + 8) (the DMA forward lets its maximum lag by 2^8) or
   4 u (|s| + |lse|).  Both enter p as a relative error eps_ij; the fast exponential adds INTR (below).
 * forward.  The device's numerator sums bf16(p) v, its denominator the unrounded p, against one running maximum per tile; half a
   bf16 spacing is at most 2^-8 relative whatever that maximum is.  So |o_dev - o64| <= (2^-8 (1 + w) + w) A + one bf16 spacing
   of o, A = sum_j p_ij |v_jd|, w = expm1(2 E + 2 acc u), E = max_j eps_ij, acc = the number of float32 additions of the row.
   lse: E + acc u + INTR + 8 u (|lse| + max |s| + 32).  A key split adds one more lse bound and two INTR to w (the partials'
   weights exp(lse_i - max)) and 2 INTR + 8 u (..) to lse (log-sum-exp is 1-Lipschitz in the partial lse).
 * backward.  P = exp(s - lse) carries eps_ij; bf16(P) then differs by that plus one spacing (_rnd).  dS = bf16(P (dP - delta)
   scale): the float32 dP and delta are off by DEPTH u sum_d |dO||v| and DEPTH u sum_d |dO||o|.  dV, dK, dQ sum these
   element bounds against |dO|, |q|, |k|, add acc u of the absolute sum and round once more.
There is no "differing share" criterion as for the decode projections: the bf16 rounding of P in the forward depends on the
running maximum at that tile, which depends on the tile order, which differs between the kernel families (64-key tiles, 32-key
tiles, a lagging maximum, key splits).  No bit-exact rounded reference exists, so sensitivity to low-weight errors comes from the
exact cases (q = 0: every allowed key weighs the same and p is exact in bf16) instead."""
import itertools
import math
import zlib
from collections import namedtuple

import torch

from tests.decode_reference import _rnd, bf16r, check_elementwise, count_separated, ulp_bf16, worst_ratio  # noqa: F401 (re-exported)

U24 = 2.0 ** -24
# Depth of the float32 summation trees over d: 8 chained v_mfma_f32_16x16x32_bf16 of 32 products each (HD 256; the order inside
# one MFMA is not documented, so it is taken as sequential: 256), the multiply by scale, and the 64 sequential fmas plus two swaps
# of the fused delta, rounded up.
DEPTH = 272
LSE_EMPTY = 1.0e30          # attention.hip: lse of a row with no allowed key, checked for equality
LSE_EMPTY32 = float(torch.tensor(LSE_EMPTY, dtype=torch.float32))       # the float32 the kernels store, as a float64
# Worst relative error of torch's float32 exp against float64 on the same float32 argument over every case below and the three
# tile orders (tests/test_attention_reference_cpu.py measures it again and asserts it is no larger).  The device's v_exp_f32 /
# v_log_f32 are 1 ulp instructions; INTR gives them 4 x the restatement's error, capped so that it can never hide a dropped key.
F32_EXP_ERR = 6.2e-8           # measured: 6.148e-08
INTR = min(4.0 * F32_EXP_ERR, 2.0 ** -18)


def acc_depth(n):
    """Float32 roundings behind a sum of n products that arrives in tiles of 32: the n additions taken as sequential, a rescale
    and a cross-lane step per tile, and 16 for what follows the loop: the 2 cross-lane steps of the final sum, 1 / l and the
    product with it, up to 4 head-split partials (hsplit <= 4) and up to 8 key-split shares in the combine kernel (the cases
    here use at most 3)."""
    return n + 2 * ((n + 31) // 32) + (2 + 2 + 4 + 8)


def mask_ok(qinfo, kinfo):
    """allowed [B, Tq, Tk] of the kernels' mask_ok: (class(q) & class(k)) != 0 && idx(k) <= idx(q); int32 >> is arithmetic."""
    qc, kc = qinfo >> 24, kinfo >> 24
    return ((qc[:, :, None] & kc[:, None, :]) != 0) & ((kinfo & 0xFFFFFF)[:, None, :] <= (qinfo & 0xFFFFFF)[:, :, None])


def _heads(k, NH):
    return k.repeat_interleave(NH // k.shape[2], dim=2)


# ------------------------------------------------------------------------------------------------ float64 references
def fwd_reference(q, k, v, allowed, scale, split=False):
    """lap_attention_fwd in float64.  Returns a dict: o, lse, A = sum_j p |v|, L = scale sum_d |q||k| (the logit sensitivity),
    s, p, and the element bounds o_bound (against bf16(o) = o16) / lse_bound.  Masked keys may hold anything finite."""
    B, Tq, NH, _ = q.shape
    q, kk, vv = q.double(), _heads(k.double(), NH), _heads(v.double(), NH)
    ok = torch.ones(B, 1, Tq, kk.shape[1], dtype=torch.bool) if allowed is None else allowed[:, None]
    s = scale * torch.einsum("bihd,bjhd->bhij", q, kk)
    L = abs(scale) * torch.einsum("bihd,bjhd->bhij", q.abs(), kk.abs())
    s = s.masked_fill(~ok, float("-inf"))
    m = s.amax(-1, keepdim=True)
    empty = torch.isinf(m)                                        # [B, NH, Tq, 1]
    e = torch.where(ok, torch.exp(s - m.masked_fill(empty, 0.0)), torch.zeros_like(s))
    l = e.sum(-1, keepdim=True)
    p = e / l.masked_fill(empty, 1.0)
    lse = torch.where(empty, torch.full_like(m, LSE_EMPTY), m + torch.log(l.masked_fill(empty, 1.0)))[..., 0]
    o = torch.einsum("bhij,bjhd->bihd", p, vv)
    A = torch.einsum("bhij,bjhd->bihd", p, vv.abs())
    sa = torch.where(ok, s.abs(), torch.zeros_like(s))
    smax = sa.amax(-1)                                            # [B, NH, Tq]
    eps = torch.where(ok, U24 * (DEPTH * L + 4.0 * (sa + smax[..., None] + 8.0)) + INTR, torch.zeros_like(s))
    E = eps.amax(-1)
    nk = int(ok.sum(-1).max())
    # lse = (m + log2 l) ln2 with m = s c2: 8 bounds the roundings on the way (c2 and ln2 as float32 constants, the two products,
    # the sum, and the 1 ulp = 2 u of v_log_f32: 7), each relative to a quantity of at most |lse| + max |s| + |log2 l|, and
    # |log2 l| <= 8 (the DMA forward's lagging maximum) + log2(keys) < 8 + 24 = 32 for any key count a 24-bit index can hold
    misc = INTR + 8.0 * U24 * (lse.abs().masked_fill(empty[..., 0], 0.0) + smax + 32.0)
    lse_bound = E + acc_depth(nk) * U24 + misc
    w = 2.0 * E + 2.0 * acc_depth(nk) * U24
    if split:
        w = w + 2.0 * lse_bound + 2.0 * INTR
        lse_bound = lse_bound + INTR + misc
    w = torch.expm1(w).transpose(1, 2)[..., None]                 # [B, Tq, NH, 1]
    o16, o_bound = _rnd(o, (2.0 ** -8 * (1.0 + w) + w) * A + 2.0 ** -126 * nk * vv.abs().amax())
    return dict(o=o, o16=o16, lse=lse, A=A, L=L, s=s, p=p, ok=ok, empty=empty[..., 0], o_bound=o_bound,
                lse_bound=lse_bound.masked_fill(empty[..., 0], 0.0))


def stop_weight(Tq, Tk, q0, k0, stop):
    """[Tq, Tk] multiplier of a (query, key) pair's contribution to dK / dV: stop_q1_to_k0 removes segment-1 queries from
    segment-0 keys (dQ keeps them)."""
    w = torch.ones(Tq, Tk, dtype=torch.float64)
    if stop:
        w[q0:, :k0] = 0.0
    return w


def bwd_reference(q, k, v, allowed, scale, o16, lse32, dO, kv_weight=None, delta=None):
    """lap_attention_bwd in float64 with the kernels' rounding points: P from the lse passed in, delta over the bf16 o passed in,
    dS = bf16(P (dP - delta) scale), dV = bf16(sum_i bf16(P) dO), dK = bf16(sum_i dS q), dQ = bf16(sum_j dS k).  kv_weight
    (broadcastable to [B, NH, Tq, Tk]) multiplies the pairs' contributions to dK / dV (stop_weight).  Returns a dict with dq, dk,
    dv (rounded), their bounds, and the sensitivities sum_i P |dO|, sum |dS||q|, sum |dS||k|, |dP| + |delta| (as the absolute
    sums sum_d |dO||v| + sum_d |dO||o| that bound their float32 error)."""
    B, Tq, NH, HD = q.shape
    NKV = k.shape[2]
    q, dO, o16 = q.double(), dO.double(), o16.double()
    kk, vv = _heads(k.double(), NH), _heads(v.double(), NH)
    Tk = kk.shape[1]
    ok = torch.ones(B, 1, Tq, Tk, dtype=torch.bool) if allowed is None else allowed[:, None]
    lse = lse32.double()[..., None]
    s = scale * torch.einsum("bihd,bjhd->bhij", q, kk)
    L = abs(scale) * torch.einsum("bihd,bjhd->bhij", q.abs(), kk.abs())
    zero = torch.zeros_like(s)
    P = torch.where(ok, torch.exp(s - lse), zero)
    eps = torch.where(ok & (P > 0), torch.expm1(U24 * (DEPTH * L + 4.0 * (s.abs() + lse.abs())) + INTR), zero)
    Pb, dPb = _rnd(P, eps * P)
    dP = torch.einsum("bihd,bjhd->bhij", dO, vv)
    SdP = torch.einsum("bihd,bjhd->bhij", dO.abs(), vv.abs())
    if delta is None:
        delta = torch.einsum("bihd,bihd->bhi", dO, o16)
    Sdl = torch.einsum("bihd,bihd->bhi", dO.abs(), o16.abs())
    edp = DEPTH * U24 * (SdP + Sdl[..., None])
    dS64 = P * (dP - delta[..., None]) * scale
    d_dS = abs(scale) * (eps * P * (dP - delta[..., None]).abs() + P * (1.0 + eps) * edp) + 4.0 * U24 * dS64.abs()
    dS, ddS = _rnd(dS64, d_dS)
    W = torch.ones(1, 1, Tq, Tk, dtype=torch.float64) if kv_weight is None else kv_weight
    G = NH // NKV
    nq, nk = int(ok.sum(-2).max()) * G, int(ok.sum(-1).max())

    def kv_sum(x, y):       # sum over the queries and over the query heads of a kv head: [B, Tk, NKV, HD]
        return torch.einsum("bhij,bihd->bjhd", x * W, y).view(B, Tk, NKV, G, HD).sum(3)

    sens_dv, sens_dk = kv_sum(Pb, dO.abs()), kv_sum(dS.abs(), q.abs())
    sens_dq = torch.einsum("bhij,bjhd->bihd", dS.abs(), kk.abs())
    dv, dv_bound = _rnd(kv_sum(Pb, dO), kv_sum(dPb, dO.abs()) + acc_depth(nq) * U24 * sens_dv)
    dk, dk_bound = _rnd(kv_sum(dS, q), kv_sum(ddS, q.abs()) + acc_depth(nq) * U24 * sens_dk)
    dq, dq_bound = _rnd(torch.einsum("bhij,bjhd->bihd", dS, kk), torch.einsum("bhij,bjhd->bihd", ddS, kk.abs()) + acc_depth(nk) * U24 * sens_dq)
    return dict(dq=dq, dk=dk, dv=dv, dq_bound=dq_bound, dk_bound=dk_bound, dv_bound=dv_bound, sens_dv=sens_dv, sens_dk=sens_dk,
                sens_dq=sens_dq, sens_dp=SdP + Sdl[..., None], P=P, dS=dS, delta=delta)


# ------------------------------------------------------------------------------------ float32 restatements of the kernels
_exp_err = [0.0]


def _exp32(x):
    """float32 exp; records its worst relative error against float64 on the same argument (results above 2^-100)."""
    y = torch.exp(x)
    y64 = torch.exp(x.double())
    big = y64 > 2.0 ** -100
    if bool(big.any()):
        _exp_err[0] = max(_exp_err[0], float(((y.double() - y64).abs() / y64)[big].max()))
    return y


def exp_error_seen():
    return _exp_err[0]


def _bf(x):
    return x.to(torch.bfloat16).float()


F32_ORDERS = ("tiles64", "tiles32", "split2")


def f32_forward(q, k, v, allowed, scale, order):
    """The forward kernels' algorithm in float32: key tiles in turn, online softmax (running maximum, rescale), bf16 P into the
    numerator and unrounded P into the denominator.  order: 64-key tiles, 32-key tiles, or 64-key tiles with the key share cut
    in two and combined as attn_fwd_combine_kernel does.  Returns (o as float64 of bf16, lse float32)."""
    B, Tq, NH, HD = q.shape
    q, kk, vv = q.float(), _heads(k.float(), NH), _heads(v.float(), NH)
    Tk = kk.shape[1]
    ok = torch.ones(B, 1, Tq, Tk, dtype=torch.bool) if allowed is None else allowed[:, None]
    tile = 32 if order == "tiles32" else 64
    starts = list(range(0, Tk, tile))
    shares = [starts] if order != "split2" else [starts[:(len(starts) + 1) // 2], starts[(len(starts) + 1) // 2:]]
    parts = []
    for share in shares:
        m = torch.full((B, NH, Tq), -1.0e30)
        l = torch.zeros(B, NH, Tq)
        acc = torch.zeros(B, NH, Tq, HD)
        for t0 in share:
            a = ok[..., t0:t0 + tile]
            s = torch.einsum("bihd,bjhd->bhij", q, kk[:, t0:t0 + tile]) * scale
            m_new = torch.maximum(m, s.masked_fill(~a, -1.0e30).amax(-1))
            alpha = _exp32(m - m_new)
            p = torch.where(a, _exp32(s - m_new[..., None]), torch.zeros_like(s))
            l = l * alpha + p.sum(-1)
            acc = acc * alpha[..., None] + torch.einsum("bhij,bjhd->bhid", _bf(p), vv[:, t0:t0 + tile])
            m = m_new
        inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
        parts.append((acc * inv[..., None], torch.where(l > 0, m + torch.log(l), torch.full_like(l, -1.0e30))))
    if len(parts) == 1:
        o, lse = parts[0]
        lse = torch.where(lse > -0.5e30, lse, torch.full_like(lse, LSE_EMPTY))
    else:
        mx = torch.maximum(parts[0][1], parts[1][1])
        den, acc = torch.zeros_like(mx), torch.zeros_like(parts[0][0])
        for op, li in parts:
            wgt = torch.where(li > -0.5e30, _exp32(li - mx), torch.zeros_like(li))
            den, acc = den + wgt, acc + op * wgt[..., None]
        o = acc * torch.where(den > 0, 1.0 / den, torch.zeros_like(den))[..., None]
        lse = torch.where(den > 0, mx + torch.log(den), torch.full_like(den, LSE_EMPTY))
    return _bf(o).double().transpose(1, 2), lse


def f32_backward(q, k, v, allowed, scale, o16, lse32, dO, order, kv_weight=None):
    """The backward kernels' algorithm in float32 (P from lse, bf16 P and dS, float32 accumulation over tiles of the streamed
    side).  Returns dq, dk, dv as float64 of bf16."""
    B, Tq, NH, HD = q.shape
    NKV = k.shape[2]
    q, dO, kk, vv = q.float(), dO.float(), _heads(k.float(), NH), _heads(v.float(), NH)
    Tk = kk.shape[1]
    ok = torch.ones(B, 1, Tq, Tk, dtype=torch.bool) if allowed is None else allowed[:, None]
    tile = 32 if order == "tiles32" else 64
    delta = (dO * o16.float()).sum(-1).transpose(1, 2)
    W = torch.ones(1, 1, Tq, Tk) if kv_weight is None else kv_weight.float().expand(1, 1, Tq, Tk) if kv_weight.dim() == 2 else kv_weight.float()
    dq, dk, dv = torch.zeros(B, Tq, NH, HD), torch.zeros(B, Tk, NH, HD), torch.zeros(B, Tk, NH, HD)
    for t0 in range(0, Tk, tile):       # dQ: key tiles in turn
        a = ok[..., t0:t0 + tile]
        s = torch.einsum("bihd,bjhd->bhij", q, kk[:, t0:t0 + tile]) * scale
        dp = torch.einsum("bihd,bjhd->bhij", dO, vv[:, t0:t0 + tile])
        ds = torch.where(a, _exp32(s - lse32[..., None]) * (dp - delta[..., None]) * scale, torch.zeros_like(s))
        dq = dq + torch.einsum("bhij,bjhd->bihd", _bf(ds), kk[:, t0:t0 + tile])
    for t0 in range(0, Tq, tile):       # dK / dV: query tiles in turn
        a = ok[:, :, t0:t0 + tile]
        s = torch.einsum("bihd,bjhd->bhij", q[:, t0:t0 + tile], kk) * scale
        dp = torch.einsum("bihd,bjhd->bhij", dO[:, t0:t0 + tile], vv)
        p = torch.where(a, _exp32(s - lse32[:, :, t0:t0 + tile, None]), torch.zeros_like(s))
        ds = p * (dp - delta[:, :, t0:t0 + tile, None]) * scale
        w = W[:, :, t0:t0 + tile]
        dv = dv + torch.einsum("bhij,bihd->bjhd", _bf(p) * w, dO[:, t0:t0 + tile])
        dk = dk + torch.einsum("bhij,bihd->bjhd", _bf(ds) * w, q[:, t0:t0 + tile])
    G = NH // NKV
    return (_bf(dq).double(), _bf(dk.view(B, Tk, NKV, G, HD).sum(3)).double(), _bf(dv.view(B, Tk, NKV, G, HD).sum(3)).double())


# ------------------------------------------------------------------------------------------------------- the cases
# mask: none | lap | edges | run | split | pow2 | causal;  layout: packed | fused (q | k | v column slices of one buffer);
# regime: rand | count (q = 0, v and dO = +-1)
Spec = namedtuple("Spec", "HD B NH NKV q_len k_len mask scaled layout regime", defaults=("none", False, "packed", "rand"))


def _words(cls, idx):
    """int32 info words from class bytes and index fields (class bit 7 makes the word negative)."""
    w = (cls.to(torch.int64) << 24) | idx.to(torch.int64)
    return ((w + 2 ** 31) % 2 ** 32 - 2 ** 31).to(torch.int32)


def lap_infos(B, Tp, S, n_lang, n_pad):
    """The token classes of test_kernels_gpu._lap_infos: prefix = [image / prompt | causal langact span | per-sample pad],
    suffix = S action tokens that see class 1 and class 4."""
    qc, qx = torch.zeros(B, Tp + S, dtype=torch.int64), torch.zeros(B, Tp + S, dtype=torch.int64)
    kc, kx = qc.clone(), qx.clone()
    for b in range(B):
        npad = (n_pad + b) % (n_pad + 1) if n_pad else 0
        nq = Tp - n_lang - npad
        qc[b, :nq], kc[b, :nq] = 3, 1
        span = torch.arange(1, n_lang + 1)
        qc[b, nq:nq + n_lang], kc[b, nq:nq + n_lang] = 3, 2
        qx[b, nq:nq + n_lang] = kx[b, nq:nq + n_lang] = span
    qc[:, Tp:], qx[:, Tp:], kc[:, Tp:] = 5, 0xFFFFFF, 4
    return _words(qc, qx), _words(kc, kx)


def infos(spec):
    """(qinfo [B, Tq], kinfo [B, Tk]) int32 of a case, or (None, None)."""
    B, (q0, q1), (k0, k1) = spec.B, spec.q_len, spec.k_len
    Tq, Tk = q0 + q1, k0 + k1
    if spec.mask == "none":
        return None, None
    if spec.mask == "lap":        # q_len == k_len == (Tp, S); the causal span crosses a 32-key or a 64-key tile boundary
        return lap_infos(B, q0, q1, min(40, q0 - 5), 3)
    qc, qx = torch.zeros(B, Tq, dtype=torch.int64), torch.zeros(B, Tq, dtype=torch.int64)
    kc, kx = torch.zeros(B, Tk, dtype=torch.int64), torch.zeros(B, Tk, dtype=torch.int64)
    if spec.mask == "edges":
        # q_len == k_len == (200, 40), B = 3.  keys [0, 64): class 1, all allowed (the fast path, next to mixed tiles);
        # [64, 128): class 0, values ~1e3 (a whole masked tile between allowed ones: the skip path) except [100, 104): class 0x80,
        # which only the action queries (class 0x85, a negative word) share; [128, 200): the causal span, index 1 .. 72, so the keys
        # at 160 and 192 (the first of a 32-key and of a 64-key tile) have idx == idx(q) + 1 for the queries at 159 and 191;
        # sample 1 pads the last 5 of the span (class 0); sample 2 has no allowed key for any query (all queries class 0);
        # suffix: action queries class 0x85 index 0xFFFFFF, action keys class 0x84, the last of them with index 0xFFFFFF.
        assert (q0, q1, k0, k1, B) == (200, 40, 200, 40, 3)
        qc[:, :64], kc[:, :64] = 3, 1
        kc[:, 100:104] = 0x80
        qc[:, 128:200], kc[:, 128:200] = 3, 2
        qx[:, 128:200] = kx[:, 128:200] = torch.arange(1, 73)
        qc[1, 195:200] = kc[1, 195:200] = 0
        qc[:, 200:], qx[:, 200:], kc[:, 200:] = 0x85, 0xFFFFFF, 0x84
        kx[:, 239] = 0xFFFFFF
        qc[2] = 0
    elif spec.mask == "run":
        # single segment, class 1 everywhere (whole tiles allowed: bits >= 32 of the fast masks), one causal run of 100 tokens
        # that ends 20 before the end, so the mixed tiles are the last ones
        qc[:], kc[:] = 1, 1
        r0 = Tq - 120
        qx[:] = 0xFFFFFF
        qx[:, r0:r0 + 100] = kx[:, r0:r0 + 100] = torch.arange(1, 101)
        kx[:, r0 + 100:] = 101
    elif spec.mask == "split":
        # few suffix queries against [prefix | suffix]: the first two thirds of the prefix are class 0 (with nsplit 2 a whole
        # share is masked), the rest class 1; action tokens class 4 / 5
        qc[:], qx[:] = 5, 0xFFFFFF
        kc[:, k0 * 2 // 3:k0], kc[:, k0:] = 1, 4
    elif spec.mask in ("pow2", "causal"):
        # single segment, keys index 1 .. Tk.  pow2: query i has index 2^(i mod n): a power-of-two number of allowed keys (P is
        # exact in bf16 at q = 0); the last query of sample 0 is class 0 (no allowed key).  causal: query i sees i + 1 keys.
        qc[:], kc[:] = 1, 1
        kx[:] = torch.arange(1, Tk + 1)
        qx[:] = 2 ** (torch.arange(Tq) % (int(math.log2(Tk)) + 1)) if spec.mask == "pow2" else torch.arange(1, Tq + 1).clamp(max=Tk)
        if spec.mask == "pow2":
            qc[0, Tq - 1] = 0
    else:
        raise ValueError(spec.mask)
    return _words(qc, qx), _words(kc, kx)


_CASES = {}
_REFS = {}


def scale_of(spec):
    return spec.HD ** -0.5 if spec.scaled else 1.0


def make_case(spec):
    """Seeded inputs of a case (cached): q, k, v, dO bf16 in the joint layout, the info words and `allowed`.  The scores have
    std 1 to 3 (query rows scaled by 1 + i % 3); class-0 keys hold |values| ~1e3 in k and v."""
    if spec in _CASES:
        return _CASES[spec]
    g = torch.Generator().manual_seed(zlib.crc32(repr(tuple(spec)).encode()))
    B, NH, NKV, HD = spec.B, spec.NH, spec.NKV, spec.HD
    Tq, Tk = sum(spec.q_len), sum(spec.k_len)
    amp = 1.0 if spec.scaled else HD ** -0.25
    rows = (1.0 + torch.arange(Tq) % 3).view(1, Tq, 1, 1)
    c = {"spec": spec}
    c["qinfo"], c["kinfo"] = infos(spec)
    c["allowed"] = None if c["qinfo"] is None else mask_ok(c["qinfo"], c["kinfo"])
    q = torch.randn(B, Tq, NH, HD, generator=g) * amp * rows
    k = torch.randn(B, Tk, NKV, HD, generator=g) * amp
    v, dO = torch.randn(B, Tk, NKV, HD, generator=g), torch.randn(B, Tq, NH, HD, generator=g)
    if spec.regime == "count":
        q = torch.zeros_like(q)
        v = (torch.randint(0, 2, v.shape, generator=g) * 2 - 1).float()
        dO = (torch.randint(0, 2, dO.shape, generator=g) * 2 - 1).float()
    if c["kinfo"] is not None:
        dead = ((c["kinfo"] >> 24) == 0)[:, :, None, None]
        big = torch.randn(B, Tk, NKV, HD, generator=g) * 1.0e3
        k, v = torch.where(dead, big, k), torch.where(dead, -big, v)
    c["q"], c["k"], c["v"], c["dO"] = (t.to(torch.bfloat16) for t in (q, k, v, dO))
    _CASES[spec] = c
    return c


def reference(spec, stop=False, split=False):
    """The float64 forward reference of a case and the backward reference fed with bf16(o64) and float32(lse64) (cached; the
    [Tq, Tk] intermediates are dropped)."""
    key = (spec, stop, split)
    if key in _REFS:
        return _REFS[key]
    c = make_case(spec)
    sc = scale_of(spec)
    f = fwd_reference(c["q"], c["k"], c["v"], c["allowed"], sc, split)
    r = {n: f[n] for n in ("o", "o16", "lse", "A", "o_bound", "lse_bound", "empty")}
    r["lse32"] = f["lse"].float()
    W = stop_weight(sum(spec.q_len), sum(spec.k_len), spec.q_len[0], spec.k_len[0], stop)
    b = bwd_reference(c["q"], c["k"], c["v"], c["allowed"], sc, f["o16"], r["lse32"], c["dO"], W)
    r.update({n: b[n] for n in ("dq", "dk", "dv", "dq_bound", "dk_bound", "dv_bound")})
    _REFS[key] = r
    return r


def drop_caches():
    _CASES.clear()
    _REFS.clear()


# ------------------------------------------------------------------------------------------------------ exact cases
def count_forward(c):
    """q = 0, v = +-1: (sum of the allowed keys' signs [B, Tq, NH, HD], their number [B, Tq, 1, 1]) as float64."""
    B, Tq, NH, HD = c["q"].shape
    Tk = c["k"].shape[1]
    ok = torch.ones(B, Tq, Tk, dtype=torch.float64) if c["allowed"] is None else c["allowed"].double()
    return torch.einsum("bij,bjhd->bihd", ok, _heads(c["v"].double(), NH)), ok.sum(-1).view(B, Tq, 1, 1)


def count_backward_dv(c, stop=False):
    """q = 0, dO = +-1, o passed in as zeros (delta = 0), lse = float32(log n): dV = bf16(sum_i bf16(exp(-lse_i)) dO_i) over the
    queries that allow the key and the query heads of its kv head.  Returns (dv [B, Tk, NKV, HD] float64, exact): exact says
    that every allowed count is a power of two, so every P is one and every sum is a short dyadic number that float32 holds."""
    B, Tq, NH, HD = c["q"].shape
    Tk, NKV = c["k"].shape[1], c["k"].shape[2]
    ok = torch.ones(B, Tq, Tk, dtype=torch.float64) if c["allowed"] is None else c["allowed"].double()
    n = ok.sum(-1)
    lse32 = torch.where(n > 0, torch.log(n.clamp(min=1.0)), torch.full_like(n, LSE_EMPTY)).float()
    P = bf16r(torch.exp(-lse32.double()))
    W = stop_weight(Tq, Tk, c["spec"].q_len[0], c["spec"].k_len[0], stop)
    dv = torch.einsum("bij,bihd->bjhd", ok * P[..., None] * W, c["dO"].double()).view(B, Tk, NKV, NH // NKV, HD).sum(3)
    exact = bool((torch.log2(n[n > 0]) % 1 == 0).all())
    return bf16r(dv), lse32[:, None, :].expand(B, NH, Tq).contiguous(), exact


# ------------------------------------------------------------------------------ one allocation with guards and sentinels
Region = namedtuple("Region", "off rows rs col0 width")
GUARD_BEFORE, GUARD_AFTER = 8, 64         # NaN rows around every input: a 64-row tile read past a segment's end lands in them
SENTINEL, LSE_SENTINEL = -24576.0, -12345.0
INPUTS, OUTPUTS = ("q", "k", "v", "dO"), ("o", "dq", "dk", "dv")


def build_arena(c):
    """One bf16 allocation that holds every buffer of the case, neighbours adjacent: each of q, k, v, dO per segment between NaN
    guard rows (NaN also in the column gap of the fused layout, whose rows are q | k | v | 8 NaN), each output per segment
    pre-filled with SENTINEL, guards included, and lse (float32, LSE_SENTINEL) the same way.  Returns (arena, regions): regions
    maps `q0`, `dk1`, ... to Region (element offset of the first valid row, rows, row stride, first column, width); `lse` is
    (offset, floats)."""
    spec = c["spec"]
    B, NH, NKV, HD = spec.B, spec.NH, spec.NKV, spec.HD
    chunks, regions, pos = [], {}, [0]

    def alloc(rows, rs, fill):
        chunks.append(torch.full(((GUARD_BEFORE + rows + GUARD_AFTER) * rs,), fill, dtype=torch.bfloat16))
        off = pos[0] + GUARD_BEFORE * rs
        pos[0] += chunks[-1].numel()
        return off

    def put(region, data):
        chunk = chunks[-1]
        start = region.off - (pos[0] - chunk.numel())
        torch.as_strided(chunk, (region.rows, region.width), (region.rs, 1), start + region.col0).copy_(data.reshape(region.rows, region.width))

    for s in range(2):
        lo_q, lo_k = (0, 0) if s == 0 else (spec.q_len[0], spec.k_len[0])
        ql, kl = spec.q_len[s], spec.k_len[s]
        Wq, Wk = NH * HD, NKV * HD
        if spec.layout == "fused" and ql:
            assert NH == NKV and ql == kl and s == 0 and spec.q_len[1] == 0
            rs = 3 * Wq + 8
            off = alloc(B * ql, rs, float("nan"))
            for j, nm in enumerate(("q", "k", "v")):
                regions[f"{nm}{s}"] = Region(off, B * ql, rs, j * Wq, Wq)
                put(regions[f"{nm}{s}"], c[nm][:, lo_q:lo_q + ql])
            off = alloc(B * ql, rs, SENTINEL)
            for j, nm in enumerate(("dq", "dk", "dv")):
                regions[f"{nm}{s}"] = Region(off, B * ql, rs, j * Wq, Wq)
        for nm in INPUTS + OUTPUTS:
            if f"{nm}{s}" in regions:
                continue
            is_q = nm in ("q", "dO", "o", "dq")
            n, lo, W = (ql, lo_q, Wq) if is_q else (kl, lo_k, Wk)
            if n == 0:
                continue
            regions[f"{nm}{s}"] = Region(alloc(B * n, W, float("nan") if nm in INPUTS else SENTINEL), B * n, W, 0, W)
            if nm in INPUTS:
                put(regions[f"{nm}{s}"], c[nm][:, lo:lo + n])
    n = B * NH * sum(spec.q_len)
    lse = torch.full((16 + n + 16,), LSE_SENTINEL, dtype=torch.float32)
    regions["lse"] = (pos[0] + 32, n)
    chunks.append(lse.view(torch.bfloat16))
    return torch.cat(chunks), regions


def region_view(arena, r):
    """The [rows, width] window of a region in `arena` (on any device): shares memory with it."""
    return torch.as_strided(arena, (r.rows, r.width), (r.rs, 1), r.off + r.col0)


def lse_view(arena, regions, B, NH, Tq):
    off, n = regions["lse"]
    return arena[off:off + 2 * n].view(torch.float32).view(B, NH, Tq)


def untouched(before, after, regions, written):
    """True when `after` equals `before` bit for bit outside the windows of the regions named in `written`."""
    free = torch.ones(before.numel(), dtype=torch.bool)
    for nm in written:
        if nm == "lse":
            free[regions["lse"][0]:regions["lse"][0] + 2 * regions["lse"][1]] = False
        elif nm in regions:
            region_view(free, regions[nm]).fill_(False)
    return torch.equal(before.view(torch.int16)[free], after.view(torch.int16)[free])


def joint(arena, regions, name, spec):
    """Output `name` (o, dq: [B, Tq, NH, HD]; dk, dv: [B, Tk, NKV, HD]) gathered from the arena's segments, float64."""
    is_q = name in ("o", "dq")
    H = spec.NH if is_q else spec.NKV
    parts = []
    for s in range(2):
        n = (spec.q_len if is_q else spec.k_len)[s]
        if n:
            parts.append(region_view(arena, regions[f"{name}{s}"]).double().reshape(spec.B, n, H, spec.HD))
    return torch.cat(parts, 1)


# ---------------------------------------------------------------------------------- the case list of the GPU module
HEADS = ((2, 2), (4, 2), (3, 1), (8, 1))        # the backward's head split: 1, 2, 1 (three heads per key head), 4
SINGLE_T = (1, 31, 32, 33, 63, 64, 65, 200)
TWO_SEG = ((70, 10), (97, 50), (33, 31), (64, 1), (128, 64))


def single_segment_specs(HD):
    """The full product T x B x head arrangement: 64 cases per head size."""
    return [Spec(HD, B, nh, nkv, (T, 0), (T, 0)) for T, B, (nh, nkv) in itertools.product(SINGLE_T, (1, 3), HEADS)]


def two_segment_specs(HD):
    nh, nkv = {16: (2, 2), 72: (4, 2), 256: (8, 1)}[HD]
    return [Spec(HD, 2, nh, nkv, (tp, s), (tp, s), "lap") for tp, s in TWO_SEG]


def edge_spec(HD):
    return Spec(HD, 3, 4, 2, (200, 40), (200, 40), "edges")


def split_specs(HD):
    """(spec, nsplit_hint): 10 suffix queries; keys (192, 10) with the first 128 masked: with nsplit 2 the first share is masked
    whole, with 3 the generic family's third share is empty (4 tiles of 64); keys (20, 10): 2 tiles in either family, nsplit 3."""
    a = Spec(HD, 1, 8, 1, (0, 10), (192, 10), "split")
    b = Spec(HD, 1, 8, 1, (0, 10), (20, 10), "split")
    return [(a, 1), (a, 2), (a, 3), (b, 3)]


def fused_spec(HD):
    return Spec(HD, 2, 4, 4, (100, 0), (100, 0), "none", True, "fused")


MANY_TILES = tuple(Spec(256, 1, 1, 1, (T, 0), (T, 0), m) for T in (1100, 2048, 2080) for m in ("none", "run"))


def scale_spec(HD):
    return Spec(HD, 2, 4, 2, (97, 0), (97, 0), "causal", True)


def count_specs(HD):
    """Exact cases: the forward on the edges and lap masks and unmasked; the backward on pow2 (equality) and causal (one spacing)."""
    fwd = [Spec(HD, 3, 4, 2, (200, 40), (200, 40), "edges", regime="count"), Spec(HD, 2, 4, 2, (70, 10), (70, 10), "lap", regime="count"),
           Spec(HD, 1, 3, 1, (65, 0), (65, 0), regime="count")]
    bwd = [Spec(HD, 2, 4, 2, (150, 0), (150, 0), "pow2", regime="count"), Spec(HD, 2, 4, 2, (70, 0), (70, 0), "causal", regime="count")]
    return fwd, bwd


def all_random_specs():
    """Every rand-regime case of the GPU module: what the float32 restatements must meet on the CPU."""
    out = []
    for HD in (16, 72, 256):
        out += single_segment_specs(HD) + two_segment_specs(HD) + [edge_spec(HD), scale_spec(HD)] + [s for s, _ in split_specs(HD)]
        if HD != 16:
            out.append(fused_spec(HD))
    return sorted(set(out)) + list(MANY_TILES)
