"""Float64 references, element bounds, float32 restatements and seeded inputs for the training step's non-GEMM kernels
(csrc/norm.hip, the training half of csrc/elementwise.hip, the loss / metric / optimizer kernels of csrc/loss_optim.hip), shared
by tests/test_train_reference_gpu.py (device against reference) and tests/test_train_reference_cpu.py (the criteria against
float32 restatements and single-fault corruptions).  Plain torch on the CPU; nothing here calls lap_amd.hip.

Every reference returns, per output, (R, bound): R restates each bf16 rounding point the kernel states in its source, bound is
per element.  bound None means "bit for bit".  u = 2^-24 is the relative error of one float32 rounding; a fused multiply-add
rounds once where the two operations round twice, so counting both covers either contraction.  Second-order terms (u^2) are
dropped against the spare roundings counted below.

 * sums.  A float32 sum of n terms whose longest chain of additions is `depth` errs by at most depth u sum|terms|.  Row
   statistics: <= 32 sequential additions per lane (4 chunks of 8) and the 6 steps of the wave butterfly: ROW = 38.  Column
   sums: the rows one wave takes in turn, the 4-wave LDS combine, and one float32 atomic per block onto the value found there;
   atomics land in any order, so the bound is the sum of absolute terms (the start value included) times the block count.
 * RMSNorm.  r = 1 / sqrt(ss / D + eps): ss has relative error ROW u (positive terms), the division and the addition one each,
   the square root halves these and adds its own, the reciprocal one more: RSTD = 24 u relative.  y = x r w (+ shift): three
   more roundings (w = 1 + scale in float32 is one of them; the adaptive w = bf16(1 + scale) is a stated rounding point and exact
   for |scale| >= 2^-16, which the cases keep), then the bf16 store (_rnd).
   Backward: gv = dy w, dot = sum gv x (ROW + 2), cc = dot r^3 / D (4 more), dx = r gv - x cc (+ old dx): each product and the
   difference round once, relative to |r gv| + |x cc| (+ |old|), which is what cancels.  dscale / dshift terms dy x r, dy.
 * LayerNorm.  mean = s / D: ROW u sum|x| / D + u |mean|.  The fast variance E[x^2] - E[x]^2 cancels: its absolute error is
   e_var = (ROW + 1) u E[x^2] + 2 |mean| e_mean + 2 u mean^2 + u var, however small var is.  It is not assumed small against
   var + eps: r = (var + eps)^-1/2 is monotone, so the device's r lies between the values at max(var - e_var, 0) (the clamp)
   and var + e_var; to first order this is 0.5 r^3 e_var.  4 u r for the addition, the root and the reciprocal.  A row with a
   common offset (3 + 0.1 noise) and a constant row (var = 0, r = eps^-1/2) are among the cases.
   y = (x - mean) (r gamma) + beta carries e_mean through r |gamma| and e_r through |x - mean| |gamma|.
   Backward: xh = (x - mean) r (2 u), s1 = sum gv / D, s2 = sum gv xh / D (ROW + 4), dx = r (gv - s1 - xh s2) (+ old), 6 u of the
   absolute terms.  dxsum is the column sum of dx as stored: it is checked against the device's own stored dx.
 * RoPE.  ts = powf(10000, 2 i / HD) (E_POW relative), angle = pos / ts (u), sincosf (E_SIN absolute; the angle's error enters
   through a slope of at most 1): e_trig = |angle| (E_POW + 2 u) + E_SIN on sin and cos.  The rotation: (|x1| + |x2|) e_trig and 3
   roundings; bf16; q heads: a float32 multiply by float32(q_scale) (u), then the bf16 store.  The backward multiplies first and
   rounds once.
 * GELU (tanh form).  arg = k0 (x + k1 x^3): 5 u |arg| through a slope of tanh: |arg| sech^2 <= 0.45.  1 + tanh cancels in the
   negative tail: absolute error E_TANH + 3 u, times 0.5 |x|, plus 2 u |gelu|.  gelu' = 0.5 (1 + t) + 0.5 x (1 - t^2) arg':
   0.5 (E_TANH + 3 u) + 0.5 |x| arg' (2 E_TANH + 8 u) + 8 u (|A| + |B|).  Products of two bf16 values are exact in float32.
 * cross-entropy.  m is a maximum: exact.  l = sum exp(x - m) over positive terms: every term passes through one __expf per
   thread step, wave step, block step and chunk (E_EXP + 3 u each; OPS of them), and the arguments' roundings (the product with
   log2 e inside __expf included) add 4 u per unit of argument, at most twice the range of the finite logits.  Terms below
   2^-126 may flush: V 2^-126 absolute.  Gradient: lse = m + __logf(l): E_LOG (|log l| + 1) + u |lse|; p = __expf(x - lse):
   E_EXP + 4 u |x - lse| + the lse error, relative; w (p - onehot): 2 u more.  hi = bf16; hi + lo: 2^-16 relative more.
 * AdamW.  As written in adamw_ema_kernel, operation by operation (ref_adamw); v_sqrt_f32 / v_rcp_f32: E_SQRT, E_RCP.
   |sqrt(a + d) - sqrt(a)| <= min(d / (2 sqrt a), sqrt d): v = 0 with g = 0 has no slope to linearise on.

Device math functions (tanhf, sincosf, powf, __expf, __logf, v_rcp_f32, v_sqrt_f32): their error cannot be derived.  As
attention_reference.F32_EXP_ERR / INTR: the worst error of torch's float32 CPU function against float64 on the arguments the
cases produce is recorded below (tests/test_train_reference_cpu.py measures it again and asserts it is no larger), the device
gets 4 x that, capped so that the allowance cannot hide a dropped term or a missing rounding point (2^-18 is 2^-10 of a bf16
spacing)."""
import math
import zlib
from collections import namedtuple

import torch

from tests.decode_reference import _rnd, bf16r, check_elementwise, ulp_bf16, worst_ratio  # noqa: F401 (re-exported)

U = 2.0 ** -24
ROW = 38
RSTD = 24
G_RMS, G_LN = 64, 32            # rows per block of rmsnorm_bwd / layernorm_bwd (LAP_NORM_BWD_ROWS unset)
K0, K1 = 0.7978845608028654, 0.044715
K0F, K1F = float(torch.tensor(K0, dtype=torch.float32)), float(torch.tensor(K1, dtype=torch.float32))

# measured by tests/test_train_reference_cpu.py::test_math_function_errors over every case below (relative, or absolute where said)
F32_ERR = {
    "exp": 6.1e-8,       # measured: 6.009e-08 relative
    "log": 1.6e-8,       # measured: 1.511e-08 relative to |log| + 1
    "tanh": 3.2e-8,      # measured: 3.140e-08 absolute
    "sincos": 3.6e-8,    # measured: 3.521e-08 absolute
    "pow": 5.9e-8,       # measured: 5.845e-08 relative
    "sqrt": 6.3e-8,      # measured: 6.290e-08 relative
    "rcp": 6.0e-8,       # measured: 5.959e-08 relative
}
CAP = 2.0 ** -18
E_EXP, E_LOG, E_TANH, E_SIN, E_POW, E_SQRT, E_RCP = (min(4.0 * F32_ERR[k], CAP) for k in ("exp", "log", "tanh", "sincos", "pow", "sqrt", "rcp"))

_seen = {k: 0.0 for k in F32_ERR}


def errors_seen():
    return dict(_seen)


def _note(kind, err):
    if err.numel():
        _seen[kind] = max(_seen[kind], float(err.max()))


def _exp32(x):
    y, y64 = torch.exp(x), torch.exp(x.double())
    big = y64 > 2.0 ** -100
    _note("exp", ((y.double() - y64).abs() / y64)[big])
    return y


def _log32(x):
    y, y64 = torch.log(x), torch.log(x.double())
    _note("log", (y.double() - y64).abs() / (y64.abs() + 1.0))
    return y


def _tanh32(x):
    y = torch.tanh(x)
    _note("tanh", (y.double() - torch.tanh(x.double())).abs())
    return y


def _sincos32(a):
    s, c = torch.sin(a), torch.cos(a)
    _note("sincos", torch.maximum((s.double() - torch.sin(a.double())).abs(), (c.double() - torch.cos(a.double())).abs()))
    return s, c


def _pow32(base, e):
    y = torch.pow(torch.tensor(base, dtype=torch.float32), e)
    y64 = torch.pow(torch.tensor(base, dtype=torch.float64), e.double())
    _note("pow", (y.double() - y64).abs() / y64)
    return y


def _sqrt32(x):
    y, y64 = torch.sqrt(x), torch.sqrt(x.double())
    ok = y64 > 2.0 ** -60
    _note("sqrt", ((y.double() - y64).abs() / y64)[ok])
    return y


def _rcp32(x):
    y, y64 = 1.0 / x, 1.0 / x.double()
    _note("rcp", (y.double() - y64).abs() / y64.abs())
    return y


def _bf(x):
    return x.to(torch.bfloat16).float()


def f32c(v):
    """A python float as the float32 the C ABI passes, back as a float."""
    return float(torch.tensor(v, dtype=torch.float32))


def gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


ORDERS = ("blocks", "tree")
BLOCK = 8


def sum32(t, order):
    """Float32 sum over the last dimension.  blocks: runs of 8 one after the other (a lane's 8 elements, a wave's rows in turn), then
    pairwise over the runs; tree: pairwise throughout.  Both stay inside the depths the bounds count (8 + log2(n / 8) <= the
    kernels' own chain for every case here); one long sequential chain would not, and no kernel has one."""
    n = t.shape[-1]
    if order == "blocks":
        t = torch.nn.functional.pad(t, (0, (-n) % BLOCK)).reshape(*t.shape[:-1], -1, BLOCK)
        acc = torch.zeros(t.shape[:-1])
        for j in range(BLOCK):
            acc = acc + t[..., j]
        t, n = acc, acc.shape[-1]
    p = 1 << max(n - 1, 0).bit_length()
    t = torch.nn.functional.pad(t, (0, p - n))
    while t.shape[-1] > 1:
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


def colsum32(t, order):
    return sum32(t.transpose(0, 1).contiguous(), order)


def cdiv(a, b):
    return (a + b - 1) // b


# =================================================================================================== normalisation
NormCase = namedtuple("NormCase", "kind D rows B rps pad shared", defaults=(0, 0, 0, False))
NORM_D = (8, 64, 512, 520, 1024, 1152, 1536, 2048)
RMS_ROWS, LN_ROWS, ADA_RPS = (1, 3, 4, 5, 64, 65, 67), (1, 5, 32, 33, 35), (1, 3, 4, 5, 50)


def norm_specs(kind):
    if kind == "rms":
        out = [NormCase("rms", D, r) for D in NORM_D for r in (5, 67)] + [NormCase("rms", D, r) for D in (64, 1152) for r in RMS_ROWS]
    elif kind == "ln":
        out = [NormCase("ln", D, r) for D in NORM_D for r in (5, 35)] + [NormCase("ln", D, r) for D in (64, 1152) for r in LN_ROWS]
    else:       # B = 3: mod is a view with row stride 3 D + 8
        out = [NormCase("ada", D, B * rps, B, rps, 8 if B == 3 else 0) for D in NORM_D for B, rps in ((3, 5), (1, 4))]
        out += [NormCase("ada", D, B * rps, B, rps, 8 if B == 3 else 0) for D in (64, 1152) for B in (1, 3) for rps in ADA_RPS]
    return sorted(set(out))


def accum_modes(D):
    return (False, True) if D in (64, 1152, 2048) else (False,)


_NORM = {}


def norm_case(spec):
    """x, dy, old dx (bf16 [rows, D]); scale / gamma / beta (float32 [D]); mod (bf16 [B, 3 D], |scale third| >= 2^-10); float32
    start values of the accumulated gradients.  LayerNorm: row 0 is 3 + 0.1 noise, row 1 constant."""
    if spec in _NORM:
        return _NORM[spec]
    g = gen(*spec)
    D, rows = spec.D, spec.rows
    amp = (1.0 + torch.arange(rows) % 3).view(rows, 1).float()
    x = torch.randn(rows, D, generator=g) * amp
    if spec.kind == "ln":
        x[0] = 3.0 + 0.1 * torch.randn(D, generator=g)
        if rows > 1:
            x[1] = 1.5
    c = dict(spec=spec, x=x.bfloat16(), dy=torch.randn(rows, D, generator=g).bfloat16(), old=torch.randn(rows, D, generator=g).bfloat16(),
             scale=0.1 * torch.randn(D, generator=g), gamma=1.0 + 0.1 * torch.randn(D, generator=g), beta=0.1 * torch.randn(D, generator=g),
             dscale0=torch.randn(D, generator=g), dgamma0=torch.randn(D, generator=g), dbeta0=torch.randn(D, generator=g),
             dxsum0=torch.randn(D, generator=g))
    if spec.kind == "ada":
        mod = (0.1 * torch.randn(spec.B, 3 * D, generator=g)).bfloat16()
        sc = mod[:, :D].float()
        mod[:, :D] = torch.where(sc.abs() < 2.0 ** -10, torch.full_like(sc, 2.0 ** -10), sc).bfloat16()
        c["mod"], c["dmod0"] = mod, torch.randn(spec.B, 3 * D, generator=g)
    _NORM[spec] = c
    return c


def _w_rows(c, shared=False):
    """(w [rows, D] float64, shift or None, roundings behind w)."""
    s = c["spec"]
    if s.kind != "ada":
        return (1.0 + c["scale"].double()).expand(s.rows, s.D), None, 1
    idx = torch.zeros(s.rows, dtype=torch.long) if shared else torch.arange(s.rows) // s.rps
    m = c["mod"].double()
    return bf16r(1.0 + m[:, :s.D])[idx], m[:, s.D:2 * s.D][idx], 0


def ref_rms_fwd(c, eps=1e-6, shared=False, rounded=True):
    x = c["x"].double()
    w, sh, kw = _w_rows(c, shared)
    if not rounded and c["spec"].kind == "ada":
        w = (1.0 + c["mod"].double()[:, :c["spec"].D])[torch.arange(c["spec"].rows) // c["spec"].rps]
    r = (x.pow(2).mean(1, keepdim=True) + f32c(eps)).rsqrt()
    core = x * r * w
    y = core if sh is None else core + sh
    if not rounded:
        return y
    d = (RSTD + 2 + kw) * U * core.abs() + (0.0 if sh is None else U * (core.abs() + sh.abs()))
    return dict(y=_rnd(y, d), rstd=(r[:, 0], RSTD * U * r[:, 0]))


def _col(terms, init, depth):
    """Column sums over the rows onto a start value: (R, bound)."""
    return init.double() + terms.sum(0), depth * U * (terms.abs().sum(0) + init.double().abs())


def ref_rms_bwd(c, rstd32, accum=False):
    s = c["spec"]
    x, g, r = c["x"].double(), c["dy"].double(), rstd32.double().view(-1, 1)
    w, _, kw = _w_rows(c)
    gv = g * w
    dot, sdot = (gv * x).sum(1, keepdim=True), (gv * x).abs().sum(1, keepdim=True)
    cc = dot * r ** 3 / s.D
    e_cc = (ROW + 2 + kw) * U * sdot * r ** 3 / s.D + 5 * U * cc.abs()
    a, b = r * gv, x * cc
    o, d = a - b, (1 + kw) * U * a.abs() + x.abs() * e_cc + 2 * U * (a.abs() + b.abs())
    if accum:
        old = c["old"].double()
        o, d = o + old, d + U * (a.abs() + b.abs() + old.abs())
    out = dict(dx=_rnd(o, d))
    t = g * x * r
    if s.kind == "ada":
        depth = cdiv(s.rps, 4) + 4 + 1 + 2
        dm, db = c["dmod0"].double().clone(), torch.zeros(s.B, 3 * s.D, dtype=torch.float64)
        for b_ in range(s.B):
            rows = slice(b_ * s.rps, (b_ + 1) * s.rps)
            for k, terms in enumerate((t[rows], g[rows])):
                ref, bound = _col(terms, c["dmod0"][b_, k * s.D:(k + 1) * s.D], depth)
                dm[b_, k * s.D:(k + 1) * s.D], db[b_, k * s.D:(k + 1) * s.D] = ref, bound
        out["dmod"] = (dm, db)          # the gate third: start value, bound 0
    else:
        out["dscale"] = _col(t, c["dscale0"], cdiv(G_RMS, 4) + 4 + cdiv(s.rows, G_RMS) + 1 + 2)
    return out


def ref_ln_fwd(c, eps=1e-6, rounded=True):
    x, D = c["x"].double(), c["spec"].D
    gm, bt = c["gamma"].double(), c["beta"].double()
    eps = f32c(eps)
    mean, ex2 = x.mean(1, keepdim=True), x.pow(2).mean(1, keepdim=True)
    var = (ex2 - mean ** 2).clamp(min=0.0)
    r = (var + eps).rsqrt()
    y = (x - mean) * (r * gm) + bt
    if not rounded:
        return y
    e_mu = ROW * U * x.abs().sum(1, keepdim=True) / D + U * mean.abs()
    e_var = (ROW + 1) * U * ex2 + 2 * mean.abs() * e_mu + 2 * U * mean ** 2 + U * var
    r_hi, r_lo = ((var - e_var).clamp(min=0.0) + eps).rsqrt(), (var + e_var + eps).rsqrt()
    e_r = torch.maximum(r_hi - r, r - r_lo) + 4 * U * r_hi
    xc = (x - mean).abs()
    core = (xc * r * gm.abs())
    d = gm.abs() * (r * e_mu + (xc + e_mu) * e_r) + 3 * U * core + U * (core + bt.abs())
    return dict(y=_rnd(y, d), mean=(mean[:, 0], e_mu[:, 0]), rstd=(r[:, 0], e_r[:, 0]))


def ref_ln_bwd(c, mean32, rstd32, accum=False):
    s = c["spec"]
    x, g, gm = c["x"].double(), c["dy"].double(), c["gamma"].double()
    mu, r = mean32.double().view(-1, 1), rstd32.double().view(-1, 1)
    xh, gv = (x - mu) * r, g * gm
    s1, s2 = gv.mean(1, keepdim=True), (gv * xh).mean(1, keepdim=True)
    e1 = (ROW + 1) * U * gv.abs().mean(1, keepdim=True) + U * s1.abs()
    e2 = (ROW + 4) * U * (gv * xh).abs().mean(1, keepdim=True) + U * s2.abs()
    T = gv.abs() + s1.abs() + (xh * s2).abs()
    o, d = r * (gv - s1 - xh * s2), r * (e1 + xh.abs() * e2 + 6 * U * T)
    if accum:
        old = c["old"].double()
        o, d = o + old, d + U * (r * T + old.abs())
    depth = cdiv(G_LN, 4) + 4 + cdiv(s.rows, G_LN) + 1
    t = g * xh
    dg, bg = _col(t, c["dgamma0"], depth + 3)
    return dict(dx=_rnd(o, d), dgamma=(dg, bg), dbeta=_col(g, c["dbeta0"], depth))


def ref_dxsum(dx_stored, init, rows):
    """dxsum against the dx the device stored (float64 of bf16): only the summation errs."""
    return _col(dx_stored.double(), init, cdiv(G_LN, 4) + 4 + cdiv(rows, G_LN) + 1)


def f32_rms_fwd(c, order, eps=1e-6, shared=False, fault=None):
    s = c["spec"]
    x = c["x"].float()
    r = 1.0 / torch.sqrt(sum32(x * x, order) / s.D + eps)
    if s.kind == "ada":
        idx = torch.zeros(s.rows, dtype=torch.long) if shared else torch.arange(s.rows) // s.rps
        if fault == "neighbour_group":
            idx = ((torch.arange(s.rows) + 1) // s.rps).clamp(max=s.B - 1)
        m = c["mod"].float()
        w = 1.0 + m[:, :s.D]
        w = (w if fault == "skip_w_rounding" else _bf(w))[idx]
        sh = m[:, :s.D][idx] if fault == "scale_for_shift" else m[:, s.D:2 * s.D][idx]
        y = x * r[:, None] * w + sh
    else:
        y = x * r[:, None] * (1.0 + c["scale"])
    return dict(y=_bf(y).double(), rstd=r.double())


def f32_rms_bwd(c, rstd32, order, accum=False, fault=None):
    s = c["spec"]
    x, g, r = c["x"].float(), c["dy"].float(), rstd32.float().view(-1, 1)
    w = _bf(1.0 + c["mod"].float()[:, :s.D])[torch.arange(s.rows) // s.rps] if s.kind == "ada" else (1.0 + c["scale"]).expand(s.rows, s.D)
    gv = g * w
    prod = gv * x
    if fault == "drop_chunk":
        prod = prod.clone()
        prod[:, :8] = 0.0
    cc = sum32(prod, order)[:, None] * r * r * r / s.D
    o = r * gv - x * cc
    if accum:
        old = c["old"].float()
        if fault == "no_accum_chunk":
            old = old.clone()
            old[:, -8:] = 0.0
        o = o + old
    out = dict(dx=_bf(o).double())
    t = g * x * r
    if fault == "drop_row":
        t = t.clone()
        t[s.rows - 1] = 0.0
    if s.kind == "ada":
        dm = c["dmod0"].clone()
        for b_ in range(s.B):
            rows = slice(b_ * s.rps, (b_ + 1) * s.rps)
            dm[b_, :s.D] += colsum32(t[rows], order)
            dm[b_, s.D:2 * s.D] += colsum32(g[rows], order)
        out["dmod"] = dm.double()
    else:
        out["dscale"] = (c["dscale0"] + colsum32(t, order)).double()
    return out


def f32_ln_fwd(c, order, eps=1e-6):
    x, D = c["x"].float(), c["spec"].D
    mean = sum32(x, order) / D
    var = (sum32(x * x, order) / D - mean * mean).clamp(min=0.0)
    r = 1.0 / torch.sqrt(var + eps)
    y = (x - mean[:, None]) * (r[:, None] * c["gamma"]) + c["beta"]
    return dict(y=_bf(y).double(), mean=mean.double(), rstd=r.double())


def f32_ln_bwd(c, mean32, rstd32, order, accum=False, fault=None):
    x, g, D = c["x"].float(), c["dy"].float(), c["spec"].D
    mu, r = mean32.float().view(-1, 1), rstd32.float().view(-1, 1)
    xh, gv = (x - mu) * r, g * c["gamma"]
    s1, s2 = sum32(gv, order)[:, None] / D, sum32(gv * xh, order)[:, None] / D
    o = r * (gv - s1 - xh * s2)
    if accum:
        o = o + c["old"].float()
    dx = _bf(o)
    t = g * xh
    src = o if fault == "dxsum_unrounded" else dx
    return dict(dx=dx.double(), dgamma=(c["dgamma0"] + colsum32(t, order)).double(), dbeta=(c["dbeta0"] + colsum32(g, order)).double(),
                dxsum=(c["dxsum0"] + colsum32(src, order)).double())


# ============================================================================================================ RoPE
RopeCase = namedtuple("RopeCase", "HD NH B T_seg T_total seg_off q_scale")
ROPE_SMALL = (RopeCase(16, 1, 2, 5, 9, 4, 0.25), RopeCase(32, 8, 2, 7, 10, 3, 1.0 / 16), RopeCase(256, 8, 1, 3, 5, 2, 32 ** -0.5),
              RopeCase(16, 8, 2, 6, 8, 2, 32 ** -0.5))
ROPE_ROWFORM = RopeCase(256, 1, 1, 4096, 4096, 0, 1.0 / 16)       # B T_seg HD / 16 = 65536: the per-row form
_ROPE = {}


def rope_case(spec):
    if spec in _ROPE:
        return _ROPE[spec]
    g = gen(*spec)
    rows, W = spec.B * spec.T_seg, (spec.NH + 2) * spec.HD
    pos = torch.randint(0, 2048, (spec.B, spec.T_total), generator=g, dtype=torch.int32)
    pos[0, spec.seg_off:spec.seg_off + 3] = torch.tensor([0, 1, 2047], dtype=torch.int32)
    c = dict(spec=spec, pos=pos, qkv=torch.randn(rows, W, generator=g).bfloat16(), dq=torch.randn(rows, spec.NH * spec.HD, generator=g).bfloat16(),
             dk=torch.randn(rows, spec.HD, generator=g).bfloat16(), dv=torch.randn(rows, spec.HD, generator=g).bfloat16())
    _ROPE[spec] = c
    return c


def _rope_trig(c, dtype):
    """sin, cos [rows, 1, HD / 2] of the case's segment, and (float64 only) their error bound."""
    s = c["spec"]
    half = s.HD // 2
    p = c["pos"][:, s.seg_off:s.seg_off + s.T_seg].reshape(-1, 1, 1)
    i = torch.arange(half, dtype=torch.float32)
    if dtype == torch.float32:
        ts = _pow32(10000.0, (2.0 / s.HD) * i)
        sn, cs = _sincos32(p.float() / ts.view(1, 1, half))
        return sn, cs, None
    ang = p.double() / torch.pow(torch.tensor(10000.0, dtype=torch.float64), (2.0 / s.HD) * i.double()).view(1, 1, half)
    return torch.sin(ang), torch.cos(ang), ang.abs() * (E_POW + 2 * U) + E_SIN


def ref_rope_fwd(c, rounded=True):
    s = c["spec"]
    half, rows = s.HD // 2, s.B * s.T_seg
    x = c["qkv"].double().view(rows, s.NH + 2, s.HD)
    sn, cs, et = _rope_trig(c, torch.float64)
    xr = x[:, :s.NH + 1]
    x1, x2 = xr[..., :half], xr[..., half:]
    rot = torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1)
    qs = f32c(s.q_scale)
    if not rounded:
        return (rot[:, :s.NH] * qs).reshape(rows, -1), rot[:, s.NH], x[:, s.NH + 1]
    e = (x1.abs() + x2.abs()) * et
    d = torch.cat([e + 3 * U * ((x1 * cs).abs() + (x2 * sn).abs()), e + 3 * U * ((x2 * cs).abs() + (x1 * sn).abs())], -1)
    r, dr = _rnd(rot, d)
    q32 = (r[:, :s.NH] * qs).float().double()           # the float32 product of the bf16-rounded rotation
    q, dq = _rnd(q32, dr[:, :s.NH] * qs + U * q32.abs())
    return dict(q=(q.reshape(rows, -1), dq.reshape(rows, -1)), k=(r[:, s.NH], dr[:, s.NH]), v=(x[:, s.NH + 1], None))


def ref_rope_bwd(c):
    s = c["spec"]
    half, rows = s.HD // 2, s.B * s.T_seg
    sn, cs, et = _rope_trig(c, torch.float64)
    qs = f32c(s.q_scale)
    d = torch.cat([(c["dq"].double().view(rows, s.NH, s.HD) * qs).float().double(), c["dk"].double().view(rows, 1, s.HD)], 1)
    d1, d2 = d[..., :half], d[..., half:]
    y = torch.cat([d1 * cs + d2 * sn, d2 * cs - d1 * sn], -1)
    e = (d1.abs() + d2.abs()) * (et + U) + 3 * U * (d1.abs() + d2.abs())
    yr, dy = _rnd(y, torch.cat([e, e], -1))
    out = torch.cat([yr, c["dv"].double().view(rows, 1, s.HD)], 1).reshape(rows, -1)
    bound = torch.cat([dy, torch.zeros(rows, 1, s.HD, dtype=torch.float64)], 1).reshape(rows, -1)
    return dict(dqkv=(out, bound))


def f32_rope_fwd(c, fault=None):
    s = c["spec"]
    half, rows = s.HD // 2, s.B * s.T_seg
    x = c["qkv"].float().view(rows, s.NH + 2, s.HD)
    sn, cs, _ = _rope_trig(c, torch.float32)
    xr = x[:, :s.NH + 1]
    x1, x2 = xr[..., :half], xr[..., half:]
    rot = torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1)
    r = rot if fault == "skip_rot_rounding" else _bf(rot)
    q = _bf(r[:, :s.NH] * torch.tensor(s.q_scale, dtype=torch.float32))
    return dict(q=q.reshape(rows, -1).double(), k=_bf(r[:, s.NH]).double(), v=x[:, s.NH + 1].double())


def f32_rope_bwd(c):
    s = c["spec"]
    half, rows = s.HD // 2, s.B * s.T_seg
    sn, cs, _ = _rope_trig(c, torch.float32)
    d = torch.cat([c["dq"].float().view(rows, s.NH, s.HD) * torch.tensor(s.q_scale, dtype=torch.float32), c["dk"].float().view(rows, 1, s.HD)], 1)
    d1, d2 = d[..., :half], d[..., half:]
    y = _bf(torch.cat([d1 * cs + d2 * sn, d2 * cs - d1 * sn], -1))
    return dict(dqkv=torch.cat([y, c["dv"].float().view(rows, 1, s.HD)], 1).reshape(rows, -1).double())


# ==================================================================================================== GeGLU / GELU
def gelu64(x):
    return 0.5 * x * (1.0 + torch.tanh(K0F * (x + K1F * x ** 3)))


def gelu_grad64(x):
    t = torch.tanh(K0F * (x + K1F * x ** 3))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * (K0F * (1.0 + 3.0 * K1F * x * x))


def _gelu_err(x):
    return 0.5 * x.abs() * (E_TANH + 3 * U + 0.45 * 5 * U) + 2 * U * gelu64(x).abs()


def _gelu_grad_err(x):
    t = torch.tanh(K0F * (x + K1F * x ** 3))
    du = K0F * (1.0 + 3.0 * K1F * x * x)
    A, B = 0.5 * (1.0 + t), 0.5 * x * (1.0 - t * t) * du
    return 0.5 * (E_TANH + 3 * U) + 0.5 * x.abs() * du * (2 * E_TANH + 8 * U) + 8 * U * (A.abs() + B.abs())


def gelu32(x):
    return 0.5 * x * (1.0 + _tanh32(K0F * (x + K1F * x * x * x)))


def gelu_grad32(x):
    t = _tanh32(K0F * (x + K1F * x * x * x))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * (K0F * (1.0 + 3.0 * K1F * x * x))


GEGLU_SHAPES = ((8, 255), (8, 256), (8, 257), (264, 7), (264, 8))        # (H, rows): 255 / 256 / 257 / 231 / 264 chunks of 8
_GEGLU = {}


def geglu_case(H, rows):
    """gu (bf16 [rows, 2 H]) spans [-12, 12] and holds 0 and -0; dact bf16 [rows, H]."""
    if (H, rows) in _GEGLU:
        return _GEGLU[H, rows]
    g = gen("geglu", H, rows)
    gu = (torch.rand(rows, 2 * H, generator=g) * 24.0 - 12.0)
    gu[0, 0], gu[0, 1], gu[0, H], gu[0, H + 1] = 0.0, -0.0, 0.0, -0.0
    gu[-1, 2], gu[-1, 3] = 12.0, -12.0
    c = dict(H=H, rows=rows, gu=gu.bfloat16(), dact=torch.randn(rows, H, generator=g).bfloat16())
    _GEGLU[H, rows] = c
    return c


def ref_geglu_fwd(c, rounded=True):
    H = c["H"]
    g, u = c["gu"].double()[:, :H], c["gu"].double()[:, H:]
    if not rounded:
        return gelu64(g) * u
    ge, dge = _rnd(gelu64(g), _gelu_err(g))
    return dict(act=_rnd(ge * u, dge * u.abs() + U * (ge * u).abs()))


def ref_geglu_bwd(c):
    H = c["H"]
    g, u, d = c["gu"].double()[:, :H], c["gu"].double()[:, H:], c["dact"].double()
    ge, dge = _rnd(gelu64(g), _gelu_err(g))
    gp = gelu_grad64(g)
    dg = _rnd(d * u * gp, (d * u).abs() * _gelu_grad_err(g) + U * (d * u * gp).abs())
    du = _rnd(d * ge, d.abs() * dge + U * (d * ge).abs())
    return dict(dgu=(torch.cat([dg[0], du[0]], 1), torch.cat([dg[1], du[1]], 1)))


def ref_gelu_fwd(x):
    return dict(y=_rnd(gelu64(x.double()), _gelu_err(x.double())))


def ref_gelu_bwd(x, dy):
    x, dy = x.double(), dy.double()
    gp = gelu_grad64(x)
    return dict(dx=_rnd(dy * gp, dy.abs() * _gelu_grad_err(x) + U * (dy * gp).abs()))


def f32_geglu_fwd(c, fault=None):
    H = c["H"]
    g, u = c["gu"].float()[:, :H], c["gu"].float()[:, H:]
    ge = gelu32(g)
    return dict(act=_bf((ge if fault == "skip_gelu_rounding" else _bf(ge)) * u).double())


def f32_geglu_bwd(c):
    H = c["H"]
    g, u, d = c["gu"].float()[:, :H], c["gu"].float()[:, H:], c["dact"].float()
    return dict(dgu=torch.cat([_bf(d * u * gelu_grad32(g)), _bf(d * _bf(gelu32(g)))], 1).double())


# ================================================================================================ gated residual
GATED_RPS = (1, 7, 8, 9, 32, 33, 50)
_GATED = {}


def gated_case(D, rps, B=2):
    if (D, rps, B) in _GATED:
        return _GATED[D, rps, B]
    g = gen("gated", D, rps, B)
    rows = B * rps
    c = dict(D=D, rps=rps, B=B, rows=rows, **{n: torch.randn(rows, D, generator=g).bfloat16() for n in ("x", "u", "dy")},
             gate=torch.randn(B, D, generator=g).bfloat16())
    _GATED[D, rps, B] = c
    return c


def ref_gated_fwd(c, gated=True):
    x, u = c["x"].double(), c["u"].double()
    if not gated:
        return dict(y=_rnd(x + u, U * (x + u).abs()))
    t = bf16r(u * c["gate"].double().repeat_interleave(c["rps"], 0))        # the product is exact in float32: one rounding
    return dict(y=_rnd(x + t, U * (x + t).abs()))


def ref_gated_bwd(c):
    dy, u, gt = c["dy"].double(), c["u"].double(), c["gate"].double().repeat_interleave(c["rps"], 0)
    t = (dy * u).view(c["B"], c["rps"], c["D"])
    depth = cdiv(c["rps"], 8) + 8
    return dict(du=(bf16r(dy * gt), None), dgate=(t.sum(1), depth * U * t.abs().sum(1)))


def f32_gated_fwd(c, gated=True, fault=None):
    x, u = c["x"].float(), c["u"].float()
    if not gated:
        return dict(y=_bf(x + u).double())
    idx = torch.arange(c["rows"]) // c["rps"]
    if fault == "neighbour_group":
        idx = ((torch.arange(c["rows"]) + 1) // c["rps"]).clamp(max=c["B"] - 1)
    t = u * c["gate"].float()[idx]
    return dict(y=_bf(x + (t if fault == "skip_product_rounding" else _bf(t))).double())


def f32_gated_bwd(c, order):
    dy, u, gt = c["dy"].float(), c["u"].float(), c["gate"].float().repeat_interleave(c["rps"], 0)
    t = (dy * u).view(c["B"], c["rps"], c["D"])
    return dict(du=_bf(dy * gt).double(), dgate=sum32(t.permute(0, 2, 1).contiguous(), order).double())


# ============================================================================ embedding, column sums, row copies
def embed_case(D):
    g = gen("embed", D)
    B, T, lo, hi = 2, 5, 10, 30
    tok = torch.randint(lo, hi, (B * T,), generator=g, dtype=torch.int32)
    tok[1], tok[4], tok[7] = lo - 1, hi, 0          # outside the shard window: exact zeros
    tok[2], tok[3] = lo, hi - 1
    stok = torch.randint(0, 6, (B * T,), generator=g, dtype=torch.int32)       # repeated tokens
    return dict(D=D, B=B, T=T, lo=lo, hi=hi, tok=tok, stok=stok, table=torch.randn(hi - lo, D, generator=g), scale=D ** 0.5,
                dtable0=torch.randn(6, D, generator=g), dout=torch.randn(B * 9, D, generator=g).bfloat16(), rps=9, off=3)


def ref_embed_gather(c):
    sc = f32c(c["scale"])
    inside = (c["tok"] >= c["lo"]) & (c["tok"] < c["hi"])
    rows = c["table"].double()[(c["tok"].long() - c["lo"]).clamp(0, c["hi"] - c["lo"] - 1)] * sc
    rows = torch.where(inside[:, None], rows, torch.zeros_like(rows))
    ref, bound = _rnd(rows, U * rows.abs())
    return dict(out=(ref, torch.where(inside[:, None], bound, torch.zeros_like(bound))))


def embed_src_rows(c):
    r = torch.arange(c["B"] * c["T"])
    return (r // c["T"]) * c["rps"] + c["off"] + r % c["T"]


def ref_embed_scatter(c):
    sc = f32c(c["scale"])
    t = c["dout"].double()[embed_src_rows(c)] * sc
    ref, mag = c["dtable0"].double().clone(), c["dtable0"].double().abs()
    ref.index_add_(0, c["stok"].long(), t)
    mag.index_add_(0, c["stok"].long(), t.abs())
    cnt = torch.bincount(c["stok"].long(), minlength=ref.shape[0]).double()[:, None]
    return dict(dtable=(ref, (cnt + 2) * U * mag))


def f32_embed_scatter(c, order):
    t = c["dout"].float()[embed_src_rows(c)] * torch.tensor(c["scale"], dtype=torch.float32)
    out = c["dtable0"].clone()
    idx = range(t.shape[0]) if order == "blocks" else reversed(range(t.shape[0]))
    for r in idx:
        out[int(c["stok"][r])] += t[r]
    return dict(dtable=out.double())


COLSUM_ROWS, COLSUM_COLS = (1, 255, 256, 257, 300), (33, 136, 520)


def colsum_shapes():
    return sorted({(r, 136) for r in COLSUM_ROWS} | {(r, c) for r in (257, 300) for c in COLSUM_COLS})


def colsum_case(rows, cols, dtype):
    g = gen("colsum", rows, cols, str(dtype))
    return dict(x=torch.randn(rows, cols, generator=g).to(dtype), out0=torch.randn(cols, generator=g))


def ref_colsum(c):
    rows = c["x"].shape[0]
    return dict(out=_col(c["x"].double(), c["out0"], min(rows, 256) // 4 + 1 + 4 + cdiv(rows, 256) + 1))


def f32_colsum(c, order, fault=None):
    x = c["x"].float()
    if fault == "drop_row":
        x = x.clone()
        x[-1] = 0.0
    return dict(out=(c["out0"] + colsum32(x, order)).double())


def ref_copy_rows_accumulate(src, dst):
    v = src.double() + dst.double()
    return _rnd(v, U * v.abs())


# =========================================================================================================== cross-entropy
CE_MAIN = dict(R=5, V=1003, ld=1005, chunks=((0, 300), (300, 513), (813, 190)))
CE_ODD = dict(R=5, V=2055, ld=2057, chunks=((0, 3), (3, 1), (4, 2051)))
M_INIT, TL_INIT = -3.0e38, -777.0
_CE = {}


def ce_case(name):
    """Logits float32 [R, V] (the device sees them as a view with row stride ld).  Rows 0-2 of the main case and rows 0-1 of the odd
    one hold ties of the row maximum; row 3 ties across chunks; row 4 holds +-80 and one -inf.  Targets: first / last column of a
    chunk, inside one, and (row 3) outside every chunk."""
    if name in _CE:
        return _CE[name]
    p = dict(CE_MAIN if name == "main" else CE_ODD)
    g = gen("ce", name)
    x = torch.randn(p["R"], p["V"], generator=g) * 3.0
    top = 20.0
    if name == "main":
        x[0, 308] = x[0, 309] = top                 # inside one thread's four (chunk 1, local 8 and 9)
        x[1, 305] = x[1, 377] = top                 # across lanes of one wave
        x[2, 310] = x[2, 600] = top                 # across waves (local 10 and 300)
        x[3, 100] = x[3, 500] = x[3, 900] = top     # across chunks: the earliest keeps it
        target = torch.tensor([300, 812, 0, 5000, 1002], dtype=torch.int32)
    else:
        x[0, 4 + 1030] = x[0, 4 + 21] = top         # lane 1's second step against lane 5's first: the lower index is in the higher lane
        x[1, 1] = x[1, 3] = top                     # the width-3 chunk against the width-1 chunk
        x[2, 3] = top                               # the width-1 chunk holds the maximum
        x[3, 2] = x[3, 2054] = top
        target = torch.tensor([2, 3, 4, -1, 2054], dtype=torch.int32)
    x[4, 7], x[4, p["V"] - 2], x[4, 50 if name == "main" else 1500] = 80.0, -80.0, float("-inf")
    p.update(logits=x, target=target, w=torch.tensor([1.0, 0.5, 0.0, 2.0, 0.25]))
    _CE[name] = p
    return p


def first_argmax(x):
    n = x.shape[-1]
    mx = x.amax(-1, keepdim=True)
    return torch.where(x == mx, torch.arange(n).expand_as(x), torch.full(x.shape, n)).amin(-1).to(torch.int32)


def ref_ce_update(c):
    """State after every chunk of the case in turn, from m = M_INIT, l = 0, tl = TL_INIT."""
    x = c["logits"].double()
    R = x.shape[0]
    m = x.amax(1)
    l = torch.exp(x - m[:, None]).sum(1)
    fin = torch.where(torch.isfinite(x), x, m[:, None].expand_as(x))
    rng = m - fin.amin(1)
    ops = sum(4 * cdiv(vc, 1024) + 6 + 4 + 1 for _, vc in c["chunks"])
    bound = l * (ops * (E_EXP + 3 * U) + 8 * U * rng) + x.shape[1] * 2.0 ** -126
    tl = torch.full((R,), f32c(TL_INIT), dtype=torch.float64)
    seen = torch.zeros(R, dtype=torch.bool)
    for v0, vc in c["chunks"]:
        seen |= (c["target"] >= v0) & (c["target"] < v0 + vc)
    tl[seen] = x[torch.arange(R)[seen], c["target"].long()[seen]]
    return dict(m=(m, None), l=(l, bound), tl=(tl, None), amax=(first_argmax(c["logits"]), None))


def f32_ce_update(c, order, fault=None):
    """The kernel's online (max, sum) in float32: per chunk, (max, sum) pairs are merged in runs of 8 and then pairwise, or pairwise
    throughout, as the wave butterfly does."""
    x = c["logits"]
    R = x.shape[0]
    m, l = torch.full((R,), M_INIT), torch.zeros(R)
    tl, amax = torch.full((R,), TL_INIT), torch.full((R,), -1, dtype=torch.int32)

    def merge(m1, l1, m2, l2):
        nm = torch.maximum(m1, m2)
        return nm, l1 * _exp32(m1 - nm) + l2 * _exp32(m2 - nm)

    for v0, vc in c["chunks"]:
        xc = x[:, v0:v0 + vc]
        pm, pl = xc, torch.ones_like(xc)
        if order == "blocks":       # a thread's run of columns in turn, then pairwise
            pm = torch.nn.functional.pad(pm, (0, (-vc) % BLOCK), value=M_INIT).reshape(R, -1, BLOCK)
            pl = torch.nn.functional.pad(pl, (0, (-vc) % BLOCK), value=0.0).reshape(R, -1, BLOCK)
            am, al = pm[..., 0], pl[..., 0]
            for j in range(1, BLOCK):
                am, al = merge(am, al, pm[..., j], pl[..., j])
            pm, pl = am, al
        n = pm.shape[1]
        p = 1 << max(n - 1, 0).bit_length()
        pm = torch.nn.functional.pad(pm, (0, p - n), value=M_INIT)
        pl = torch.nn.functional.pad(pl, (0, p - n), value=0.0)
        while pm.shape[1] > 1:
            pm, pl = merge(pm[:, 0::2], pl[:, 0::2], pm[:, 1::2], pl[:, 1::2])
        cm, cl = pm[:, 0], pl[:, 0]
        ci = first_argmax(xc)
        if fault == "tie_high":
            ci = (vc - 1 - first_argmax(xc.flip(1))).to(torch.int32)
        take = cm >= m if fault == "later_chunk_takes_tie" else cm > m
        amax = torch.where(take, v0 + ci, amax)
        m, l = merge(m, l, cm, cl)
        t = c["target"].long() - v0
        hit = (t >= 0) & (t < vc)
        tl = torch.where(hit, xc[torch.arange(R), t.clamp(0, vc - 1)], tl)
    return dict(m=m.double(), l=l.double(), tl=tl.double(), amax=amax)


def ref_ce_grad(c, m32, l32, v0, vc):
    """dlogits of one chunk from the float32 state (m, l) handed in: (hi, hi + lo) references and bounds."""
    x = c["logits"].double()[:, v0:v0 + vc]
    m, l, w = m32.double()[:, None], l32.double()[:, None], c["w"].double()[:, None]
    lse = m + torch.log(l)
    e_lse = (E_LOG + 2 * U) * (torch.log(l).abs() + 1.0) + U * lse.abs()      # 2 u: the product with ln 2 inside __logf
    p = torch.exp(x - lse)
    e_p = p * (E_EXP + 4 * U * (x - lse).abs().nan_to_num(posinf=0.0) + e_lse + U) + 2.0 ** -126
    hot = torch.arange(v0, v0 + vc)[None, :] == c["target"].long()[:, None]
    q = p - hot.double()
    dv = w * q
    d = w.abs() * (e_p + U * q.abs()) + U * dv.abs()
    zero = (w == 0).expand_as(dv)
    dv, d = torch.where(zero, torch.zeros_like(dv), dv), torch.where(zero, torch.zeros_like(d), d)
    hi, dhi = _rnd(dv, d)
    return dict(hi=(hi, torch.where(zero, torch.zeros_like(dhi), dhi)), sum=(dv, 2.0 ** -16 * dv.abs() + d + U * dv.abs()))


def f32_ce_grad(c, m32, l32, v0, vc, fault=None):
    if fault == "target_not_subtracted":
        c = dict(c, target=torch.full_like(c["target"], -1))
    x = c["logits"][:, v0:v0 + vc]
    lse = (m32 + _log32(l32))[:, None]
    w = c["w"][:, None]
    p = torch.where(w != 0, _exp32(x - lse), torch.zeros_like(x))
    hot = torch.arange(v0, v0 + vc)[None, :] == c["target"].long()[:, None]
    dv = w * (p - hot.float())
    hi = _bf(dv)
    return dict(hi=hi.double(), sum=hi.double() + _bf(dv - hi).double())


# ----------------------------------------------------------------------------------------- token metrics, row argmax
METRIC_LM = (1, 255, 256, 257, 600)


def metrics_case(Lm, with_sel, with_masks=True, B=2):
    g = gen("metrics", Lm, with_sel, with_masks)
    Ls = max(1, (Lm * 2) // 3) if with_sel else Lm
    c = dict(B=B, Lm=Lm, Ls=Ls, pred=torch.randint(0, 3, (B * Ls,), generator=g, dtype=torch.int32),
             target=torch.randint(0, 3, (B * Ls,), generator=g, dtype=torch.int32), nll=torch.rand(B * Ls, generator=g) * 5.0,
             lm=(torch.rand(B, Lm, generator=g) * (torch.rand(B, Lm, generator=g) < 0.7)).float(), sel=None)
    for n in ("crit", "num", "dir"):
        c[n] = (torch.rand(B, Lm, generator=g) < 0.3) if with_masks and n != "dir" else None        # dir: a NULL mask counts zero
    if with_sel:
        sel = torch.stack([torch.randperm(Lm, generator=g)[:Ls] for _ in range(B)]).to(torch.int32)
        sel[0, 0] = -1
        if Ls > 1:
            sel[1, Ls - 1] = Lm
        c["sel"] = sel
    return c


def ref_token_metrics(c, fault=None):
    """(per_token_loss float32 [B, Lm], counts float32 [B, 4, 2]): both exact."""
    B, Lm, Ls = c["B"], c["Lm"], c["Ls"]
    ptl = torch.zeros(B, Lm)
    counts = torch.zeros(B, 4, 2)
    masks = [c["lm"] != 0] + [c[n] if c[n] is not None else torch.zeros(B, Lm, dtype=torch.bool) for n in ("crit", "num", "dir")]
    for k in range(4):
        counts[:, k, 1] = masks[k].sum(1).float()
    for b in range(B):
        for j in range(Ls):
            r = b * Ls + j
            p = int(c["sel"][b, j]) if c["sel"] is not None else j
            if p < 0 or p >= Lm:
                if fault != "count_skipped_rows":
                    continue
                p = min(max(p, 0), Lm - 1)
            ptl[b, p] = c["nll"][r] * c["lm"][b, p]
            ok = float(c["pred"][r] == c["target"][r])
            for k in range(4):
                if bool(masks[k][b, p]):
                    counts[b, k, 0] += ok
    return ptl, counts


ARGMAX_N = (1, 255, 256, 257, 1000)


def argmax_case(n):
    """float32 [6, n]: ties inside one thread's stride (c, c + 256), across lanes, across waves; an all -inf row (index 0)."""
    g = gen("argmax", n)
    x = torch.randn(6, n, generator=g)
    if n >= 257:
        x[0, 0] = x[0, 256] = 9.0
    if n >= 1000:
        x[0, 0] = -1.0
        x[0, 300] = x[0, 556] = 9.0                # thread 44, its second and third column
    if n >= 255:
        x[1, 70] = x[1, 3] = 9.0                   # lanes 6 and 3 of wave 1 and wave 0 ... (70 = wave 1)
        x[2, 5] = x[2, 40] = 9.0                   # two lanes of wave 0
        x[3, 200] = x[3, 130] = 9.0                # waves 3 and 2
    x[4] = float("-inf")
    x[5, n - 1] = 9.0
    return x


# ============================================================================================== sum of squares, AdamW
SUMSQ_F32 = (1, 255, 4095, 4096, 4097, 12293, 2 * 2048 * 4096 + 4099)
SUMSQ_BF16 = (1, 8191, 8192, 8193, 16401, 2 * 2048 * 8192 + 8195)


def sumsq_case(n, dtype):
    g = gen("sumsq", n, str(dtype))
    return dict(x=torch.randn(n, generator=g).to(dtype), out0=torch.tensor([3.25]))


def ref_sumsq(c):
    x, n = c["x"].double(), c["x"].numel()
    chunk = 4096 if c["x"].dtype == torch.float32 else 8192
    blocks = min(cdiv(n, chunk), 2048)
    iters = cdiv(cdiv(n, chunk), blocks)
    depth = (chunk // 256) * iters + 16 + 2 + 6 + 4 + blocks + 1 + 1        # per-thread chain (tail: 16), a0..a3, wave, block, atomics, x^2
    tot = (x * x).sum() + c["out0"].double()
    return dict(out=(tot, depth * U * tot.abs()))


def f32_sumsq(c, order, fault=None):
    x = c["x"].float()
    if fault == "drop_tail":
        x = x[:-1]
    sq = x * x
    chunk = 4096
    if order == "blocks" and sq.numel() > chunk:          # blocks of 4096 in turn, pairwise inside
        pad = cdiv(sq.numel(), chunk) * chunk - sq.numel()
        part = sum32(torch.nn.functional.pad(sq, (0, pad)).view(-1, chunk), "tree")
        acc = c["out0"].clone()
        for b in range(0, part.numel(), 64):
            acc = acc + sum32(part[b:b + 64][None], "tree")
        return dict(out=acc.double()[0])
    return dict(out=(c["out0"] + sum32(sq[None], order if sq.numel() <= chunk else "tree")).double()[0])


ADAM_N = (2, 510, 512, 514, 300006)
ADAM_HP = dict(b1=0.9, b2=0.95, eps=1e-8, wd=1e-4, lr=1e-3, ed=0.99, step=3)


def adam_case(n, clip="clipped", ema="on", gdtype=torch.float32):
    """clip: clipped (gnorm > max_norm = 1) | below (gnorm < max_norm = 1e6) | off (max_norm = 0).  ema: on | flag0 | none.
    Some v and g are zero (sqrt at 0)."""
    g_ = gen("adam", n)
    p, m = torch.randn(n, generator=g_), 0.1 * torch.randn(n, generator=g_)
    v, g = torch.randn(n, generator=g_).abs(), (3.0 * torch.randn(n, generator=g_)).to(gdtype)
    v[0], g[0], m[0] = 0.0, 0.0, 0.0
    h = ADAM_HP
    sumsq = float((g.double() ** 2).sum())
    sc = torch.tensor([sumsq, h["lr"], 1 - h["b1"] ** h["step"], 1 - h["b2"] ** h["step"], h["ed"], 0.0 if ema == "flag0" else 1.0, 0.0, 0.0])
    return dict(n=n, p=p, m=m, v=v, g=g, ema=p + 0.1, sc=sc, max_norm={"clipped": 1.0, "below": 1.0e6, "off": 0.0}[clip], clip=clip, ema_mode=ema)


def _sqrt_err(a, d):
    return torch.minimum(d / (2.0 * a.sqrt()).clamp(min=1e-300), d.sqrt())


def ref_adamw(c):
    h = ADAM_HP
    b1, b2, eps, wd = (f32c(h[k]) for k in ("b1", "b2", "eps", "wd"))
    sc = c["sc"].double()
    p, m, v, g, ema = (c[k].double() for k in ("p", "m", "v", "g", "ema"))
    gnorm = math.sqrt(float(sc[0]))
    mn = f32c(c["max_norm"])
    clipped = not (mn <= 0.0 or gnorm < mn)
    clip, kc = (mn / gnorm, 3) if clipped else (1.0, 0)         # sqrt, division, and the product with g
    lr, rbc1, rbc2, ed = float(sc[1]), 1.0 / float(sc[2]), 1.0 / float(sc[3]), float(sc[4])
    ob1, ob2, oed = f32c(1.0 - b1), f32c(1.0 - b2), f32c(1.0 - ed)     # 1 - b in float32: a rounding of its own, counted below
    gg = g * clip
    m2 = b1 * m + (1.0 - b1) * gg
    e_m = (kc + 4) * U * ((b1 * m).abs() + ((1.0 - b1) * gg).abs()) + abs(ob1 - (1.0 - b1)) * gg.abs()
    v2 = b2 * v + (1.0 - b2) * gg * gg
    e_v = (2 * kc + 5) * U * ((b2 * v).abs() + (1.0 - b2) * gg * gg) + abs(ob2 - (1.0 - b2)) * gg * gg
    mh, vh = m2 * rbc1, v2 * rbc2
    e_mh, e_vh = e_m * rbc1 + 2 * U * mh.abs(), e_v * rbc2 + 2 * U * vh
    s = vh.sqrt()
    den = s + eps
    e_den = _sqrt_err(vh, e_vh) + E_SQRT * s + U * den
    q = mh / den
    e_q = e_mh / den + q.abs() * e_den / (den - e_den).clamp(min=eps / 2) + (E_RCP + 2 * U) * q.abs()
    upd = q + wd * p
    e_u = e_q + 2 * U * (wd * p).abs() + U * (q.abs() + (wd * p).abs())
    p2 = p - lr * upd
    e_p = lr * e_u + U * (lr * upd).abs() + U * (p.abs() + (lr * upd).abs())
    out = dict(p=(p2, e_p), m=(m2, e_m), v=(v2, e_v))
    if c["ema_mode"] == "on":
        e2 = ed * ema + (1.0 - ed) * p2
        out["ema"] = (e2, (1.0 - ed) * e_p + 3 * U * ((ed * ema).abs() + ((1.0 - ed) * p2).abs()) + abs(oed - (1.0 - ed)) * p2.abs())
    return out


def f32_adamw(c, fault=None):
    h = ADAM_HP
    t = lambda z: torch.tensor(z, dtype=torch.float32)      # noqa: E731
    b1, b2, eps, wd, mn = t(h["b1"]), t(h["b2"]), t(h["eps"]), t(h["wd"]), t(c["max_norm"])
    sc = c["sc"]
    gnorm = _sqrt32(sc[0])
    keep = bool(mn <= 0) or bool(gnorm < mn)
    if fault == "clip_below":
        keep = bool(mn <= 0)
    clip = t(1.0) if keep else mn / gnorm
    lr, rbc1, rbc2, ed = sc[1], 1.0 / sc[2], 1.0 / sc[3], sc[4]
    if fault == "no_bias_correction":
        rbc1 = rbc2 = t(1.0)
    p, m, v, ema = c["p"], c["m"], c["v"], c["ema"]
    gg = c["g"].float() * clip
    m2 = b1 * m + (1.0 - b1) * gg
    v2 = b2 * v + (1.0 - b2) * gg * gg
    upd = (m2 * rbc1) * _rcp32(_sqrt32(v2 * rbc2) + eps) + wd * p
    p2 = p - lr * upd
    out = dict(p=p2.double(), m=m2.double(), v=v2.double())
    ema_on = c["ema_mode"] == "on" or (fault == "ema_ignores_flag" and c["ema_mode"] == "flag0")
    out["ema"] = (ed * ema + (1.0 - ed) * p2).double() if ema_on else ema.double()
    hi = _bf(p2)
    out["p16"], out["p16lo"] = hi.double(), _bf(p2 - (p2 if fault == "skip_hi_rounding" else hi)).double()
    return out


def p16_planes(p_dev):
    """(p16, p16lo) as float64 from the device's own float32 p: bf16(p) and bf16(p - bf16(p)), both exact restatements."""
    hi = p_dev.float().bfloat16()
    return hi.double(), (p_dev.float() - hi.float()).bfloat16().double()


def drop_caches():
    for d in (_NORM, _ROPE, _GEGLU, _GATED, _CE):
        d.clear()


# ================================================================================= one allocation, guards, sentinels
Region = namedtuple("Region", "off dtype rows width rs")      # off: bytes from the start of the arena to the first valid element
SENT = {torch.bfloat16: -24576.0, torch.float32: -12345.0, torch.int32: 0x5A5A5A5A, torch.uint8: 0x5A}
GUARD = 512       # bytes of guard in front of and behind every buffer


class Arena:
    """Every buffer of a case in one uint8 allocation.  add(): an input sits between NaN guards (integers: zeros, which index
    nothing out of range), with NaN in the padding columns of a strided view; an output is pre-filled with its sentinel, padding
    columns and guards included, under the start values given.  Every buffer starts 16-byte aligned, plus `shift` elements."""

    def __init__(self):
        self.chunks, self.regions, self.pos = [], {}, 0

    def add(self, name, dtype, rows, width, rs=None, data=None, out=False, shift=0):
        rs = width if rs is None else rs
        isz = torch.empty(0, dtype=dtype).element_size()
        g = GUARD // isz
        body = rows * rs
        fill = SENT[dtype] if out else (0 if dtype in (torch.int32, torch.uint8) else float("nan"))
        buf = torch.full((g + shift + body + g,), fill, dtype=dtype)
        if data is not None:
            torch.as_strided(buf, (rows, width), (rs, 1), g + shift).copy_(data.reshape(rows, width).to(dtype))
        raw = buf.view(torch.uint8)
        pad = (-raw.numel()) % 16
        self.regions[name] = Region(self.pos + (g + shift) * isz, dtype, rows, width, rs)
        self.chunks.append(torch.cat([raw, torch.full((pad,), 0x5A, dtype=torch.uint8)]))
        self.pos += self.chunks[-1].numel()
        return self

    def build(self):
        return torch.cat(self.chunks), self.regions


def view(arena, r):
    """The [rows, width] window of a region in `arena` (uint8, any device); shares memory with it."""
    isz = torch.empty(0, dtype=r.dtype).element_size()
    n = (r.rows - 1) * r.rs + r.width
    return torch.as_strided(arena[r.off:r.off + n * isz].view(r.dtype), (r.rows, r.width), (r.rs, 1))


def untouched(before, after, regions, written, windows=()):
    """True when `after` equals `before` byte for byte outside the windows of the regions named in `written` and the extra
    `windows` (Region tuples)."""
    free = torch.ones(before.numel(), dtype=torch.bool)
    for r in [regions[n] for n in written] + list(windows):
        isz = torch.empty(0, dtype=r.dtype).element_size()
        n = (r.rows - 1) * r.rs + r.width
        torch.as_strided(free[r.off:r.off + n * isz].view(-1, isz), (r.rows, r.width, isz), (r.rs * isz, isz, 1)).fill_(False)
    return torch.equal(before[free], after[free])


def sub(r, row0=0, rows=None, col0=0, width=None):
    """A window of a region: rows [row0, row0 + rows), columns [col0, col0 + width)."""
    isz = torch.empty(0, dtype=r.dtype).element_size()
    return Region(r.off + (row0 * r.rs + col0) * isz, r.dtype, r.rows - row0 if rows is None else rows, r.width - col0 if width is None else width, r.rs)
