"""Element-wise criteria, float64 references and committed inputs for the fused decode kernels (csrc/decode.hip), shared by
tests/test_decode_reference_gpu.py (device against reference) and tests/test_decode_reference_cpu.py (the criteria against
corrupted references).  Everything here is plain torch on the CPU; nothing calls lap_amd.hip."""
import torch

U24 = 2.0 ** -24
DEPTH = 64              # bounds the depth of every summation tree of the kernels: <= 32 fmas per lane, 6 wave levels, 4 K slices, hi + lo
TIE_MARGIN = 2.0 ** -19    # relative clearance of every normalised h from a bf16 rounding tie (see settle_gamma)
DD, DNH, DHD, DH = 2048, 8, 256, 16384


def bf16r(x):
    """A bf16 rounding point restated in float64."""
    return x.to(torch.bfloat16).double()


def ulp_bf16(x):
    """Spacing of the bfloat16 numbers at |x| (float64; 2^-133 at zero and in the subnormal range)."""
    _, e = torch.frexp(x.abs().double())
    e = torch.where(x == 0, torch.full_like(e, -125), e)
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), (e - 8).clamp(min=-133))


def worst_ratio(dev, ref, bound):
    """max |dev - ref| / bound; inf when the device value is not finite."""
    err = (dev.detach().double().cpu() - ref).abs()
    ratio = torch.where(torch.isfinite(err), err / bound, torch.full_like(err, float("inf")))
    return float(ratio.max())


def differing_share(dev, ref):
    """Share of elements that differ from the reference at all."""
    return float((dev.detach().double().cpu() != ref).double().mean())


def check_elementwise(dev, ref, bound, cap=None, what=""):
    """(a) every element within its own bound; (b) at most `cap` of the elements differ from `ref` at all.  Prints and returns
    (worst error / bound, differing share)."""
    ratio, share = worst_ratio(dev, ref, bound), differing_share(dev, ref)
    print(f"{what}: worst error / bound {ratio:.3f}, differing share {share:.2e}" + (f" (cap {cap:.2e})" if cap is not None else ""))
    assert ratio <= 1.0, (what, "element bound", ratio)
    if cap is not None:
        assert share <= cap, (what, "differing share", share, cap)
    return ratio, share


def _rnd(v, d):
    """One bf16 rounding point: the rounded value, and the bound on |device - reference| after it when it was d before it
    (rounding is monotone, so two values d apart round to numbers at most d + one spacing apart)."""
    return bf16r(v), d + ulp_bf16(v.abs() + d)


def dot_and_sens(h, w, chunk=4096):
    """h [B, K], w [N, K] (any dtype, taken to float64) -> (h w^T, S = |h| |w|^T), both [B, N] float64."""
    h = h.double()
    out, sens = [], []
    for n0 in range(0, w.shape[0], chunk):
        wc = w[n0:n0 + chunk].double()
        out.append(h @ wc.T)
        sens.append(h.abs() @ wc.abs().T)
    return torch.cat(out, 1), torch.cat(sens, 1)


def norm_rows64(x, gamma, eps=1e-6):
    """R64 of the RMSNorm prologue: x r (1 + gamma), r = 1 / sqrt(mean(x^2) + eps), unrounded."""
    xd = x.double()
    return xd * (xd.pow(2).mean(1, keepdim=True) + eps).rsqrt() * (1.0 + gamma.double())


def tie_distance(v):
    """Relative distance of every element of v (float64) from the nearest bf16 rounding tie."""
    m, _ = torch.frexp(v.abs())
    s = m * 256.0                                   # in [128, 256): bf16 numbers are the integers, ties the half-integers
    return ((s - s.floor()) - 0.5).abs() / s.clamp(min=1.0)


def settle_gamma(x, gamma, eps=1e-6):
    """The normalised row h = bf16(x r (1 + gamma)) is the kernels' first rounding point, and the kernels compute its argument in
    float32 (relative error below 2^-20: ~18 roundings in the sum of squares, halved by the square root, and 6 more).  An h within
    that of a rounding tie could round either way, which neither criterion is about.  So gamma (float32, an input) is nudged by
    2^-12 where any row has such an element, until every |h| keeps TIE_MARGIN (2^-19, relative) from every tie: the reference's h
    is then the kernel's h, bit for bit.  Returns the settled gamma."""
    gamma = gamma.clone()
    for _ in range(64):
        close = (tie_distance(norm_rows64(x, gamma, eps)) < TIE_MARGIN).any(0)
        if not bool(close.any()):
            return gamma
        gamma[close] += 2.0 ** -12
    raise AssertionError("settle_gamma did not converge")


def gelu_tanh64(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x ** 3)))


def ref_residual(a, w, res, rounded=True, depth=DEPTH):
    """proj_res: y = bf16(a W^T + res).  One rounding point (n = 1).  Returns (R16, bound) or R64.  depth: the summation depth of
    the kernel under test (the decode kernels': DEPTH), here and in ref_gate_up / ref_qkv."""
    dot, sens = dot_and_sens(a, w)
    y = dot + res.double()
    return _rnd(y, depth * U24 * sens) if rounded else y


def ref_gate_up(h, w, H, rounded=True, depth=DEPTH):
    """gate_up on the normalised rows h [B, D] (float64): act = bf16(bf16(gelu(bf16 g)) * bf16 u), g | u = h W^T.  Four rounding
    points (n = 4: g, u, gelu, the stored product), each entering with its gain: gelu's slope is at most 1.13, and the float32
    form 0.5 x (1 + tanh(.)) carries an absolute error of up to 2^-23 |g| from the cancellation in its negative tail."""
    dot, sens = dot_and_sens(h, w)
    if not rounded:
        return gelu_tanh64(dot[:, :H]) * dot[:, H:]
    d0 = depth * U24 * sens
    g, dg = _rnd(dot[:, :H], d0[:, :H])
    u, du = _rnd(dot[:, H:], d0[:, H:])
    ge, dge = _rnd(gelu_tanh64(g), 1.13 * dg + g.abs() * 2.0 ** -23)
    return _rnd(ge * u, dge * u.abs() + ge.abs() * du + dge * du)


def ref_qkv(h, w, pos, NH, HD, q_scale, rounded=True, depth=DEPTH):
    """qkv on the normalised rows h [B, D] (float64), positions pos [B]: x = bf16(h W^T); q and k heads r = bf16(RoPE(x)), q
    scaled by q_scale (a power of two here: exact, and so is the store); v = x.  Rounding points: projection and rotation for q / k
    (n = 2 with gains |cos| and |sin|; the store the header lists is exact), projection alone for v (n = 1).  The float32 angle
    pos / 10000^(2 i / HD) is off by up to 2^-22 pos (powf, the division) and sincosf by 2^-22: that enters with |x1| + |x2|.
    Returns (q [B, NH HD], k [B, HD], v [B, HD]), each (R16, bound), or the three R64."""
    B, half = h.shape[0], HD // 2
    dot, sens = dot_and_sens(h, w)
    dot, d0 = dot.view(B, NH + 2, HD), (depth * U24 * sens).view(B, NH + 2, HD)
    ang = pos.double().view(B, 1, 1) / (10000.0 ** (2.0 * torch.arange(half, dtype=torch.float64) / HD)).view(1, 1, half)
    sn, cs = torch.sin(ang), torch.cos(ang)

    def rot(x):
        x1, x2 = x[..., :half], x[..., half:]
        return torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1)

    if not rounded:
        r = rot(dot[:, :NH + 1])
        return (r[:, :NH] * q_scale).reshape(B, NH * HD), r[:, NH], dot[:, NH + 1]
    x, d = _rnd(dot, d0)
    xr, dr = x[:, :NH + 1], d[:, :NH + 1]
    mag = xr[..., :half].abs() + xr[..., half:].abs()
    dang = mag * (pos.double().view(B, 1, 1) + 1.0) * 2.0 ** -22
    dr = torch.cat([cs.abs() * dr[..., :half] + sn.abs() * dr[..., half:] + dang,
                    cs.abs() * dr[..., half:] + sn.abs() * dr[..., :half] + dang], -1)
    r, dr = _rnd(rot(xr), dr)
    return (((r[:, :NH] * q_scale).reshape(B, NH * HD), (dr[:, :NH] * q_scale).reshape(B, NH * HD)),
            (r[:, NH], dr[:, NH]), (x[:, NH + 1], d[:, NH + 1]))


def ref_logits(h, planes):
    """LM head: R64 of sum_p plane_p . h on the bf16-rounded normalised rows h (the one rounding point), and the bound
    DEPTH 2^-24 S with S = sum_p |plane_p| |h|."""
    dot = sens = 0.0
    for p in planes:
        d, s = dot_and_sens(h, p)
        dot, sens = dot + d, sens + s
    return dot, DEPTH * U24 * sens


def ref_attention(q, pk, pv, allowed, gk, gv, t, drop=None):
    """R64 of the decode attention of one step: q [B, NH HD]; prefix keys / values [B, Pn, HD] with `allowed` [B, Pn] (bool);
    generated keys / values [B, cap, HD], of which the first t are attended.  Softmax over the allowed keys with no rounding of
    the weights.  drop = (b, j): sample b does not see generated key j (a corrupted reference).  Returns (o [B, NH HD], A [B, NH HD] = sum_j softmax_j |v_jd|)."""
    B = q.shape[0]
    qd = q.double().view(B, DNH, DHD)
    k = torch.cat([pk.double(), gk[:, :t].double()], 1)
    v = torch.cat([pv.double(), gv[:, :t].double()], 1)
    ok = torch.cat([allowed, torch.ones(B, t, dtype=torch.bool)], 1)
    if drop is not None:
        ok[drop[0], allowed.shape[1] + drop[1]] = False
    k, v = torch.where(ok[..., None], k, 0.0), torch.where(ok[..., None], v, 0.0)       # masked rows may hold anything, NaN included
    s = torch.einsum("bhd,bjd->bhj", qd, k).masked_fill(~ok[:, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    return torch.einsum("bhj,bjd->bhd", p, v).reshape(B, -1), torch.einsum("bhj,bjd->bhd", p, v.abs()).reshape(B, -1)


def query_allows(kinfo):
    """The decode query (class 1, index 0xFFFFFF: no key's 24-bit index is above it) against key words: the classes share bit 0."""
    return ((kinfo >> 24) & 1) != 0


# ---- float32 restatements of the projections in three summation orders (the measurement behind the differing-share caps)
def _acc_f32(h, w, order):
    """h [B, K], w [N, K] float32 holding bf16 values (every product is exact in float32, so add-after-multiply is the fma)."""
    B, K = h.shape
    if order == "sequential":
        wt = w.T.contiguous()
        acc = torch.zeros(B, w.shape[0])
        for k in range(K):
            acc = acc + h[:, k:k + 1] * wt[k]
        return acc
    out = []
    for n0 in range(0, w.shape[0], 512):
        p = h[:, None, :] * w[None, n0:n0 + 512, :]
        if order == "lanes":                        # k = 512 i + 8 lane + e: 8 per lane per load, in turn, then a tree over the lanes
            p = p.view(B, -1, K // 512, 64, 8).permute(0, 1, 3, 2, 4).reshape(B, -1, 64, K // 64)
            acc = torch.zeros(p.shape[:-1])
            for j in range(p.shape[-1]):
                acc = acc + p[..., j]
            p = acc
        while p.shape[-1] > 1:
            p = p[..., 0::2] + p[..., 1::2]
        out.append(p[..., 0])
    return torch.cat(out, 1)


F32_ORDERS = ("sequential", "pairwise", "lanes")
# (kind, fp8, N): the number of elements (of those at B = 8) at which a float32 order differs from the float64 R16, per order; the
# cap on the device's differing share is 4 x the largest share.  tests/test_decode_reference_cpu.py measures them again.
DIFFERING = {("res2048", False, None): ((4, 1, 0), 16384), ("res2048", True, None): ((0, 0, 0), 16384),
             ("res16384", False, None): ((9, 2, 3), 16384), ("res16384", True, None): ((4, 1, 2), 16384),
             ("qkv", False, None): ((19, 21, 19), 20480), ("qkv", True, None): ((19, 18, 19), 20480),
             ("gate_up", False, None): ((52, 23, 18), 131072), ("gate_up", True, None): ((1280, 1283, 1287), 131072),
             ("res2048", False, 4098): ((9, 0, 2), 32784), ("res2048", True, 4098): ((0, 1, 0), 32784)}


def share_cap(kind, fp8, N=None):
    counts, numel = DIFFERING[kind, fp8, N]
    return 4.0 * max(counts) / numel


def projection_reference(kind, c):
    """(R16, bound) of projection `kind` on case c, the outputs concatenated as f32_projection does."""
    if kind.startswith("res"):
        return ref_residual(c["a"], c["wd"], c["res"])
    if kind == "gate_up":
        return ref_gate_up(c["h16"], c["wd"], DH)
    parts = ref_qkv(c["h16"], c["wd"], c["pos"], DNH, DHD, c["q_scale"])
    return torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1)


def measure_differing(kind, fp8, N=None):
    c = decode_case(kind, fp8, N)
    r, _ = projection_reference(kind, c)
    return tuple(int((f32_projection(kind, c, o) != r).sum()) for o in F32_ORDERS), r.numel()


def f32_projection(kind, case, order):
    """The bf16 output(s) of projection `kind` on `case` (decode_case) with float32 accumulation in `order` and a float32
    epilogue, as float64, concatenated along the last axis in the order the test compares them."""
    f = torch.float32
    w = case["wd"].to(f)
    if kind.startswith("res"):
        return (_acc_f32(case["a"].to(f), w, order) + case["res"].to(f)).to(torch.bfloat16).double()
    h = case["h16"].to(f)
    dot = _acc_f32(h, w, order).to(torch.bfloat16).to(f)
    if kind == "gate_up":
        g, u = dot[:, :DH], dot[:, DH:]
        ge = (0.5 * g * (1.0 + torch.tanh(0.7978845608028654 * (g + 0.044715 * g * g * g)))).to(torch.bfloat16).to(f)
        return (ge * u).to(torch.bfloat16).double()
    B, half = h.shape[0], DHD // 2
    x = dot.view(B, DNH + 2, DHD)
    ts = torch.pow(torch.tensor(10000.0), (2.0 / DHD) * torch.arange(half, dtype=f))
    ang = case["pos"].to(f).view(B, 1, 1) / ts.view(1, 1, half)
    sn, cs = torch.sin(ang), torch.cos(ang)
    x1, x2 = x[:, :DNH + 1, :half], x[:, :DNH + 1, half:]
    r = torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1).to(torch.bfloat16).to(f)
    return torch.cat([(r[:, :DNH] * case["q_scale"]).reshape(B, -1), r[:, DNH], x[:, DNH + 1]], 1).to(torch.bfloat16).double()


# ---- the committed inputs (CPU generator, so that what is measured on the CPU is what the device is given)
QKV_CAP, QKV_T = 40, 18
_CASES = {}


def alternate_rows(w):
    """w [N, K] with its even rows scaled by 2^6 and its odd rows by 2^-6: neighbouring rows 12 binades apart."""
    s = torch.where(torch.arange(w.shape[0]) % 2 == 0, 64.0, 1.0 / 64.0).to(torch.float32)
    return (w.float() * s[:, None]).to(w.dtype)


def fp8_rows(w, alternate=True):
    """w bf16 / f32 [N, K], by default through alternate_rows, quantised with lap_amd/fp8.py on the host -> (codes, scales, the
    dequantised weights as float64)."""
    from lap_amd import fp8 as F8

    codes, scales = F8.quantize_rows(alternate_rows(w) if alternate else w)
    return codes, scales, F8.dequantize_rows(codes, scales, torch.float32).double()


def decode_case(kind, fp8=False, N=None):
    """Inputs of one projection at B = 8 (smaller batches take the first rows: a row's result does not depend on B) with the
    float64 references.  kind: qkv | gate_up | res2048 | res16384; N: the output width of a res kind (default 2048).  Row b of the
    activations is scaled by 1 + b."""
    key = (kind, fp8, N)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(1000 + 10 * ("qkv", "gate_up", "res2048", "res16384").index(kind) + (1 if fp8 else 0) + 7 * (N or 0))
    rows = (1.0 + torch.arange(8.0)).view(8, 1)
    c = {"kind": kind, "fp8": fp8}
    if kind.startswith("res"):
        K, N = int(kind[3:]), N or 2048
        c["a"] = (torch.randn(8, K, generator=g) * rows).to(torch.bfloat16)
        c["res"] = (torch.randn(8, N, generator=g) * rows).to(torch.bfloat16)
        w = (torch.randn(N, K, generator=g) * (0.02 if K == 2048 else 0.01)).to(torch.bfloat16)
    else:
        N = (DNH + 2) * DHD if kind == "qkv" else 2 * DH
        c["x"] = (torch.randn(8, DD, generator=g) * rows).to(torch.bfloat16)
        w = (torch.randn(N, DD, generator=g) * 0.02).to(torch.bfloat16)
        c["gamma"] = settle_gamma(c["x"], torch.randn(DD, generator=g) * 0.1)
        c["h16"] = bf16r(norm_rows64(c["x"], c["gamma"]))
    if fp8:
        c["codes"], c["scales"], c["wd"] = fp8_rows(w)
    else:
        c["w"], c["wd"] = w, w.double()
    if kind == "qkv":
        c["plen"] = torch.tensor([800, 3, 257, 512, 64, 799, 1, 130], dtype=torch.int32)
        c["pos"] = c["plen"] + QKV_T - 1
        c["q_scale"] = DHD ** -0.5
    _CASES[key] = c
    return c


def hilo_planes(table):
    """The bf16 hi / lo planes of an f32 table: hi = bf16(x), lo = bf16(x - hi)."""
    hi = table.to(torch.bfloat16)
    return hi, (table - hi.float()).to(torch.bfloat16)


LM_FORMS = ("hilo", "hi", "fp8")


def lm_case(V, form, dup=False):
    """LM-head inputs at B = 8: an f32 table of std 0.03 as hi / lo bf16 planes (`hilo`), the hi plane alone (`hi`, lo=None) or
    e4m3 codes (`fp8`, alternate rows scaled by 2^+-6), with R64 of the logits on the planes and its bound.  dup: the row that
    wins sample 0 is copied to a lower index and to the last (odd) row; `ref` then holds equal logits at the three."""
    key = ("lm", V, form, dup)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(2000 + V)
    c = {"V": V, "form": form}
    table = torch.randn(V, DD, generator=g) * 0.03
    c["table"] = table = alternate_rows(table) if form == "fp8" else table
    c["x"] = (torch.randn(8, DD, generator=g) * (1.0 + torch.arange(8.0)).view(8, 1)).to(torch.bfloat16)
    c["gamma"] = settle_gamma(c["x"], torch.randn(DD, generator=g) * 0.1)
    c["h16"] = bf16r(norm_rows64(c["x"], c["gamma"]))
    if dup:
        best = int(lm_case(V, form)["ref"][0].argmax())
        c["dups"] = sorted({7 if best > 7 else best + 1, best, V - 1 if best != V - 1 else V - 2})
        table = table.clone()
        table[c["dups"]] = table[best].clone()
        c["table"] = table
    if form == "fp8":
        c["codes"], c["scales"], wd = fp8_rows(table, alternate=False)
        c["planes"] = [wd]
    else:
        c["hi"], c["lo"] = hilo_planes(table)
        c["planes"] = [c["hi"], c["lo"]] if form == "hilo" else [c["hi"]]
    c["ref"], c["bound"] = ref_logits(c["h16"], c["planes"])
    if dup:
        c["ref"][:, c["dups"]] = c["ref"][:, c["dups"][:1]]         # identical rows: identical logits, whatever the BLAS blocking
    _CASES[key] = c
    return c


def first_argmax(a):
    """Lowest index of the row maximum (numpy's argmax rule), int64 [rows]."""
    import numpy as np

    return torch.from_numpy(np.argmax(a.numpy(), axis=1))


def top2_margin(a):
    """Row-wise gap between the row maximum and the largest value below it (exact copies of the best row count as the best)."""
    best = a.max(1).values
    return best - a.masked_fill(a == best[:, None], float("-inf")).max(1).values


def check_tokens(tok, ref, bound, what=""):
    """Tokens against the float64 logits `ref` [B, V] with their bound [B, V]: the lowest index of the row maximum wherever the
    top-2 margin exceeds twice the logit bound; below that either of the top two.  Returns how many rows used that allowance."""
    want, clear = first_argmax(ref), top2_margin(ref) > 2 * bound.max(1).values
    second = ref.scatter(1, want[:, None], float("-inf")).argmax(1)
    tok = tok.long().cpu()
    ok = (tok == want) | (~clear & (tok == second))
    assert bool(ok.all()), (what, tok.tolist(), want.tolist())
    return int((tok != want).sum())


ATTN_SHAPES = ((157, 40), (16, 16))
ATTN_REGIMES = {"flat": 0.5, "peaked": 4.0}        # the std of the scores


def attn_kinfo(Pn):
    """Key words [8, Pn] in the prefill's vocabulary: ((pm | pm << 1) << 24) | cumsum(pm), that is class 0 (padding and holes) and
    class 3 keys with their running index; a left-padding run of 35 keys (5 at Pn = 16): two whole masked chunks and a partial
    one; class 2 (suffix-only) and class 4 (action suffix) words near the end, which the decode query (class 1) must not see;
    sample 1 has no allowed prefix key at all."""
    g = torch.Generator().manual_seed(3000 + Pn)
    pad = 35 if Pn > 40 else 5
    pm = (torch.rand(8, Pn, generator=g) > (0.1 if Pn > 40 else 0.0)).to(torch.int32)      # (Pn = 16: 8 allowed keys per sample)
    for b in range(8):
        pm[b, :pad + (b if Pn > 40 else 0)] = 0
    pm[1] = 0
    cs = pm.cumsum(1).to(torch.int32)
    word = ((pm | (pm << 1)) << 24) | cs
    n4, n2 = (4, 3) if Pn > 40 else (2, 1)
    word[:, Pn - n4:] = (4 << 24) | cs[:, Pn - n4:]
    word[:, Pn - n4 - n2:Pn - n4] = (2 << 24) | cs[:, Pn - n4 - n2:Pn - n4]
    if Pn > 40:
        word[:, Pn // 2] = (4 << 24) | 0               # a class-4 word with index 0 in the middle of the allowed keys
    return word.contiguous()


def attn_case(Pn, cap, regime):
    """Decode-attention inputs at B = 8.  regime: flat | peaked (q scaled for that score std) | count (q = 0, every v = +-1)."""
    key = ("attn", Pn, cap, regime)
    if key in _CASES:
        return _CASES[key]
    g = torch.Generator().manual_seed(4000 + Pn + len(regime))
    c = {"kinfo": attn_kinfo(Pn)}
    c["allowed"] = query_allows(c["kinfo"])
    c["pk"], c["gk"] = torch.randn(8, Pn, DHD, generator=g).to(torch.bfloat16), torch.randn(8, cap, DHD, generator=g).to(torch.bfloat16)
    if regime == "count":
        c["q"] = torch.zeros(8, DNH * DHD, dtype=torch.bfloat16)
        c["pv"] = (torch.randint(0, 2, (8, Pn, DHD), generator=g) * 2 - 1).to(torch.bfloat16)
        c["gv"] = (torch.randint(0, 2, (8, cap, DHD), generator=g) * 2 - 1).to(torch.bfloat16)
    else:
        c["q"] = (torch.randn(8, DNH * DHD, generator=g) * (ATTN_REGIMES[regime] / 16.0)).to(torch.bfloat16)   # |k| ~ 16
        c["pv"], c["gv"] = torch.randn(8, Pn, DHD, generator=g).to(torch.bfloat16), torch.randn(8, cap, DHD, generator=g).to(torch.bfloat16)
    _CASES[key] = c
    return c


def count_reference(c, t):
    """The exact-count case at step t: (sum of the allowed keys' signs [B, HD], their number [B]) as float64."""
    ok = torch.cat([c["allowed"], torch.ones(8, t, dtype=torch.bool)], 1)
    v = torch.cat([c["pv"], c["gv"][:, :t]], 1).double()
    return (v * ok[..., None]).sum(1), ok.sum(1).double()


def count_separated(sm, n):
    """Exact-count elements worth asserting: the reference sum is not 0, and bf16(mean) with any one key dropped or added lies
    more than the allowance (one bf16 spacing; nothing at a power-of-two count) from bf16(sm / n).  sm [B, HD] sums of signs, n [B, 1] counts (float64)."""
    ref = bf16r(sm / n)
    keep = sm != 0
    for dn, ds, possible in ((-1, -1, (n + sm) > 0), (-1, 1, (n - sm) > 0), (1, 1, None), (1, -1, None)):
        other = bf16r(torch.where(n + dn > 0, (sm + ds) / (n + dn).clamp(min=1), torch.zeros_like(sm)))
        far = (other - ref).abs() > torch.where(torch.log2(n) % 1 == 0, 0.0, 1.0) * ulp_bf16(ref)      # (a power-of-two count is asserted exactly)
        keep &= far if possible is None else (far | ~possible)
    return keep
