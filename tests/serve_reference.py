"""Float64 references, element bounds, float32 restatements and seeded inputs for the serving-path kernels: the skinny-M fused
projections and the per-step head / tail of the denoise loop (csrc/serve_skinny.hip, csrc/serve_skinny_body.hpp), the few-query
attention (csrc/attention_serve.hpp), the split-K consumers (csrc/serve_fused.hip) and the row-panel GEMM (csrc/serve_panel.hip;
the last two have their criteria in their sections below).  Shared by tests/test_serve_reference_gpu.py (device against reference) and
tests/test_serve_reference_cpu.py (the criteria against float32 restatements and corrupted references).  Plain torch on the CPU;
nothing here calls lap_amd.hip.

Conventions (tests/decode_reference.py, tests/attention_reference.py): R64 is the operation unrounded, R16 the same with the
kernel's documented bf16 rounding points restated.  (a) every element within its own bound: one bf16 spacing per rounding point
carried through its gain (decode_reference._rnd) plus DEPTH 2^-24 S_e, S_e = sum_k |w_k| |h_k|; (b) at most CAP of the elements
differ from R16 at all, CAP = 4 x the largest share at which a float32 restatement differs from the float64 R16 (DIFFERING).

DEPTH, each read from the kernel's source:
 * skinny projections: K / 8 + 8.  serve_skinny_body.hpp skinny_rest: wave w contracts the contiguous slice k in [w KS 32,
   (w + 1) KS 32) through KS chained v_mfma_f32_16x16x32_bf16 (`acc[f][t] = mfma16(wf[f][s], xf[t][s], acc[f][t])`, the order
   inside one MFMA taken as sequential: KS 32 = K / 8 additions), then `y += part[ww]` over the 8 waves in wave order.
   136 at K = 1024 (qkv, gate|up, out), 264 at 2048, 520 at 4096.
 * embed_actions (serve_skinny.hip embed_actions_kernel; the tail of final_euler_embed_kernel): `a += xt * w` over action_dim
   float32 products, each rounded unless contracted, and the bias: 2 action_dim + 1.
 * final_euler (final_norm_out_euler_kernel / final_euler_embed_kernel at D = 1024, NCH = 2): 16 float32 products and 16
   additions per lane, the 6 levels of the wave sum and the bias: 39, taken as FINAL_DEPTH = 40.  x_t += dt v_t adds a product
   and a sum: 2 2^-24 (|x_t| + |dt| |v_t|) on top of |dt| times the bound of v_t.
 * prologue: h = bf16(x r bf16(1 + scale) + shift).  Its float32 argument is off by less than 2^-19 of |x r s| + |shift| (32
   squares and additions per lane, 2 lane steps, 8 waves: 42 roundings of the sum of squares, halved by the square root; the
   division by K, eps, sqrtf, the reciprocal and the three operations of the argument: under 32 2^-24), so `settle_mod` nudges
   shift (bf16, an input) by one bf16 spacing until every h keeps TIE_MARGIN (2^-19 of |x r s| + |shift|, which is at least
   2^-19 of |h|) from every rounding tie: the reference's h is then the kernel's, bit for bit.
 * few-query attention: attention_reference.fwd_reference(split=True).  Its DEPTH (272) covers the 8 chained MFMAs of S^T = K Q^T
   (attention_serve.hpp attn_run_body, `for kk < KS`), acc_depth its P V sum (at most 128 keys a run in 4 chained MFMAs, the run's
   `acc * inv`, and the combine over at most 8 runs: serve_run_cap returns at most 8 and acc_depth allows 8 shares).
"""
import zlib

import torch

from tests.attention_reference import Region, SENTINEL, fwd_reference, mask_ok, region_view, untouched  # noqa: F401 (re-exported)
from tests.decode_reference import (F32_ORDERS, TIE_MARGIN, U24, _acc_f32, _rnd, bf16r, check_elementwise, count_separated,  # noqa: F401
                                    differing_share, dot_and_sens, gelu_tanh64, ref_gate_up, ref_qkv, tie_distance, ulp_bf16, worst_ratio)

D, NH, HD, H = 1024, 8, 256, 4096          # the smallest shapes the skinny kernels take; H = 4096 for gate | up
EPS = 1e-6
Q_SCALE = HD ** -0.5                       # 2^-4: exact, and so is the store behind it
M_MAX, RPS = 130, 50
FINAL_DEPTH = 40
DT = float(torch.tensor(-0.1, dtype=torch.float32))       # the Euler step as the float32 the kernel is handed
RES_K = (1024, 2048, 4096)
ACTION_DIMS = (7, 8)
ORDERS = F32_ORDERS + ("slices8",)         # decode_reference's three and the kernel's own: 8 slices of chained 32-deep steps, then wave order
# (M, rows per sample, shared modulation row): tests/test_serve_reference_gpu.py runs every kind at each of them
SKINNY_CASES = ((50, 50, True), (50, 50, False), (130, 50, False), (64, 16, True), (1, 1, True), (17, 17, True))
# Extended rows: the references are computed once, on the 130 rows of the per-sample case (row r with modulation row r // 50)
# followed by rows 50 .. 63 with modulation row 0 (the shared cases reach past row 49 only at M = 64).
XROW = torch.cat([torch.arange(M_MAX), torch.arange(50, 64)])
MROW = torch.cat([torch.arange(M_MAX) // RPS, torch.zeros(14, dtype=torch.long)])


def skinny_depth(K):
    return K // 8 + 8


def embed_depth(ad):
    return 2 * ad + 1


def case_rows(M, shared):
    """Extended-row indices of the M rows of a case."""
    r = torch.arange(M)
    return torch.where(r >= 50, r + 80, r) if shared else r


def slice_alternate(w):
    """w [N, K]: the K columns of the even wave slices (K / 8 contiguous columns each) scaled by 2, of the odd ones by 1 / 2, so
    that a dropped or doubled slice of either kind moves an output far beyond its bound."""
    K = w.shape[1]
    s = torch.where((torch.arange(K) // (K // 8)) % 2 == 0, 2.0, 0.5)
    return w * s[None, :]


# ------------------------------------------------------------------------------------------------------- the prologue
def h_argument(x, mod, xrow=XROW, mrow=MROW):
    """(v, mag): the float64 argument of h = bf16(v), v = x r bf16(1 + scale) + shift, r = 1 / sqrt(mean x^2 + eps), and
    mag = |x r s| + |shift|, which the float32 error of v is relative to."""
    xd = x[xrow].double()
    r = (xd.pow(2).mean(1, keepdim=True) + EPS).rsqrt()
    p = xd * r * bf16r(1.0 + mod[mrow, :D].double())
    sh = mod[mrow, D:2 * D].double()
    return p + sh, p.abs() + sh.abs()


def tie_clear(v, mag):
    """Per element: v keeps TIE_MARGIN mag from the nearest bf16 rounding tie (tie_distance is relative to |v|)."""
    return tie_distance(v) * v.abs() >= TIE_MARGIN * mag


def settle_mod(x, mod, xrow=XROW, mrow=MROW):
    """settle_gamma for a bf16 modulation: shift[col] of a modulation row moves up by one bf16 spacing where any row that uses
    that modulation row has an h closer than the margin to a rounding tie, until none is left.  The shift alone does not always
    get there: where h is no larger than the shift (the product cancels against it) a spacing of the shift is a whole number of
    spacings of h, and where the shift is tiny it hardly moves h at all; so every other round scale[col] moves up with it, by one
    spacing of bf16(1 + scale), which moves the product by 2^-8 of itself.  Returns the settled mod."""
    mod = mod.clone()
    for it in range(64):
        v, mag = h_argument(x, mod, xrow, mrow)
        close = ~tie_clear(v, mag)
        if not bool(close.any()):
            return mod
        for m in range(mod.shape[0]):
            cols = close[mrow == m].any(0)
            sh, sc = mod[m, D:2 * D].double(), mod[m, :D].double()
            mod[m, D:2 * D] = torch.where(cols, sh + ulp_bf16(sh), sh).to(torch.bfloat16)     # (the next bf16 number: exact)
            if it % 2 == 0:     # (every other round: the two steps can cancel where the product cancels against the shift)
                mod[m, :D] = torch.where(cols, sc + ulp_bf16(bf16r(1.0 + sc)), sc).to(torch.bfloat16)
    raise AssertionError("settle_mod did not converge")


# --------------------------------------------------------------------------------------------------------- the inputs
_IN = {}
_REFS = {}
_DOTS = {}


def skinny_inputs():
    """Seeded inputs of every skinny kind (cached): x / a / res rows scaled by 1 + row % 8, mod = scale | shift | gate [3, 3 D]
    settled, slice-alternating weights, positions, and the float32 operands of the head and tail."""
    if _IN:
        return _IN
    g = torch.Generator().manual_seed(5101)
    bf = torch.bfloat16
    rows = (1.0 + torch.arange(M_MAX) % 8).view(-1, 1)
    c = {}
    c["x"] = (torch.randn(M_MAX, D, generator=g) * rows).to(bf)
    c["wqkv"] = slice_alternate(torch.randn((NH + 2) * HD, D, generator=g) * 0.02).to(bf)
    c["wgu"] = slice_alternate(torch.randn(2 * H, D, generator=g) * 0.02).to(bf)
    for K in RES_K:
        c[f"a{K}"] = (torch.randn(M_MAX, K, generator=g) * rows).to(bf)
        c[f"w{K}"] = slice_alternate(torch.randn(D, K, generator=g) * (0.02 * (1024.0 / K) ** 0.5)).to(bf)
    c["res"] = (torch.randn(M_MAX, D, generator=g) * rows).to(bf)
    c["pos"] = ((torch.arange(M_MAX) * 37) % 811).to(torch.int32)            # 0 at row 0, up to 810
    c["mod"] = settle_mod(c["x"], (torch.randn(3, 3 * D, generator=g) * 0.1).to(bf))
    v, _ = h_argument(c["x"], c["mod"])
    c["h16"] = bf16r(v)
    for ad in ACTION_DIMS:
        c[f"xt{ad}"] = torch.randn(M_MAX, ad, generator=g)
        c[f"win{ad}"] = torch.randn(D, ad, generator=g) * 0.3
        c[f"bin{ad}"] = torch.randn(D, generator=g) * 0.1
        c[f"wout{ad}"] = torch.randn(ad, D, generator=g) * 0.03
        c[f"bout{ad}"] = torch.randn(ad, generator=g) * 0.1
    _IN.update(c)
    return _IN


def gate_rows(c):
    return c["mod"][MROW, 2 * D:].double()


# ------------------------------------------------------------------------------------------------- float64 references
def ref_proj_residual(a, w, x, gate, depth, rounded=True):
    """out / down: bf16(x + bf16(bf16(a W^T) gate)), three rounding points; gate None: bf16(x + bf16(a W^T)), two."""
    dot, sens = dot_and_sens(a, w)
    if not rounded:
        return x + (dot if gate is None else dot * gate)
    y, d = _rnd(dot, depth * U24 * sens)
    if gate is not None:
        y, d = _rnd(y * gate, d * gate.abs())
    return _rnd(x + y, d)


def ref_embed(xt, w, b, dx=None, rounded=True):
    """embed_actions: bf16(x_t W_in^T + b), float32 operands; dx: the bound of a device-computed x_t."""
    xt, w, b = xt.double(), w.double(), b.double()
    y = xt @ w.T + b
    if not rounded:
        return y
    d = embed_depth(xt.shape[1]) * U24 * (xt.abs() @ w.abs().T + b.abs())
    return _rnd(y, d if dx is None else d + dx @ w.abs().T)


def ref_final(h16, w, b, xt, dt):
    """final_euler in float64 on the bf16 normalised rows: (v_t, bound), (x_t + dt v_t, bound)."""
    w, b, xt = w.double(), b.double(), xt.double()
    v = h16 @ w.T + b
    dv = FINAL_DEPTH * U24 * (h16.abs() @ w.abs().T + b.abs())
    return (v, dv), (xt + dt * v, abs(dt) * dv + 2.0 * U24 * (xt.abs() + abs(dt) * (v.abs() + dv)))


KINDS = ("qkv", "gate_up") + tuple(f"res{K}{g}" for K in RES_K for g in ("", "g")) + tuple(f"embed{ad}" for ad in ACTION_DIMS)


def skinny_reference(kind):
    """(R16, bound) of a kind on the 144 extended rows (cached); qkv as q | k | v along the columns."""
    if kind in _REFS:
        return _REFS[kind]
    c = skinny_inputs()
    if kind == "qkv":
        parts = ref_qkv(c["h16"], c["wqkv"].double(), c["pos"][XROW], NH, HD, Q_SCALE, depth=skinny_depth(D))
        r = torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1)
    elif kind == "gate_up":
        r = ref_gate_up(c["h16"], c["wgu"].double(), H, depth=skinny_depth(D))
    elif kind.startswith("res"):
        K = int(kind[3:7])
        r = ref_proj_residual(c[f"a{K}"][XROW], c[f"w{K}"], c["res"][XROW].double(), gate_rows(c) if kind.endswith("g") else None, skinny_depth(K))
    elif kind.startswith("embed"):
        ad = int(kind[5:])
        r = ref_embed(c[f"xt{ad}"][XROW], c[f"win{ad}"], c[f"bin{ad}"])
    else:
        raise ValueError(kind)
    _REFS[kind] = r
    return r


def final_reference(ad):
    """((v_t, bound), (x_t new, bound), (tokens R16, bound)) of the final step on the extended rows (cached)."""
    key = ("final", ad)
    if key not in _REFS:
        c = skinny_inputs()
        vt, xn = ref_final(c["h16"], c[f"wout{ad}"], c[f"bout{ad}"], c[f"xt{ad}"][XROW], DT)
        _REFS[key] = (vt, xn, ref_embed(xn[0], c[f"win{ad}"], c[f"bin{ad}"], dx=xn[1]))
    return _REFS[key]


def rope_table64(pos):
    """float64 sin / cos [rows, HD / 2, 2] of lap_rope_table, and the bound ref_qkv uses for the float32 angle and sincosf:
    2^-22 (pos + 1)."""
    half = HD // 2
    ang = pos.double().view(-1, 1) / (10000.0 ** (2.0 * torch.arange(half, dtype=torch.float64) / HD)).view(1, half)
    return torch.stack([torch.sin(ang), torch.cos(ang)], -1), ((pos.double() + 1.0) * 2.0 ** -22).view(-1, 1, 1)


# --------------------------------------------------------------------------- float32 restatements (the measurement behind CAP)
def _acc_slices8(h, w):
    """The kernel's own order in float32: per wave slice a chain over its 32-deep k-steps (each step summed pairwise), then the 8
    slices in wave order.  h [B, K], w [N, K] float32 holding bf16 values."""
    B, K = h.shape
    out = []
    for n0 in range(0, w.shape[0], 512):
        p = (h[:, None, :] * w[None, n0:n0 + 512, :]).view(B, -1, 8, K // 256, 32)
        while p.shape[-1] > 1:
            p = p[..., 0::2] + p[..., 1::2]
        p = p[..., 0]
        acc = torch.zeros(p.shape[:-1])
        for s in range(p.shape[-1]):
            acc = acc + p[..., s]
        tot = acc[..., 0]
        for ww in range(1, 8):
            tot = tot + acc[..., ww]
        out.append(tot)
    return torch.cat(out, 1)


def f32_dot(h, w, order):
    """h w^T with float32 accumulation in `order`, 16 rows at a time (the products of a chunk are held at once)."""
    h, w = h.float(), w.float()
    fn = _acc_slices8 if order == "slices8" else (lambda a, b: _acc_f32(a, b, order))
    return torch.cat([fn(h[r0:r0 + 16].contiguous(), w) for r0 in range(0, h.shape[0], 16)], 0)


def _bf(x):
    return x.to(torch.bfloat16).float()


def f32_skinny(kind, order, corrupt=None):
    """The bf16 output of a kind on the 130 rows of the per-sample case with float32 accumulation in `order` and a float32
    epilogue, as float64.  embed kinds: order `seq` (product and sum rounded) or `fma`.  corrupt = "slice": wave slice 5 is left
    out of every dot product (a corrupted restatement)."""
    c = skinny_inputs()
    f = torch.float32
    M = M_MAX
    if kind.startswith("embed"):
        ad = int(kind[5:])
        xt, w, b = c[f"xt{ad}"], c[f"win{ad}"], c[f"bin{ad}"]
        acc = torch.zeros(M, D)
        for k in range(ad):
            if order == "fma":
                acc = (acc.double() + xt[:, k:k + 1].double() * w[:, k].double()).float()
            else:
                acc = acc + xt[:, k:k + 1] * w[:, k]
        return (acc + b).to(torch.bfloat16).double()
    if kind.startswith("res"):
        K = int(kind[3:7])
        hin, w = c[f"a{K}"], c[f"w{K}"]
    else:
        hin, w = c["h16"][:M], c["wqkv"] if kind == "qkv" else c["wgu"]
    key = (kind[:7] if kind.startswith("res") else kind, order, corrupt)
    if key not in _DOTS:
        if corrupt == "slice":
            K = w.shape[1]
            keep = (torch.arange(K) // (K // 8)) != 5
            _DOTS[key] = f32_dot(hin, w, order) - f32_dot(hin.float() * ~keep, w, order)
        else:
            _DOTS[key] = f32_dot(hin, w, order)
    dot = _bf(_DOTS[key])
    if kind.startswith("res"):
        y = _bf(dot * gate_rows(c)[:M].to(f)) if kind.endswith("g") else dot
        return (c["res"].to(f) + y).to(torch.bfloat16).double()
    if kind == "gate_up":
        gt, u = dot[:, :H], dot[:, H:]
        ge = _bf(0.5 * gt * (1.0 + torch.tanh(0.7978845608028654 * (gt + 0.044715 * gt * gt * gt))))
        return (ge * u).to(torch.bfloat16).double()
    half = HD // 2
    x = dot.view(M, NH + 2, HD)
    ts = torch.pow(torch.tensor(10000.0), (2.0 / HD) * torch.arange(half, dtype=f))
    ang = c["pos"].to(f).view(M, 1, 1) / ts.view(1, 1, half)
    sn, cs = torch.sin(ang), torch.cos(ang)
    x1, x2 = x[:, :NH + 1, :half], x[:, :NH + 1, half:]
    r = _bf(torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1))
    return torch.cat([(r[:, :NH] * Q_SCALE).reshape(M, -1), r[:, NH], x[:, NH + 1]], 1).to(torch.bfloat16).double()


def kind_orders(kind):
    return ("seq", "fma") if kind.startswith("embed") else ORDERS


def measure_differing(kind):
    r, _ = skinny_reference(kind)
    r = r[:M_MAX]
    return tuple(int((f32_skinny(kind, o) != r).sum()) for o in kind_orders(kind)), r.numel()


# kind: the number of elements (of the 130 rows of the per-sample case) at which a float32 order differs from the float64 R16, per
# order of kind_orders, and the number of elements; CAP = 4 x the largest share.  tests/test_serve_reference_cpu.py measures them again.
DIFFERING = {"qkv": ((348, 342, 337, 340), 332800), "gate_up": ((185, 81, 67, 67), 532480),
             "res1024": ((5, 0, 0, 0), 133120), "res1024g": ((1, 0, 0, 0), 133120),
             "res2048": ((7, 0, 1, 1), 133120), "res2048g": ((3, 0, 0, 1), 133120),
             "res4096": ((9, 1, 3, 3), 133120), "res4096g": ((2, 0, 0, 0), 133120),
             "embed7": ((8, 8), 133120), "embed8": ((5, 5), 133120),
             # the tokens of final_euler_embed with the whole tail in float32 (f32_tokens: seq, fma)
             "tokens7": ((8, 10), 133120), "tokens8": ((5, 4), 133120),
             # the split-K consumers (measure_fused): output -> (count, elements)
             "fused_rope": {"q": (112, 102400), "k": (9, 12800)}, "fused_geglu": {"act": (71, 25600)},
             "fused_resnorm": {"h": (0, 51200)}, "fused_norm1": {"h": (0, 102400)}, "fused_norm2": {"h": (0, 102400)},
             # the row-panel GEMM (measure_panel: sequential, pairwise, lanes, chain32 at K = 1024; sequential, chain32 otherwise)
             "panel_plain": ((6, 3, 3, 4), 51200), "panel_bias": ((12, 4, 3, 3), 51200), "panel_bias_res": ((13, 2, 1, 5), 51200),
             "panel_gelu": ((93, 87, 87, 87), 51200), "panel_exp2": ((125, 123, 123, 123), 51200), "panel_thin": ((4, 1), 74880),
             "panel_ln": ((4, 4), 20480), "panel_rms": ((6, 2, 2, 3), 20480)}


def share_cap(kind):
    counts, numel = DIFFERING[kind]
    return 4.0 * max(counts) / numel


# ------------------------------------------------------------------------------------- one allocation, guards between views
GUARD_ROWS = 16


def build_arena(outs, fill=None):
    """outs: (name, rows, width, row stride) in bf16 elements (a float32 [rows, n] output has width 2 n).  One bf16 allocation
    filled with SENTINEL in which every output is a window between GUARD_ROWS guard rows of its stride; `fill` maps a name to
    the [rows, width] bf16 data an in / out buffer starts with.  Returns (arena, regions: name -> Region)."""
    chunks, regions, pos = [], {}, 0
    for name, rows, width, rs in outs:
        n = ((2 * GUARD_ROWS + rows) * rs + 7) // 8 * 8
        chunk = torch.full((n,), SENTINEL, dtype=torch.bfloat16)
        regions[name] = Region(pos + GUARD_ROWS * rs, rows, rs, 0, width)
        if fill and name in fill:
            torch.as_strided(chunk, (rows, width), (rs, 1), GUARD_ROWS * rs).copy_(fill[name])
        chunks.append(chunk)
        pos += n
    return torch.cat(chunks), regions


def f32_bits(x):
    """A float32 [rows, n] tensor as the bf16-typed [rows, 2 n] words build_arena stores (bit pattern kept)."""
    return x.contiguous().view(torch.bfloat16)


def f32_window(arena, r):
    """The float32 [rows, width / 2] view of a contiguous float32 region."""
    assert r.rs == r.width and r.off % 2 == 0
    return arena[r.off:r.off + r.rows * r.width].view(torch.float32).view(r.rows, r.width // 2)


# ----------------------------------------------------------------------------------------------- few-query attention
# (B, NH, NKV, cached prefix keys, suffix queries, fresh keys)
ATTN_SHAPES = ((1, 8, 1, 77, 1, 1), (2, 8, 1, 77, 1, 5), (1, 8, 1, 0, 3, 40), (2, 4, 2, 100, 40, 40), (1, 8, 8, 130, 64, 64),
               (1, 8, 1, 256, 16, 16), (1, 8, 1, 300, 1, 200))
ATTN_COUNT = (1, 2, 3)                       # the shapes that also run as exact cases (q = 0, v = +-1)
ATTN_SCALE = HD ** -0.5
ATTN_FULLY_MASKED = {1: 1}                   # shape index -> the sample with no allowed key
GARBAGE = 1.0e4
_ATTN = {}


def attn_infos(shape, idx):
    """(qinfo [B, S], kinfo [B, Tp + F]) in the sampler's vocabulary (serve_fused.hip serve_infos_kernel): queries class 6, cached
    keys class 3 with a running index, fresh keys class 4, all at the suffix index.  Class 0: a padded prompt tail of 5 + 4 b
    keys at the end of the prefix (inside its last run), a hole at key 3, and every key of the fully masked sample."""
    B, _, _, Tp, S, F = shape
    sidx = 0xFFFFF
    qinfo = torch.full((B, S), (6 << 24) | sidx, dtype=torch.int32)
    kinfo = torch.empty(B, Tp + F, dtype=torch.int32)
    kinfo[:, :Tp] = (3 << 24) | torch.arange(1, Tp + 1, dtype=torch.int32)
    kinfo[:, Tp:] = (4 << 24) | sidx
    for b in range(B):
        if Tp:
            kinfo[b, Tp - (5 + 4 * b):Tp] &= 0xFFFFFF
    if Tp + F > 4:
        kinfo[:, 3] &= 0xFFFFFF
    if idx in ATTN_FULLY_MASKED:
        kinfo[ATTN_FULLY_MASKED[idx]] &= 0xFFFFFF
    return qinfo, kinfo


def attn_case(idx, regime="rand"):
    """Seeded inputs (cached): q [B, S, NH, HD], k / v [B, Tp + F, NKV, HD] bf16 (prefix then fresh keys), info words, allowed
    [B, S, Tp + F].  rand: scores of std 1 to 3; count: q = 0, v = +-1.  Class-0 keys hold values of size GARBAGE in k and v."""
    key = (idx, regime)
    if key in _ATTN:
        return _ATTN[key]
    shape = ATTN_SHAPES[idx]
    B, nh, nkv, Tp, S, F = shape
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, regime)).encode()))
    c = {"shape": shape}
    c["qinfo"], c["kinfo"] = attn_infos(shape, idx)
    c["allowed"] = mask_ok(c["qinfo"], c["kinfo"])
    q = torch.randn(B, S, nh, HD, generator=g) * (1.0 + torch.arange(S) % 3).view(1, S, 1, 1)
    k, v = torch.randn(B, Tp + F, nkv, HD, generator=g), torch.randn(B, Tp + F, nkv, HD, generator=g)
    if regime == "count":
        q = torch.zeros_like(q)
        v = (torch.randint(0, 2, v.shape, generator=g) * 2 - 1).float()
    dead = ((c["kinfo"] >> 24) == 0)[:, :, None, None]
    big = torch.randn(B, Tp + F, nkv, HD, generator=g) * GARBAGE
    k, v = torch.where(dead, big, k), torch.where(dead, -big, v)
    c["q"], c["k"], c["v"] = (t.to(torch.bfloat16) for t in (q, k, v))
    _ATTN[key] = c
    return c


def attn_reference(idx, regime="rand"):
    """fwd_reference(split=True) of a case (cached): o16 and o_bound [B, S, NH, HD], empty [B, NH, S]."""
    key = ("ref", idx, regime)
    if key not in _ATTN:
        c = attn_case(idx, regime)
        f = fwd_reference(c["q"], c["k"], c["v"], c["allowed"], ATTN_SCALE, split=True)
        _ATTN[key] = {n: f[n] for n in ("o", "o16", "o_bound", "empty", "A", "p")}
    return _ATTN[key]


def attn_count(c):
    """q = 0, v = +-1: (sum of the allowed keys' signs [B, S, NH, HD], their number [B, S, 1, 1]) as float64."""
    B, nh, nkv = c["shape"][:3]
    ok = c["allowed"].double()
    v = c["v"].double().repeat_interleave(nh // nkv, dim=2)
    return torch.einsum("bij,bjhd->bihd", ok, torch.where(c["allowed"].any(1)[:, :, None, None], v, torch.zeros_like(v))), ok.sum(-1).view(B, -1, 1, 1)


def attn_count_check(c):
    """(want, keep, allowance): bf16(mean) of the exact case, the elements at which one key more or fewer would show
    (count_separated) and the allowance there: one bf16 spacing, nothing at a power-of-two count."""
    sm, n = attn_count(c)
    live = (n > 0).expand_as(sm)
    nn = n.clamp(min=1.0)
    want = bf16r(sm / nn)
    keep = count_separated(sm, nn.expand_as(sm)) & live
    allow = torch.where(torch.log2(nn) % 1 == 0, 0.0, 1.0) * ulp_bf16(want)
    return want, keep, allow, live


# ------------------------------------------------------------------------------- tokens of final_euler_embed (the cap)
def f32_tokens(ad, order):
    """The tokens of final_euler_embed with the whole tail in float32 (v_t, x_t, then the embedding in `order`: seq | fma), on
    the 130 rows of the per-sample case, as float64."""
    c = skinny_inputs()
    v = c["h16"][:M_MAX].float() @ c[f"wout{ad}"].T + c[f"bout{ad}"]
    xn = c[f"xt{ad}"] + torch.tensor(DT) * v
    w, acc = c[f"win{ad}"], torch.zeros(M_MAX, D)
    for k in range(ad):
        acc = (acc.double() + xn[:, k:k + 1].double() * w[:, k].double()).float() if order == "fma" else acc + xn[:, k:k + 1] * w[:, k]
    return (acc + c[f"bin{ad}"]).to(torch.bfloat16).double()


def measure_tokens(ad):
    r = final_reference(ad)[2][0][:M_MAX]
    return tuple(int((f32_tokens(ad, o) != r).sum()) for o in ("seq", "fma")), r.numel()


# ------------------------------------------------------------------- split-K consumers (csrc/serve_fused.hip)
# The slab sum is float32 in slab order (sum8: "bit-identical to splitk_reduce_kernel"; reduce_norm_kernel restates the same
# loops, then `y += bias`, `y += resid`), so R16 sums in float32 in that order and rounds: x = bf16(sum) is exact, and so is
# every output that is a rounding of exact float32 arithmetic on it: v of rope_split, xn of residual_norm (a product of two bf16
# numbers is exact in float32, and so is the sum with x at these magnitudes) and xn of fused_reduce_norm (CAP = 0: equality).
# The rest is float64 on x with the documented rounding points:
#  * rope_split q / k: bf16(rotation), the float32 angle term of ref_qkv and 4 2^-24 (|x1| + |x2|) for rope_rotate's two
#    products and sum (reduce_rope_kernel: rope_rotate, round_bf16, `r1 *= q_scale`, exact).
#  * geglu: bf16(bf16(gelu g) u) with ref_gate_up's 2^-23 |g| for the float32 tanh form (reduce_geglu_kernel).
#  * h of residual_norm / fused_reduce_norm: one rounding point whose float32 argument is settled off the ties (settle_mod,
#    decode_reference.settle_gamma, settle_layernorm): 16 to 32 squares per lane and 6 wave levels (reduce_residual_norm_kernel,
#    reduce_norm_kernel: `ss += t * t`, wave_sum), under the same 2^-19.  The reference's h is then the kernel's.
FUSED_KS = (1, 3, 4, 7, 8, 12)              # sum8: the single-slab tail alone, 3 = tail, 4 = the 4 loop, 7 = 4 + tail, 8 = the 8 loop, 12 = 8 + 4
FUSED_ROWS = (50, 37)
FUSED_H, FUSED_RPS = 512, 25
NORM_D = (1152, 2048)
_FUSED = {}


def slab_sum(part, bias=None, resid=None):
    """float32 sum of the slabs in slab order (+ float32 bias) (+ bf16 residual), the kernels' order; float32."""
    acc = torch.zeros_like(part[0])
    for s in range(part.shape[0]):
        acc = acc + part[s]
    if bias is not None:
        acc = acc + bias
    if resid is not None:
        acc = acc + resid.float()
    return acc


def _slabs(g, ks, rows, W):
    return torch.randn(ks, rows, W, generator=g) * (1.0 + torch.arange(rows) % 8).view(1, -1, 1) / ks ** 0.5


def ref_rope_split(x, pos, q_scale, rounded=True):
    """x [rows, (NH + 2) HD] float64 (bf16 numbers): (q, k) as (R16, bound) and v (exact)."""
    rows, half = x.shape[0], HD // 2
    x = x.view(rows, NH + 2, HD)
    tab, dang = rope_table64(pos)
    sn, cs = tab[..., 0].view(rows, 1, half), tab[..., 1].view(rows, 1, half)
    x1, x2 = x[:, :NH + 1, :half], x[:, :NH + 1, half:]
    rot = torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1)
    mag = (x1.abs() + x2.abs()) * (dang.view(rows, 1, 1) + 4.0 * U24)
    r, d = _rnd(rot, torch.cat([mag, mag], -1)) if rounded else (rot, None)
    qk = torch.cat([(r[:, :NH] * q_scale).reshape(rows, -1), r[:, NH]], 1)
    return (qk, None if d is None else torch.cat([(d[:, :NH] * q_scale).reshape(rows, -1), d[:, NH]], 1)), x[:, NH + 1]


def ref_geglu(g, u):
    ge, d = _rnd(gelu_tanh64(g), g.abs() * 2.0 ** -23)
    return _rnd(ge * u, d * u.abs())


def ln_argument(x, gamma, beta, eps=EPS):
    """(v, mag) of the LayerNorm h = bf16(v), v = (x - mean) r gamma + beta with the variance as mean(x^2) - mean^2."""
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    r = ((xd.pow(2).mean(1, keepdim=True) - mean ** 2).clamp(min=0.0) + eps).rsqrt()
    g, b = gamma.double(), beta.double()
    return (xd - mean) * (r * g) + b, (xd.abs() + mean.abs()) * r * g.abs() + b.abs()


def settle_layernorm(x, gamma, beta, eps=EPS):
    """settle_gamma for the LayerNorm: gamma and beta (float32 inputs) move up by 2^-12 in the columns where any row's h is closer
    than the margin to a rounding tie.  Returns the settled (gamma, beta)."""
    gamma, beta = gamma.clone(), beta.clone()
    for _ in range(64):
        v, mag = ln_argument(x, gamma, beta, eps)
        close = (~tie_clear(v, mag)).any(0)
        if not bool(close.any()):
            return gamma, beta
        gamma[close] += 2.0 ** -12
        beta[close] += 2.0 ** -12
    raise AssertionError("settle_layernorm did not converge")


def rms_argument(x, gamma, eps=EPS):
    xd = x.double()
    v = xd * (xd.pow(2).mean(1, keepdim=True) + eps).rsqrt() * (1.0 + gamma.double())
    return v, v.abs()


def settle_rms(x, gamma, eps=EPS):
    """decode_reference.settle_gamma (the same nudge of 2^-12) under this module's margin."""
    gamma = gamma.clone()
    for _ in range(64):
        v, mag = rms_argument(x, gamma, eps)
        close = (~tie_clear(v, mag)).any(0)
        if not bool(close.any()):
            return gamma
        gamma[close] += 2.0 ** -12
    raise AssertionError("settle_rms did not converge")


def fused_case(kind, ks, rows, **kw):
    """Inputs and references of one consumer case (cached).  kind: rope | geglu | resnorm (gated=) | norm (D=, norm=, bias=,
    resid=).  `part` f32 [ks, rows, W]; outputs as name -> (R16, bound or None = exact)."""
    key = (kind, ks, rows, tuple(sorted(kw.items())))
    if key in _FUSED:
        return _FUSED[key]
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    bf = torch.bfloat16
    c = {}
    if kind == "rope":
        c["part"] = _slabs(g, ks, rows, (NH + 2) * HD)
        c["pos"] = ((torch.arange(rows) * 37) % 811).to(torch.int32)
        c["x16"] = bf16r(slab_sum(c["part"]))
        (qk, d), v = ref_rope_split(c["x16"], c["pos"], Q_SCALE)
        c["out"] = {"q": (qk[:, :NH * HD], d[:, :NH * HD]), "k": (qk[:, NH * HD:], d[:, NH * HD:]), "v": (v, None)}
    elif kind == "geglu":
        c["part"] = _slabs(g, ks, rows, 2 * FUSED_H) * 0.25      # |g| of 0.25 to 2: outside the cancelling tail of the float32 tanh form
        x = bf16r(slab_sum(c["part"]))
        c["x16"] = x
        c["out"] = {"act": ref_geglu(x[:, :FUSED_H], x[:, FUSED_H:])}
    elif kind == "resnorm":
        c["part"] = _slabs(g, ks, rows, D)
        c["x"] = (torch.randn(rows, D, generator=g) * (1.0 + torch.arange(rows) % 8).view(-1, 1)).to(bf)
        y = bf16r(slab_sum(c["part"]))
        mrow = torch.arange(rows) // FUSED_RPS
        if kw["gated"]:
            mod = (torch.randn(2, 3 * D, generator=g) * 0.1).to(bf)
            xn = bf16r(c["x"].double() + bf16r(y * mod[mrow, 2 * D:].double()))
            c["mod"] = settle_mod(xn.to(bf), mod, torch.arange(rows), mrow)
            v, _ = h_argument(xn.to(bf), c["mod"], torch.arange(rows), mrow)
            c["out"] = {"xn": (xn, None), "h": (bf16r(v), None)}
        else:
            c["out"] = {"xn": (bf16r(c["x"].double() + y), None)}
    elif kind == "norm":
        Dn, norm = kw["D"], kw["norm"]
        c["part"] = _slabs(g, ks, rows, Dn)
        c["bias"] = torch.randn(Dn, generator=g) * 0.5 if kw["bias"] else None
        c["resid"] = (torch.randn(rows, Dn, generator=g) * (1.0 + torch.arange(rows) % 8).view(-1, 1)).to(bf) if kw["resid"] else None
        xn = bf16r(slab_sum(c["part"], c["bias"], c["resid"]))
        c["out"] = {"xn": (xn, None)}
        gamma, beta = torch.randn(Dn, generator=g) * 0.1, torch.randn(Dn, generator=g) * 0.1
        if norm == 1:
            c["gamma"] = settle_rms(xn, gamma)
            c["out"]["h"] = (bf16r(rms_argument(xn, c["gamma"])[0]), None)
        elif norm == 2:
            c["gamma"], c["beta"] = settle_layernorm(xn, 1.0 + gamma, beta)
            c["out"]["h"] = (bf16r(ln_argument(xn, c["gamma"], c["beta"])[0]), None)
    else:
        raise ValueError(kind)
    _FUSED[key] = c
    return c


def f32_fused(kind, c):
    """The outputs of a consumer case that are not exact by construction, restated in float32 (name -> float64 of bf16)."""
    f = torch.float32
    if kind == "rope":
        rows, half = c["x16"].shape[0], HD // 2
        x = c["x16"].to(f).view(rows, NH + 2, HD)
        ts = torch.pow(torch.tensor(10000.0), (2.0 / HD) * torch.arange(half, dtype=f))
        ang = c["pos"].to(f).view(rows, 1, 1) / ts.view(1, 1, half)
        sn, cs = torch.sin(ang), torch.cos(ang)
        x1, x2 = x[:, :NH + 1, :half], x[:, :NH + 1, half:]
        r = _bf(torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1))
        return {"q": (r[:, :NH] * Q_SCALE).reshape(rows, -1).double(), "k": r[:, NH].double()}
    if kind == "geglu":
        x = c["x16"].to(f)
        gt, u = x[:, :FUSED_H], x[:, FUSED_H:]
        ge = _bf(0.5 * gt * (1.0 + torch.tanh(0.7978845608028654 * (gt + 0.044715 * gt * gt * gt))))
        return {"act": (ge * u).to(torch.bfloat16).double()}
    xn = c["out"]["xn"][0].to(f)
    if kind == "resnorm":
        rows = xn.shape[0]
        mod = c["mod"][torch.arange(rows) // FUSED_RPS].to(f)
        r = 1.0 / torch.sqrt(xn.pow(2).sum(1, keepdim=True) / D + EPS)
        return {"h": (xn * r * _bf(1.0 + mod[:, :D]) + mod[:, D:2 * D]).to(torch.bfloat16).double()}
    Dn = xn.shape[1]
    if "beta" in c:
        mean = xn.sum(1, keepdim=True) / Dn
        r = 1.0 / torch.sqrt((xn.pow(2).sum(1, keepdim=True) / Dn - mean * mean).clamp(min=0.0) + EPS)
        return {"h": ((xn - mean) * (r * c["gamma"]) + c["beta"]).to(torch.bfloat16).double()}
    r = 1.0 / torch.sqrt(xn.pow(2).sum(1, keepdim=True) / Dn + EPS)
    return {"h": (xn * r * (1.0 + c["gamma"])).to(torch.bfloat16).double()}


# The consumers' counts, on the ks = 12, rows = 50 case of each (resnorm gated; norm with bias and residual at D = 2048): the
# elements at which the float32 restatement differs from R16, and their number.  Exact outputs (None bounds) have CAP = 0.
FUSED_MEASURED = {"rope": dict(), "geglu": dict(), "resnorm": dict(gated=True), "norm1": dict(D=2048, norm=1, bias=True, resid=True),
                  "norm2": dict(D=2048, norm=2, bias=True, resid=True)}


def measure_fused(name):
    kind = name.rstrip("12")
    c = fused_case(kind, 12, 50, **FUSED_MEASURED[name])
    got = f32_fused(kind, c)
    return {n: (int((got[n] != c["out"][n][0]).sum()), got[n].numel()) for n in got}


def fused_cap(name, out):
    n, numel = DIFFERING["fused_" + name][out]
    return 4.0 * n / numel


# ------------------------------------------------------- row-panel GEMM with its prologues and epilogues (csrc/serve_panel.hip)
# C = epi(norm(A) W^T).  DEPTH: a wave contracts the whole K of its tiles through K / 32 chained MFMAs (panel_gemm_kernel's main
# loop: `acc[i][j] = mfma16(wb[u][j], fa[u & 1][i], acc[i][j])` over the KS = K >> 5 k-steps, the order inside an MFMA taken as
# sequential): K additions, K / ksplit for a slab of panel_partials, plus one for `v += bv` and one for `v[e] += (float)r[e]`.
# Rounding points, from the kernel's epilogue: the product is NOT rounded before bias and residual (`f32x4 v = acc * 1.0f`, then
# `f2bf(v[e])`): bf16(a W^T + b + r) is one point; with GELU the pre-activation is rounded first (`round_bf16(v[e])`, flags GELU |
# GELU_BF16) and the activation stored: two points.  The prologue's bf16(norm(x)) is a point of its own, settled off the ties
# through the float32 gamma / beta (settle_rms, settle_layernorm: 2^-12 steps as settle_gamma; the statistics are at most 24
# squares per lane and 6 wave levels, wave_sum_dpp, under the same 2^-19 margin).
# gelu_exp2_f (common.hpp): y = x rcp(1 + exp2(p)), p = x fma(x x, c1, c0), c0 = -2 sqrt(2 / pi) log2 e and c1 = 0.044715 c0 as
# float32 constants.  With u = 2^-24: p carries the roundings of x x, of the fma, of x p and of the two constants, all relative to
# quantities of one sign: |dp| <= 4 u |p|.  e = exp2(p) by v_exp_f32 (1 ulp = 2 u): relative (ln 2) 4 u |p| + 2 u.  d = 1 + e is
# rounded (u), and e's error reaches d with weight e / (1 + e) = 1 - sigmoid =: t <= 1.  v_rcp_f32 is 1 ulp (2 u), the product
# with x rounds once (u).  So |dy| <= |y| u (4 + t (2 + 4 ln 2 |p|)) (+ 2^-120: exp2 overflows to inf and y to 0 where the true
# |y| is below that).  It is relative to |y|, not to |g| as the 2^-23 |g| of the tanh form.  Its float64 reference is the sigmoid
# form x / (1 + exp(-2 k0 (x + k1 x^3))), which does not cancel in the negative tail as 1 + tanh does.
PANEL_KINDS = {"plain": (50, 1024, 1024), "bias": (50, 1024, 1024), "bias_res": (50, 1024, 1024), "gelu": (50, 1024, 1024),
               "exp2": (50, 1024, 1024), "thin": (520, 144, 64), "ln": (80, 256, 1152), "rms": (80, 256, 1024)}
_PANEL = {}
K0, K1 = 0.7978845608028654, 0.044715
C0 = float(torch.tensor([0xc0135761 - (1 << 32)], dtype=torch.int32).view(torch.float32))      # the kernel's constants
C1 = float(torch.tensor([0xbdd2d3e8 - (1 << 32)], dtype=torch.int32).view(torch.float32))


def gelu_sigmoid64(x):
    return x / (1.0 + torch.exp(-2.0 * K0 * (x + K1 * x ** 3)))


def gelu_exp2_bound(g):
    """|device - gelu(g)| of gelu_exp2_f on the same float32 g (derivation above)."""
    p = (g * (C1 * g * g + C0)).clamp(max=1000.0)
    t = 1.0 - 1.0 / (1.0 + torch.exp2(p))
    return gelu_sigmoid64(g).abs() * U24 * (4.0 + t * (2.0 + 4.0 * 0.6931471805599453 * p.abs())) + 2.0 ** -120


def panel_case(kind):
    """Seeded inputs and the (R16, bound) of a panel kind (cached): x [M, K] bf16 rows scaled by 1 + row % 8, w [N, K] with
    alternating K slices, f32 bias, bf16 residual, settled gamma / beta."""
    if kind in _PANEL:
        return _PANEL[kind]
    M, N, K = PANEL_KINDS[kind]
    g = torch.Generator().manual_seed(zlib.crc32(("panel" + kind).encode()))
    bf = torch.bfloat16
    rows = (1.0 + torch.arange(M) % 8).view(-1, 1)
    c = {"M": M, "N": N, "K": K, "norm": {"ln": 2, "rms": 1}.get(kind, 0)}
    c["x"] = (torch.randn(M, K, generator=g) * rows).to(bf)
    # pre-activations of std 1 to 7; 0.2 to 1.8 for the tanh form, whose float32 1 + tanh cancels in the negative tail (the exp2
    # form does not, and keeps the large ones)
    c["w"] = slice_alternate(torch.randn(N, K, generator=g) * ((0.15 if kind == "gelu" else 0.6) / K ** 0.5)).to(bf)
    c["bias"] = torch.randn(N, generator=g) * 0.3 if kind in ("bias", "bias_res", "gelu", "exp2") else None
    c["res"] = (torch.randn(M, N, generator=g) * rows).to(bf) if kind == "bias_res" else None
    gamma, beta = torch.randn(K, generator=g) * 0.1, torch.randn(K, generator=g) * 0.1
    h = c["x"].double()
    if kind == "rms":
        c["gamma"] = settle_rms(c["x"].double(), gamma)
        h = bf16r(rms_argument(h, c["gamma"])[0])
    elif kind == "ln":
        c["gamma"], c["beta"] = settle_layernorm(c["x"].double(), 1.0 + gamma, beta)
        h = bf16r(ln_argument(h, c["gamma"], c["beta"])[0])
    c["h16"] = h
    dot, sens = dot_and_sens(h, c["w"])
    depth = K
    if c["bias"] is not None:
        dot, sens, depth = dot + c["bias"].double(), sens + c["bias"].double().abs(), depth + 1
    if c["res"] is not None:
        dot, sens, depth = dot + c["res"].double(), sens + c["res"].double().abs(), depth + 1
    c["r64"] = dot
    y, d = _rnd(dot, depth * U24 * sens)
    if kind == "gelu":
        y, d = _rnd(gelu_tanh64(y), 1.13 * d + y.abs() * 2.0 ** -23)
    elif kind == "exp2":
        y, d = _rnd(gelu_sigmoid64(y), 1.13 * d + gelu_exp2_bound(y))
    c["ref"] = (y, d)
    _PANEL[kind] = c
    return c


def panel_partials_reference(ks=2):
    """R64 of the ks float32 slabs of the plain case and their bounds (K / ks) 2^-24 S."""
    c = panel_case("plain")
    K = c["K"] // ks
    parts = [dot_and_sens(c["h16"][:, s * K:(s + 1) * K], c["w"][:, s * K:(s + 1) * K]) for s in range(ks)]
    return torch.stack([p[0] for p in parts]), torch.stack([K * U24 * p[1] for p in parts])


def _acc_chain32(h, w):
    """The panel's own order in float32: one chain over the 32-deep k-steps, each step summed pairwise."""
    B, K = h.shape
    p = (h[:, None, :] * w[None, :, :]).view(B, -1, K // 32, 32)
    while p.shape[-1] > 1:
        p = p[..., 0::2] + p[..., 1::2]
    acc = torch.zeros(p.shape[:2])
    for s in range(p.shape[2]):
        acc = acc + p[:, :, s, 0]
    return acc


def panel_orders(kind):
    return ORDERS[:3] + ("chain32",) if PANEL_KINDS[kind][2] == 1024 else ("sequential", "chain32")


def f32_panel(kind, order, drop_step=None):
    """The bf16 output of a panel kind with float32 accumulation in `order` and a float32 epilogue, as float64.  drop_step: that
    32-deep k-step is left out (a corrupted restatement)."""
    c = panel_case(kind)
    f = torch.float32
    h, w = c["h16"].to(f), c["w"].to(f)
    if drop_step is not None:
        h = h.clone()
        h[:, 32 * drop_step:32 * drop_step + 32] = 0.0
    fn = _acc_chain32 if order == "chain32" else (lambda a, b: _acc_f32(a, b, order))
    v = torch.cat([fn(h[r0:r0 + 16].contiguous(), w) for r0 in range(0, h.shape[0], 16)], 0)
    if c["bias"] is not None:
        v = v + c["bias"]
    if kind == "gelu":
        x = _bf(v)
        v = 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * (x + 0.044715 * x * x * x)))
    elif kind == "exp2":
        x = _bf(v)
        v = x * (1.0 / (1.0 + torch.exp2(x * (x * x * torch.tensor(C1) + torch.tensor(C0)))))
    if c["res"] is not None:
        v = v + c["res"].to(f)
    return v.to(torch.bfloat16).double()


def measure_panel(kind):
    r = panel_case(kind)["ref"][0]
    return tuple(int((f32_panel(kind, o) != r).sum()) for o in panel_orders(kind)), r.numel()
