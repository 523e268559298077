"""Float64 references, element bounds, float32 restatements and seeded cases for the five kernels of csrc/lora.hip (lora_down,
lora_up_add, lora_wgrad + lora_wgrad_reduce, lora_merge), shared by tests/test_lora_reference_gpu.py (device against reference) and
tests/test_lora_reference_cpu.py (the criteria against float32 restatements and single-fault corruptions).  Plain torch on the
CPU; nothing here calls lap_amd.hip.

Every reference returns, per output, (R, bound).  R restates each bf16 rounding point the kernel states in its source; bound is
per element: depth u S carried through every later rounding point with _rnd, where S is the sum of the absolute terms of the
float32 sum, u = 2^-24 the relative error of one float32 rounding to nearest, and depth the longest chain of float32 additions a
term passes through.  Second-order terms (u^2) are dropped against the spare roundings counted (the first addition of every
chain is onto zero and exact).  Products of two bf16 numbers are exact in float32.  s is 1.0, 2.0 or 0.75 only: the float32
product of any of them with a bf16 number is exact (0.75 has two significant bits, bf16 eight), so bf16(s x) is one rounding of
the exact product and is restated as bf16r(s x).  The kernels test `s != 1.0f`: at s = 1 no scaling and no rounding takes place,
and the references skip them in the same way.

 * down (lora_down_kernel).  xs = X, or bf16(s X) (scale8) when s != 1.  acc = sum over the nsum copies and the ceil(K / 32)
   k-steps of one v_mfma_f32_16x16x32_bf16 each (columns at or past K are loaded as zeros: k_ok); t = bf16(acc), the only
   rounding point (f2bf at the store).  Group g reads columns [g xg, g xg + K) of X and rows [(n G + g) R, (n G + g + 1) R) of W.
   Depth: the 32 products inside one MFMA count as 32 sequential additions, and every MFMA step of the loop adds one more (its
   sum onto the accumulator).  The order and the rounding mode of the additions inside the instruction are not documented
   in this repository, so round-to-nearest is NOT assumed there: a truncating adder errs by up to one spacing, 2 u, and every one
   of these additions is counted twice.  DOWN depth = 2 (32 + nsum ceil(K / 32)).
 * up_add (lora_up_add_kernel).  acc = the __builtin_fmaf chain over n < nsum, j < R (one rounding per step, the products are
   exact anyway): depth nsum R.  p = round_bf16(acc); when s != 1, p = round_bf16(p s) (exact product, one rounding, bound times
   s); y = f2bf(bf2f(y) + p): the float32 sum of two bf16 numbers rounds once (u |y0 + p|), then the bf16 store.
 * wgrad (lora_wgrad_kernel, lora_wgrad_reduce_kernel).  bs = B, or bf16(s B) when s != 1.  mchunk = the rows of M per split
   rounded up to 32, S = ceil(M / mchunk) <= msplit.  One block chains ceil(rows of its chunk / 32) MFMAs (rows past the chunk are
   zeros), counted as for down: 2 (32 + mchunk / 32).  S > 1: the partials go to float32 scratch and the reduce pass adds them in
   order z = 0 .. S - 1 onto 0.f: S more additions of u each (plain float32, to nearest).  The float32 output is the sum itself;
   the bf16 output carries one rounding.  Every one of the ncopy copies is stored from the same register: the same reference.
 * merge (lora_merge_kernel).  Everything in float32: acc = the fma chain over n < nsum, j < R of B[.][c] A[.][i] (the product is
   not exact, but an fma rounds once): depth nsum R on S = sum |B| |A|; w + s acc: the product and the sum round once each (or
   once together when contracted; counting both covers either); then the bf16 store.

Criterion (b), the share of elements that differ from R at all, applies to the bf16 outputs.  Its cap for a case is
max(4 x the largest share at which a float32 restatement of that case differs from R, 4 / numel), and never more than CAP_LIMIT =
1 / 128: one fragment column of one wave's 16 x 64 strip is 1 / 64 of it, and no cap may be able to hide that.  So an output of 256
elements or fewer may differ in one element (numel >= 128) or in none.  The shares are the only numbers here that are measured
and not derived: F32_SHARE records them per case (cases not listed: no restatement differs in any element);
tests/test_lora_reference_cpu.py measures them again and asserts that none is larger than recorded.

Cases: the smallest shapes that reach each branch of the kernels (tests/test_lora_reference_gpu.py names the branch per case).
Inputs are seeded here on the CPU; adapter operands are scaled by 0.05; rows 0 and M / 2 of the activation operand (column 0 of
wgrad's `a`, row 0 of merge's A) hold a common offset 3 + 0.1 noise, so that sums cancel and S is well above |R|."""
from collections import namedtuple

import torch

from tests.decode_reference import _rnd, bf16r, check_elementwise, differing_share, ulp_bf16, worst_ratio  # noqa: F401 (re-exported)
from tests.train_reference import Arena, gen, sub, sum32, untouched, view  # noqa: F401 (re-exported)

U = 2.0 ** -24
CAP_LIMIT = 1.0 / 128
S_VALUES = (1.0, 0.75, 2.0)
BF16_OUTPUTS = ("t", "y", "out_bf16", "weff")

Down = namedtuple("Down", "M K G R nsum s xg px pw pt", defaults=(1, 1.0, 0, 0, 0, 0))       # px / pw / pt: padding of ldx / ldw / ldt
Up = namedtuple("Up", "M Ng G R nsum s tw py pb pt", defaults=(1, 1.0, 0, 0, 0, 0))          # tw: columns of t beyond G R
Wgrad = namedtuple("Wgrad", "M Ng G R ncopy s msplit bg pa pb po", defaults=(1, 1.0, 1, 0, 0, 0, 0))
Merge = namedtuple("Merge", "I Ng G R nsum s pw pa pb po", defaults=(1, 1.0, 0, 0, 0, 0))

_PAD = dict(px=8, pw=16, pt=3)
DOWN_CASES = (
    Down(1, 8, 1, 16),
    Down(77, 48, 1, 48), Down(77, 72, 1, 48, s=0.75), Down(77, 88, 1, 48, s=2.0),
    Down(77, 48, 1, 48, **_PAD), Down(77, 72, 1, 48, s=0.75, **_PAD), Down(77, 88, 1, 48, s=2.0, **_PAD),
    Down(130, 200, 1, 80, s=0.75), Down(130, 200, 1, 128),
    Down(45, 40, 3, 16, nsum=2, s=0.75, xg=40, px=8),
    Down(64, 16, 10, 16, s=2.0, xg=16),
    Down(33, 64, 1, 32, nsum=8),
)
UP_CASES = (
    Up(1, 40, 3, 16), Up(17, 40, 3, 16, s=0.75), Up(70, 40, 3, 16, s=2.0),
    Up(17, 8, 1, 16, nsum=8),
    Up(17, 104, 5, 16, s=0.75),
    Up(17, 40, 3, 24, s=2.0),
    Up(17, 72, 1, 320),
    Up(17, 40, 3, 16, s=0.75, tw=16, pt=1),
    Up(70, 40, 3, 16, nsum=8, s=0.75, py=8, pb=8),
)
WGRAD_CASES = (
    Wgrad(1, 40, 1, 16), Wgrad(31, 40, 1, 16, s=0.75), Wgrad(32, 40, 1, 16, s=2.0), Wgrad(33, 40, 1, 16),
    Wgrad(100, 40, 1, 16, s=0.75), Wgrad(100, 40, 1, 16, s=0.75, msplit=2), Wgrad(100, 40, 1, 16, s=0.75, msplit=3),
    Wgrad(100, 40, 1, 16, s=0.75, msplit=4),
    Wgrad(33, 8, 1, 16, s=2.0), Wgrad(33, 72, 1, 16, ncopy=8),
    Wgrad(33, 40, 3, 16, ncopy=8, s=0.75, bg=40),
    Wgrad(33, 40, 1, 48, s=2.0),
    Wgrad(100, 40, 3, 16, ncopy=8, s=2.0, msplit=4, bg=40, pa=8, pb=8, po=5),
)
MERGE_CASES = (
    Merge(4, 3, 2, 5),
    Merge(1028, 3, 2, 5, nsum=8, s=0.75),
    Merge(36, 8, 1, 16, s=2.0),
    Merge(36, 3, 2, 5, nsum=8, s=2.0, pw=4, pa=4, pb=1, po=4),
)
CASES = dict(down=DOWN_CASES, up_add=UP_CASES, wgrad=WGRAD_CASES, merge=MERGE_CASES)

# Largest share of elements at which a float32 restatement (any order) of a case differs from R, measured by
# tests/test_lora_reference_cpu.py::test_float32_restatements_meet_both_criteria; a case that is not listed differs in none.
F32_SHARE = {
    "down-77-72-1-48-1-0.75-0-8-16-3:t": 2.71e-4,       # measured: 1 of 3696 (seq)
    "down-130-200-1-80-1-0.75-0-0-0-0:t": 9.62e-5,      # measured: 1 of 10400
}


def case_id(spec, out=""):
    return type(spec).__name__.lower() + "-" + "-".join(f"{v:g}" for v in spec) + (":" + out if out else "")


def cap(spec, out, numel):
    """The cap of criterion (b) for one bf16 output of a case; None for a float32 output."""
    if out not in BF16_OUTPUTS:
        return None
    return min(max(4.0 * F32_SHARE.get(case_id(spec, out), 0.0), 4.0 / numel), CAP_LIMIT)


def cdiv(a, b):
    return (a + b - 1) // b


def wgrad_split(M, msplit):
    """(mchunk, S) as lap_lora_wgrad computes them."""
    mchunk = (cdiv(M, msplit) + 31) & ~31
    return mchunk, cdiv(M, mchunk)


def down_depth(p):
    return 2 * (32 + p.nsum * cdiv(p.K, 32))


def wgrad_depth(p):
    mchunk, S = wgrad_split(p.M, p.msplit)
    return 2 * (32 + cdiv(min(mchunk, p.M), 32)) + (S if S > 1 else 0)


# ============================================================================================================= inputs
_CASES = {}


def _offset_rows(x, g, rows):
    for r in rows:
        x[r] = 3.0 + 0.1 * torch.randn(x.shape[1], generator=g)
    return x


def make_case(spec):
    """The seeded operands of a case (contiguous; the device test lays them out with the case's leading dimensions)."""
    if spec in _CASES:
        return _CASES[spec]
    g = gen(case_id(spec))
    rnd = lambda *s: torch.randn(*s, generator=g)       # noqa: E731
    p, c = spec, dict(spec=spec)
    if isinstance(p, Down):
        c["x"] = _offset_rows(rnd(p.M, (p.G - 1) * p.xg + p.K), g, {0, p.M // 2}).bfloat16()
        c["w"] = (0.05 * rnd(p.nsum * p.G * p.R, p.K)).bfloat16()
    elif isinstance(p, Up):
        c["t_raw"] = _offset_rows(rnd(p.M, p.G * p.R), g, {0, p.M // 2})      # the float32 sum t is the rounding of (fault t_unrounded)
        c["t"] = c["t_raw"].bfloat16()
        c["b"] = (0.05 * rnd(p.nsum * p.G * p.R, p.Ng)).bfloat16()
        c["y0"] = rnd(p.M, p.G * p.Ng).bfloat16()
    elif isinstance(p, Wgrad):
        a = rnd(p.M, p.G * p.R)
        a[:, 0] = 3.0 + 0.1 * torch.randn(p.M, generator=g)
        c["a"] = a.bfloat16()
        c["b"] = rnd(p.M, (p.G - 1) * p.bg + p.Ng).bfloat16()
    else:
        c["w"] = 0.02 * rnd(p.G * p.Ng, p.I)
        c["a"] = 0.05 * _offset_rows(rnd(p.G * p.R, p.I), g, {0})
        c["b"] = 0.05 * rnd(p.nsum * p.G * p.R, p.Ng)
    _CASES[spec] = c
    return c


def drop_caches():
    _CASES.clear()


# ================================================================================================ float64 references
def ref_down(c, rounded=True):
    p = c["spec"]
    xs = p.s * c["x"].double()
    if rounded and p.s != 1.0:
        xs = bf16r(xs)
    W = c["w"].double().view(p.nsum, p.G, p.R, p.K)
    val, mag = [], []
    for g in range(p.G):
        xg = xs[:, g * p.xg:g * p.xg + p.K]
        val.append(xg @ W[:, g].sum(0).T)
        mag.append(xg.abs() @ W[:, g].abs().sum(0).T)
    val, mag = torch.cat(val, 1), torch.cat(mag, 1)
    if not rounded:
        return val
    return dict(t=_rnd(val, down_depth(p) * U * mag))


def ref_up_add(c, rounded=True, t=None):
    p = c["spec"]
    t = (c["t"] if t is None else t).double()
    B = c["b"].double().view(p.nsum, p.G, p.R, p.Ng)
    acc, mag = [], []
    for g in range(p.G):
        tg = t[:, g * p.R:(g + 1) * p.R]
        acc.append(tg @ B[:, g].sum(0))
        mag.append(tg.abs() @ B[:, g].abs().sum(0))
    acc, mag = torch.cat(acc, 1), torch.cat(mag, 1)
    y0 = c["y0"].double()
    if not rounded:
        return y0 + p.s * acc
    v, d = _rnd(acc, p.nsum * p.R * U * mag)
    if p.s != 1.0:
        v, d = _rnd(p.s * v, p.s * d)
    return dict(y=_rnd(y0 + v, d + U * (y0 + v).abs()))


def ref_wgrad(c, rounded=True):
    p = c["spec"]
    a = c["a"].double()
    bs = p.s * c["b"].double()
    if rounded and p.s != 1.0:
        bs = bf16r(bs)
    val, mag = [], []
    for g in range(p.G):
        ag, bg = a[:, g * p.R:(g + 1) * p.R], bs[:, g * p.bg:g * p.bg + p.Ng]
        val.append(ag.T @ bg)
        mag.append(ag.abs().T @ bg.abs())
    val, mag = torch.cat(val, 0).repeat(p.ncopy, 1), torch.cat(mag, 0).repeat(p.ncopy, 1)
    if not rounded:
        return val
    d = wgrad_depth(p) * U * mag
    return dict(out_f32=(val, d), out_bf16=_rnd(val, d))


def ref_merge(c, rounded=True):
    p = c["spec"]
    W, A = c["w"].double(), c["a"].double().view(p.G, p.R, p.I)
    B = c["b"].double().view(p.nsum, p.G, p.R, p.Ng)
    acc, mag = [], []
    for g in range(p.G):
        acc.append(B[:, g].sum(0).T @ A[g])
        mag.append(B[:, g].abs().sum(0).T @ A[g].abs())
    acc, mag = torch.cat(acc, 0), torch.cat(mag, 0)
    v = W + p.s * acc
    if not rounded:
        return v
    return dict(weff=_rnd(v, p.s * p.nsum * p.R * U * mag + U * (p.s * acc).abs() + U * v.abs()))


REFS = dict(down=ref_down, up_add=ref_up_add, wgrad=ref_wgrad, merge=ref_merge)


# ========================================================================================== float32 restatements
def _bf(x):
    return x.to(torch.bfloat16).float()


def dot32(a, b, order, acc=None):
    """acc + a b^T in float32 (a [M, K], b [C, K]).  seq: one product after the other; chunk32: runs of 32 summed pairwise, the
    runs chained onto the accumulator one after the other (an MFMA step)."""
    acc = torch.zeros(a.shape[0], b.shape[0]) if acc is None else acc
    K = a.shape[1]
    if order == "seq":
        for k in range(K):
            acc = acc + a[:, k, None] * b[None, :, k]
        return acc
    for k0 in range(0, K, 32):
        acc = acc + sum32(a[:, None, k0:k0 + 32] * b[None, :, k0:k0 + 32], "tree")
    return acc


DOWN_ORDERS = UP_ORDERS = MERGE_ORDERS = ("seq", "chunk32")
WGRAD_ORDERS = ("seq", "chunk32", "split")


def _scaled(x, s, fault):
    """bf16(s x), or x at s = 1; s1_shortcut: the s == 1 path taken whatever s is."""
    return x if s == 1.0 or fault == "s1_shortcut" else _bf(s * x)


def f32_down(c, order, fault=None):
    p = c["spec"]
    xs = _scaled(c["x"].float(), p.s, fault)
    W = c["w"].float().view(p.nsum, p.G, p.R, p.K)
    K = p.K - 8 if fault == "drop_k8" else p.K
    cols = []
    for g in range(p.G):
        x0 = 0 if fault == "group0_cols" and g == 1 else g * p.xg
        acc = None
        for n in range(p.nsum - 1 if fault == "drop_copy" and p.nsum > 1 else p.nsum):
            acc = dot32(xs[:, x0:x0 + K], W[n, g][:, :K], order, acc)
        cols.append(acc)
    t = _bf(torch.cat(cols, 1))
    if fault == "cd_rows":       # the four C/D rows of a lane stored to 4 i + (lane >> 4) instead of 4 (lane >> 4) + i
        r = torch.arange(cdiv(p.M, 16) * 16)
        dst = (r // 16) * 16 + 4 * (r % 4) + (r % 16) // 4
        full = torch.zeros(r.numel(), t.shape[1])
        full[dst[:p.M]] = t
        t = full[:p.M]
    return dict(t=t.double())


def f32_up_add(c, order, fault=None):
    p = c["spec"]
    t = c["t_raw"] if fault == "t_unrounded" else c["t"].float()
    B = c["b"].float().view(p.nsum, p.G, p.R, p.Ng)
    cols = []
    for g in range(p.G):
        acc = None
        for n in range(p.nsum - 1 if fault == "drop_copy" and p.nsum > 1 else p.nsum):
            acc = dot32(t[:, g * p.R:(g + 1) * p.R], B[n, g].T, order, acc)
        cols.append(acc)
    acc = torch.cat(cols, 1)
    if fault == "s_before_rounding":
        v = _bf(p.s * acc)
    else:
        v = _bf(acc)
        if p.s != 1.0 and fault != "s1_shortcut":
            v = _bf(v * p.s)
    return dict(y=_bf(c["y0"].float() + v).double())


def f32_wgrad(c, order, fault=None):
    p = c["spec"]
    a = c["a"].float()
    bs = c["b"].float() if fault == "bs_unscaled" else _scaled(c["b"].float(), p.s, fault)
    M = p.M
    if fault == "drop_short_chunk" and M % 32:
        M = 32 * (M // 32)
    mchunk, _ = wgrad_split(p.M, p.msplit)
    rows = []
    for g in range(p.G):
        ag, bg = a[:M, g * p.R:(g + 1) * p.R].T, bs[:M, g * p.bg:g * p.bg + p.Ng].T
        if order == "split":
            v = torch.zeros(p.R, p.Ng)
            for m0 in range(0, M, mchunk):
                v = v + dot32(ag[:, m0:m0 + mchunk], bg[:, m0:m0 + mchunk], "chunk32")
        else:
            v = dot32(ag, bg, order)
        rows.append(v)
    v = torch.cat(rows, 0)
    f32, b16 = v.repeat(p.ncopy, 1), _bf(v).repeat(p.ncopy, 1)
    if fault == "copy0_only":
        f32[v.shape[0]:], b16[v.shape[0]:] = 0.0, 0.0
    return dict(out_f32=f32.double(), out_bf16=b16.double())


def f32_merge(c, order, fault=None):
    p = c["spec"]
    W, A = c["w"], c["a"].view(p.G, p.R, p.I)
    B = c["b"].view(p.nsum, p.G, p.R, p.Ng)
    rows = []
    for g in range(p.G):
        acc = None
        for n in range(p.nsum - 1 if fault == "drop_copy" and p.nsum > 1 else p.nsum):
            acc = dot32(B[n, g].T, A[g].T, order, acc)
        rows.append(acc)
    acc = torch.cat(rows, 0)
    s = 1.0 if fault == "no_s" else p.s
    if fault == "w_after_rounding":
        return dict(weff=_bf(_bf(s * acc) + W).double())
    return dict(weff=_bf(W + s * acc).double())


F32 = dict(down=(f32_down, DOWN_ORDERS), up_add=(f32_up_add, UP_ORDERS), wgrad=(f32_wgrad, WGRAD_ORDERS), merge=(f32_merge, MERGE_ORDERS))


def judge(spec, got, ref):
    """{output: (worst error / bound, differing share or None, cap or None)} of a restatement's or the device's outputs."""
    res = {}
    for n, (r, b) in ref.items():
        g = got[n].double().reshape(r.shape)
        cp = cap(spec, n, r.numel())
        res[n] = (worst_ratio(g, r, b.clamp(min=1e-300)), None if cp is None else differing_share(g, r), cp)
    return res


def passes(res):
    return all(ratio <= 1.0 and (cp is None or share <= cp) for ratio, share, cp in res.values())
