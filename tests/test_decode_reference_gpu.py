"""The fused decode kernels (csrc/decode.hip) element by element against float64 restatements of their formulas (GPU).

The references (tests/decode_reference.py) are plain torch in float64 on the CPU, written from the header of decode.hip and DESIGN.md 4.4;
they call nothing of lap_amd.hip.  R64 is the operation without intermediate rounding, R16 the same with the kernels' documented
bf16 rounding points restated (h, the projection output, the rotation, g / gelu(g) / the product, the residual sum).  The inputs
are drawn with a CPU generator, so what is measured on the CPU below is what the device is given; B < 8 takes the first B rows of
the B = 8 inputs (row b scaled by 1 + b), whose reference rows are computed once.

Criteria for the bf16 outputs (q, cache rows, y, act), against R16:
 (a) every element: |dev - R16| <= sum over the rounding points of one bf16 spacing times the gain to the output, plus
     64 2^-24 S_e carried through the same gains, S_e = sum_k |w_k| |h_k| of the element's dot product(s) in float64; 64 bounds the
     depth of every summation tree (<= 32 fmas per lane, 6 wave levels, 4 K slices, hi + lo).  Rounding points per epilogue:
       RES    n = 1  the residual sum (gain 1): exactly n ulp(R16) + 64 2^-24 S_e.
       QKV    n = 2  for q and k: the projection (gains |cos|, |sin|) and the rotation; q_scale = 2^-4 and the store of an
                     already rounded number are exact, so the third point of the header adds nothing; n = 1 for v.  The float32
                     angle adds (|x1| + |x2|) 2^-22 (pos + 1) (powf, the division, sincosf): 2e-4 at pos 839, 0.05 spacings.
       GeGLU  n = 4  g (gain 1.13 |u|: gelu's slope is at most 1.13), u (gain |gelu g|), gelu (gain |u|), the stored product.
                     The float32 form 0.5 g (1 + tanh(.)) cancels in its negative tail: 2^-23 |g| absolute, with gain |u|.
     Where every gain is 1 this is n ulp_bf16(R16) + 64 2^-24 S_e.  A single flipped rounding already gives error / bound ~ 0.99.
 (b) at most CAP of the elements may differ from R16 at all.  CAP = 4 x the largest share of elements at which R16 restated with
     float32 accumulation (and a float32 epilogue) differs from the float64 R16, over three summation orders (sequential, pairwise,
     8 per lane x 64 lanes with a tree), measured on the CPU on the B = 8 inputs of each case (decode_reference.DIFFERING holds the
     counts; tests/test_decode_reference_cpu.py measures them again):
       kind            weights   sequential  pairwise   lanes      CAP
       res2048         bf16      2.44e-04    6.10e-05   0          9.77e-04
       res2048         fp8       0           0          0          0          (the device must reproduce R16 bit for bit)
       res16384        bf16      5.49e-04    1.22e-04   1.83e-04   2.20e-03
       res16384        fp8       2.44e-04    6.10e-05   1.22e-04   9.77e-04
       qkv (t 18)      bf16      9.28e-04    1.03e-03   9.28e-04   4.10e-03
       qkv (t 18)      fp8       9.28e-04    8.79e-04   9.28e-04   3.71e-03
       gate_up         bf16      3.97e-04    1.75e-04   1.37e-04   1.59e-03
       gate_up         fp8       9.77e-03    9.79e-03   9.82e-03   3.93e-02  (rows scaled by 2^6: |g| ~ 58, the cancelling gelu tail)
       res2048 N 4098  bf16      2.75e-04    0          6.10e-05   1.10e-03
       res2048 N 4098  fp8       0           3.05e-05   0          1.22e-04
     Resolution.  The caps are measured on 8 rows and applied to the B rows of a test, so at B = 1 the res caps stand for whole
     elements of 2048: at most 2 (res2048 bf16), 4 (res16384 bf16), 2 (res16384 fp8), and none for res2048 fp8 at any B.  The N = 2
     and N = 6 edge cases (6 to 48 elements) assert (a) and print the share; N = 4098 has its own measured cap.
     Both terms of (a) beyond the spacings (the float32 RoPE angle, the tanh cancellation) were derived from common.hpp's rope_sincos
     and gelu_tanh_f and written down before the module first ran on a device; nothing in (a) or (b) was changed after a device run
     except that the res2048 caps, first pooled over both weight forms (4.88e-4), are now the two measured ones above.
The f32 debug logits of the LM head, against R64 of hi.h + lo.h on the bf16-rounded normalised row h (the one rounding point):
|dev - R64| <= 64 2^-24 S_e; and R64 on the planes agrees with R64 on the f32 table to 2^-16 S_e (the split itself).
Attention, against R64 (softmax over the allowed keys, no rounding of p): |o - R64| <= 2^-7 A_d, A_d = sum_j softmax_j |v_jd|.

Inputs chosen so that the reference alone stays clear of an allowance (all checked on the CPU again by the tests):
 * h.  The kernels compute the argument of h = bf16(x r (1 + gamma)) in float32 (error < 2^-20 relative).  gamma is nudged
   (decode_reference.settle_gamma) until every |h| keeps 2^-19 (relative) from every bf16 rounding tie, so the reference's h is the kernel's.
 * Tokens.  The float64 top-2 logit margin exceeds twice the logit bound in every row: smallest margin / (2 bound) is 75 (V 4097,
   hi plane alone: 0.0242 against 3.2e-4); with fp8 rows 13.0 (V 4097: 0.264 against 0.0203).  The allowance is asserted unused.
 * Draws.  SAMPLING lists seeds at which the top-2 margin of the host-restated scores exceeds 2 (TIE + bound inv_t) in every row
   (smallest ratio over the rows, B = 8: 10.8 at V 4097, T 0.5, fp8 rows; 64 or more elsewhere).  The allowance is asserted unused.
 * Exact count.  Elements whose reference sum is 0, or where adding or dropping one key would move bf16(mean) by no more than the
   one-spacing allowance, are not asserted: 3.7 / 7.7 / 5.1 % of the elements at Pn 157 and 3.5 / 8.2 / 5.4 % at Pn 16 (B = 1 / 3 / 8); the test requires
   < 10 %.  Pn 16 steps through the odd t (odd counts: no zero sum) plus 8 and 16 (the powers of two), Pn 157 through every t.
"""
import numpy as np
import pytest
import torch

from lap_amd import sampling as S
from tests import decode_reference as C
from tests.decode_reference import DD, DH, DHD, DNH, check_elementwise

pytestmark = pytest.mark.gpu
DEV = "cuda"
TIE = 4 * 3.814697265625e-06          # tests/test_ar_sampling_gpu.py's TIE (the last bits of the noise's two logarithms)
NAN = float("nan")
BATCHES = list(range(1, 9))
# (V, temperature, seed, step)
SAMPLING = ((4097, 1.0, 11, 2), (4097, 0.5, 12, 5), (20481, 1.0, 13, 2), (20481, 0.5, 14, 5))


@pytest.fixture(scope="module", autouse=True)
def _drop_device_copies():
    """The inputs are uploaded once per module (_dev); hand the device memory back to the tests after it."""
    yield
    for c in C._CASES.values():
        c.pop("_dev", None)
    torch.cuda.empty_cache()


def _state(hip, B, t, plen):
    st = hip.decode_state(B, DEV)
    st[0] = t
    st[16:16 + B] = torch.as_tensor(plen, dtype=torch.int32)[:B]
    return st


def _dev(c, key, B=None):
    """c[key] on the device (uploaded once), its first B rows."""
    d = c.setdefault("_dev", {})
    if key not in d:
        d[key] = c[key].to(DEV).contiguous()
    return d[key] if B is None else d[key][:B].contiguous()


def _weight(c, name="w"):
    """(weight argument, wscale) of a projection case."""
    return (_dev(c, "codes"), _dev(c, "scales")) if c["fp8"] else (_dev(c, name), None)


def _ref(c, key, fn):
    if key not in c:
        c[key] = fn()
    return c[key]


# --------------------------------------------------------------------------------------------------------------- embed
@pytest.mark.parametrize("B", [1, 3, 8])
def test_embed_live_window(hip, B):
    g = torch.Generator().manual_seed(7)
    row_lo, row_hi, cap, t = 1000, 1064, 5, 3
    table = torch.randn(row_hi - row_lo, DD, generator=g)
    toks = torch.tensor([row_lo, row_hi - 1, row_lo - 1, 1031, 0, row_hi, 1063, 250000], dtype=torch.int32)
    out = torch.randint(row_lo, row_hi, (8, cap), generator=g, dtype=torch.int32)   # live tokens in every other column
    out[:, t - 1] = toks
    scale = float(np.sqrt(2048.0))
    ref = (table * torch.tensor(scale, dtype=torch.float32)).to(torch.bfloat16)
    xpad = torch.full((B + 2, DD), 3.0, dtype=torch.bfloat16, device=DEV)
    for first in range(0, 8 - B + 1, B):        # B = 1: every token in turn; B = 3: rows 0-2 (lo, hi - 1, lo - 1) and 3-5 (.., hi)
        o = out[first:first + B].contiguous()
        xpad.fill_(3.0)
        hip.decode_embed(_state(hip, B, t, [5] * 8), table.to(DEV), row_lo, row_hi, o.to(DEV), xpad[:B], scale)
        x = xpad.cpu()
        for b in range(B):
            tok = int(o[b, t - 1])
            want = ref[tok - row_lo] if row_lo <= tok < row_hi else torch.zeros(DD, dtype=torch.bfloat16)
            assert torch.equal(x[b], want), (b, tok)
        assert bool((x[B:] == 3.0).all())


# --------------------------------------------------------------------------------------------------------- projections
def _qkv_ref(c, t):
    pos = c["plen"] + t - 1
    return _ref(c, ("qkv", t), lambda: C.ref_qkv(c["h16"], c["wd"], pos, DNH, DHD, c["q_scale"]))


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("B", BATCHES)
def test_qkv(hip, B, fp8):
    c = C.decode_case("qkv", fp8)
    assert float(np.log2(c["q_scale"])).is_integer()           # the q scale and the store are exact (n = 2)
    assert float(C.tie_distance(C.norm_rows64(c["x"], c["gamma"])).min()) >= C.TIE_MARGIN
    w, ws = _weight(c)
    cap = C.QKV_CAP
    for t in (1, C.QKV_T, cap):
        ck = torch.full((B, cap, DHD), NAN, dtype=torch.bfloat16, device=DEV)
        cv, q = ck.clone(), torch.full((B, DNH * DHD), NAN, dtype=torch.bfloat16, device=DEV)
        hip.decode_qkv(_state(hip, B, t, c["plen"]), _dev(c, "x", B), _dev(c, "gamma"), w, q, ck, cv, DNH, DHD, c["q_scale"], wscale=ws)
        (qr, qb), (kr, kb), (vr, vb) = _qkv_ref(c, t)
        dev = torch.cat([q, ck[:, t - 1], cv[:, t - 1]], 1)
        check_elementwise(dev, torch.cat([qr, kr, vr], 1)[:B], torch.cat([qb, kb, vb], 1)[:B], C.share_cap("qkv", fp8), f"qkv B {B} t {t}")
        others = [r for r in range(cap) if r != t - 1]          # NaN before, the same NaN bits after
        for cache in (ck, cv):
            assert bool((cache[:, others].view(torch.int16) == torch.tensor(NAN, dtype=torch.bfloat16).view(torch.int16).item()).all())


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("B", BATCHES)
def test_gate_up(hip, B, fp8):
    c = C.decode_case("gate_up", fp8)
    assert float(C.tie_distance(C.norm_rows64(c["x"], c["gamma"])).min()) >= C.TIE_MARGIN
    w, ws = _weight(c)
    act = torch.full((B, DH), NAN, dtype=torch.bfloat16, device=DEV)
    hip.decode_gate_up(_state(hip, B, 1, [10] * 8), _dev(c, "x", B), _dev(c, "gamma"), w, act, wscale=ws)
    r, bound = _ref(c, "ref", lambda: C.ref_gate_up(c["h16"], c["wd"], DH))
    check_elementwise(act, r[:B], bound[:B], C.share_cap("gate_up", fp8), f"gate_up B {B}")


def _residual(hip, c, B, kwaves, cap, what):
    w, ws = _weight(c)
    y = torch.full((B, c["res"].shape[1]), NAN, dtype=torch.bfloat16, device=DEV)
    hip.decode_proj_residual(_state(hip, B, 1, [10] * 8), _dev(c, "a", B), w, _dev(c, "res", B), y, kwaves=kwaves, wscale=ws)
    r, bound = _ref(c, "ref", lambda: C.ref_residual(c["a"], c["wd"], c["res"]))
    check_elementwise(y, r[:B], bound[:B], cap, what)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("B", BATCHES)
def test_proj_residual(hip, B, fp8):
    for kind, kwaves in (("res2048", 1), ("res2048", 4), ("res16384", 4)):
        _residual(hip, C.decode_case(kind, fp8), B, kwaves, C.share_cap(kind, fp8), f"proj_residual {kind} kwaves {kwaves} B {B}")


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("B", [3, 8])
def test_proj_residual_edges(hip, B, fp8):
    """N = 2; N = 6: three units, a partial last block at kwaves 1; N = 4098: past the 2048-block grid cap at kwaves 4."""
    for N in (2, 6, 4098):
        for kwaves in (1, 4):
            _residual(hip, C.decode_case("res2048", fp8, N=N), B, kwaves, C.share_cap("res2048", fp8, N) if N == 4098 else None, f"proj_residual N {N} kwaves {kwaves} B {B}")


# ------------------------------------------------------------------------------------------------------------- LM head
def _lm_run(hip, c, B, sample, t=2, cap=6, samp=None, logits=True):
    V = c["V"]
    fp8 = c["form"] == "fp8"
    hi, lo, ws = (_dev(c, "codes"), None, _dev(c, "scales")) if fp8 else (_dev(c, "hi"), _dev(c, "lo") if c["form"] == "hilo" else None, None)
    st = _state(hip, B, t, [5] * 8)
    out = torch.zeros(B, cap, dtype=torch.int32, device=DEV)
    pval, pidx = hip.decode_lm_partials(B, DEV)
    pval.fill_(NAN); pidx.fill_(-7)
    lg = torch.full((B, V), NAN, dtype=torch.float32, device=DEV) if logits else None
    if sample:
        samp = hip.decode_sampling(DEV) if samp is None else samp
        hip.decode_lm_head_sample(st, samp, _dev(c, "x", B), _dev(c, "gamma"), hi, lo, pval, pidx, logits=lg, wscale=ws)
    else:
        hip.decode_lm_head(st, _dev(c, "x", B), _dev(c, "gamma"), hi, lo, pval, pidx, logits=lg, wscale=ws)
    hip.decode_finish(st, pval, pidx, out, eos_token=-1)
    assert int(st[0]) == t + 1 and int(out[:, :t].abs().sum()) == 0 and int(out[:, t + 1:].abs().sum()) == 0
    return lg, out[:, t].cpu().long()


@pytest.mark.parametrize("V", [2, 4097, 20481])
@pytest.mark.parametrize("B", BATCHES)
def test_lm_head_logits_and_tokens(hip, B, V):
    for form in C.LM_FORMS:
        c = C.lm_case(V, form)
        assert float(C.tie_distance(C.norm_rows64(c["x"], c["gamma"])).min()) >= C.TIE_MARGIN
        ref, bound = c["ref"][:B], c["bound"][:B]
        if form == "hilo":          # the split: hi + lo against the f32 table
            full, sens = _ref(c, "full", lambda: C.dot_and_sens(c["h16"], c["table"]))
            assert bool(((c["ref"] - full).abs() <= 2.0 ** -16 * sens).all())
        margin = C.top2_margin(ref)
        assert bool((margin > 2 * bound.max(1).values).all()), (form, margin, bound.max())     # the committed inputs never need the allowance
        for sample in (False, True):                                     # the sampling head at temperature 0 (zeroed words)
            lg, tok = _lm_run(hip, c, B, sample)
            ratio = C.worst_ratio(lg, ref, bound)
            print(f"lm_head{'_sample' if sample else ''} V {V} {form} B {B}: worst logit error / bound {ratio:.3f}, "
                  f"smallest margin / (2 bound) {float((margin / (2 * bound.max(1).values)).min()):.1f}")
            assert ratio <= 1.0
            assert C.check_tokens(tok, ref, bound, f"{form} sample {sample}") == 0
        if V > 2:                   # the best row of sample 0 again at a lower index and at the last (odd) row: the lowest wins
            d = C.lm_case(V, form, dup=True)
            ref = d["ref"][:B]
            assert bool((C.top2_margin(ref) > 2 * d["bound"][:B].max(1).values).all())
            assert int(C.first_argmax(ref)[0]) == d["dups"][0]
            for sample in (False, True):
                _, tok = _lm_run(hip, d, B, sample, logits=False)
                assert C.check_tokens(tok, ref, d["bound"][:B], f"{form} sample {sample}, duplicated rows") == 0


def sampling_clearance(c, B, T, seed, step):
    """(host-restated scores [B, V] of the float64 logits, per row: top-2 score margin / (2 (TIE + logit bound inv_t)))."""
    sc = S.scores_from_logits(c["ref"][:B].float().numpy(), T, seed, step)
    allow = TIE + c["bound"][:B].max(1).values.numpy() * float(S.inverse_temperature(T))
    top2 = np.partition(sc, -2, axis=1)[:, -2:]
    return sc, allow, (top2[:, 1] - top2[:, 0]) / (2 * allow)


@pytest.mark.parametrize("B", [8, 5])
def test_sampling_head_draws(hip, B):
    for V, T, seed, step in SAMPLING:
        for form in C.LM_FORMS:
            c = C.lm_case(V, form)
            sc, allow, clear = sampling_clearance(c, B, T, seed, step)
            assert float(clear.min()) > 1.0, (V, T, seed, form, clear)   # the committed seeds never need the allowance
            samp = hip.decode_sampling(DEV)
            hip.decode_set_sampling(samp, seed, T)
            lg, tok = _lm_run(hip, c, B, True, t=step, cap=8, samp=samp)
            assert C.worst_ratio(lg, c["ref"][:B], c["bound"][:B]) <= 1.0          # the debug logits stay raw
            best = np.argmax(sc, axis=1)
            gap = sc[np.arange(B), best] - sc[np.arange(B), tok.numpy()]
            used = int((tok.numpy() != best).sum())
            print(f"sampling V {V} T {T} {form} B {B}: smallest margin / allowance {float(clear.min()):.1f}, {used} draws used the allowance")
            assert bool((gap <= allow).all()) and used == 0, (V, T, form, tok, best, gap)


# ----------------------------------------------------------------------------------------------------------- attention
def _attention(hip, c, B, Pn, cap, t):
    """One decode-attention step with NaN in every generated row >= t, in the scratch and in o."""
    gk, gv = _dev(c, "gk", B).clone(), _dev(c, "gv", B).clone()
    gk[:, t:], gv[:, t:] = NAN, NAN
    scratch = hip.decode_attn_scratch(B, Pn, cap, DEV).fill_(NAN)
    o = torch.full((B, DNH * DHD), NAN, dtype=torch.bfloat16, device=DEV)
    hip.decode_attention(_state(hip, B, t, [Pn] * 8), _dev(c, "q", B), _dev(c, "pk", B).view(B * Pn, DHD), _dev(c, "pv", B).view(B * Pn, DHD),
                         _dev(c, "kinfo", B), Pn, gk, gv, o, scratch, DNH, 1, DHD)
    return o


@pytest.mark.parametrize("shape", C.ATTN_SHAPES, ids=lambda s: f"Pn{s[0]}cap{s[1]}")
@pytest.mark.parametrize("B", [1, 3, 8])
def test_attention(hip, B, shape):
    Pn, cap = shape
    for regime in C.ATTN_REGIMES:
        c = C.attn_case(Pn, cap, regime)
        assert int(c["allowed"][1].sum()) == 0 and bool((~c["allowed"][:, :32]).all()) == (Pn > 40)
        for t in sorted({1, 16, min(17, cap), cap}):
            o = _attention(hip, c, B, Pn, cap, t)
            r, A = _ref(c, ("ref", t), lambda: C.ref_attention(c["q"], c["pk"], c["pv"], c["allowed"], c["gk"], c["gv"], t))
            assert bool(torch.isfinite(o.float()).all())
            check_elementwise(o, r[:B], 2.0 ** -7 * A[:B], None, f"attention {regime} Pn {Pn} cap {cap} t {t} B {B}")


@pytest.mark.parametrize("shape", C.ATTN_SHAPES, ids=lambda s: f"Pn{s[0]}cap{s[1]}")
@pytest.mark.parametrize("B", [1, 3, 8])
def test_attention_exact_count(hip, B, shape):
    """q = 0 and v = +-1: o is the mean of the allowed keys' signs, so one key too many or too few moves it by ~ 1 / count."""
    Pn, cap = shape
    c = C.attn_case(Pn, cap, "count")
    asserted = total = pow2 = 0
    worst = 0.0
    # Pn 16: 8 allowed keys per sample (none for sample 1), so an odd t is an odd count and no sum is 0; 8 and 16 for the powers of two
    for t in range(1, cap + 1) if Pn > 40 else (1, 3, 5, 7, 8, 9, 11, 13, 15, 16):
        o = _attention(hip, c, B, Pn, cap, t).double().cpu().view(B, DNH, DHD)
        sm, n = C.count_reference(c, t)
        sm, n = sm[:B], n[:B].view(B, 1)
        ref = C.bf16r(sm / n)
        keep = C.count_separated(sm, n)
        is_pow2 = (torch.log2(n) % 1 == 0).expand_as(sm)
        err = (o - ref.view(B, 1, DHD)).abs()
        allow = torch.where(is_pow2, 0.0, C.ulp_bf16(ref)).view(B, 1, DHD)
        k = keep.view(B, 1, DHD).expand_as(err)
        assert bool((err[k] <= allow.expand_as(err)[k]).all()), (t, float(err[k].max()))
        worst = max(worst, float((err / C.ulp_bf16(ref).view(B, 1, DHD))[k].max()))
        asserted, total, pow2 = asserted + int(keep.sum()), total + keep.numel(), pow2 + int((is_pow2 & keep).sum())
    print(f"attention exact count Pn {Pn} cap {cap} B {B}: worst error {worst:.2f} spacings, {1 - asserted / total:.1%} of the elements "
          f"not asserted, {pow2} elements at a power-of-two count")
    assert 1 - asserted / total < 0.10 and pow2 > 0
