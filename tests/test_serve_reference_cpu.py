"""The criteria of tests/test_serve_reference_gpu.py against float32 restatements and corrupted references (CPU, no kernel involved),
and the float32 summation-order measurement behind its caps on the share of differing elements.

Corruptions and which criterion sees them:
 * one K slice of one wave dropped from a dot product: (a) rejects it at every element (the slices alternate in magnitude).
 * row 50, the first of the second sample, computed with the first sample's modulation row: (a).
 * one key dropped from the attention sum: (a) for a key of moderate weight; the exact case for any key.
 * a row >= M written: the arena's guard comparison.
 * one flipped bf16 rounding in one element: at the bit-exact targets (xn, v and h of the split-K consumers, CAP 0) it fails.  At
   the outputs that carry a bound, (a) allows one spacing per rounding point by its definition, so no single flip, at the last
   rounding point or at an earlier one carried through its gain, can exceed it (n = 1: error / bound ~ 0.99; n = 2: ~ 0.5); there
   it is what (b) counts, and flips at more than CAP of the elements fail.  Both are shown below.
 * one slab dropped from a split-K sum: every bit-exact target differs, q / k and act exceed their bounds.
 * one 32-deep k-step dropped from the row-panel GEMM: (a), in every epilogue and behind both prologues."""
import pytest
import torch

from tests import attention_reference as A
from tests import serve_reference as S
from tests.serve_reference import check_elementwise


def test_settled_modulation_keeps_h_off_rounding_ties():
    c = S.skinny_inputs()                    # (settle_mod raises if it does not converge)
    v, mag = S.h_argument(c["x"], c["mod"])
    assert bool(S.tie_clear(v, mag).all()) and float(S.tie_distance(v).min()) >= S.TIE_MARGIN
    assert torch.equal(S.bf16r(v), c["h16"]) and v.shape[0] == 144
    for M, _, shared in S.SKINNY_CASES:      # every case's rows are among the settled (row, modulation row) pairs
        rows = S.case_rows(M, shared)
        assert torch.equal(S.XROW[rows], torch.arange(M))
        assert torch.equal(S.MROW[rows], torch.zeros(M, dtype=torch.long) if shared else torch.arange(M) // S.RPS)
    g = torch.Generator().manual_seed(1)      # an unsettled draw is not clear: the settling does something
    v, mag = S.h_argument(c["x"], (torch.randn(3, 3 * S.D, generator=g) * 0.1).to(torch.bfloat16))
    assert not bool(S.tie_clear(v, mag).all())


@pytest.mark.parametrize("kind", S.KINDS)
def test_float32_restatements_meet_the_criteria(kind):
    """Every float32 order stays inside (a) and within a quarter of (b); the DIFFERING counts are reproduced."""
    r, bound = S.skinny_reference(kind)
    r, bound = r[:S.M_MAX], bound[:S.M_MAX]
    counts = []
    for o in S.kind_orders(kind):
        ratio, share = check_elementwise(S.f32_skinny(kind, o), r, bound, S.share_cap(kind) / 4.0, f"{kind} float32 {o}")
        counts.append(round(share * r.numel()))
    assert (tuple(counts), r.numel()) == S.DIFFERING[kind]
    assert bool(((r - r.to(torch.bfloat16).double()) == 0).all())          # R16 holds bf16 numbers


def test_final_step_references_are_consistent():
    c = S.skinny_inputs()
    for ad in S.ACTION_DIMS:
        (vt, dv), (xn, dx), (tok, dtok) = S.final_reference(ad)
        f = torch.float32
        v32 = c["h16"].to(f) @ c[f"wout{ad}"].T + c[f"bout{ad}"]
        assert S.worst_ratio(v32, vt, dv) <= 1.0
        x32 = c[f"xt{ad}"][S.XROW] + torch.tensor(S.DT) * v32
        assert S.worst_ratio(x32, xn, dx) <= 1.0
        t32 = (x32 @ c[f"win{ad}"].T + c[f"bin{ad}"]).to(torch.bfloat16)
        assert S.worst_ratio(t32, tok, dtok) <= 1.0
        bad = v32.clone()
        bad[3, ad - 1] = (c["h16"][3, :-8].to(f) @ c[f"wout{ad}"][ad - 1, :-8]) + c[f"bout{ad}"][ad - 1]      # one lane's 8 columns dropped
        assert S.worst_ratio(bad, vt, dv) > 1.0


@pytest.mark.parametrize("kind", ["res1024", "qkv"])
def test_dropped_k_slice_fails_the_element_bound(kind):
    r, bound = S.skinny_reference(kind)
    r, bound = r[:S.M_MAX], bound[:S.M_MAX]
    bad = S.f32_skinny(kind, "slices8", corrupt="slice")
    over = ((bad - r).abs() > bound).double().mean()
    print(f"{kind}: wave slice 5 dropped: {float(over):.3f} of the elements exceed their bound, worst ratio {S.worst_ratio(bad, r, bound):.0f}")
    assert float(over) > 0.9
    with pytest.raises(AssertionError):
        check_elementwise(bad, r, bound, S.share_cap(kind), f"{kind}, one K slice dropped")


@pytest.mark.parametrize("kind", ["qkv", "gate_up", "res1024g", "res4096g"])
def test_wrong_modulation_row_at_a_seam_fails_the_element_bound(kind):
    """Row 50 opens the second sample inside the tile of rows 48 .. 63; extended row 130 is row 50 under the first sample's row."""
    r, bound = S.skinny_reference(kind)
    bad = r[:S.M_MAX].clone()
    bad[50] = r[130]
    with pytest.raises(AssertionError):
        check_elementwise(bad, r[:S.M_MAX], bound[:S.M_MAX], S.share_cap(kind), f"{kind}, row 50 with sample 0's modulation")


def test_one_flipped_rounding_is_counted_by_the_share_cap():
    r, bound = S.skinny_reference("res1024")
    r, bound = r[:S.M_MAX], bound[:S.M_MAX]
    bad = r.clone()
    bad[7, 77] += S.ulp_bf16(r[7, 77])
    ratio, share = check_elementwise(bad, r, bound, None, "res1024, one rounding flipped")
    assert 0.45 < ratio <= 0.5 and share == 1.0 / r.numel()              # (two rounding points: the flip of one is half the bound)
    with pytest.raises(AssertionError):
        check_elementwise(bad, r, bound, 0.0, "a bit-exact target")
    n = int(S.share_cap("res1024") * r.numel()) + 1
    bad = r.clone()
    bad.view(-1)[:n] += S.ulp_bf16(r.view(-1)[:n])
    with pytest.raises(AssertionError):
        check_elementwise(bad, r, bound, S.share_cap("res1024"), "res1024, flips at more than CAP of the elements")
    bad = r.clone()
    bad[7, 77] += bound[7, 77] + S.ulp_bf16(r[7, 77])                  # one spacing more than the rounding points allow
    with pytest.raises(AssertionError):
        check_elementwise(bad, r, bound, None, "res1024, one spacing beyond the bound")


def test_stale_row_past_m_fails_the_guard():
    arena, regs = S.build_arena([("q", 50, 2048, 2048), ("xt", 50, 14, 14), ("o", 50, 256, 320)], fill={"xt": S.f32_bits(torch.ones(50, 7))})
    after = arena.clone()
    S.region_view(after, regs["q"]).fill_(1.0)              # the kernel's own rows
    S.f32_window(after, regs["xt"]).fill_(2.0)
    S.region_view(after, regs["o"]).fill_(3.0)
    assert S.untouched(arena, after, regs, tuple(regs))
    for name, off in (("q", 50 * 2048 + 5), ("xt", 50 * 14), ("o", 50 * 320), ("o", 256), ("q", -1)):     # row M, the stride gap, the row before
        bad = after.clone()
        bad[regs[name].off + off] = 1.0
        assert not S.untouched(arena, bad, regs, tuple(regs)), (name, off)
    assert float(S.f32_window(arena, regs["xt"])[49, 6]) == 1.0


# ------------------------------------------------------------------------------------------------------- attention
def test_attention_float32_restatements_meet_the_bound():
    for idx in range(len(S.ATTN_SHAPES)):
        c, ref = S.attn_case(idx), S.attn_reference(idx)
        for order in A.F32_ORDERS:
            o, _ = A.f32_forward(c["q"], c["k"], c["v"], c["allowed"], S.ATTN_SCALE, order)
            assert S.worst_ratio(o, ref["o16"], ref["o_bound"]) <= 1.0, (idx, order)
        if idx in S.ATTN_FULLY_MASKED:
            b = S.ATTN_FULLY_MASKED[idx]
            assert bool(ref["empty"][b].all()) and bool((ref["o16"][b] == 0).all()) and bool((ref["o_bound"][b] < 2.0 ** -100).all())
        assert bool((~c["allowed"][:, :, 3]).all())                       # the hole at key 3


def test_dropped_key_fails_the_attention_criteria():
    idx = 3
    c, ref = S.attn_case(idx), S.attn_reference(idx)
    b, i, h = 0, 5, 1
    p = ref["p"][b, h, i]
    j = int((p - 0.02).abs().argmin())                # a key of moderate weight
    allowed = c["allowed"].clone()
    allowed[b, i, j] = False
    bad = A.fwd_reference(c["q"], c["k"], c["v"], allowed, S.ATTN_SCALE, split=True)["o16"]
    print(f"key {j} (weight {float(p[j]):.3f}) dropped for query {i}: worst error / bound {S.worst_ratio(bad, ref['o16'], ref['o_bound']):.1f}")
    with pytest.raises(AssertionError):
        check_elementwise(bad, ref["o16"], ref["o_bound"], None, "attention, one key dropped")
    for idx in S.ATTN_COUNT:                          # the exact case sees any key, whatever its weight would be
        c = S.attn_case(idx, "count")
        want, keep, allow, live = S.attn_count_check(c)
        sm, n = S.attn_count(c)
        b, i = 0, 0
        j = int(c["allowed"][b, i].float().argmax())
        v = c["v"].double().repeat_interleave(c["shape"][1] // c["shape"][2], dim=2)[b, j]
        lost = S.bf16r((sm[b, i] - v) / (n[b, i] - 1).clamp(min=1.0))
        k = keep[b, i]
        assert int(k.sum()) > 0 and bool(((lost - want[b, i]).abs() > allow[b, i].expand_as(lost))[k].all())


def test_exact_case_share_not_asserted():
    for idx in S.ATTN_COUNT:
        c = S.attn_case(idx, "count")
        want, keep, allow, live = S.attn_count_check(c)
        ref = S.attn_reference(idx, "count")
        some = live & (S.attn_count(c)[0] != 0)
        assert torch.equal(ref["o16"][some], want[some])
        share = 1.0 - float(keep[live].double().mean())
        print(f"attention {S.ATTN_SHAPES[idx]}: {share:.3f} of the exact-case elements are not asserted")
        assert share < 0.10


# ------------------------------------------------------------------------------------------------- split-K consumers
def _all_fused():
    for ks in S.FUSED_KS:
        for rows in S.FUSED_ROWS:
            yield "rope", "rope", S.fused_case("rope", ks, rows)
            yield "geglu", "geglu", S.fused_case("geglu", ks, rows)
            yield "resnorm", "resnorm", S.fused_case("resnorm", ks, rows, gated=True)
            for Dn in S.NORM_D:
                for norm in (1, 2):
                    yield "norm", f"norm{norm}", S.fused_case("norm", ks, rows, D=Dn, norm=norm, bias=ks % 2 == 0, resid=rows == 50)


def test_consumer_restatements_meet_the_criteria_and_counts():
    """The float32 restatement of every consumer case stays inside (a) and within a quarter of (b) scaled to the case; every h is
    reproduced bit for bit (the settled margin holds); the recorded counts are measured again."""
    for name in S.FUSED_MEASURED:
        assert S.measure_fused(name) == S.DIFFERING["fused_" + name], name
    for kind, name, c in _all_fused():
        got = S.f32_fused(kind, c)
        for n, out in got.items():
            r, bound = c["out"][n]
            if bound is None:
                assert torch.equal(out, r), (name, n)
            else:
                assert S.worst_ratio(out, r, bound) <= 1.0 and S.differing_share(out, r) <= S.fused_cap(name, n), (name, n)
        if kind == "resnorm":
            rows = c["x"].shape[0]
            v, mag = S.h_argument(c["out"]["xn"][0].to(torch.bfloat16), c["mod"], torch.arange(rows), torch.arange(rows) // S.FUSED_RPS)
            assert bool(S.tie_clear(v, mag).all())
        elif kind == "norm":
            xn = c["out"]["xn"][0]
            v, mag = S.ln_argument(xn, c["gamma"], c["beta"]) if "beta" in c else S.rms_argument(xn, c["gamma"])
            assert bool(S.tie_clear(v, mag).all())


def test_dropped_slab_and_flipped_rounding_fail_the_consumer_targets():
    ks, rows = 7, 37
    c = S.fused_case("norm", ks, rows, D=1152, norm=0, bias=True, resid=True)
    xn = c["out"]["xn"][0]
    bad = S.bf16r(S.slab_sum(c["part"][:-1], c["bias"], c["resid"]))             # the single-slab tail of sum8 left out
    assert float((bad != xn).double().mean()) > 0.9
    flip = xn.clone()
    flip[11, 500] += S.ulp_bf16(xn[11, 500])                                      # one flipped rounding in one element
    assert not torch.equal(flip, xn) and S.differing_share(flip, xn) > 0.0       # CAP 0: the GPU module asserts a share of 0
    rev = S.bf16r(S.slab_sum(c["part"].flip(0), c["bias"], c["resid"]))
    print(f"slabs summed in the reverse order: {int((rev != xn).sum())} of {xn.numel()} elements differ (the order is part of the contract)")
    for kind in ("rope", "geglu"):
        c = S.fused_case(kind, ks, rows)
        x = S.bf16r(S.slab_sum(c["part"][:-1]))
        if kind == "rope":
            (qk, _), _ = S.ref_rope_split(x, c["pos"], S.Q_SCALE)
            r = torch.cat([c["out"]["q"][0], c["out"]["k"][0]], 1)
            bound = torch.cat([c["out"]["q"][1], c["out"]["k"][1]], 1)
            bad = qk
        else:
            bad, _ = S.ref_geglu(x[:, :S.FUSED_H], x[:, S.FUSED_H:])
            r, bound = c["out"]["act"]
        with pytest.raises(AssertionError):
            check_elementwise(bad, r, bound, None, f"{kind}, one slab dropped")
    # a wrong modulation row at the seam (row 25 opens the second sample inside the wave group of rows 24 .. 27)
    c = S.fused_case("resnorm", ks, rows, gated=True)
    xn16 = c["out"]["xn"][0].to(torch.bfloat16)
    v, _ = S.h_argument(xn16, c["mod"], torch.arange(rows), torch.zeros(rows, dtype=torch.long))
    assert not torch.equal(S.bf16r(v)[25], c["out"]["h"][0][25])


def test_tokens_cap_counts_are_reproduced():
    for ad in S.ACTION_DIMS:
        assert S.measure_tokens(ad) == S.DIFFERING[f"tokens{ad}"]
        (_, _), (_, _), (tok, dtok) = S.final_reference(ad)
        for o in ("seq", "fma"):
            check_elementwise(S.f32_tokens(ad, o), tok[:S.M_MAX], dtok[:S.M_MAX], S.share_cap(f"tokens{ad}") / 4.0, f"tokens {ad} float32 {o}")


def test_unrounded_references_lie_within_the_rounding_points():
    """R16 against R64 (rounded=False) of the references this module adds: at most the spacings of their rounding points apart."""
    c = S.skinny_inputs()
    r16, bound = S.skinny_reference("res1024g")
    r64 = S.ref_proj_residual(c["a1024"][S.XROW], c["w1024"], c["res"][S.XROW].double(), S.gate_rows(c), S.skinny_depth(1024), rounded=False)
    assert bool(((r16 - r64).abs() <= bound).all())
    r16, bound = S.skinny_reference("embed7")
    r64 = S.ref_embed(c["xt7"][S.XROW], c["win7"], c["bin7"], rounded=False)
    assert bool(((r16 - r64).abs() <= S.ulp_bf16(r16)).all())


# ------------------------------------------------------------------------------------------------- row-panel GEMM
@pytest.mark.parametrize("kind", list(S.PANEL_KINDS))
def test_panel_restatements_meet_the_criteria(kind):
    c = S.panel_case(kind)
    r, bound = c["ref"]
    counts = []
    for o in S.panel_orders(kind):
        _, share = check_elementwise(S.f32_panel(kind, o), r, bound, S.share_cap("panel_" + kind) / 4.0, f"panel {kind} float32 {o}")
        counts.append(round(share * r.numel()))
    assert (tuple(counts), r.numel()) == S.DIFFERING["panel_" + kind]
    if c["norm"] == 2:
        assert bool(S.tie_clear(*S.ln_argument(c["x"].double(), c["gamma"], c["beta"])).all())
    elif c["norm"] == 1:
        assert bool(S.tie_clear(*S.rms_argument(c["x"].double(), c["gamma"])).all())
    bad = S.f32_panel(kind, "chain32", drop_step=1)                  # one 32-deep k-step left out
    assert float(((bad - r).abs() > bound).double().mean()) > (0.5 if kind in ("gelu", "exp2") else 0.9), kind
    with pytest.raises(AssertionError):
        check_elementwise(bad, r, bound, None, f"panel {kind}, one k-step dropped")


def test_exp2_gelu_bound_is_its_own():
    """The exp2 form's term is relative to |y|: far below the tanh form's 2^-23 |g| in the negative tail, and the float32
    restatement of the formula meets it there; a result with the tanh form's error would not."""
    g = S.bf16r(torch.linspace(-9.0, 9.0, 4001, dtype=torch.float64))
    y, b = S.gelu_sigmoid64(g), S.gelu_exp2_bound(g)
    x = g.float()
    y32 = (x * (1.0 / (1.0 + torch.exp2(x * (x * x * torch.tensor(S.C1) + torch.tensor(S.C0)))))).double()
    assert bool(((y32 - y).abs() <= b).all())
    tail = g < -4.0
    assert bool((b[tail] < 2.0 ** -8 * g[tail].abs() * 2.0 ** -23).all())
    assert bool((((y + g.abs() * 2.0 ** -23) - y).abs()[tail] > b[tail]).all())
    assert bool(((y - S.gelu_tanh64(g)).abs() <= 1e-12 + 1e-9 * y.abs())[g > -3.0].all())          # the two float64 forms agree where 1 + tanh does not cancel


def test_panel_partials_reference_adds_up():
    r, bound = S.panel_partials_reference(2)
    c = S.panel_case("plain")
    assert bool(((r.sum(0) - c["r64"]).abs() <= 1e-12 * (1.0 + c["r64"].abs())).all()) and bool((bound > 0).all())
