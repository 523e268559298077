"""The element-wise criteria of tests/test_train_reference_gpu.py on the CPU, no kernel involved: float32 restatements of each
kernel's arithmetic (two summation orders where there is a sum) must meet every bound on every case; single-fault corruptions of
the restatements must fail on at least one case; every backward reference must be the gradient of its forward (torch autograd in
float64 on the unrounded function); the float32 math functions must err no more than train_reference.F32_ERR records."""
import pytest
import torch

from tests import train_reference as T
from tests.common import rel


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    T.drop_caches()


def ratio(got, ref):
    """Worst error / bound of a restatement's outputs against a reference dict; bound None: equality."""
    worst = 0.0
    for n, (r, b) in ref.items():
        if n not in got:
            continue
        g = got[n].double()
        if b is None:
            worst = max(worst, 0.0 if torch.equal(g, r.double()) else float("inf"))
        else:
            worst = max(worst, T.worst_ratio(g, r, b.clamp(min=1e-300)))
    return worst


# ------------------------------------------------------------------------------------------------- the runs per family
def run_norm(order, fault=None, kinds=("rms", "ada", "ln"), small=False):
    worst = {}
    for kind in kinds:
        for spec in T.norm_specs(kind):
            if small and spec.D > 520:
                continue
            c = T.norm_case(spec)
            if kind == "ln":
                f = T.ref_ln_fwd(c)
                worst["ln_fwd"] = max(worst.get("ln_fwd", 0), ratio(T.f32_ln_fwd(c, order), f))
                mean32, rstd32 = f["mean"][0].float(), f["rstd"][0].float()
                for acc in T.accum_modes(spec.D):
                    got = T.f32_ln_bwd(c, mean32, rstd32, order, acc, fault)
                    ref = T.ref_ln_bwd(c, mean32, rstd32, acc)
                    ref["dxsum"] = T.ref_dxsum(got["dx"], c["dxsum0"], spec.rows)
                    worst["ln_bwd"] = max(worst.get("ln_bwd", 0), ratio(got, ref))
            else:
                f = T.ref_rms_fwd(c)
                worst[kind + "_fwd"] = max(worst.get(kind + "_fwd", 0), ratio(T.f32_rms_fwd(c, order, fault=fault), f))
                if kind == "ada" and fault is None:
                    worst["ada_fwd"] = max(worst["ada_fwd"], ratio(T.f32_rms_fwd(c, order, shared=True), T.ref_rms_fwd(c, shared=True)))
                rstd32 = f["rstd"][0].float()
                for acc in T.accum_modes(spec.D):
                    worst[kind + "_bwd"] = max(worst.get(kind + "_bwd", 0),
                                               ratio(T.f32_rms_bwd(c, rstd32, order, acc, fault), T.ref_rms_bwd(c, rstd32, acc)))
    return worst


def run_elementwise(order, fault=None):
    worst = {}
    for spec in T.ROPE_SMALL:
        c = T.rope_case(spec)
        worst["rope_fwd"] = max(worst.get("rope_fwd", 0), ratio(T.f32_rope_fwd(c, fault), T.ref_rope_fwd(c)))
        worst["rope_bwd"] = max(worst.get("rope_bwd", 0), ratio(T.f32_rope_bwd(c), T.ref_rope_bwd(c)))
    for H, rows in T.GEGLU_SHAPES:
        c = T.geglu_case(H, rows)
        worst["geglu_fwd"] = max(worst.get("geglu_fwd", 0), ratio(T.f32_geglu_fwd(c, fault), T.ref_geglu_fwd(c)))
        worst["geglu_bwd"] = max(worst.get("geglu_bwd", 0), ratio(T.f32_geglu_bwd(c), T.ref_geglu_bwd(c)))
        x, dy = c["gu"][:, :H], c["dact"]
        worst["gelu_fwd"] = max(worst.get("gelu_fwd", 0), ratio(dict(y=T._bf(T.gelu32(x.float()))), T.ref_gelu_fwd(x)))
        worst["gelu_bwd"] = max(worst.get("gelu_bwd", 0), ratio(dict(dx=T._bf(dy.float() * T.gelu_grad32(x.float()))), T.ref_gelu_bwd(x, dy)))
    for D in (8, 264):
        for rps in T.GATED_RPS:
            c = T.gated_case(D, rps)
            worst["gated_fwd"] = max(worst.get("gated_fwd", 0), ratio(T.f32_gated_fwd(c, True, fault), T.ref_gated_fwd(c)),
                                     ratio(T.f32_gated_fwd(c, False), T.ref_gated_fwd(c, False)))
            worst["gated_bwd"] = max(worst.get("gated_bwd", 0), ratio(T.f32_gated_bwd(c, order), T.ref_gated_bwd(c)))
        c = T.embed_case(D)
        worst["embed_scatter"] = max(worst.get("embed_scatter", 0), ratio(T.f32_embed_scatter(c, order), T.ref_embed_scatter(c)))
    for rows, cols in T.colsum_shapes():
        for dt in (torch.bfloat16, torch.float32):
            c = T.colsum_case(rows, cols, dt)
            worst["colsum"] = max(worst.get("colsum", 0), ratio(T.f32_colsum(c, order, fault), T.ref_colsum(c)))
    return worst


def run_loss(order, fault=None):
    worst = {}
    for name in ("main", "odd"):
        c = T.ce_case(name)
        ref = T.ref_ce_update(c)
        got = T.f32_ce_update(c, order, fault)
        worst["ce_update"] = max(worst.get("ce_update", 0), ratio({k: v for k, v in got.items() if k != "amax"}, ref))
        worst["ce_argmax"] = max(worst.get("ce_argmax", 0), 0.0 if torch.equal(got["amax"], ref["amax"][0]) else float("inf"))
        m32, l32 = ref["m"][0].float(), ref["l"][0].float()
        for v0, vc in c["chunks"]:
            worst["ce_grad"] = max(worst.get("ce_grad", 0), ratio(T.f32_ce_grad(c, m32, l32, v0, vc, fault), T.ref_ce_grad(c, m32, l32, v0, vc)))
    return worst


def run_optim(order, fault=None, big=True):
    worst = {}
    for sizes, dt in ((T.SUMSQ_F32, torch.float32), (T.SUMSQ_BF16, torch.bfloat16)):
        for n in sizes if big else sizes[:-1]:
            c = T.sumsq_case(n, dt)
            worst["sumsq"] = max(worst.get("sumsq", 0), ratio(T.f32_sumsq(c, order, fault), T.ref_sumsq(c)))
    for n in T.ADAM_N:
        for clip, ema, gd in (("clipped", "on", torch.float32), ("below", "flag0", torch.float32), ("off", "none", torch.bfloat16)):
            c = T.adam_case(n, clip, ema, gd)
            got = T.f32_adamw(c, fault)
            ref = T.ref_adamw(c)
            if ema != "on":
                ref["ema"] = (c["ema"].double(), None)          # untouched
            hi, lo = T.p16_planes(got["p"])
            ref["p16"], ref["p16lo"] = (hi, None), (lo, None)
            worst["adamw"] = max(worst.get("adamw", 0), ratio(got, ref))
    return worst


FAMILIES = dict(norm=run_norm, elementwise=run_elementwise, loss=run_loss, optim=run_optim)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_float32_restatements_meet_every_bound(family):
    for order in T.ORDERS:
        for what, r in sorted(FAMILIES[family](order).items()):
            print(f"float32 {order} {what}: worst error / bound {r:.3f}")
            assert r <= 1.0, (order, what, r)


def test_token_metrics_and_argmax_references():
    """The exact references against a vectorised restatement (counts) and a flipped tie-break (argmax)."""
    for Lm in T.METRIC_LM:
        for with_sel in (False, True):
            c = T.metrics_case(Lm, with_sel)
            ptl, counts = T.ref_token_metrics(c)
            assert float(counts[:, 0, 1].sum()) == float((c["lm"] != 0).sum())
            assert bool((counts[:, :, 0] <= counts[:, :, 1]).all()) and bool((counts[:, 3] == 0).all())
            if with_sel:
                bad = T.ref_token_metrics(c, "count_skipped_rows")
                assert not (torch.equal(bad[0], ptl) and torch.equal(bad[1], counts)), Lm
    caught = False
    for n in T.ARGMAX_N:
        x = T.argmax_case(n)
        lo = T.first_argmax(x)
        assert int(lo[4]) == 0 and int(lo[5]) == n - 1
        hi = (n - 1 - T.first_argmax(x.flip(1))).to(torch.int32)
        caught |= not torch.equal(lo[:4], hi[:4])
    assert caught


# fault -> (family run, result keys that must exceed their bound on at least one case)
CORRUPTIONS = {
    "drop_row": ("norm", ("rms_bwd", "ada_bwd")),                       # one row missing from a column gradient
    "drop_chunk": ("norm", ("rms_bwd",)),                                # one 8-wide chunk missing from the row's dot product
    "skip_w_rounding": ("norm", ("ada_fwd",)),                           # bf16(1 + scale) not rounded
    "skip_product_rounding": ("elementwise", ("gated_fwd",)),            # bf16(u * gate) not rounded
    "dxsum_unrounded": ("norm", ("ln_bwd",)),                            # dxsum over the unrounded dx
    "skip_hi_rounding": ("optim", ("adamw",)),                           # p16lo = bf16(p - p)
    "neighbour_group": ("norm", ("ada_fwd",)),                           # the modulation row of the neighbouring block
    "scale_for_shift": ("norm", ("ada_fwd",)),                           # the scale third where the shift third belongs
    "no_accum_chunk": ("norm", ("rms_bwd",)),                            # accum_dx add omitted for one chunk
    "tie_high": ("loss", ("ce_argmax",)),                                # argmax ties to the higher index
    "later_chunk_takes_tie": ("loss", ("ce_argmax",)),                   # a later CE chunk takes an equal maximum
    "target_not_subtracted": ("loss", ("ce_grad",)),                     # the one-hot term missing
    "no_bias_correction": ("optim", ("adamw",)),
    "clip_below": ("optim", ("adamw",)),                                 # clips although gnorm < max_norm
    "ema_ignores_flag": ("optim", ("adamw",)),                           # writes the EMA although sc[5] == 0
    "drop_tail": ("optim", ("sumsq",)),
}


@pytest.mark.parametrize("fault", list(CORRUPTIONS))
def test_single_fault_corruptions_fail(fault):
    family, keys = CORRUPTIONS[fault]
    kw = dict(small=True) if family == "norm" and fault != "no_accum_chunk" else dict(big=False) if family == "optim" else {}
    worst = FAMILIES[family]("tree", fault, **kw)
    for k in keys:
        print(f"{fault}: {k} worst error / bound {worst[k]:.2f}")
        assert worst[k] > 1.0, (fault, k, worst[k])


@pytest.mark.parametrize("fault,key", [("skip_gelu_rounding", "geglu_fwd"), ("skip_rot_rounding", "rope_fwd")])
def test_double_rounding_slack_is_reported(fault, key):
    """Two skipped roundings the element bounds cannot see: where one bf16 rounding feeds a product that is rounded to bf16 again,
    skipping the inner one moves the result by at most half a spacing, and the bound after two rounding points is one spacing
    more than the float32 error.  Printed for docs/EXPERIMENTS.md; the other four skipped roundings above are caught."""
    worst = run_elementwise("tree", fault)[key]
    print(f"{fault}: {key} worst error / bound {worst:.2f} (not caught)")
    assert worst <= 1.0


def test_math_function_errors():
    """Worst error of torch's float32 exp / log / tanh / sin / cos / pow / sqrt / reciprocal against float64 over the arguments
    every restatement above produces: no larger than the recorded constants, and the device's allowance (4 x, capped) stays under
    2^-18."""
    for order in T.ORDERS:
        run_elementwise(order), run_loss(order), run_optim(order, big=False)
    seen = T.errors_seen()
    for k, v in sorted(seen.items()):
        print(f"float32 {k}: worst error {v:.3e} (recorded {T.F32_ERR[k]:.3e})")
        assert 0 < v <= T.F32_ERR[k], (k, v)
    assert max(T.E_EXP, T.E_LOG, T.E_TANH, T.E_SIN, T.E_POW, T.E_SQRT, T.E_RCP) <= 2.0 ** -18


# --------------------------------------------------------------------------------------------------------- autograd
def _close(ref, grad, roundings, what):
    r = rel(ref, grad)
    print(f"{what}: reference against autograd, rel {r:.2e}")
    assert r < roundings * 2.0 ** -9, (what, r)


def test_backward_references_agree_with_autograd():
    """Each backward reference against torch autograd in float64 on the unrounded forward, up to its bf16 rounding points
    (2^-9 relative each): a check of the references themselves, so a norm is the instrument."""
    for spec in (T.NormCase("rms", 520, 67), T.NormCase("ada", 264 * 2, 15, 3, 5, 8)):
        c = T.norm_case(spec)
        x = c["x"].double().requires_grad_(True)
        par = (c["mod"] if spec.kind == "ada" else c["scale"]).double().requires_grad_(True)
        r = (x.pow(2).mean(1, keepdim=True) + T.f32c(1e-6)).rsqrt()
        if spec.kind == "ada":
            idx = torch.arange(spec.rows) // spec.rps
            y = x * r * (1.0 + par[:, :spec.D])[idx] + par[:, spec.D:2 * spec.D][idx]
        else:
            y = x * r * (1.0 + par)
        assert rel(y.detach(), T.ref_rms_fwd(c, rounded=False)) < 1e-12
        (y * c["dy"].double()).sum().backward()
        ref = T.ref_rms_bwd(c, r.detach().float()[:, 0])
        _close(ref["dx"][0], x.grad, 2, f"{spec.kind} dx")
        if spec.kind == "ada":
            _close(ref["dmod"][0] - c["dmod0"].double(), par.grad, 2, "dmod")
            assert torch.equal(ref["dmod"][0][:, 2 * spec.D:], c["dmod0"].double()[:, 2 * spec.D:])
        else:
            _close(ref["dscale"][0] - c["dscale0"].double(), par.grad, 1, "dscale")
    c = T.norm_case(T.NormCase("ln", 520, 35))
    x, gm, bt = (c[n].double().requires_grad_(True) for n in ("x", "gamma", "beta"))
    y = torch.nn.functional.layer_norm(x, (520,), gm, bt, T.f32c(1e-6))
    assert rel(y.detach(), T.ref_ln_fwd(c, rounded=False)) < 1e-9
    (y * c["dy"].double()).sum().backward()
    f = T.ref_ln_fwd(c)
    ref = T.ref_ln_bwd(c, f["mean"][0].float(), f["rstd"][0].float())
    _close(ref["dx"][0][2:], x.grad[2:], 2, "ln dx")          # rows 0 and 1 cancel: the float32 statistics move them by more
    _close(ref["dgamma"][0] - c["dgamma0"].double(), gm.grad, 1, "dgamma")
    _close(ref["dbeta"][0] - c["dbeta0"].double(), bt.grad, 1, "dbeta")

    c = T.rope_case(T.ROPE_SMALL[2])
    s = c["spec"]
    rows, half = s.B * s.T_seg, s.HD // 2
    qkv = c["qkv"].double().requires_grad_(True)
    sn, cs, _ = T._rope_trig(c, torch.float64)
    x = qkv.view(rows, s.NH + 2, s.HD)
    x1, x2 = x[:, :s.NH + 1, :half], x[:, :s.NH + 1, half:]
    rot = torch.cat([x1 * cs - x2 * sn, x2 * cs + x1 * sn], -1)
    q, k, v = (rot[:, :s.NH] * T.f32c(s.q_scale)).reshape(rows, -1), rot[:, s.NH], x[:, s.NH + 1]
    for a, b in zip((q, k, v), T.ref_rope_fwd(c, rounded=False)):
        assert rel(a.detach(), b) < 1e-12
    ((q * c["dq"].double()).sum() + (k * c["dk"].double()).sum() + (v * c["dv"].double()).sum()).backward()
    _close(T.ref_rope_bwd(c)["dqkv"][0], qkv.grad, 1, "rope dqkv")

    c = T.geglu_case(264, 8)
    gu = c["gu"].double().requires_grad_(True)
    act = T.gelu64(gu[:, :264]) * gu[:, 264:]
    assert rel(act.detach(), T.ref_geglu_fwd(c, rounded=False)) < 1e-12
    (act * c["dact"].double()).sum().backward()
    _close(T.ref_geglu_bwd(c)["dgu"][0], gu.grad, 2, "geglu dgu")
    x = c["gu"][:, :264].double().requires_grad_(True)
    (T.gelu64(x) * c["dact"].double()).sum().backward()
    _close(T.ref_gelu_bwd(c["gu"][:, :264], c["dact"])["dx"][0], x.grad, 1, "gelu dx")

    c = T.gated_case(264, 9)
    u, gt = c["u"].double().requires_grad_(True), c["gate"].double().requires_grad_(True)
    y = c["x"].double() + u * gt.repeat_interleave(9, 0)
    (y * c["dy"].double()).sum().backward()
    ref = T.ref_gated_bwd(c)
    _close(ref["du"][0], u.grad, 1, "gated du")
    _close(ref["dgate"][0], gt.grad, 1, "dgate")

    c = T.ce_case("main")
    st = T.ref_ce_update(c)
    x = c["logits"].double().requires_grad_(True)
    tgt = c["target"].long().clamp(0, c["V"] - 1)
    inside = (c["target"] >= 0) & (c["target"] < c["V"])
    nll = torch.logsumexp(x, 1) - torch.where(inside, x[torch.arange(c["R"]), tgt], torch.zeros(c["R"], dtype=torch.float64))
    (nll * c["w"].double()).sum().backward()
    full = torch.cat([T.ref_ce_grad(c, st["m"][0].float(), st["l"][0].float(), v0, vc)["sum"][0] for v0, vc in c["chunks"]], 1)
    _close(full, x.grad.nan_to_num(), 1, "ce dlogits")

    c = T.embed_case(8)
    dt = torch.zeros(6, 8, dtype=torch.float64, requires_grad=True)
    out = dt[c["stok"].long()] * T.f32c(c["scale"])
    (out * c["dout"].double()[T.embed_src_rows(c)]).sum().backward()
    _close(T.ref_embed_scatter(c)["dtable"][0] - c["dtable0"].double(), dt.grad, 1, "embed dtable")


def test_arena_guards_and_windows():
    """untouched() sees one changed byte in a guard, in a padding column and behind the last row, and ignores the owned windows."""
    a = T.Arena()
    a.add("x", torch.bfloat16, 3, 8, rs=16, data=torch.ones(3, 8)).add("y", torch.float32, 2, 5, rs=7, out=True, shift=1)
    arena, reg = a.build()
    assert all(r.off % 4 == 0 for r in reg.values()) and reg["x"].off % 16 == 0
    assert bool(torch.isnan(T.view(arena, T.sub(reg["x"], col0=8, width=8, rows=2))).all())
    after = arena.clone()
    T.view(after, reg["y"]).fill_(1.0)
    assert T.untouched(arena, after, reg, ["y"]) and not T.untouched(arena, after, reg, [])
    for off in (reg["y"].off - 1, reg["y"].off + 5 * 4, reg["y"].off + (7 + 5) * 4, reg["x"].off + 16):
        bad = after.clone()
        bad[off] ^= 1
        assert not T.untouched(arena, bad, reg, ["y"]), off
    assert T.untouched(arena, after, reg, [], [T.sub(reg["y"], 0, 2, 0, 5)])
