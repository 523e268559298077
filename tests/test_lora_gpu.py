"""LoRA Gemma variants on the GPU: the low-rank kernels of csrc/lora.hip against torch f32 restatements, and the model (loss, every
gradient, a frozen train step, the merged-weight sampler) against the f32 oracle run on the MERGED parameter tree.

[UPSTREAM-RECALL] lora.Einsum: y = einsum(x, w) + einsum(einsum(x, lora_a), lora_b) * (alpha / rank), each einsum a bf16 tensor;
lora.FeedForward: _dot(x, w, (a, b)) = x w + (x a) b (no scaling), the gate / up terms before the GELU.  In f32 the merged tree
W + s * merge(A, B) is exactly that function, and the gradients of leaf A / B through it are the reference's adapter gradients.

Kernel tolerances: every kernel sums in f32 in a fixed order (bitwise repeatable, checked) but not in torch's order, so results are
compared with the torch restatement to one bf16 ulp of the result at the stated rounding points (plus an f32 summation term)."""
import collections
import dataclasses

import pytest
import torch

from oracle import lap_oracle as O
from tests.common import debug_model_cfg, make_inputs, oracle_cfg, rel, to_observation

pytestmark = pytest.mark.gpu
DEV = "cuda"
LAY = "PaliGemma/llm/layers"


def _bf(t):
    return t.to(torch.bfloat16).float()


def _close_ulp(got, ref, mag, what, inner=None):
    """|got - ref| <= one bf16 ulp of |ref| (2^-7 relative: the rounding may fall either side) + 2^-16 of the absolute-sum bound;
    `inner`: a bf16-rounded product added before the final rounding may itself sit one ulp (of |inner|) away."""
    got, ref = got.float(), ref.float()
    tol = ref.abs() * 2.0 ** -7 + mag * 2.0 ** -16 + 1e-30
    if inner is not None:
        tol = tol + inner.abs() * 2.0 ** -7
    bad = (got - ref).abs() > tol
    assert not bool(bad.any()), (what, int(bad.sum()), float((got - ref).abs().max()))


# ------------------------------------------------------------------------------------------------------------------ kernels
# (K, r, G) of the down products at the bench shapes: q|k|v (G = 10 heads), out (one group, 8 copies of B), gate|up (2), down
_PROD = [  # name, K (input width), Ng (output per group), G, r, nsum
    ("vlm_qkv", 2048, 256, 10, 16, 1), ("vlm_o", 2048, 2048, 1, 16, 8), ("vlm_gu", 2048, 16384, 2, 16, 1), ("vlm_d", 16384, 2048, 1, 16, 1),
    ("exp_qkv", 1024, 256, 10, 32, 1), ("exp_o", 2048, 1024, 1, 32, 8), ("exp_gu", 1024, 4096, 2, 32, 1), ("exp_d", 4096, 1024, 1, 32, 1),
]


def _operands(M, K, Ng, G, r, nsum, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, device=DEV)
    x = rnd(M, K).bfloat16()
    A = (rnd(G * r, K) * 0.05).bfloat16()
    Bm = (rnd(nsum * G * r, Ng) * 0.05).bfloat16()
    y = rnd(M, G * Ng).bfloat16()
    return x, A, Bm, y


def _bsum(Bm, G, r, nsum):
    return Bm.float().view(nsum, G * r, -1).sum(0)


@pytest.mark.parametrize("case", _PROD, ids=[c[0] for c in _PROD])
@pytest.mark.parametrize("M,s", [(1600, 1.0), (333, 2.0)])
def test_lora_kernels_match_torch(hip, case, M, s):
    from lap_amd import hip as H

    name, K, Ng, G, r, nsum = case
    x, A, Bm, y = _operands(M, K, Ng, G, r, nsum, seed=M + K + Ng)
    # down: t = bf16(x A^T)
    t = H.lora_down(x, A)
    ref_t = x.float() @ A.float().t()
    _close_ulp(t, ref_t, (x.float().abs() @ A.float().abs().t()), f"{name} down")
    assert torch.equal(t, H.lora_down(x, A))
    # up-add: y <- bf16(y + bf16(s bf16(t_g B_g)))  (B summed over its nsum copies)
    Bs = _bsum(Bm, G, r, nsum)
    prod = torch.cat([t[:, gi * r:(gi + 1) * r].float() @ Bs[gi * r:(gi + 1) * r] for gi in range(G)], 1)
    p = _bf(_bf(prod) * s)
    ref_y = y.float() + p
    y1 = y.clone()
    H.lora_up_add(y1, t, Bm, G=G, nsum=nsum, s=s)
    _close_ulp(y1, ref_y, y.float().abs() + p.abs(), f"{name} up-add", inner=p)
    y2 = y.clone()
    H.lora_up_add(y2, t, Bm, G=G, nsum=nsum, s=s)
    assert torch.equal(y1, y2)
    # dgrad-down: dt = bf16(bf16(s dy) B^T) per group
    dy = y
    dys = _bf(dy.float() * s)
    dt = H.lora_down(dy, Bm, G=G, nsum=nsum, xg=Ng if G > 1 else 0, s=s)
    ref_dt = torch.cat([dys[:, gi * Ng:(gi + 1) * Ng] @ Bs[gi * r:(gi + 1) * r].t() for gi in range(G)], 1)
    mag = torch.cat([dys[:, gi * Ng:(gi + 1) * Ng].abs() @ Bs[gi * r:(gi + 1) * r].abs().t() for gi in range(G)], 1)
    _close_ulp(dt, ref_dt, mag, f"{name} dgrad-down")
    # dx add: dx <- bf16(dx + bf16(dt A))
    dx = x.clone()
    H.lora_up_add(dx, dt, A)
    q = _bf(dt.float() @ A.float())
    _close_ulp(dx, x.float() + q, x.float().abs() + q.abs(), f"{name} dx-add", inner=q)
    # rank-r weight gradients into bf16 and f32 buffers: dA = dt^T x, dB = t^T bf16(s dy), every copy of B gets dB
    for dt_out in (torch.bfloat16, torch.float32):
        dA = torch.full((G * r, K), float("nan"), dtype=dt_out, device=DEV)
        H.lora_wgrad(dt, x, dA)
        _close_ulp(dA, dt.float().t() @ x.float(), dt.float().abs().t() @ x.float().abs(), f"{name} dA")
        dB = torch.full((nsum * G * r, Ng), float("nan"), dtype=dt_out, device=DEV)
        H.lora_wgrad(t, dy, dB, G=G, bg=Ng if G > 1 else 0, ncopy=nsum, s=s)
        ref_dB = torch.cat([t[:, gi * r:(gi + 1) * r].float().t() @ dys[:, gi * Ng:(gi + 1) * Ng] for gi in range(G)], 0)
        mag = torch.cat([t[:, gi * r:(gi + 1) * r].float().abs().t() @ dys[:, gi * Ng:(gi + 1) * Ng].abs() for gi in range(G)], 0)
        for n in range(nsum):
            _close_ulp(dB[n * G * r:(n + 1) * G * r], ref_dB, mag, f"{name} dB copy {n}")
        dB1 = torch.empty_like(dB)
        H.lora_wgrad(t, dy, dB1, G=G, bg=Ng if G > 1 else 0, ncopy=nsum, s=s, msplit=1)   # unsplit: same sums, another order
        _close_ulp(dB1, dB, mag.repeat(nsum, 1), f"{name} dB unsplit")
        dB2 = torch.empty_like(dB)
        H.lora_wgrad(t, dy, dB2, G=G, bg=Ng if G > 1 else 0, ncopy=nsum, s=s)
        assert torch.equal(dB, dB2)


@pytest.mark.parametrize("case", [_PROD[0], _PROD[1], _PROD[2], _PROD[7]], ids=["vlm_qkv", "vlm_o", "vlm_gu", "exp_d"])
def test_lora_merge_matches_torch(hip, case):
    from lap_amd import hip as H

    _, K, Ng, G, r, nsum = case
    g = torch.Generator(device=DEV).manual_seed(9)
    W = torch.randn(G * Ng, K, generator=g, device=DEV) * 0.02
    A = torch.randn(G * r, K, generator=g, device=DEV) * 0.05
    Bm = torch.randn(nsum * G * r, Ng, generator=g, device=DEV) * 0.05
    out = torch.empty(G * Ng, K, dtype=torch.bfloat16, device=DEV)
    H.lora_merge(W, A, Bm, out, G=G, nsum=nsum, s=2.0)
    Bs = Bm.view(nsum, G * r, Ng).sum(0)
    delta = torch.cat([Bs[gi * r:(gi + 1) * r].t() @ A[gi * r:(gi + 1) * r] for gi in range(G)], 0)
    _close_ulp(out, W + 2.0 * delta, W.abs() + 2.0 * delta.abs(), "merge")


def test_lora_launchers_reject_bad_shapes(hip):
    from lap_amd import hip as H

    x = torch.zeros(64, 72, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(H.LapHipError):
        H.lora_down(x, torch.zeros(24, 72, dtype=torch.bfloat16, device=DEV))      # rank 24: not a multiple of 16
    with pytest.raises(H.LapHipError):
        H.lora_down(torch.zeros(64, 70, dtype=torch.bfloat16, device=DEV), torch.zeros(16, 70, dtype=torch.bfloat16, device=DEV))


# ------------------------------------------------------------------------------------------------------------------ model
def _lora_cfg(vlm="dummy_lora", expert="dummy_lora", **kw):
    return debug_model_cfg(paligemma_variant=vlm, action_expert_variant=expert, **kw)


def _base_name(v):
    return v.replace("_lora", "")


def _adapters(cfg, seed, std=0.05):
    from lap_amd.params import reference_shapes

    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(s, generator=g) * std for k, s in reference_shapes(cfg).items() if "lora" in k}


def _merged_tree(cfg, P, LA):
    """The reference tree with every LoRA'd weight replaced by W + s * merge(A, B), an autograd expression of the leaves."""
    from lap_amd.config import get_gemma_config

    M = dict(P)
    for sfx, var in (("", cfg.paligemma_variant), ("_1", cfg.action_expert_variant)):
        c = get_gemma_config(var)
        if c.lora_attn is not None:
            s = c.lora_attn[1] / c.lora_attn[0]
            a = lambda n: LA[f"{LAY}/attn/{n}{sfx}/lora_a"]
            b = lambda n: LA[f"{LAY}/attn/{n}{sfx}/lora_b"]
            M[f"{LAY}/attn/q_einsum{sfx}/w"] = P[f"{LAY}/attn/q_einsum{sfx}/w"] + s * torch.einsum("lndr,lnrh->lndh", a("q_einsum"), b("q_einsum"))
            M[f"{LAY}/attn/kv_einsum{sfx}/w"] = P[f"{LAY}/attn/kv_einsum{sfx}/w"] + s * torch.einsum("lckdr,lckrh->lckdh", a("kv_einsum"), b("kv_einsum"))
            M[f"{LAY}/attn/attn_vec_einsum{sfx}/w"] = P[f"{LAY}/attn/attn_vec_einsum{sfx}/w"] + s * torch.einsum(
                "lnhr,lrd->lnhd", a("attn_vec_einsum"), b("attn_vec_einsum").sum(1))       # N summed out of lora_b
        if c.lora_ffn is not None:     # lora.FeedForward: no scaling
            M[f"{LAY}/mlp{sfx}/gating_einsum"] = P[f"{LAY}/mlp{sfx}/gating_einsum"] + torch.einsum(
                "lcdr,lcrf->lcdf", LA[f"{LAY}/mlp{sfx}/gating_einsum_lora_a"], LA[f"{LAY}/mlp{sfx}/gating_einsum_lora_b"])
            M[f"{LAY}/mlp{sfx}/linear"] = P[f"{LAY}/mlp{sfx}/linear"] + torch.einsum(
                "lfr,lrd->lfd", LA[f"{LAY}/mlp{sfx}/linear_lora_a"], LA[f"{LAY}/mlp{sfx}/linear_lora_b"])
    return M


def _oracle_cfg(cfg, **kw):
    return oracle_cfg(dataclasses.replace(cfg, paligemma_variant=_base_name(cfg.paligemma_variant),
                                          action_expert_variant=_base_name(cfg.action_expert_variant)), **kw)


@pytest.mark.parametrize("vlm,expert,pi05", [("dummy_lora", "dummy_lora", True), ("dummy_lora", "dummy", True), ("dummy", "dummy_lora", True),
                                              ("dummy_lora", "dummy_lora", False)])
def test_lora_loss_and_every_gradient_match_the_merged_oracle(hip, vlm, expert, pi05):
    """Debug model, B = 2, ragged inputs, base weights trainable: the loss and every gradient (base weights and adapters, mapped back to
    the reference tree) against the f32 oracle on the merged tree; pi05=False: the pi0 suffix (plain norms, fused residuals)."""
    from lap_amd.model import LAP
    from lap_amd.params import engine_to_reference

    cfg = _lora_cfg(vlm, expert, **({} if pi05 else dict(pi05=False, discrete_state_input=False)))
    oc = _oracle_cfg(cfg)
    P = O.init_params(oc, seed=7)
    LA = _adapters(cfg, seed=8)
    obs, actions, noise, time = make_inputs(cfg, B=2, ragged=True)
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    LAg = {k: v.clone().requires_grad_(True) for k, v in LA.items()}
    loss32, _ = O.compute_loss(_merged_tree(cfg, Pg, LAg), oc, obs, actions, noise, time)
    loss32.backward()
    with torch.no_grad():
        loss16, _ = O.compute_loss(_merged_tree(cfg, P, LA), dataclasses.replace(oc, emulate_bf16=True), obs, actions, noise, time)
    model = LAP(cfg, params=P | LA, device=DEV)
    for g in model.ps.grad.values():
        g.zero_()
    loss, _ = model.loss_and_grad(0, to_observation(obs, DEV), actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV))
    torch.cuda.synchronize()
    ref_noise = abs(loss16.item() - loss32.item()) / abs(loss32.item())
    assert abs(loss.item() - loss32.item()) / abs(loss32.item()) < max(3 * ref_noise, 5e-3), (loss.item(), loss32.item())
    gref = engine_to_reference(cfg, {n: model.ps.g(n).detach().float().cpu() for n in model.ps.names()})
    checked = 0
    for k, leaf in list(Pg.items()) + list(LAg.items()):
        if leaf.grad is None:
            continue
        r = rel(gref[k], leaf.grad)
        # (SigLIP's key bias has an analytically zero gradient — softmax is shift invariant — so it is compared absolutely)
        tol_abs = 1e-3 if k.endswith("key/bias") else 1e-4
        assert r < 5e-2 or (gref[k] - leaf.grad).abs().max() < tol_abs, (k, r)
        checked += 1
    assert checked == len(P) + len(LA) and len(LA) == 10 * (("lora" in vlm) + ("lora" in expert))


def test_lora_train_step_with_the_reference_freeze_filter(hip):
    """One train step under LAPConfig.get_freeze_filter(): frozen base weights bitwise unchanged, every adapter, SigLIP and action-head
    array moves, the gradient norm is the oracle's over the trainable set, and the prefix backward runs (its adapters are trainable)."""
    from lap_amd.config import get_config
    from lap_amd.train import TrainingStepRunner, init_train_state

    tc = get_config("debug")
    cfg = dataclasses.replace(tc.model, paligemma_variant="dummy_lora", action_expert_variant="dummy_lora")
    tc = dataclasses.replace(tc, model=cfg)
    oc = _oracle_cfg(cfg)
    frz = cfg.get_freeze_filter()
    P = O.init_params(oc, seed=5)
    P = {k: (v.to(torch.bfloat16).float() if frz(k) else v) for k, v in P.items()}
    LA = _adapters(cfg, seed=6)
    obs, actions, noise, time = make_inputs(cfg, B=2, ragged=True)
    tcf = dataclasses.replace(tc, freeze_filter=frz)
    state = init_train_state(tcf, params=P | LA, device="cuda")
    assert not state.model._prefix_frozen()
    runner = TrainingStepRunner(tcf)
    state, info = runner(0, state, (to_observation(obs, "cuda"), actions.cuda()), 0, noise=noise.cuda(), time=time.cuda())
    torch.cuda.synchronize()
    Pg = {k: v.clone().requires_grad_(not frz(k)) for k, v in P.items()}
    LAg = {k: v.clone().requires_grad_(True) for k, v in LA.items()}
    loss32, _ = O.compute_loss(_merged_tree(cfg, Pg, LAg), oc, obs, actions, noise, time)
    loss32.backward()
    gn = torch.sqrt(sum((v.grad ** 2).sum() for v in list(Pg.values()) + list(LAg.values()) if v.grad is not None))
    assert abs(info["grad_norm"].item() - gn.item()) / gn.item() < 3e-2, (info["grad_norm"].item(), gn.item())
    assert abs(info["loss"].item() - loss32.item()) / abs(loss32.item()) < 1e-2
    new = state.model.ps.to_reference_tree("master")
    for k, v in (P | LA).items():
        if frz(k):
            assert torch.equal(new[k], v), k
        else:
            assert not torch.equal(new[k], v), k
    assert sum(not frz(k) for k in P | LA) > 20 and any(k.startswith("PaliGemma/img/") and not frz(k) for k in P)


def test_lora_sampler_graph_eager_oracle_and_parameter_updates(hip):
    """sample_actions of a LoRA model runs on merged weights: eager == graph replay bitwise, within the sampler tolerance of the f32
    oracle on the merged tree; after the parameters move, replay == eager == a freshly built model."""
    from lap_amd.model import LAP
    from lap_amd.serve import GraphedSampler

    cfg = _lora_cfg()
    oc = _oracle_cfg(cfg)
    P = O.init_params(oc, seed=17)
    LA = _adapters(cfg, seed=18)
    with torch.no_grad():
        M = _merged_tree(cfg, P, LA)
    model = LAP(cfg, params=P | LA, device=DEV)
    sampler = GraphedSampler(model, 1, 10).capture()
    obs, _, noise, _ = make_inputs(cfg, B=1, ragged=False, seed=3)
    so = {k: v for k, v in obs.items() if k != "tokenized_langact_mask"}
    o = to_observation(so | {"tokenized_langact_mask": None}, DEV)
    got = sampler(o, noise.to(DEV)).clone()
    eager = model.sample_actions(0, o, num_steps=10, noise=noise.to(DEV))
    assert torch.equal(got, eager)
    ref = O.sample_actions(M, oc, so, noise, num_steps=10)
    ref16 = O.sample_actions(M, dataclasses.replace(oc, emulate_bf16=True), so, noise, num_steps=10)
    err, base = rel(got, ref), rel(ref16, ref)
    assert err < max(3 * base, 1e-2), (err, base)
    # without the adapters the answer differs (the merge is live)
    plain = LAP(dataclasses.replace(cfg, paligemma_variant="dummy", action_expert_variant="dummy"), params=P, device=DEV)
    assert not torch.equal(plain.sample_actions(0, o, num_steps=10, noise=noise.to(DEV)), got)
    with torch.no_grad():
        for name in model.ps.master:
            model.ps.master[name].mul_(1.03)
    model.ps.refresh_mirror_local()
    out2 = sampler(o, noise.to(DEV)).clone()
    assert torch.equal(out2, model.sample_actions(0, o, num_steps=10, noise=noise.to(DEV)))
    assert not torch.equal(out2, got)
    fresh = LAP(cfg, params=P | LA, device=DEV)
    with torch.no_grad():
        for name in fresh.ps.master:
            fresh.ps.master[name].mul_(1.03)
    fresh.ps.refresh_mirror_local()
    assert torch.equal(out2, fresh.sample_actions(0, o, num_steps=10, noise=noise.to(DEV)))


def _lora_width_cfg(monkeypatch, **kw):
    """LAP-3B widths with 2 layers per tower (tests/test_model_parity_gpu.py _full_width_cfg) and the reference's LoRA ranks."""
    from lap_amd import config as C
    from lap_amd.config import LAPConfig

    monkeypatch.setitem(C._GEMMA, "gemma_2b_lora_x2", C.GemmaConfig(2048, 2, 16384, 8, 1, 256, lora_attn=(16, 16.0), lora_ffn=(16, 16.0)))
    monkeypatch.setitem(C._GEMMA, "gemma_300m_lora_x2", C.GemmaConfig(1024, 2, 4096, 8, 1, 256, lora_attn=(32, 32.0), lora_ffn=(32, 32.0)))
    monkeypatch.setitem(C._SIGLIP, "So400m/14_x2", C.SiglipConfig(1152, 2, 4304, 16))
    monkeypatch.setitem(O.GEMMA, "gemma_2b_x2", O.GemmaCfg(2048, 2, 16384, 8, 1, 256))
    monkeypatch.setitem(O.GEMMA, "gemma_300m_x2", O.GemmaCfg(1024, 2, 4096, 8, 1, 256))
    monkeypatch.setitem(O.SIGLIP, "So400m/14_x2", O.SiglipCfg(1152, 2, 4304, 16))
    base = dict(paligemma_variant="gemma_2b_lora_x2", action_expert_variant="gemma_300m_lora_x2", siglip_variant="So400m/14_x2",
                image_size=224, vocab_size=16384, action_dim=32, action_horizon=50, max_token_len=48,
                language_loss_weight=0.4, enable_image_augmentation=False, enable_action_training=True)
    return LAPConfig(**(base | kw))


def test_lora_full_width_adapter_gradients_frozen_wgrads_and_merged_sampler(hip, monkeypatch):
    """LAP-3B widths x 2 layers (gemma_2b_lora + gemma_300m_lora): the production routes (assembly GEMMs, padded gate|up rows, the off-path
    weight-gradient stream, panel prefill, skinny / packed-chain serving).  (a) loss and every ADAPTER gradient against the f32 merged-tree
    oracle; (b) under get_freeze_filter() no weight-gradient launch writes a frozen VLM projection (and the assembly kernels' launch
    counters drop); (c) the merged sampler against the oracle and against the unmerged generic layer path."""
    from lap_amd import flow_sample, hip as H
    from lap_amd.model import LAP
    from lap_amd.params import engine_to_reference

    cfg = _lora_width_cfg(monkeypatch)
    oc = _oracle_cfg(cfg)
    P = O.init_params(oc, seed=7)
    LA = _adapters(cfg, seed=8, std=0.01)
    obs, actions, noise, time = make_inputs(cfg, B=2, ragged=True)
    LAg = {k: v.clone().requires_grad_(True) for k, v in LA.items()}
    loss32, _ = O.compute_loss(_merged_tree(cfg, P, LAg), oc, obs, actions, noise, time)
    loss32.backward()
    model = LAP(cfg, params=P | LA, device=DEV)

    written = []        # gradient buffers the weight-gradient launches write
    grad_ptrs = {model.ps.g(n).data_ptr() for n in model.ps.names()}    # (the SigLIP stem's product goes through a temporary: its address is the allocator's choice)
    orig = {n: getattr(H, n) for n in ("linear_wgrad", "linear_wgrad_sumsq")}
    for n, f in orig.items():
        monkeypatch.setattr(H, n, (lambda f: lambda dy, x, out, *a, **kw: (written.append(out.data_ptr()), f(dy, x, out, *a, **kw))[1])(f))

    def step():
        for g in model.ps.grad.values():
            g.zero_()
        written.clear()
        before = H.gemm_asm_launch_counts()
        loss, _ = model.loss_and_grad(0, to_observation(obs, DEV), actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV))
        torch.cuda.synchronize()
        after = H.gemm_asm_launch_counts()
        return loss, [p for p in written if p in grad_ptrs], sum(after[k] - before[k] for k in after)

    loss, wg_all, asm_all = step()
    assert abs(loss.item() - loss32.item()) / abs(loss32.item()) < 1e-2, (loss.item(), loss32.item())
    gref = engine_to_reference(cfg, {n: model.ps.g(n).detach().float().cpu() for n in model.ps.names() if "/lora_" in n} |
                               {n: torch.zeros(model.ps.tensor_spec[n].shape) for n in model.ps.names() if "/lora_" not in n})
    worst = 0.0
    for k, leaf in LAg.items():
        r = rel(gref[k], leaf.grad)
        worst = max(worst, r)
        assert r < 5e-2, (k, r)
    print(f"\nLAP-3B widths x 2 layers: worst adapter-gradient rel-L2 vs the f32 merged oracle {worst:.3e}")
    # (b) frozen VLM base weights: their weight-gradient products are not issued at all
    frz = cfg.get_freeze_filter()
    model.ps.set_frozen(frz)
    vlm_ptrs = {model.ps.g(f"llm/{l}/{n}0").data_ptr() for l in range(2) for n in ("wqkv", "wo", "wgu", "wd")}
    frozen_ptrs = {model.ps.g(n).data_ptr() for n in model.ps.names() if not model.ps.is_trainable(n)}
    assert vlm_ptrs <= set(wg_all) and vlm_ptrs <= frozen_ptrs
    assert not model._prefix_frozen()
    _, wg_frozen, asm_frozen = step()
    for n, f in orig.items():
        monkeypatch.setattr(H, n, f)
    assert wg_frozen and not (set(wg_frozen) & frozen_ptrs)
    # exactly the products of the frozen tensors are gone (both experts' base projections, the adaRMS bank: LoRA on both experts
    # freezes every `llm` array but the adapters), and no more assembly-kernel launches than unfrozen
    assert len(wg_all) - len(wg_frozen) == sum(p in frozen_ptrs for p in wg_all), (len(wg_all), len(wg_frozen))
    assert collections.Counter(wg_frozen) == collections.Counter(p for p in wg_all if p not in frozen_ptrs)
    assert asm_frozen <= asm_all, (asm_frozen, asm_all)
    # (c) the sampler on merged weights (panel prefill, packed chain) vs the oracle and vs the unmerged layer loop
    so = {k: v for k, v in make_inputs(cfg, B=1, ragged=False)[0].items() if k != "tokenized_langact_mask"}
    nz = make_inputs(cfg, B=1, ragged=False)[2]
    o = to_observation(so | {"tokenized_langact_mask": None}, DEV)
    del model
    model = LAP(cfg, params=P | LA, device=DEV, with_grads=False)     # (set_frozen rounded the frozen masters: start again from P)
    merged = model.sample_actions(0, o, num_steps=10, noise=nz.to(DEV))
    unmerged = flow_sample.sample_actions(model, 0, o, num_steps=10, noise=nz.to(DEV), fused=False)   # (outside _serving_weights: base + adapters)
    with torch.no_grad():
        M = _merged_tree(cfg, P, LA)
    ref = O.sample_actions(M, oc, so, nz, num_steps=10)
    ref16 = O.sample_actions(M, dataclasses.replace(oc, emulate_bf16=True), so, nz, num_steps=10)
    err, base, mu = rel(merged, ref), rel(ref16, ref), rel(merged, unmerged)
    print(f"merged sampler vs f32 oracle {err:.3e}, unmerged vs oracle {rel(unmerged, ref):.3e}, merged vs unmerged {mu:.3e}, "
          f"bf16 oracle vs f32 {base:.3e}")
    assert err < max(3 * base, 1e-2) and rel(unmerged, ref) < max(3 * base, 1e-2), (err, base)


def test_lora_train_resume_matches_uninterrupted_run(hip, tmp_path):
    """Save / resume of a LoRA run under get_freeze_filter() (tests/test_train_loop_gpu.py pattern): 3 steps + resume + 1 step equals 4
    uninterrupted steps up to the run-to-run noise, and the checkpoint carries the adapters."""
    from lap_amd import checkpoints as ck
    from lap_amd.config import get_config
    from lap_amd.train import main

    tc = get_config("debug")
    cfg = dataclasses.replace(tc.model, paligemma_variant="dummy_lora", action_expert_variant="dummy_lora")
    base = dataclasses.replace(tc, model=cfg, freeze_filter=cfg.get_freeze_filter(), checkpoint_base_dir=str(tmp_path), batch_size=4,
                               log_interval=2, save_interval=3, keep_period=None, seed=3)
    a = main(dataclasses.replace(base, exp_name="full", num_train_steps=4), log=lambda s: None)
    a2 = main(dataclasses.replace(base, exp_name="full2", num_train_steps=4), log=lambda s: None)
    main(dataclasses.replace(base, exp_name="split", num_train_steps=3), log=lambda s: None)
    saved = ck.restore_params(tmp_path / base.name / "split")
    assert sum("lora" in k for k in saved) == 20
    lines = []
    c = main(dataclasses.replace(base, exp_name="split", num_train_steps=4), log=lines.append)
    assert c.step == 4 and lines[0].startswith("resumed from step 3")

    def worst(p, q):
        w = 0.0
        for buf in ("master", "m", "v"):
            num = sum(float((getattr(p, buf)[u.name] - getattr(q, buf)[u.name]).double().pow(2).sum()) for u in p.units)
            den = sum(float(getattr(p, buf)[u.name].double().pow(2).sum()) for u in p.units)
            w = max(w, (num / (den + 1e-30)) ** 0.5)
        return w

    noise = worst(a.model.ps, a2.model.ps)
    assert worst(a.model.ps, c.model.ps) <= max(5 * noise, 1e-2), (worst(a.model.ps, c.model.ps), noise)


def test_lora_policy_infer_end_to_end(hip, tmp_path):
    """Policy.infer on a LoRA checkpoint (create_trained_policy, captured sampler): the served actions equal the transforms + the eager
    sampler done by hand."""
    import json

    import numpy as np

    from lap_amd import checkpoints, policy_io as pio
    from lap_amd.config import get_config
    from lap_amd.model import LAP
    from lap_amd.observation import CoTObservation
    from lap_amd.serve import create_trained_policy
    from tests.common import tiny_sentencepiece_proto

    tc = get_config("debug")
    tc = dataclasses.replace(tc, model=dataclasses.replace(tc.model, paligemma_variant="dummy_lora", action_expert_variant="dummy_lora"),
                             data=dataclasses.replace(tc.data, asset_id="debug", wrist_image_dropout_prob=0.0, random_mask_prob=0.0))
    cfg = tc.model
    model = LAP(cfg, seed=5, device=DEV, with_grads=False)
    with torch.no_grad():       # adapters well away from their small init, and the zero-initialised adaRMS bank randomised: with zero
        for n in model.ps.names():  # gates the expert's layers (and their adapters) never reach the actions
            if "/lora_" in n:
                model.ps.f32(n).normal_(0.0, 0.1)
        model.ps.f32("ada/w").normal_(0.0, 0.02)
    model.ps.refresh_mirror_local()
    (tmp_path / "params").mkdir()
    tree = model.ps.to_reference_tree("master")
    checkpoints._save_tensors(tmp_path / "params" / "params.safetensors", {"params/" + k: v for k, v in tree.items()})
    stats = {"state": {"mean": [0.0] * 7, "std": [1.0] * 7, "q01": [-2.0] * 7, "q99": [2.0] * 7},
             "actions": {"mean": [0.0] * 7, "std": [1.0] * 7, "q01": [-0.5] * 7, "q99": [0.5] * 7}}
    (tmp_path / "assets" / "debug").mkdir(parents=True)
    (tmp_path / "assets" / "debug" / "norm_stats.json").write_text(json.dumps({"norm_stats": stats}))
    tok = pio.PaligemmaTokenizer(model_proto=tiny_sentencepiece_proto(), max_len=cfg.max_token_len)
    policy = create_trained_policy(tc, tmp_path, tokenizer=tok, default_prompt="pick up the block", use_graph=True, device=DEV)
    rs = np.random.RandomState(3)
    req = {"observation": {"base_0_rgb": (rs.rand(56, 56, 3) * 255).astype(np.uint8),
                           "left_wrist_0_rgb": (rs.rand(56, 56, 3) * 255).astype(np.uint8), "state": rs.uniform(-1, 1, 7)}}
    noise = rs.randn(cfg.action_horizon, cfg.action_dim).astype(np.float32)
    out = policy.infer(req, noise=noise)
    assert out["actions"].shape == (cfg.action_horizon, cfg.action_dim) and np.isfinite(out["actions"]).all()
    inp = pio.compose([pio.InjectDefaultPrompt("pick up the block"), pio.CoTInputs(action_dim=cfg.action_dim), pio.Normalize(stats, "bounds_q99"),
                       pio.TokenizePromptAndReasoning(tok, discrete_state_input=True), pio.PadStatesAndActions(cfg.action_dim)])(dict(req))
    batched = {k: ({kk: np.asarray(vv)[None] for kk, vv in v.items()} if isinstance(v, dict) else np.asarray(v)[None])
               for k, v in inp.items() if v is not None and not isinstance(v, str)}
    o = CoTObservation.from_dict(batched, device=DEV)
    a = model.sample_actions(0, o, num_steps=10, noise=torch.from_numpy(noise)[None].to(DEV))[0].cpu().numpy()
    np.testing.assert_array_equal(out["actions"], pio.Unnormalize(stats, "bounds_q99")({"actions": a})["actions"])
    plain = LAP(dataclasses.replace(cfg, paligemma_variant="dummy", action_expert_variant="dummy"),
                params={k: v for k, v in tree.items() if "lora" not in k}, device=DEV, with_grads=False)
    b = plain.sample_actions(0, o, num_steps=10, noise=torch.from_numpy(noise)[None].to(DEV))[0].cpu().numpy()
    assert np.abs(a - b).max() > 1e-3          # the adapters reach the served actions
