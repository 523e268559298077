"""Fused single-token decode (csrc/decode.hip) and its graph-replayed LAP_AR surface (GPU).

Bound.  Every fused stage keeps the eager step's rounding points and differs from it only in the summation order of its dot
products (f32 accumulation in both), so the two agree to bf16 rounding noise: bf16 outputs within BF16_TOL relative
(Frobenius norm) of the eager kernels' outputs, f32 logits within LOGIT_TOL.  Tokens are required to be identical wherever
the eager logits' top-2 margin exceeds MARGIN (absolute, in logit units); below it a summation-order flip is allowed.
"""
import dataclasses
import time

import pytest
import torch

from oracle import lap_oracle as O
from tests.common import debug_model_cfg, make_inputs, oracle_cfg, rel, to_observation

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16_TOL = 1e-2
LOGIT_TOL = 1e-3
MARGIN = 5e-2

D, NH, HD, H = 2048, 8, 256, 16384


def _gemma2b_x2_cfg(monkeypatch, **kw):
    """LAP-3B widths with 2 layers per tower and a 16k vocabulary (tests/test_model_parity_gpu.py's _full_width_cfg)."""
    from lap_amd import config as C
    from lap_amd.config import LAPConfig

    monkeypatch.setitem(C._GEMMA, "gemma_2b_x2", C.GemmaConfig(2048, 2, 16384, 8, 1, 256))
    monkeypatch.setitem(C._GEMMA, "gemma_300m_x2", C.GemmaConfig(1024, 2, 4096, 8, 1, 256))
    monkeypatch.setitem(C._SIGLIP, "So400m/14_x2", C.SiglipConfig(1152, 2, 4304, 16))
    monkeypatch.setitem(O.GEMMA, "gemma_2b_x2", O.GemmaCfg(2048, 2, 16384, 8, 1, 256))
    monkeypatch.setitem(O.GEMMA, "gemma_300m_x2", O.GemmaCfg(1024, 2, 4096, 8, 1, 256))
    monkeypatch.setitem(O.SIGLIP, "So400m/14_x2", O.SiglipCfg(1152, 2, 4304, 16))
    base = dict(paligemma_variant="gemma_2b_x2", action_expert_variant="gemma_300m_x2", siglip_variant="So400m/14_x2",
                image_size=224, vocab_size=16384, action_dim=32, action_horizon=50, max_token_len=48,
                language_loss_weight=0.4, enable_image_augmentation=False, enable_action_training=True)
    return LAPConfig(**(base | kw))


def _state(hip, B, t, plen, done=0):
    st = hip.decode_state(B, DEV)
    st[0], st[1] = t, done
    st[16:16 + B] = torch.as_tensor(plen, dtype=torch.int32)
    return st


def _bf(*shape, scale=1.0, g=None):
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("B", [1, 3])
def test_qkv_appends_at_device_step(hip, B):
    g = torch.Generator(device=DEV).manual_seed(1)
    cap, s = 40, 17
    x = _bf(B, D, g=g)
    gamma = torch.randn(D, generator=g, device=DEV) * 0.1
    w = _bf((NH + 2) * HD, D, scale=0.02, g=g)
    plen = [30 + 5 * b for b in range(B)]
    ck0, cv0 = _bf(B, cap, HD, g=g), _bf(B, cap, HD, g=g)
    ck, cv = ck0.clone(), cv0.clone()
    q = torch.zeros(B, NH * HD, dtype=torch.bfloat16, device=DEV)
    hip.decode_qkv(_state(hip, B, s + 1, plen), x, gamma, w, q, ck, cv, NH, HD, HD ** -0.5)
    h, _ = hip.rmsnorm_fwd(x, scale=gamma, save_rstd=False)
    pos = (torch.tensor(plen, dtype=torch.int32, device=DEV) + s).view(B, 1).contiguous()
    qe, ke, ve = hip.rope_split_fwd(hip.linear_fwd(h, w), pos, B, 1, 1, 0, NH, HD, HD ** -0.5)
    assert rel(q.float(), qe.float()) < BF16_TOL
    assert rel(ck[:, s].float(), ke.float()) < BF16_TOL and rel(cv[:, s].float(), ve.float()) < BF16_TOL
    others = [r for r in range(cap) if r != s]
    assert torch.equal(ck[:, others], ck0[:, others]) and torch.equal(cv[:, others], cv0[:, others])


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("step", [0, 1, 37, 63])
def test_attention_matches_two_segment_attention(hip, B, step):
    g = torch.Generator(device=DEV).manual_seed(2)
    cap, Pn = 64, 157
    q = _bf(B, NH * HD, scale=HD ** -0.5, g=g)
    pk, pv = _bf(B * Pn, HD, g=g), _bf(B * Pn, HD, g=g)
    gk, gv = _bf(B, cap, HD, g=g), _bf(B, cap, HD, g=g)
    ok = torch.rand(B, Pn, generator=g, device=DEV) < 0.8
    ok[:, :3] = False                          # a masked run at the start (the right-aligned prefix's left padding)
    kinfo = (ok.to(torch.int32) << 24).contiguous()
    o = torch.zeros(B, NH * HD, dtype=torch.bfloat16, device=DEV)
    scratch = hip.decode_attn_scratch(B, Pn, cap, DEV)
    hip.decode_attention(_state(hip, B, step + 1, [Pn] * B), q, pk, pv, kinfo, Pn, gk, gv, o, scratch, NH, 1, HD)
    n = step + 1
    ki = torch.cat([kinfo, torch.full((B, n), 1 << 24, dtype=torch.int32, device=DEV)], 1).contiguous()
    qinfo = torch.full((B, 1), (1 << 24) | 0xFFFFFF, dtype=torch.int32, device=DEV)
    oe, _ = hip.attention_fwd([None, q], [pk, gk[:, :n].reshape(B * n, HD).contiguous()], [pv, gv[:, :n].reshape(B * n, HD).contiguous()],
                              [0, 1], [Pn, n], B, NH, 1, HD, qinfo, ki, need_lse=False)
    assert rel(o.float(), oe[1].float()) < BF16_TOL


@pytest.mark.parametrize("B", [1, 3])
def test_projections_match_eager_kernels(hip, B):
    g = torch.Generator(device=DEV).manual_seed(3)
    st = _state(hip, B, 1, [10] * B)
    x, a = _bf(B, D, g=g), _bf(B, NH * HD, g=g)
    gamma = torch.randn(D, generator=g, device=DEV) * 0.1
    wo, wgu, wd = _bf(D, NH * HD, scale=0.02, g=g), _bf(2 * H, D, scale=0.02, g=g), _bf(D, H, scale=0.01, g=g)
    y = torch.empty_like(x)
    hip.decode_proj_residual(st, a, wo, x, y)
    assert rel(y.float(), hip.linear_fwd(a, wo, residual=x).float()) < BF16_TOL
    act = torch.empty(B, H, dtype=torch.bfloat16, device=DEV)
    hip.decode_gate_up(st, x, gamma, wgu, act)
    h, _ = hip.rmsnorm_fwd(x, scale=gamma, save_rstd=False)
    ae = hip.geglu_fwd(hip.linear_fwd(h, wgu))
    assert rel(act.float(), ae.float()) < BF16_TOL
    for kw in (1, 4):
        y2 = torch.empty_like(x)
        hip.decode_proj_residual(st, act, wd, x, y2, kwaves=kw)
        assert rel(y2.float(), hip.linear_fwd(act, wd, residual=x).float()) < BF16_TOL


def _eager_logits(hip, x, gamma, hi, lo):
    pl, _ = hip.rmsnorm_fwd(x, scale=gamma, save_rstd=False)
    V = hi.shape[0]
    lg = torch.empty((x.shape[0], V), dtype=torch.float32, device=DEV)
    hip.gemm(pl, hi, lg, M=x.shape[0], N=V, K=D, lda=D, ldb=D, ldc=V)
    hip.gemm(pl, lo, lg, M=x.shape[0], N=V, K=D, lda=D, ldb=D, ldc=V, accum=True)
    return lg


@pytest.mark.parametrize("B", [1, 3])
def test_lm_head_argmax_and_finish(hip, B):
    g = torch.Generator(device=DEV).manual_seed(4)
    V, cap = 257152, 6
    table = torch.randn(V, D, generator=g, device=DEV) * 0.03
    hi, lo = hip.split_f32_hilo(table)
    gamma = torch.randn(D, generator=g, device=DEV) * 0.1
    x = _bf(B, D, g=g)
    st = _state(hip, B, 2, [5] * B)
    out = torch.zeros(B, cap, dtype=torch.int32, device=DEV)
    pval, pidx = hip.decode_lm_partials(B, DEV)
    lg = torch.empty(B, V, dtype=torch.float32, device=DEV)
    hip.decode_lm_head(st, x, gamma, hi, lo, pval, pidx, logits=lg)
    hip.decode_finish(st, pval, pidx, out, eos_token=-1)
    ref = _eager_logits(hip, x, gamma, hi, lo)
    assert rel(lg, ref) < LOGIT_TOL
    top2 = ref.topk(2, dim=1).values
    tok = hip.argmax_rows(ref)
    for b in range(B):
        if float(top2[b, 0] - top2[b, 1]) > MARGIN:
            assert int(out[b, 2]) == int(tok[b])
    assert int(out[:, :2].abs().sum()) == 0 and int(out[:, 3:].abs().sum()) == 0
    assert int(st[0]) == 3 and int(st[1]) == 0
    # duplicated rows: the lowest index wins (jnp.argmax / lap_argmax_rows_f32)
    V2 = 4096
    t2 = torch.randn(V2, D, generator=g, device=DEV) * 0.03
    xb = _bf(B, D, g=g)
    best = int(hip.argmax_rows(_eager_logits(hip, xb, gamma, *hip.split_f32_hilo(t2)))[0])
    lo_i = 7 if best > 7 else best + 1
    t2[lo_i] = t2[best]
    t2[V2 - 1] = t2[best]
    h2, l2 = hip.split_f32_hilo(t2)
    st2 = _state(hip, B, 0, [5] * B)
    out2 = torch.zeros(B, cap, dtype=torch.int32, device=DEV)
    hip.decode_lm_head(st2, xb, gamma, h2, l2, pval, pidx)
    hip.decode_finish(st2, pval, pidx, out2, eos_token=-1)
    ref2 = hip.argmax_rows(_eager_logits(hip, xb, gamma, h2, l2))
    assert int(out2[0, 0]) == int(ref2[0]) == min(lo_i, best)
    # EOS of every sample -> done
    st3 = _state(hip, B, 0, [5] * B)
    hip.decode_finish(st3, pval, pidx, out2, eos_token=int(out2[0, 0]) if B == 1 else -5)
    assert int(st3[1]) == (1 if B == 1 else 0)


@pytest.mark.parametrize("B", [1, 3])
def test_done_state_writes_nothing(hip, B):
    g = torch.Generator(device=DEV).manual_seed(5)
    cap, Pn = 16, 40
    st = _state(hip, B, 3, [20] * B, done=1)
    st0 = st.clone()
    x = _bf(B, D, g=g)
    bufs = dict(x=x, xa=_bf(B, D, g=g), q=_bf(B, NH * HD, g=g), o=_bf(B, NH * HD, g=g), act=_bf(B, H, g=g),
                ck=_bf(B, cap, HD, g=g), cv=_bf(B, cap, HD, g=g), out=torch.randint(0, 9, (B, cap), dtype=torch.int32, device=DEV))
    before = {k: v.clone() for k, v in bufs.items()}
    gamma = torch.ones(D, device=DEV)
    table = torch.randn(64, D, generator=g, device=DEV)
    hip.decode_embed(st, table, 0, 64, bufs["out"], bufs["x"], 45.25)
    hip.decode_qkv(st, bufs["x"], gamma, _bf((NH + 2) * HD, D, g=g), bufs["q"], bufs["ck"], bufs["cv"], NH, HD, HD ** -0.5)
    hip.decode_attention(st, bufs["q"], _bf(B * Pn, HD, g=g), _bf(B * Pn, HD, g=g), torch.full((B, Pn), 1 << 24, dtype=torch.int32, device=DEV),
                         Pn, bufs["ck"], bufs["cv"], bufs["o"], hip.decode_attn_scratch(B, Pn, cap, DEV), NH, 1, HD)
    hip.decode_proj_residual(st, bufs["o"], _bf(D, NH * HD, g=g), bufs["x"], bufs["xa"])
    hip.decode_gate_up(st, bufs["xa"], gamma, _bf(2 * H, D, g=g), bufs["act"])
    hip.decode_proj_residual(st, bufs["act"], _bf(D, H, g=g), bufs["xa"], bufs["x"])
    hi, lo = hip.split_f32_hilo(table)
    pval, pidx = hip.decode_lm_partials(B, DEV)
    hip.decode_lm_head(st, bufs["x"], gamma, hi, lo, pval, pidx)
    hip.decode_finish(st, pval, pidx, bufs["out"], eos_token=1)
    torch.cuda.synchronize()
    assert torch.equal(st, st0)
    for k, v in bufs.items():
        assert torch.equal(v, before[k]), k


# ---------------------------------------------------------------------------------------------------------------- model
def _obs(cfg, case, B=3):
    obs, _, _, _ = make_inputs(cfg, B=B, ragged=True)
    so = dict(obs)
    if case != "langact":
        so.pop("tokenized_langact_mask")
    so["image_masks"] = {k: torch.ones_like(m) for k, m in so["image_masks"].items()}
    if case == "masked_image":
        so["image_masks"][cfg.image_keys[-1]][1] = False
    return so


def _to_obs(so):
    return to_observation(so if "tokenized_langact_mask" in so else so | {"tokenized_langact_mask": None}, DEV)


def _agrees_with_eager(out, ref, col):
    """tokens equal step by step while the eager top-2 margins exceed MARGIN (from the first step where one does not, the
    contexts may diverge)."""
    for s in range(ref.shape[1]):
        if not torch.equal(out[:, :s], ref[:, :s]):
            return False
        lg = col.get(f"logit/{s}")
        if lg is None:
            break
        top2 = lg.topk(2, dim=1).values
        if bool(((top2[:, 0] - top2[:, 1]) <= MARGIN).any()):
            return True
    return torch.equal(out, ref)


@pytest.mark.parametrize("case", ["ragged", "masked_image", "langact"])
def test_fused_and_graphed_decode_match_oracle(hip, monkeypatch, case):
    from lap_amd.model import LAP
    from lap_amd.serve import GraphedTokenDecoder

    cfg = _gemma2b_x2_cfg(monkeypatch)
    oc = oracle_cfg(cfg)
    P = O.init_params(oc, seed=13)
    so = _obs(cfg, case)
    steps = 5
    c32, c16 = {}, {}
    ref = O.sample_tokens(P, oc, so, max_decoding_steps=steps, collect=c32)
    ref16 = O.sample_tokens(P, dataclasses.replace(oc, emulate_bf16=True), so, max_decoding_steps=steps, collect=c16)
    model = LAP(cfg, params=P, device=DEV)
    o = _to_obs(so)
    col, cole = {}, {}
    out = model.sample_tokens(0, o, max_decoding_steps=steps, collect=col, decode="fused")
    eager = model.sample_tokens(0, o, max_decoding_steps=steps, collect=cole)
    assert out.shape == (3, steps) and out.dtype == torch.int32
    agree = 0
    for s in range(steps):
        if not (torch.equal(ref[:, :s], ref16[:, :s]) and torch.equal(out[:, :s].cpu(), ref[:, :s])):
            break
        err, base = rel(col[f"logit/{s}"].cpu(), c32[f"logit/{s}"]), rel(c16[f"logit/{s}"], c32[f"logit/{s}"])
        assert err < max(3 * base, 1e-2), (s, err, base)
        agree += 1
        if case == "masked_image":
            break
    assert agree >= (1 if case == "masked_image" else 2)
    assert _agrees_with_eager(out, eager, cole)
    dec = GraphedTokenDecoder(model, 3, steps, prompt_len=cfg.max_token_len)
    got = dec(o)
    assert _agrees_with_eager(got, eager, cole)
    assert torch.equal(got, out)       # same kernels, same order: the replay is the fused path bit for bit


def test_stop_logic_matches_eager(hip, monkeypatch):
    from lap_amd.model import LAP
    from lap_amd.serve import GraphedTokenDecoder

    cfg = _gemma2b_x2_cfg(monkeypatch)
    P = O.init_params(oracle_cfg(cfg), seed=21)
    model = LAP(cfg, params=P, device=DEV)
    o = _to_obs(_obs(cfg, "ragged"))
    # budgets that are not multiples of the replay length
    for steps in (1, 5, 13):
        eager = model.sample_tokens(0, o, max_decoding_steps=steps)
        dec = GraphedTokenDecoder(model, 3, steps, steps_per_replay=8)
        got = dec(o)
        assert torch.equal(got, eager), steps
        assert torch.equal(model.sample_tokens(0, o, max_decoding_steps=steps, decode="fused"), eager), steps
    steps = 13
    eager = model.sample_tokens(0, o, max_decoding_steps=steps).cpu()
    # one sample of three reaches EOS early (its first token) while the other two continue to the budget
    eos = int(eager[1, 0])
    assert not bool((eager[[0, 2]] == eos).any())
    model.EOS_TOKEN = eos
    ref = model.sample_tokens(0, o, max_decoding_steps=steps)
    assert int(ref[1, 0]) == eos and int(ref[0, steps - 1]) != 0
    got = GraphedTokenDecoder(model, 3, steps)(o)
    assert torch.equal(got, ref)
    assert torch.equal(model.sample_tokens(0, o, max_decoding_steps=steps, decode="fused"), ref)
    # EOS as the first token of every sample: stops after one step, the rest stays zero
    o1 = _to_obs({k: ({kk: vv[:1] for kk, vv in v.items()} if isinstance(v, dict) else v[:1]) for k, v in _obs(cfg, "ragged").items()})
    model.EOS_TOKEN = 1
    first = int(model.sample_tokens(0, o1, max_decoding_steps=5)[0, 0])
    model.EOS_TOKEN = first
    ref = model.sample_tokens(0, o1, max_decoding_steps=5)
    got = GraphedTokenDecoder(model, 1, 5)(o1)
    assert int(ref[0, 0]) == first and int(ref[0, 1:].abs().sum()) == 0
    assert torch.equal(got, ref)


def test_graph_follows_parameter_updates(hip, monkeypatch):
    from lap_amd.model import LAP
    from lap_amd.serve import GraphedTokenDecoder

    cfg = _gemma2b_x2_cfg(monkeypatch)
    oc = oracle_cfg(cfg)
    model = LAP(cfg, params=O.init_params(oc, seed=31), device=DEV)
    o = _to_obs(_obs(cfg, "ragged"))
    dec = GraphedTokenDecoder(model, 3, 6)
    first = dec(o)
    assert torch.equal(first, model.sample_tokens(0, o, max_decoding_steps=6, decode="fused"))
    # new parameters whose tokens differ: random weights echo the last prompt token, so blank its embedding row
    P2 = O.init_params(oc, seed=32)
    key = "PaliGemma/llm/embedder/input_embedding"
    E = torch.as_tensor(P2[key]).clone()
    E[first[:, 0].long().cpu()] = 0
    P2[key] = E
    model.ps.load_reference_tree(P2)
    second = dec(o)
    fused = model.sample_tokens(0, o, max_decoding_steps=6, decode="fused")
    assert torch.equal(second, fused)
    assert not torch.equal(second, first)


def test_declined_shapes(hip):
    import numpy as np

    from lap_amd.model import LAP
    from lap_amd.serve import ARPolicy, GraphedTokenDecoder, Policy

    cfg = debug_model_cfg()
    model = LAP(cfg, params=O.init_params(oracle_cfg(cfg), seed=3), device=DEV)
    so = _obs(cfg, "ragged", B=1)
    o = _to_obs(so)
    assert not model.decode_supported(1)
    with pytest.raises(ValueError):
        model.sample_tokens(0, o, max_decoding_steps=4, decode="fused")
    with pytest.raises(ValueError):
        GraphedTokenDecoder(model, 1, 4)
    eager = model.sample_tokens(0, o, max_decoding_steps=4)
    pol = ARPolicy(Policy(model, use_graph=False), sample_kwargs={"max_decoding_steps": 4}, use_graph=True)
    assert pol._decoder is None
    req = {"image": {k: v[0].numpy() for k, v in so["images"].items()},
           "image_mask": {k: v[0].numpy() for k, v in so["image_masks"].items()},
           "state": so["state"][0].numpy(), "tokenized_prompt": so["tokenized_prompt"][0].numpy(),
           "tokenized_prompt_mask": so["tokenized_prompt_mask"][0].numpy()}
    got = pol.infer(req)["tokens"]
    assert np.array_equal(got, eager.cpu().numpy())


def test_full_depth_graphed_decode(hip):
    """Full-depth LAP-3B, B = 1, 64 tokens, EOS disabled: graphed tokens equal the eager ones wherever the margins allow."""
    from lap_amd.config import get_config
    from lap_amd.model import LAP
    from lap_amd.observation import CoTObservation
    from lap_amd.serve import GraphedTokenDecoder

    cfg = get_config("lap_bench").model
    model = LAP(cfg, seed=0, device=DEV, with_grads=False)
    model.EOS_TOKEN = -1
    n = 64
    dec = GraphedTokenDecoder(model, 1, n)
    gen = torch.Generator(device="cpu").manual_seed(0)
    for k in dec.obs.images:
        dec.obs.images[k].copy_(torch.rand(dec.obs.images[k].shape, generator=gen) * 2 - 1)
    dec.obs.tokenized_prompt.copy_(torch.randint(0, cfg.vocab_size, dec.obs.tokenized_prompt.shape, generator=gen, dtype=torch.int32))
    g = dec.obs
    o = CoTObservation(images={k: v.clone() for k, v in g.images.items()}, image_masks={k: v.clone() for k, v in g.image_masks.items()},
                       state=g.state.clone(), tokenized_prompt=g.tokenized_prompt.clone(), tokenized_prompt_mask=g.tokenized_prompt_mask.clone())
    col = {}
    eager = model.sample_tokens(0, o, max_decoding_steps=n, collect=col)
    got = dec(o)
    assert _agrees_with_eager(got, eager, col)

    def ms(fn, reps):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3

    t_eager = ms(lambda: model.sample_tokens(0, o, max_decoding_steps=n), 2)
    t_graph = ms(lambda: dec(o), 3)
    print(f"full-depth LAP-3B B=1 {n} tokens incl. prefill: eager {t_eager / n:.3f} ms/token, graphed {t_graph / n:.3f} ms/token")
    assert t_graph < t_eager
