"""fp8 weight-only decoding of the fused LAP_AR decoder (GPU): lap_quantize_fp8_rows, the *_fp8 decode kernels of csrc/decode.hip
and `decode_weights=` / `GraphedTokenDecoder(weights=)`.

Bound.  The format (lap_amd/fp8.py) has power-of-two row scales, so every dequantised weight is a bf16 number and the scale
commutes with f32 accumulation: an fp8 kernel computes what the bf16 kernel of the same name computes on the dequantised weights,
with the same rounding points.  The fp8 stream keeps the bf16 stream's k-to-lane map (8 codes per lane per load) and its order of
additions, so nothing differs: every comparison with the bf16 twin below is torch.equal (outputs, logits, tokens), which is
stronger than the BF16_TOL / LOGIT_TOL / MARGIN bounds of tests/test_ar_decode_gpu.py that a reordered sum would get.  The codes and scales the kernels are fed here are built with torch.float8_e4m3fn, not with
the code under test.  Against the UNQUANTISED weights a linear projection differs by 1 % .. 2^-4: 2^-4 is the worst-case
rounding error of one e4m3 weight, a Gaussian matrix gives 2.6 - 2.7 %, and less than 1 % would mean the bf16 weights were read.
"""
import dataclasses
import time

import pytest
import torch

from oracle import lap_oracle as O
from tests.common import oracle_cfg, rel
from tests.test_ar_decode_gpu import D, H, HD, NH, _bf, _gemma2b_x2_cfg, _obs, _state, _to_obs
from tests.test_fp8_decode_cpu import SHAPES, _inputs, _statement

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _quant(w):
    """(codes float8_e4m3fn, scales f32 = 2^e, dequantised bf16) of a bf16 / f32 matrix by the words of the format, in torch."""
    amax = w.abs().amax(dim=1).double()
    e = torch.floor(torch.log2(448.0 / amax))
    e = torch.where(amax * torch.exp2(e + 1) <= 448.0, e + 1, e)
    e = torch.where(amax * torch.exp2(e) > 448.0, e - 1, e)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    s = torch.exp2(e).float()
    codes = (w.float() * s[:, None]).to(torch.float8_e4m3fn)
    return codes, s, (codes.float() / s[:, None]).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("shape,std", SHAPES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_device_quantiser_equals_the_cpu_statement(hip, shape, std, dtype):
    w = _inputs(shape, std, dtype)
    rc, rs = _statement(w)
    codes, scales = hip.quantize_fp8_rows(w.to(DEV))
    assert codes.dtype == torch.float8_e4m3fn and scales.dtype == torch.float32
    assert torch.equal(scales.cpu(), rs)
    assert torch.equal(codes.view(torch.uint8).cpu(), rc.view(torch.uint8))
    # in place into the caller's buffers (what a captured graph holds)
    c2, s2 = torch.zeros_like(codes), torch.zeros_like(scales)
    p = (c2.data_ptr(), s2.data_ptr())
    r = hip.quantize_fp8_rows(w.to(DEV), c2, s2)
    assert (r[0].data_ptr(), r[1].data_ptr()) == p and torch.equal(c2.view(torch.uint8), codes.view(torch.uint8)) and torch.equal(s2, scales)


@pytest.mark.parametrize("B", [1, 3])
def test_fp8_qkv_matches_bf16_twin(hip, B):
    g = torch.Generator(device=DEV).manual_seed(1)
    cap, s = 40, 17
    x = _bf(B, D, g=g)
    gamma = torch.randn(D, generator=g, device=DEV) * 0.1
    w = _bf((NH + 2) * HD, D, scale=0.02, g=g)
    codes, sc, deq = _quant(w)
    plen = [30 + 5 * b for b in range(B)]
    ck0, cv0 = _bf(B, cap, HD, g=g), _bf(B, cap, HD, g=g)

    def run(wt, **kw):
        ck, cv = ck0.clone(), cv0.clone()
        q = torch.zeros(B, NH * HD, dtype=torch.bfloat16, device=DEV)
        hip.decode_qkv(_state(hip, B, s + 1, plen), x, gamma, wt, q, ck, cv, NH, HD, HD ** -0.5, **kw)
        return q, ck, cv

    q8, ck8, cv8 = run(codes, wscale=sc)
    q8b, _, _ = run(codes.view(torch.uint8), wscale=sc)      # the codes as plain bytes
    qt, ckt, cvt = run(deq)
    qw, ckw, cvw = run(w)
    assert torch.equal(q8, q8b)
    for a, b in ((q8, qt), (ck8, ckt), (cv8, cvt)):
        assert torch.equal(a, b)
    others = [r for r in range(cap) if r != s]
    assert torch.equal(ck8[:, others], ck0[:, others]) and torch.equal(cv8[:, others], cv0[:, others])
    for a, b in ((q8, qw), (ck8[:, s], ckw[:, s]), (cv8[:, s], cvw[:, s])):
        e = rel(a.float(), b.float())
        print(f"qkv B={B}: fp8 vs unquantised {e:.4f}")
        assert 0.01 < e < 2.0 ** -4, e


@pytest.mark.parametrize("B", [1, 3])
def test_fp8_projections_match_bf16_twins(hip, B):
    g = torch.Generator(device=DEV).manual_seed(3)
    st = _state(hip, B, 1, [10] * B)
    x, a, act = _bf(B, D, g=g), _bf(B, NH * HD, g=g), _bf(B, H, g=g)
    zero = torch.zeros_like(x)
    gamma = torch.randn(D, generator=g, device=DEV) * 0.1
    wo, wgu, wd = _bf(D, NH * HD, scale=0.02, g=g), _bf(2 * H, D, scale=0.02, g=g), _bf(D, H, scale=0.01, g=g)

    def res(inp, wt, r, kwaves, **kw):
        y = torch.empty_like(x)
        hip.decode_proj_residual(st, inp, wt, r, y, kwaves=kwaves, **kw)
        return y

    for name, inp, w, kws in (("wo", a, wo, (1, 4)), ("wd", act, wd, (1, 4))):
        codes, sc, deq = _quant(w)
        for kwv in kws:
            assert torch.equal(res(inp, codes, x, kwv, wscale=sc), res(inp, deq, x, kwv)), (name, kwv)
            # the projection itself (no residual) against the unquantised weights
            eq = rel(res(inp, codes, zero, kwv, wscale=sc).float(), res(inp, w, zero, kwv).float())
            print(f"{name} B={B} kwaves={kwv}: fp8 vs unquantised {eq:.4f}")
            assert 0.01 < eq < 2.0 ** -4, (name, kwv, eq)
    codes, sc, deq = _quant(wgu)
    a8, at, aw = (torch.empty(B, H, dtype=torch.bfloat16, device=DEV) for _ in range(3))
    hip.decode_gate_up(st, x, gamma, codes, a8, wscale=sc)
    hip.decode_gate_up(st, x, gamma, deq, at)
    hip.decode_gate_up(st, x, gamma, wgu, aw)
    eq = rel(a8.float(), aw.float())
    print(f"gate_up B={B}: fp8 vs unquantised {eq:.4f}")
    assert torch.equal(a8, at)
    assert 0.01 < eq < 2.0 ** -4, eq          # (gate and up both carry the weight error through the GeGLU product)


@pytest.mark.parametrize("B", [1, 3])
def test_fp8_lm_head_matches_bf16_twin(hip, B):
    g = torch.Generator(device=DEV).manual_seed(4)
    V, cap = 32001, 6           # odd: the last unit has one row; 16001 units walk the 1024 x 4 waves four times
    table = torch.randn(V, D, generator=g, device=DEV) * 0.03
    codes, sc, deq = _quant(table)
    zeros = torch.zeros_like(deq)
    gamma = torch.randn(D, generator=g, device=DEV) * 0.1
    x = _bf(B, D, g=g)

    def run(sampling, hi, lo, **kw):
        st = _state(hip, B, 2, [5] * B)
        out = torch.zeros(B, cap, dtype=torch.int32, device=DEV)
        pval, pidx = hip.decode_lm_partials(B, DEV)
        lg = torch.empty(B, V, dtype=torch.float32, device=DEV)
        if sampling is None:
            hip.decode_lm_head(st, x, gamma, hi, lo, pval, pidx, logits=lg, **kw)
        else:
            hip.decode_lm_head_sample(st, sampling, x, gamma, hi, lo, pval, pidx, logits=lg, **kw)
        hip.decode_finish(st, pval, pidx, out, eos_token=-1)
        assert int(st[0]) == 3 and int(st[1]) == 0
        assert int(out[:, :2].abs().sum()) == 0 and int(out[:, 3:].abs().sum()) == 0
        return lg, out[:, 2].clone(), pval.clone(), pidx.clone()

    lg8, tok8, pv8, pi8 = run(None, codes, None, wscale=sc)
    lgt, tokt, _, _ = run(None, deq, zeros)
    assert torch.equal(lg8, lgt) and torch.equal(tok8, tokt)
    assert torch.equal(tok8.long(), lg8.argmax(1))         # the partials are over the logits the kernel wrote
    # the sampling head: greedy words give the greedy head's partials bit for bit; a temperature draw is the host restatement's
    from lap_amd import sampling as S

    words = hip.decode_sampling(DEV)
    lgs, toks, pvs, pis = run(words, codes, None, wscale=sc)
    assert torch.equal(lgs, lg8) and torch.equal(toks, tok8) and torch.equal(pvs, pv8) and torch.equal(pis, pi8)
    hip.decode_set_sampling(words, 11, 0.8)
    lgs, toks, _, _ = run(words, codes, None, wscale=sc)
    assert torch.equal(lgs, lg8)
    assert torch.equal(toks.cpu(), torch.from_numpy(S.sample_from_logits(lg8.cpu().numpy(), 0.8, 11, 2)))


@pytest.mark.parametrize("B", [1, 3])
def test_done_state_writes_nothing_fp8(hip, B):
    g = torch.Generator(device=DEV).manual_seed(5)
    cap = 16
    st = _state(hip, B, 3, [20] * B, done=1)
    st0 = st.clone()
    bufs = dict(x=_bf(B, D, g=g), xa=_bf(B, D, g=g), q=_bf(B, NH * HD, g=g), o=_bf(B, NH * HD, g=g), act=_bf(B, H, g=g),
                ck=_bf(B, cap, HD, g=g), cv=_bf(B, cap, HD, g=g), out=torch.randint(0, 9, (B, cap), dtype=torch.int32, device=DEV))
    pval, pidx = hip.decode_lm_partials(B, DEV)
    pval.fill_(-3.0)
    pidx.fill_(7)
    lg = torch.full((B, 64), 5.0, device=DEV)
    bufs |= dict(pval=pval, pidx=pidx, lg=lg)
    before = {k: v.clone() for k, v in bufs.items()}
    gamma = torch.ones(D, device=DEV)
    q = lambda *shape: _quant(_bf(*shape, g=g))[:2]
    c, s = q((NH + 2) * HD, D)
    hip.decode_qkv(st, bufs["x"], gamma, c, bufs["q"], bufs["ck"], bufs["cv"], NH, HD, HD ** -0.5, wscale=s)
    c, s = q(D, NH * HD)
    hip.decode_proj_residual(st, bufs["o"], c, bufs["x"], bufs["xa"], kwaves=1, wscale=s)
    c, s = q(2 * H, D)
    hip.decode_gate_up(st, bufs["xa"], gamma, c, bufs["act"], wscale=s)
    c, s = q(D, H)
    hip.decode_proj_residual(st, bufs["act"], c, bufs["xa"], bufs["x"], kwaves=4, wscale=s)
    c, s = q(64, D)
    hip.decode_lm_head(st, bufs["x"], gamma, c, None, pval, pidx, logits=lg, wscale=s)
    hip.decode_lm_head_sample(st, hip.decode_sampling(DEV), bufs["x"], gamma, c, None, pval, pidx, logits=lg, wscale=s)
    torch.cuda.synchronize()
    assert torch.equal(st, st0)
    for k, v in bufs.items():
        assert torch.equal(v, before[k]), k


def test_fp8_entry_points_reject_bad_arguments(hip):
    st = _state(hip, 1, 1, [4])
    x = _bf(1, D)
    y = torch.empty_like(x)
    codes, sc, deq = _quant(_bf(D, 2048, scale=0.02))
    with pytest.raises(hip.LapHipError):
        hip.decode_proj_residual(st, x, codes, x, y, kwaves=2, wscale=sc)
    with pytest.raises(TypeError):
        hip.decode_proj_residual(st, x, deq, x, y, kwaves=1, wscale=sc)          # bf16 weight with scales
    with pytest.raises(TypeError):
        hip.decode_proj_residual(st, x, codes, x, y, kwaves=1, wscale=sc[:-1].contiguous())
    with pytest.raises(TypeError):
        hip.decode_proj_residual(st, x, codes, x, y, kwaves=1)                   # codes without scales


# ---------------------------------------------------------------------------------------------------------------- model
def _prefill_once(model, o, mp):
    """Run the (unquantised) prefill once and make `model` hand that result to every decode under `mp`: the fp8 decode and its
    twin then start from the same prefix cache and the same last rows, bit for bit."""
    from lap_amd import ar_decode

    with model._serving_weights():
        pre = ar_decode.prefill(model, o)
    mp.setattr(ar_decode, "prefill", lambda m, obs: pre)
    return pre


def _twin_decode(hip, model, pre, steps, mode):
    """`DecodeCtx.first_token` / `DecodeCtx.step` restated over the hip.decode_* calls (the bf16 kernels) with the weights `mode`
    quantises replaced by their dequantised bf16 twins, behind the prefill `pre`.  Returns (tokens, logits)."""
    from lap_amd.ar_decode import DecodeCtx

    v = model.v
    KV = v.num_kv_heads
    with model._serving_weights():
        Wd = {f"llm/{l}/{n}": _quant(model.W(f"llm/{l}/{n}"))[2] for l in range(v.depth) for n in ("wqkv0", "wo0", "wgu0", "wd0")}
    if mode == "fp8":
        hi = _quant(model.F("llm/embed"))[2]
        lo = torch.zeros_like(hi)
    else:
        hi, lo = model.W("llm/embed"), model.ps.w16lo("llm/embed")
    B, Pn, cache, kinfo_prefix, _, plen, x_last = pre
    ctx = DecodeCtx(model, B, Pn, steps)
    ctx.bind(cache, kinfo_prefix)
    ctx.plen.copy_(plen)
    hip.decode_init(ctx.state, ctx.plen, ctx.out)
    lg = torch.empty((B, model.config.vocab_size), dtype=torch.float32, device=DEV)
    col = {}

    def token(x):
        hip.decode_lm_head(ctx.state, x, model.F("llm/final_norm"), hi, lo, ctx.pval, ctx.pidx, lg)
        hip.decode_finish(ctx.state, ctx.pval, ctx.pidx, ctx.out, model.EOS_TOKEN)
        col[f"logit/{int(ctx.state[0].item()) - 1}"] = lg.clone()

    token(x_last)
    rows, r_lo, r_hi = model.ps.embed_rows()
    while not bool(ctx.state[1].item()):
        hip.decode_embed(ctx.state, rows, r_lo, r_hi, ctx.out, ctx.x, v.width ** 0.5)
        for l in range(v.depth):
            p = f"llm/{l}/"
            gk, gv = ctx.gen[l, 0], ctx.gen[l, 1]
            hip.decode_qkv(ctx.state, ctx.x, model.F(p + "n_attn"), Wd[p + "wqkv0"], ctx.q, gk, gv, NH, HD, HD ** -0.5)
            ck, cv = ctx.prefix[l]
            hip.decode_attention(ctx.state, ctx.q, ck, cv, ctx.kinfo, ctx.Pn, gk, gv, ctx.o, ctx.attn_scratch, NH, KV, HD)
            hip.decode_proj_residual(ctx.state, ctx.o, Wd[p + "wo0"], ctx.x, ctx.xa)
            hip.decode_gate_up(ctx.state, ctx.xa, model.F(p + "n_ffw"), Wd[p + "wgu0"], ctx.act)
            hip.decode_proj_residual(ctx.state, ctx.act, Wd[p + "wd0"], ctx.xa, ctx.x, kwaves=hip.DECODE_KWAVES_DOWN)
        token(ctx.x)
    return ctx.out.clone(), col


def _check_against_twin(out, col, ref, rcol, steps):
    """Every step's logits and every token equal the twin's, bit for bit (no margin rule is needed, none is applied)."""
    assert sorted(col) == sorted(rcol) == sorted(f"logit/{s}" for s in range(steps))
    for s in range(steps):
        assert torch.equal(col[f"logit/{s}"], rcol[f"logit/{s}"]), (s, rel(col[f"logit/{s}"], rcol[f"logit/{s}"]))
    assert torch.equal(out, ref)


def test_fp8_decode_matches_dequantised_twin_graph_and_policy(hip, monkeypatch):
    import numpy as np

    from lap_amd.model import LAP
    from lap_amd.serve import ARPolicy, GraphedTokenDecoder, Policy

    cfg = _gemma2b_x2_cfg(monkeypatch)
    model = LAP(cfg, params=O.init_params(oracle_cfg(cfg), seed=13), device=DEV)
    so = _obs(cfg, "ragged")
    o = _to_obs(so)
    steps = 5
    plain = model.sample_tokens(0, o, max_decoding_steps=steps, decode="fused")
    assert torch.equal(model.sample_tokens(0, o, max_decoding_steps=steps, decode="fused", decode_weights="bf16"), plain)
    for mode in ("fp8_layers", "fp8"):
        col = {}
        with monkeypatch.context() as mp:
            pre = _prefill_once(model, o, mp)
            out = model.sample_tokens(0, o, max_decoding_steps=steps, decode="fused", decode_weights=mode, collect=col)
            ref, rcol = _twin_decode(hip, model, pre, steps, mode)
        _check_against_twin(out, col, ref, rcol, steps)
        assert torch.equal(model.sample_tokens(0, o, max_decoding_steps=steps, decode="fused", decode_weights=mode), out)
        # graph replay: the same kernels in the same order
        assert torch.equal(GraphedTokenDecoder(model, 3, steps, prompt_len=cfg.max_token_len, weights=mode)(o), out)
        sdec = GraphedTokenDecoder(model, 3, steps, sampling=True, weights=mode)
        assert torch.equal(sdec(o), out)
        drawn = model.sample_tokens(9, o, max_decoding_steps=steps, temperature=0.7, decode="fused", sampler="device", decode_weights=mode)
        assert torch.equal(sdec(o, temperature=0.7, seed=9), drawn)
    with pytest.raises(ValueError, match="decode_weights"):
        GraphedTokenDecoder(model, 3, steps, weights="int8")
    with pytest.raises(ValueError, match='decode="fused"'):
        model.sample_tokens(0, o, max_decoding_steps=steps, decode_weights="fp8")
    # ARPolicy: the captured decoder and the direct call decode on the same weights (B = 1)
    so1 = _obs(cfg, "ragged", B=1)
    direct = model.sample_tokens(0, _to_obs(so1), max_decoding_steps=steps, decode="fused", decode_weights="fp8")
    req = {"image": {k: v[0].numpy() for k, v in so1["images"].items()},
           "image_mask": {k: v[0].numpy() for k, v in so1["image_masks"].items()},
           "state": so1["state"][0].numpy(), "tokenized_prompt": so1["tokenized_prompt"][0].numpy(),
           "tokenized_prompt_mask": so1["tokenized_prompt_mask"][0].numpy()}
    kw = {"max_decoding_steps": steps, "decode_weights": "fp8"}
    pol = ARPolicy(Policy(model, use_graph=False), sample_kwargs=kw, use_graph=True)
    assert pol._decoder is not None and pol._decoder.weights == "fp8"
    assert np.array_equal(pol.infer(req)["tokens"], direct.cpu().numpy())
    assert np.array_equal(ARPolicy(Policy(model, use_graph=False), sample_kwargs=kw).infer(req)["tokens"], direct.cpu().numpy())
    with pytest.raises(ValueError):
        ARPolicy(Policy(model, use_graph=False), sample_kwargs=kw | {"decode": "eager"})


def test_fp8_graph_follows_parameter_updates(hip, monkeypatch):
    from lap_amd.model import LAP
    from lap_amd.serve import GraphedTokenDecoder

    cfg = _gemma2b_x2_cfg(monkeypatch)
    oc = oracle_cfg(cfg)
    model = LAP(cfg, params=O.init_params(oc, seed=31), device=DEV)
    o = _to_obs(_obs(cfg, "ragged"))
    dec = GraphedTokenDecoder(model, 3, 6, weights="fp8")
    first = dec(o)
    assert torch.equal(first, model.sample_tokens(0, o, max_decoding_steps=6, decode="fused", decode_weights="fp8"))
    ptrs = {k: (r[0].data_ptr(), r[1].data_ptr()) for k, r in model.serving_cache.entries("dec8").items()}
    assert len(ptrs) == 4 * model.v.depth + 1
    # new parameters whose tokens differ: random weights echo the last prompt token, so blank its embedding row
    P2 = O.init_params(oc, seed=32)
    key = "PaliGemma/llm/embedder/input_embedding"
    E = torch.as_tensor(P2[key]).clone()
    E[first[:, 0].long().cpu()] = 0
    P2[key] = E
    model.ps.load_reference_tree(P2)
    second = dec(o)
    assert {k: (r[0].data_ptr(), r[1].data_ptr()) for k, r in model.serving_cache.entries("dec8").items()} == ptrs      # re-quantised in place
    fresh = LAP(cfg, params=P2, device=DEV)
    assert torch.equal(second, fresh.sample_tokens(0, o, max_decoding_steps=6, decode="fused", decode_weights="fp8"))
    assert torch.equal(second, model.sample_tokens(0, o, max_decoding_steps=6, decode="fused", decode_weights="fp8"))
    assert not torch.equal(second, first)


def test_fp8_decode_of_a_lora_model_reads_the_merged_weights(hip, monkeypatch):
    from lap_amd import config as C
    from lap_amd.model import LAP
    from lap_amd.params import reference_shapes

    base = _gemma2b_x2_cfg(monkeypatch)
    monkeypatch.setitem(C._GEMMA, "gemma_2b_lora_x2", C.GemmaConfig(2048, 2, 16384, 8, 1, 256, lora_attn=(16, 16.0), lora_ffn=(16, 16.0)))
    cfg = dataclasses.replace(base, paligemma_variant="gemma_2b_lora_x2")
    P = O.init_params(oracle_cfg(base), seed=13)
    g = torch.Generator().manual_seed(18)
    LA = {k: torch.randn(s, generator=g) * 0.05 for k, s in reference_shapes(cfg).items() if "lora" in k}
    model = LAP(cfg, params=P | LA, device=DEV)
    o = _to_obs(_obs(base, "ragged"))
    steps = 4
    col = {}
    with monkeypatch.context() as mp:
        pre = _prefill_once(model, o, mp)
        out = model.sample_tokens(0, o, max_decoding_steps=steps, decode="fused", decode_weights="fp8", collect=col)
        ref, rcol = _twin_decode(hip, model, pre, steps, "fp8")       # (the twin quantises the MERGED weights)
    _check_against_twin(out, col, ref, rcol, steps)
    with model._serving_weights():
        merged = model.W("llm/0/wgu0")
    assert not torch.equal(merged, model.ps.w16("llm/0/wgu0"))                      # the adapters are live
    assert torch.equal(model.serving_cache.entries("dec8")["llm/0/wgu0"][0].view(torch.uint8), _quant(merged)[0].view(torch.uint8))


# ----------------------------------------------------------------------------------------------------------- full depth
def test_full_depth_fp8_graph_is_faster_than_bf16_graph(hip):
    """Full-depth LAP-3B, B = 1, 64 tokens, EOS disabled: a graphed fp8 token costs less than a graphed bf16 token in the same
    process (the bf16 graph is the baseline; the weight bytes of a token drop from 6.07 GB to 2.6 GB, so no margin is given).
    Printed, not gated (random weights say little about a trained policy): the share of the 64 tokens that equal the bf16
    decoder's, and the relative error of the first two tokens' logits against bf16 decoding."""
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
    decs = {"bf16": dec, "fp8_layers": GraphedTokenDecoder(model, 1, n, weights="fp8_layers"), "fp8": GraphedTokenDecoder(model, 1, n, weights="fp8")}
    toks = {k: d(o) for k, d in decs.items()}           # (captures)
    torch.cuda.synchronize()

    def ms(d):
        """(ms per call, ms per prefill replay) -> ms per token after the prefill; the best of 3 interleaved rounds is taken"""
        t0 = time.perf_counter()
        d(o)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        d.g_prefill.replay()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return ((t1 - t0) - (t2 - t1)) / (n - 1) * 1e3

    per = {k: ms(d) for k, d in decs.items()}
    for _ in range(2):
        for k, d in decs.items():
            per[k] = min(per[k], ms(d))
    c16 = {}
    model.sample_tokens(0, o, max_decoding_steps=2, decode="fused", collect=c16)
    for k in ("fp8_layers", "fp8"):
        c8 = {}
        model.sample_tokens(0, o, max_decoding_steps=2, decode="fused", decode_weights=k, collect=c8)
        print(f"full-depth LAP-3B B=1 {n} tokens graphed: bf16 {per['bf16']:.3f} ms/token, {k} {per[k]:.3f} ms/token; "
              f"{float((toks[k] == toks['bf16']).float().mean()):.3f} of the tokens equal bf16's; logit rel. error vs bf16: first token "
              f"{rel(c8['logit/0'], c16['logit/0']):.4f}, second {rel(c8['logit/1'], c16['logit/1']):.4f}")
    assert per["fp8"] < per["bf16"]
    assert per["fp8_layers"] < per["bf16"]
