"""The serving prefill, shared by the action sampler (lap_amd/flow_sample.py) and token decoding (lap_amd/ar_decode.py): the SigLIP
tower and the prefix-only Gemma pass on the fused consumers, and the packed weight images of the row-panel kernel.  Nothing is kept
for a backward.  The weights are read through the model (`W`, `F`), as `LAP._serving_weights` presents them.
"""
from __future__ import annotations

import torch

from lap_amd import hip
from lap_amd.model import LAP
from lap_amd.siglip import siglip_stem


def panel_weight(model: LAP, name):
    """Fragment-packed image (lap_serve_pack_weight kind 3) of a prefill projection for the row-panel kernel, persistent like
    `flow_sample.serve_packed_weights` and re-packed in place per parameter version."""
    def build(old):
        kind, l = name.split("/")[:2]
        model.comm.wait_unit(f"{kind}{l}")
        return hip.serve_pack_weight(model.W(name), hip.PACK_PLAIN, out=old)
    return model.serving_cache.get(("panel", name), None, build)


def siglip_fwd_serve(model: LAP, images: torch.Tensor):
    """The tower of `siglip.siglip_fwd` for the serving prefill: same operations and rounding points, fewer launches — GELU in fc1's
    epilogue (after the bf16 rounding of the Dense output), and fc2's split-K reduce, bias, residual add and the NEXT LayerNorm in
    one consumer pass (`lap_fused_reduce_norm`).  12 -> 10 launches per block, on block tiles sized for 512 rows
    (lap_gemm_bf16_ex serving rule)."""
    s, T = model.s, model.n_img_tok
    W = s.width
    hd = W // s.num_heads
    N = images.shape[0]
    pw = lambda name: panel_weight(model, name)
    x, _ = siglip_stem(model, images)
    scratch = hip._gemm_scratch(model.device)
    model.comm.wait_unit("img0")
    y, _, _ = hip.layernorm_fwd(x, model.F("img/0/ln1_g"), model.F("img/0/ln1_b"))
    rows = x.shape[0]
    mlp = model.W("img/0/w1").shape[0]
    panel = (model.serve_panel and rows <= 640 and hip.panel_gemm_ok(rows, 3 * W, W) and hip.panel_gemm_ok(rows, mlp, W)
             and hip.panel_gemm_ok(rows, W, mlp, 4))
    pf = pw if panel and model.serve_prefetch else (lambda name: None)   # the next launch's weights
    for l in range(s.depth):
        p = f"img/{l}/"
        if panel:    # us per launch at 512 rows, replayed graph (tools/probes/panel_bench.py): 11.6 -> 11.0, 9.0 -> 8.0, 14.5 -> 12.8, 14.9 -> 12.0
            qkv = hip.panel_linear(y, pw(p + "wqkv"), 3 * W, bias=model.F(p + "bqkv"), nt=model._panel_nt[0], prefetch=pf(p + "wo"))
        else:
            qkv = hip.linear_fwd(y, model.W(p + "wqkv"), bias=model.F(p + "bqkv"))
        (o, _), _ = hip.attention_fwd([qkv[:, :W]], [qkv[:, W:2 * W]], [qkv[:, 2 * W:]], [T], [T], N, s.num_heads, s.num_heads, hd,
                                      scale=hd ** -0.5, q_rs=(3 * W, 0), kv_rs=(3 * W, 0), need_lse=False)
        if panel:
            x1 = hip.panel_linear(o, pw(p + "wo"), W, bias=model.F(p + "bo"), residual=x, nt=model._panel_nt[1], prefetch=pf(p + "w1"))
        else:
            x1 = hip.linear_fwd(o, model.W(p + "wo"), bias=model.F(p + "bo"), residual=x)
        y2, _, _ = hip.layernorm_fwd(x1, model.F(p + "ln2_g"), model.F(p + "ln2_b"))
        if panel:
            a = hip.panel_linear(y2, pw(p + "w1"), mlp, bias=model.F(p + "b1"), gelu=model._panel_gelu, nt=model._panel_nt[2], prefetch=pf(p + "w2"))
            if l + 1 < s.depth:
                model.comm.wait_unit(f"img{l + 1}")
            part, ks = hip.panel_partials(a, pw(p + "w2"), W, scratch, 4, nt=model._panel_nt[3], prefetch=pf(f"img/{l + 1}/wqkv") if l + 1 < s.depth else None)
        else:
            a = hip.linear_fwd(y2, model.W(p + "w1"), bias=model.F(p + "b1"), gelu="bf16")
            part, ks = hip.linear_partials(a, model.W(p + "w2"), scratch)
        if l + 1 < s.depth:
            model.comm.wait_unit(f"img{l + 1}")
            g, b = model.F(f"img/{l + 1}/ln1_g"), model.F(f"img/{l + 1}/ln1_b")
        else:
            model.comm.wait_unit("img_head")
            g, b = model.F("img/norm_g"), model.F("img/norm_b")
        x, y = hip.fused_reduce_norm(part, ks, x1.shape[0], W, bias=model.F(p + "b2"), residual=x1, norm=2, gamma=g, beta=b)
    return hip.linear_fwd(y, model.W("img/head_w"), bias=model.F("img/head_b"))


def llm_prefill(model: LAP, x0, pos, qinfo, kinfo, B, n0, cache_out, kv_events=None):
    """The prefix-only pass of `joint_layers.llm_fwd` (x1 = None, nothing saved) for the serving prefill: K / V of every layer go to
    `cache_out`, the last layer's residual stream is returned.  Same operations and rounding points; the split-K projections
    leave f32 slabs and their consumers do the rest in one pass each — qkv: reduce + RoPE + head split (sin / cos of the
    prefix positions from one table for all layers), out / down: reduce + residual + the NEXT RMSNorm — 14 -> 10 launches
    per layer."""
    v = model.v
    NH, HD, KV = v.num_heads, v.head_dim, v.num_kv_heads
    Ttot = pos.shape[1]
    Dv = v.width
    pw = lambda name: panel_weight(model, name)
    scratch = hip._gemm_scratch(model.device)
    tab = hip.rope_table(pos, B, n0, Ttot, 0, HD)
    model.comm.wait_unit("llm0")
    h, _ = hip.rmsnorm_fwd(x0, scale=model.F("llm/0/n_attn"), save_rstd=False)
    rows = x0.shape[0]
    panel = (model.serve_panel and rows <= 640 and hip.panel_gemm_ok(rows, (NH + 2 * KV) * HD, Dv) and hip.panel_gemm_ok(rows, Dv, NH * HD))
    panel_q, panel_o = panel and "q" in model._panel_llm, panel and "o" in model._panel_llm
    pf = pw if panel_o and model.serve_prefetch else (lambda name: None)   # the next panel launch's weights
    for l in range(v.depth):
        p = f"llm/{l}/"
        if panel_q:   # one f32 slab, no K split (us, 560 rows: 23.5 -> 16.9 in front of the same consumer)
            part, ks = hip.panel_partials(h, pw(p + "wqkv0"), (NH + 2 * KV) * HD, scratch, 1, nt=2, prefetch=pf(p + "wo0"))
        else:
            part, ks = hip.linear_partials(h, model.W(p + "wqkv0"), scratch, ksplit=model._prefill_ks[0])
        q, k, vv = hip.fused_reduce_rope_split(part, ks, pos, B, n0, Ttot, 0, NH, HD, HD ** -0.5, table=tab)
        cache_out.append((k, vv))
        if kv_events is not None:     # layer l's K / V exist from here on: the first denoise step may use them (flow_sample)
            ev = torch.cuda.Event()
            ev.record()
            kv_events.append(ev)
        o, _ = hip.attention_fwd([q, None], [k, None], [vv, None], [n0, 0], [n0, 0], B, NH, KV, HD, qinfo, kinfo, need_lse=False)
        if panel_o:   # (16.2 -> 14.6)
            xa = hip.panel_linear(o[0], pw(p + "wo0"), Dv, residual=x0, nt=4)   # (the next panel launch is 200 MB of gate|up and down weights away)
            hf, _ = hip.rmsnorm_fwd(xa, scale=model.F(p + "n_ffw"), save_rstd=False)
        elif model._prefill_ks[1] > 1:
            part, ks = hip.linear_partials(o[0], model.W(p + "wo0"), scratch, ksplit=model._prefill_ks[1])
            xa, hf = hip.fused_reduce_norm(part, ks, rows, Dv, residual=x0, norm=1, gamma=model.F(p + "n_ffw"))
        else:   # (measured: the unsplit 64-row tile with the residual epilogue + a norm launch beats split + fused consumer here)
            xa = hip.linear_fwd(o[0], model.W(p + "wo0"), residual=x0)
            hf, _ = hip.rmsnorm_fwd(xa, scale=model.F(p + "n_ffw"), save_rstd=False)
        if rows <= 640 and (v.mlp_dim & 127) == 0:    # gate|up projection + GeGLU in one launch (the 320-row tile's paired epilogue)
            act = hip.linear_geglu(hf, model.W(p + "wgu0"), exp2=model._panel_gelu == "exp2")
        else:
            act = hip.geglu_fwd(hip.linear_fwd(hf, model.W(p + "wgu0")))
        part, ks = hip.linear_partials(act, model.W(p + "wd0"), scratch, ksplit=model._prefill_ks[2], tile=model._prefill_ks[3])
        if l + 1 < v.depth:
            model.comm.wait_unit(f"llm{l + 1}")
            x0, h = hip.fused_reduce_norm(part, ks, rows, Dv, residual=xa, norm=1, gamma=model.F(f"llm/{l + 1}/n_attn"))
        else:
            x0, h = hip.fused_reduce_norm(part, ks, rows, Dv, residual=xa, norm=0)
    return x0
