"""The SigLIP training tower (openpi siglip, restated in siglip_gemma3.py:382-545 minus :432, plus head bias): forward with the saved
context, hand-written backward.  Functions on the model; the serving prefill's tower on fused consumers is prefill.siglip_fwd_serve
(it shares `siglip_stem`).  Weight and bias gradients leave the data-gradient path for the third stream (lap_amd/streams.py)."""
from __future__ import annotations

import os
from typing import NamedTuple

import torch

from lap_amd import hip
from lap_amd.streams import unit_done


class BlockCtx(NamedTuple):
    """What one encoder block keeps for its backward."""
    x: torch.Tensor         # block input
    y: torch.Tensor         # LN1 output, its statistics
    mean1: torch.Tensor
    rstd1: torch.Tensor
    qkv: torch.Tensor
    o: torch.Tensor         # attention output, its log-sum-exp
    lse: torch.Tensor
    x1: torch.Tensor        # behind the attention residual
    y2: torch.Tensor        # LN2 output, its statistics
    mean2: torch.Tensor
    rstd2: torch.Tensor
    h: torch.Tensor         # fc1 output, GELU output
    a: torch.Tensor


def siglip_fwd(model, images: torch.Tensor, save: bool, collect=None, x_in=None, blocks=None):
    """images f32 [N,H,W,3] -> tokens bf16 [N*T, Dv].  openpi siglip (missing) restated in
    siglip_gemma3.py:382-545 minus :432, plus head bias.
    Test hook (teacher-forced per-block parity): with `x_in` (bf16 [N*T, W]) the stem is skipped, only `blocks` run
    and the block output is returned instead of the projected tokens."""
    s, T = model.s, model.n_img_tok
    W = s.width
    hd = W // s.num_heads
    ctx = {"blocks": []} if save else None
    if x_in is not None:
        x, N = x_in, x_in.shape[0] // T
        for l in blocks:
            x = siglip_block(model, l, x, N, T, W, hd, None, False)
        return x, None
    N = images.shape[0]
    x, patches = siglip_stem(model, images)
    if collect is not None:
        collect["img/stem"] = x
    if save:
        ctx["patches"] = patches
    for l in range(s.depth):
        x = siglip_block(model, l, x, N, T, W, hd, ctx, save)
        if collect is not None:
            collect[f"img/block{l:02d}"] = x
    model.comm.wait_unit("img_head")
    enc, mean, rstd = hip.layernorm_fwd(x, model.F("img/norm_g"), model.F("img/norm_b"))
    tok = hip.linear_fwd(enc, model.W("img/head_w"), bias=model.F("img/head_b"))
    if save:
        ctx["final"] = (x, enc, mean, rstd)
    if collect is not None:
        collect["img/out"] = tok
    return tok, ctx


def siglip_stem(model, images: torch.Tensor):
    """f32 stem (siglip_gemma3.py:398-408) on the MFMA path -> (x bf16 [N*T, W], the (hi, lo) patches its weight gradient reads):
    x = hi + lo (2 x bf16, 16 mantissa bits), products exact in the f32 accumulator, the lo.lo term (2^-18 relative) dropped."""
    p_hi, p_lo = hip.split_f32_hilo(hip.im2col_patch(images.contiguous(), model.s.patch))
    w_hi, w_lo = hip.split_f32_hilo(model.F("img/stem_w"))
    (R, Kp), W = p_hi.shape, model.s.width
    stem = torch.empty((R, W), dtype=torch.float32, device=p_hi.device)
    hip.gemm(p_hi, w_hi, stem, M=R, N=W, K=Kp, lda=Kp, ldb=Kp, ldc=W, bias=model.F("img/stem_b"))
    hip.gemm(p_hi, w_lo, stem, M=R, N=W, K=Kp, lda=Kp, ldb=Kp, ldc=W, accum=True)
    hip.gemm(p_lo, w_hi, stem, M=R, N=W, K=Kp, lda=Kp, ldb=Kp, ldc=W, accum=True)
    return hip.add_posemb_cast(stem, model.F("img/pos"), model.n_img_tok), (p_hi, p_lo)


def siglip_block(model, l, x, N, T, W, hd, ctx, save):
    """One pre-LN encoder block (siglip_gemma3.py:59-167): x + MHA(LN(x)), then + MLP(LN(.))."""
    s = model.s
    model.comm.wait_unit(f"img{l}")
    p = f"img/{l}/"
    y, mean1, rstd1 = hip.layernorm_fwd(x, model.F(p + "ln1_g"), model.F(p + "ln1_b"))
    qkv = hip.linear_fwd(y, model.W(p + "wqkv"), bias=model.F(p + "bqkv"))
    (o, _), lse = hip.attention_fwd([qkv[:, :W]], [qkv[:, W:2 * W]], [qkv[:, 2 * W:]], [T], [T], N, s.num_heads, s.num_heads, hd,
                                    scale=hd ** -0.5, q_rs=(3 * W, 0), kv_rs=(3 * W, 0), need_lse=save)
    x1 = hip.linear_fwd(o, model.W(p + "wo"), bias=model.F(p + "bo"), residual=x)
    y2, mean2, rstd2 = hip.layernorm_fwd(x1, model.F(p + "ln2_g"), model.F(p + "ln2_b"))
    model.comm.pace(f"img{l}")
    if save:
        if model.fuse_gelu and hip.linear_bias_gelu_train_ok(y2, model.W(p + "w1"), model.F(p + "b1")):
            h, a = hip.linear_bias_gelu_train(y2, model.W(p + "w1"), model.F(p + "b1"))     # fc1 + bias with the GELU in its epilogue
        else:
            h = hip.linear_fwd(y2, model.W(p + "w1"), bias=model.F(p + "b1"))
            a = hip.gelu_fwd(h)
    else:   # nothing keeps the pre-activation: GELU in the GEMM epilogue, after the bf16 rounding of the Dense output (same bits)
        h, a = None, hip.linear_fwd(y2, model.W(p + "w1"), bias=model.F(p + "b1"), gelu="bf16")
    x2 = hip.linear_fwd(a, model.W(p + "w2"), bias=model.F(p + "b2"), residual=x1)
    if save:
        ctx["blocks"].append(BlockCtx(x, y, mean1, rstd1, qkv, o, lse, x1, y2, mean2, rstd2, h, a))
    return x2


def siglip_bwd(model, ctx, dtok: torch.Tensor):
    s, T = model.s, model.n_img_tok
    W = s.width
    hd = W // s.num_heads
    x, enc, mean, rstd = ctx["final"]
    N = x.shape[0] // T
    model._bgrad(dtok, "img/head_b")
    model._wgrad(dtok, enc, "img/head_w")
    denc = hip.linear_dgrad(dtok, model.W("img/head_w"))
    unit_done(model, "img_head")
    # Bias gradients = column sums of a dy.  Two of a block's four (fc2's and the out projection's) come out of the LayerNorm
    # backward that PRODUCES that dy instead of a pass of their own over 38 MB (+1.8 us in that kernel against a 15.5 us
    # column-sum launch; a GELU backward that sums its columns was 2.3 x slower than the two kernels it replaced).
    fuse_b = os.environ.get("LAP_FUSE_BGRAD", "1") != "0"
    last = s.depth - 1
    dx = hip.layernorm_bwd(x, denc, model.F("img/norm_g"), mean, rstd, model.G("img/norm_g"), model.G("img/norm_b"),
                           dxsum=model.G(f"img/{last}/b2") if fuse_b else None)
    for l in reversed(range(s.depth)):
        p = f"img/{l}/"
        c = ctx["blocks"][l]
        if not fuse_b:
            model._bgrad(dx, p + "b2")
        model._wgrad(dx, c.a, p + "w2")
        if model.fuse_gelu and hip.dgrad_gelu_bwd_ok(dx, model.W(p + "w2"), c.h):
            dh = hip.linear_dgrad_gelu_bwd(dx, model.W(p + "w2"), c.h)      # fc2's data gradient with the GELU backward as its epilogue
        else:
            da = hip.linear_dgrad(dx, model.W(p + "w2"))
            dh = hip.gelu_bwd(c.h, da)
            del da
        model._bgrad(dh, p + "b1")
        model._wgrad(dh, c.y2, p + "w1")
        dy2 = hip.linear_dgrad(dh, model.W(p + "w1"))
        del dh
        model.wg.join(dx)    # (the fc2 weight / bias gradients read dx)
        hip.layernorm_bwd(c.x1, dy2, model.F(p + "ln2_g"), c.mean2, c.rstd2, model.G(p + "ln2_g"), model.G(p + "ln2_b"), dx=dx, accum_dx=True,
                          dxsum=model.G(p + "bo") if fuse_b else None)
        if not fuse_b:
            model._bgrad(dx, p + "bo")
        model._wgrad(dx, c.o, p + "wo")
        do = hip.linear_dgrad(dx, model.W(p + "wo"))
        dqkv = torch.empty_like(c.qkv)
        hip.attention_bwd([c.qkv[:, :W]], [c.qkv[:, W:2 * W]], [c.qkv[:, 2 * W:]], [c.o], [do], c.lse, [T], [T], N, s.num_heads, s.num_heads, hd,
                          scale=hd ** -0.5, q_rs=(3 * W, 0), kv_rs=(3 * W, 0),
                          dq_out=[dqkv[:, :W]], dk_out=[dqkv[:, W:2 * W]], dv_out=[dqkv[:, 2 * W:]])
        model._bgrad(dqkv, p + "bqkv")
        model._wgrad(dqkv, c.y, p + "wqkv")
        dy = hip.linear_dgrad(dqkv, model.W(p + "wqkv"))
        model.wg.join(dx)    # (the out-projection's read dx)
        hip.layernorm_bwd(c.x, dy, model.F(p + "ln1_g"), c.mean1, c.rstd1, model.G(p + "ln1_g"), model.G(p + "ln1_b"), dx=dx, accum_dx=True,
                          dxsum=model.G(f"img/{l - 1}/b2") if (fuse_b and l > 0) else None)
        ctx["blocks"][l] = None
        unit_done(model, f"img{l}")
    dstem = hip.add_posemb_cast_bwd(dx, model.G("img/pos"), T)     # f32 copy of a bf16 gradient: exact in bf16
    p_hi, p_lo = ctx["patches"]
    gw = model.G("img/stem_w")
    tmp = torch.empty((gw.shape[0], p_hi.shape[1]), dtype=torch.float32, device=gw.device)   # [W, 592]
    hip.linear_wgrad(dx, p_hi, tmp)
    hip.linear_wgrad(dx, p_lo, tmp, accum=True)
    gw.add_(tmp[:, :gw.shape[1]])
    hip.colsum(dstem, model.G("img/stem_b"))
