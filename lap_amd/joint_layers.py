"""The joint two-expert Gemma layers (gemma.py:455-531) of the train step and of the generic serving loops, as functions on the model.

The prefix stream (SigLIP tokens + prompt, width of the VLM) and the suffix stream (action tokens, width of the action expert) keep
separate activations and weights and meet only inside the attention kernel, which takes both as segments.  One layer, forward:

    qkv per stream          norm -> qkv projection (+ LoRA) -> RoPE / split; the suffix's on the second HIP stream
    hand-off                the compute stream waits for the suffix stream's q / k / v
    attention               both streams as two segments, on the compute stream
    hand-off                the suffix stream waits for its attention output
    suffix tail             out projection + residual -> norm -> gate | up -> GeGLU -> down + residual, on the second stream
    prefix tail             the same on the compute stream: the suffix's 8 short kernels run under these GEMMs

and the backward walks it in reverse (tails, hand-off, attention, hand-off, qkv).  The expert's tail exists once for its two variants:
pi0 (plain norms, the residual fused into the GEMM epilogue) and pi05 (adaRMS: modulation slots of `mod`, gated residuals); the
helpers `_suffix_norm*`, `_suffix_proj_res` and `_suffix_dproj` pick the variant.  The prefix tail holds the fp8 route, the fused
GeGLU routes, the padded gate | up rows and the last layer's row subset (`last_layer_rows`).  The streams are lap_amd/streams.py's.
"""
from __future__ import annotations

import contextlib
import os
from typing import NamedTuple

import torch

from lap_amd import hip
from lap_amd.streams import handoff, suffix_stream, unit_done


def mod_slot(model, mod, slot):
    W3 = 3 * model.e.width
    return mod[:, slot * W3:(slot + 1) * W3]


class LastRows:
    """The prefix rows the LAST joint layer keeps in a train step (`last_layer_rows`): those the language head reads."""

    def __init__(self, sel, qinfo, B, n0, Lt):
        dev, n_sel = sel.device, sel.shape[1]
        self.n_sel = n_sel
        idx = sel + (n0 - Lt)                                                       # [B, n_sel] prefix positions, the head's order
        self.rowid = (torch.arange(B, device=dev)[:, None] * n0 + idx).to(torch.int32).reshape(-1).contiguous()   # rows of x0
        self.inv = torch.full((B * n0,), -1, dtype=torch.int32, device=dev)         # row of x0 -> its compact row, or -1
        self.inv[self.rowid.long()] = torch.arange(B * n_sel, dtype=torch.int32, device=dev)
        # info words of the kept queries, then the suffix queries': class bits and ar index travel with the row, so every kept
        # row meets the keys under the mask it had
        self.qinfo = torch.cat([qinfo[:, :n0].gather(1, idx), qinfo[:, n0:]], 1).to(torch.int32).contiguous()


def last_layer_rows(model, lr, qinfo, B, n0, Lt, *, save, x1, collect, verbose):
    """The row subset of the last layer's prefix stream, or None: every row.  Nothing behind the last layer's K / V reads a
    prefix row but the language head, and it reads `lr.sel`'s rows only (16 of 560 per sample at the benchmark's shapes), so
    in a train step Q, the attention output, the out projection, the FFN and their backward run on those rows alone.
    Anything that looks at the layer's other rows (`collect`, the per-layer hooks, eval, serving) or runs products this
    path has no route for (fp8, LoRA) keeps all rows; so does a step without a row selection or with a frozen prefix."""
    if not (model.last_layer_rows and save and x1 is not None and collect is None and not verbose and lr is not None
            and lr.sel is not None and model.gemm_dtype == "bf16" and not model._prefix_frozen()):
        return None
    p = f"llm/{model.v.depth - 1}/"
    if any(model._lora(p + k) is not None for k in ("wqkv0", "wo0", "wgu0", "wd0")):
        return None
    return LastRows(lr.sel, qinfo, B, n0, Lt)


def rows_res_tile(model, x, name):
    """Tile request for the out / down projection (+ residual) of the last layer's row subset: 14, the assembly residual kernel
    the other layers' out / down products run on, where the library takes the shape (M a multiple of 256) and no A/B switch has
    the assembly routes off; else -1, the planner's choice.  Left to itself the planner's fill rule sends the 16 tiles of
    512 x 2048 to the HIP tiles: the step's out / down products would no longer all be the one kernel."""
    if os.environ.get("LAP_GEMM_NO_ASM") is not None or os.environ.get("LAP_GEMM_NO_ASM_RES") is not None or \
            os.environ.get("LAP_UNFUSED_RESIDUAL", "0") == "1":
        return -1
    w = model.W(name)
    ok = hip._lib.lap_gemm_asm_res_ok(0, x.shape[0], w.shape[0], x.shape[1], x.stride(0), w.stride(0), w.shape[0])
    return 14 if ok and x.stride(1) == 1 else -1


class StreamCtx(NamedTuple):
    """What one stream of a joint layer keeps for its backward."""
    x: torch.Tensor             # the layer's input (every row)
    h: torch.Tensor             # attention norm output, its 1 / rms
    rstd_a: torch.Tensor
    lt: dict                    # LoRA down products t per projection ("wqkv", "wo", "wgu", "wd"), None without adapters
    xa: torch.Tensor            # behind the attention residual
    hf: torch.Tensor            # FFN norm output, its 1 / rms
    rstd_f: torch.Tensor
    gu: torch.Tensor            # gate | up, GeGLU output
    act: torch.Tensor
    y: torch.Tensor = None      # adaRMS: the out / down products in front of their gates
    yf: torch.Tensor = None


class LayerCtx(NamedTuple):
    """What a joint layer keeps for its backward: the attention's operands as [prefix, suffix] segments, and each stream's own."""
    q: list
    k: list
    v: list
    o: list
    lse: torch.Tensor
    prefix: StreamCtx
    suffix: StreamCtx


# ---------------------------------------------------------------------------------------------------------------- forward, per stream
def _prefix_qkv(model, p, x0, pos, B, n0, Ttot, rows0, save, lt):
    v = model.v
    h, rstd = hip.rmsnorm_fwd(x0, scale=model.F(p + "n_attn"), save_rstd=save)
    qkv = model._lin0(h, p + "wqkv0")
    lt["wqkv"] = model._lora_fwd(h, qkv, p + "wqkv0")
    if rows0 is None:
        return (h, rstd), hip.rope_split_fwd(qkv, pos, B, n0, Ttot, 0, v.num_heads, v.head_dim, v.head_dim ** -0.5)
    # K / V of every row, Q of the kept rows
    return (h, rstd), hip.rope_split_fwd(qkv, pos, B, n0, Ttot, 0, v.num_heads, v.head_dim, v.head_dim ** -0.5, q_row=rows0.inv,
                                         q_rows=B * rows0.n_sel)


def _suffix_norm(model, x, name, mod, slot, n1, mld, save):
    """The expert's RMSNorm: pi0's plain scale (`use_adarms=[False, False]`, lap.py:51), or adaRMS from `mod`'s slot."""
    if mod is None:
        return hip.rmsnorm_fwd(x, scale=model.F(name), save_rstd=save)
    return hip.rmsnorm_fwd(x, mod=mod_slot(model, mod, slot), rows_per_sample=n1, save_rstd=save, mod_ld=mld)


def _suffix_proj_res(model, x, name, res, mod, slot, n1, mld):
    """res + x W^T (+ LoRA) of the expert's out / down projection -> (sum, LoRA t, the product in front of its gate or None).
    pi0: plain residuals (gemma.py:577-583 with gate None), fused into the GEMM; adaRMS: gated by the slot's third chunk."""
    if mod is None:
        y = hip.linear_fwd(x, model.W(name), residual=res)
        return y, model._lora_fwd(x, y, name), None
    y = hip.linear_fwd(x, model.W(name))
    t = model._lora_fwd(x, y, name)
    return hip.gated_residual_fwd(res, y, mod_slot(model, mod, slot)[:, 2 * model.e.width:], n1, mld), t, y


def _suffix_qkv(model, p, l, x1, mod, pos, B, n1, Ttot, mld, save, lt):
    v = model.v
    h, rstd = _suffix_norm(model, x1, p + "n_attn1", mod, 2 * l, n1, mld, save)
    qkv = hip.linear_fwd(h, model.W(p + "wqkv1"))
    lt["wqkv"] = model._lora_fwd(h, qkv, p + "wqkv1")
    return (h, rstd), hip.rope_split_fwd(qkv, pos, B, n1, Ttot, Ttot - n1, v.num_heads, v.head_dim, v.head_dim ** -0.5)


def _suffix_tail_fwd(model, p, l, x1, o1, mod, n1, mld, save, lt):
    """-> (what the backward keeps: `StreamCtx` from xa on, the layer's output)."""
    xa, lt["wo"], y = _suffix_proj_res(model, o1, p + "wo1", x1, mod, 2 * l, n1, mld)
    hf, rstd_f = _suffix_norm(model, xa, p + "n_ffw1", mod, 2 * l + 1, n1, mld, save)
    gu = hip.linear_fwd(hf, model.W(p + "wgu1"))
    lt["wgu"] = model._lora_fwd(hf, gu, p + "wgu1")
    act = hip.geglu_fwd(gu)
    xn, lt["wd"], yf = _suffix_proj_res(model, act, p + "wd1", xa, mod, 2 * l + 1, n1, mld)
    return (xa, hf, rstd_f, gu, act, y, yf), xn


def _prefix_tail_fwd(model, p, l, x0, o0, rows0, save, lt):
    """x0: the residual operand (the kept rows' under `rows0`).  -> (what the backward keeps: `StreamCtx` from xa on, the layer's output)."""
    xa = model._lin0(o0, p + "wo0", residual=x0, tile=-1 if rows0 is None else rows_res_tile(model, o0, p + "wo0"))
    lt["wo"] = model._lora_fwd(o0, xa, p + "wo0")
    hf, rstd_f = hip.rmsnorm_fwd(xa, scale=model.F(p + "n_ffw"), save_rstd=save)
    model.comm.pace(f"llm{l}")     # optimizer units released here start under the longest MFMA-bound GEMM of the layer
    if save and model.fuse_geglu_fwd and model._lora(p + "wgu0") is None and hip.linear_geglu_train_ok(hf, model.W(p + "wgu0")):
        # gate | up projection with the GeGLU in its epilogue: gu (kept for the backward pass) and act leave one launch
        gu, act = hip.linear_geglu_train(hf, model.W(p + "wgu0"))
    else:
        gu_out = None
        if save and model.fuse_geglu_bwd:    # rows padded like d(gate | up): the fused backward kernel shares one row stride
            gu_out = hip._padded_rows(hf.shape[0], 2 * model.v.mlp_dim, hf.device, hip._row_pad(2 * model.v.mlp_dim))
        gu = model._lin0(hf, p + "wgu0", out=gu_out)
        lt["wgu"] = model._lora_fwd(hf, gu, p + "wgu0")   # (before the GeGLU: lora.FeedForward's _dot)
        act = hip.geglu_fwd(gu, pad=model.gemm_dtype != "fp8")
    xn = model._lin0(act, p + "wd0", residual=xa, tile=-1 if rows0 is None else rows_res_tile(model, act, p + "wd0"))
    lt["wd"] = model._lora_fwd(act, xn, p + "wd0")
    return (xa, hf, rstd_f, gu, act), xn


def llm_fwd(model, x0, x1, mod, pos, qinfo, kinfo, B, n0, n1, save: bool, *, kv_cache=None, cache_out=None, collect=None,
            mod_shared: bool = False, layers=None, last_rows=None):
    """gemma.Module.__call__ layers (gemma.py:336-387,167-290).  x0 [B*n0, Dv] or None, x1 [B*n1, De] or None.
    kv_cache: per-layer (k, v) of the prefix used as key segment 0 when x0 is None (serving).
    last_rows (`last_layer_rows`): the last layer's prefix stream is compact behind K / V, and so is the x0 returned.
    Returns final pre-norm activations and the saved context."""
    v = model.v
    NH, HD, KV = v.num_heads, v.head_dim, v.num_kv_heads
    Ttot = pos.shape[1]
    ctx = [] if save else None
    mld = 0 if mod_shared else (mod.stride(0) if mod is not None else 0)  # 0: one modulation row for every sample
    sfx = suffix_stream(model, *([x1, mod] if mod is not None else [x1])) if (x0 is not None and x1 is not None) else None
    main = torch.cuda.current_stream() if sfx is not None else None
    on_sfx = (lambda: torch.cuda.stream(sfx)) if sfx is not None else contextlib.nullcontext
    if last_rows is not None and not (save and x0 is not None and x1 is not None and layers is None and collect is None):
        raise ValueError("llm_fwd: last_rows goes with a saved two-stream pass over all layers without `collect`")
    for l in (range(v.depth) if layers is None else layers):    # `layers`: test hook (teacher-forced per-layer parity)
        model.comm.wait_unit(f"llm{l}", also=sfx)
        p = f"llm/{l}/"
        rows0 = last_rows if l == v.depth - 1 else None
        q = [None, None]; k = [None, None]; vv = [None, None]
        pre = [None, None]; tail = [None, None]; xn = [None, None]    # per stream: (h, 1 / rms) of the attention norm, what its tail keeps
        lt = [{}, {}]       # LoRA down products t per stream and projection (kept for the backward)
        # ---- qkv per stream
        if x0 is not None:
            pre[0], (q[0], k[0], vv[0]) = _prefix_qkv(model, p, x0, pos, B, n0, Ttot, rows0, save, lt[0])
        elif kv_cache is not None:
            k[0], vv[0] = kv_cache[l]
        if x1 is not None:
            with on_sfx():
                pre[1], (q[1], k[1], vv[1]) = _suffix_qkv(model, p, l, x1, mod, pos, B, n1, Ttot, mld, save, lt[1])
            handoff(sfx, main, q[1], k[1], vv[1])
        if cache_out is not None:
            cache_out.append((k[0], vv[0]))
        # ---- attention
        qlen = [n0 if x0 is not None else 0, n1 if x1 is not None else 0]
        klen = [k[0].shape[0] // B if k[0] is not None else 0, n1 if x1 is not None else 0]
        xin = [x0, x1]
        if rows0 is not None:     # a query segment shorter than its key segment, as serving runs it against a cached prefix
            qlen[0] = rows0.n_sel
            x0 = hip.gather_rows_bf16(x0, rows0.rowid)      # the residual operand of the out projection, its only other reader
            model.last_rows_steps += 1
        o, lse = hip.attention_fwd(q, k, vv, qlen, klen, B, NH, KV, HD, qinfo if rows0 is None else rows0.qinfo, kinfo, need_lse=save)
        handoff(main, sfx, o[1])
        # ---- the tails: the suffix's issued first (8 short kernels that then run under the prefix stream's GEMMs)
        if x1 is not None:
            with on_sfx():
                tail[1], xn[1] = _suffix_tail_fwd(model, p, l, x1, o[1], mod, n1, mld, save, lt[1])
        if x0 is not None:
            tail[0], xn[0] = _prefix_tail_fwd(model, p, l, x0, o[0], rows0, save, lt[0])
        if save:
            ctx.append(LayerCtx(q, k, vv, o, lse, *(None if xin[i] is None else StreamCtx(xin[i], *pre[i], lt[i], *tail[i]) for i in (0, 1))))
        x0, x1 = xn
        if collect is not None:
            collect[f"llm/layer{l:02d}/x0"], collect[f"llm/layer{l:02d}/x1"] = x0, x1
    handoff(sfx, main, x1)
    return x0, x1, ctx


# ---------------------------------------------------------------------------------------------------------------- backward, per stream
def _suffix_dproj(model, dx1, y, mod, dmod, slot, n1, ldm):
    """Cotangent of the out / down projection's output under its residual: dx1 itself (pi0: xn = xa + y), or through the gate
    (adaRMS: xn = xa + y * gate; the gate's gradient goes into `dmod`'s slot)."""
    if mod is None:
        return dx1
    W2 = 2 * model.e.width
    return hip.gated_residual_bwd(dx1, y, mod_slot(model, mod, slot)[:, W2:], n1, ldm, mod_slot(model, dmod, slot)[:, W2:], dmod.stride(0))


def _suffix_norm_bwd(model, x, dy, rstd, name, mod, dmod, slot, n1, dx1):
    """Backward of `_suffix_norm`, added onto dx1 in place (the residual passes dx1 through)."""
    if mod is None:
        hip.rmsnorm_bwd(x, dy, rstd, scale=model.F(name), dx=dx1, dscale=model.G(name), accum_dx=True)
    else:
        hip.rmsnorm_bwd(x, dy, rstd, mod=mod_slot(model, mod, slot), rows_per_sample=n1, dx=dx1, dmod=mod_slot(model, dmod, slot),
                        accum_dx=True)


def _suffix_tail_bwd(model, p, l, s, o1, dx1, mod, dmod, n1, ldm):
    """FFN + attention output of the expert: xn = xa + yf [* gate_f], xa = x + y [* gate_a].  Updates dx1 in place -> d(o1)."""
    dyf = _suffix_dproj(model, dx1, s.yf, mod, dmod, 2 * l + 1, n1, ldm)
    model._wgrad(dyf, s.act, p + "wd1")
    dact = hip.linear_dgrad(dyf, model.W(p + "wd1"))
    model._lora_bwd(dyf, s.act, s.lt.get("wd"), dact, p + "wd1")
    dgu = hip.geglu_bwd(s.gu, dact)
    model._wgrad(dgu, s.hf, p + "wgu1")
    dhf = hip.linear_dgrad(dgu, model.W(p + "wgu1"))
    model._lora_bwd(dgu, s.hf, s.lt.get("wgu"), dhf, p + "wgu1")
    _suffix_norm_bwd(model, s.xa, dhf, s.rstd_f, p + "n_ffw1", mod, dmod, 2 * l + 1, n1, dx1)
    dy = _suffix_dproj(model, dx1, s.y, mod, dmod, 2 * l, n1, ldm)
    model._wgrad(dy, o1, p + "wo1")
    d_o1 = hip.linear_dgrad(dy, model.W(p + "wo1"))
    model._lora_bwd(dy, o1, s.lt.get("wo"), d_o1, p + "wo1")
    return d_o1


def _suffix_qkv_bwd(model, p, l, s, dq, dk, dv, dx1, mod, dmod, pos, B, n1, Ttot):
    v = model.v
    dqkv = hip.rope_split_bwd(dq, dk, dv, pos, B, n1, Ttot, Ttot - n1, v.num_heads, v.head_dim, v.head_dim ** -0.5)
    model._wgrad(dqkv, s.h, p + "wqkv1")
    dh = hip.linear_dgrad(dqkv, model.W(p + "wqkv1"))
    model._lora_bwd(dqkv, s.h, s.lt.get("wqkv"), dh, p + "wqkv1")
    _suffix_norm_bwd(model, s.x, dh, s.rstd_a, p + "n_attn1", mod, dmod, 2 * l, n1, dx1)


def _prefix_tail_bwd(model, p, s, o0, dx0):
    """FFN + attention output of the prefix stream: xn = xa + act @ wd^T, xa = x + o @ wo^T.  Updates dx0 in place -> d(o0)."""
    model._wgrad(dx0, s.act, p + "wd0")
    if model.fuse_geglu_bwd and model._lora(p + "wd0") is None and hip.dgrad_geglu_bwd_ok(dx0, model.W(p + "wd0"), s.gu):
        # the down projection's data gradient with the GeGLU backward as its epilogue: d(act) never reaches memory
        dgu = hip.linear_dgrad_geglu_bwd(dx0, model.W(p + "wd0"), s.gu)
    else:
        dact = model._dgrad0(dx0, p + "wd0")
        model._lora_bwd(dx0, s.act, s.lt.get("wd"), dact, p + "wd0")
        dgu = hip.geglu_bwd(s.gu, dact, pad=model.gemm_dtype != "fp8")
        del dact
    model._wgrad(dgu, s.hf, p + "wgu0")
    dhf = model._dgrad0(dgu, p + "wgu0")
    model._lora_bwd(dgu, s.hf, s.lt.get("wgu"), dhf, p + "wgu0")
    del dgu
    model.wg.join(dx0)   # (the down projection's weight gradient reads dx0)
    hip.rmsnorm_bwd(s.xa, dhf, s.rstd_f, scale=model.F(p + "n_ffw"), dx=dx0, dscale=model.G(p + "n_ffw"), accum_dx=True)
    del dhf
    model._wgrad(dx0, o0, p + "wo0")
    d_o0 = model._dgrad0(dx0, p + "wo0")
    model._lora_bwd(dx0, o0, s.lt.get("wo"), d_o0, p + "wo0")
    return d_o0


def _prefix_qkv_bwd(model, p, s, dq, dk, dv, dx0, pos, B, n0, Ttot, rows0):
    """-> dx0 of the layer's input: updated in place, or, under `rows0`, a new tensor with every row."""
    v = model.v
    dqkv = hip.rope_split_bwd(dq, dk, dv, pos, B, n0, Ttot, 0, v.num_heads, v.head_dim, v.head_dim ** -0.5,
                              q_row=None if rows0 is None else rows0.inv)      # (compact dq: zeros in the other rows' q columns)
    model._wgrad(dqkv, s.h, p + "wqkv0")
    dh = model._dgrad0(dqkv, p + "wqkv0")
    model._lora_bwd(dqkv, s.h, s.lt.get("wqkv"), dh, p + "wqkv0")
    if rows0 is None:
        model.wg.join(dx0)   # (the out projection's reads dx0)
        hip.rmsnorm_bwd(s.x, dh, s.rstd_a, scale=model.F(p + "n_attn"), dx=dx0, dscale=model.G(p + "n_attn"), accum_dx=True)
        return dx0
    # all rows from here on: the norm's backward of every row, the compact residual cotangent added at its rows
    return hip.rmsnorm_bwd(s.x, dh, s.rstd_a, scale=model.F(p + "n_attn"), dscale=model.G(p + "n_attn"), add_row=rows0.inv, addend=dx0)


def llm_bwd(model, ctx, dx0, dx1, mod, dmod, pos, qinfo, kinfo, B, n0, n1, last_rows=None):
    """last_rows: as in `llm_fwd` — dx0 arrives with the kept rows only and leaves the last layer with all of them.
    dx0 is None: the whole prefix side is frozen; dx1 is None: prefix-only backward (enable_action_training=False, lap.py:449-455)."""
    v = model.v
    NH, HD, KV = v.num_heads, v.head_dim, v.num_kv_heads
    Ttot = pos.shape[1]
    has_sfx = dx1 is not None
    ada = has_sfx and mod is not None  # False with a suffix stream: pi0 (plain norms and residuals in the expert)
    if not ada:
        mod = dmod = None
    ldm = mod.stride(0) if ada else 0
    zero_do0 = None
    sfx = suffix_stream(model, *([dx1, dmod, mod] if ada else [dx1]))
    main = torch.cuda.current_stream() if sfx is not None else None
    on_sfx = (lambda: torch.cuda.stream(sfx)) if sfx is not None else contextlib.nullcontext
    for l in reversed(range(v.depth)):
        p = f"llm/{l}/"
        c = ctx[l]
        d_o = [None, None]
        rows0 = last_rows if l == v.depth - 1 else None
        # ---- the tails (the suffix's on the second HIP stream, see the module doc)
        if has_sfx:
            with on_sfx():
                d_o[1] = _suffix_tail_bwd(model, p, l, c.suffix, c.o[1], dx1, mod, dmod, n1, ldm)
        if dx0 is not None:
            d_o[0] = _prefix_tail_bwd(model, p, c.prefix, c.o[0], dx0)
        else:   # the attention backward still needs a dO for the prefix queries: zero (their dq / dk / dv are discarded)
            if zero_do0 is None:
                zero_do0 = torch.zeros_like(c.o[0])
            d_o[0] = zero_do0
        # ---- attention
        handoff(sfx, main, d_o[1])
        dq, dk, dv = hip.attention_bwd(c.q, c.k, c.v, c.o, d_o, c.lse, [n0 if rows0 is None else rows0.n_sel, n1], [n0, n1],
                                       B, NH, KV, HD, qinfo if rows0 is None else rows0.qinfo, kinfo,
                                       stop_q1_to_k0=model.config.stop_action_to_vlm_grad)
        handoff(main, sfx, dq[1], dk[1], dv[1])
        # ---- qkv per stream
        if has_sfx:
            with on_sfx():
                _suffix_qkv_bwd(model, p, l, c.suffix, dq[1], dk[1], dv[1], dx1, mod, dmod, pos, B, n1, Ttot)
        if dx0 is not None:
            dx0 = _prefix_qkv_bwd(model, p, c.prefix, dq[0], dk[0], dv[0], dx0, pos, B, n0, Ttot, rows0)
        ctx[l] = None
        unit_done(model, f"llm{l}", sfx)   # complete once both streams are through: the optimizer's stream waits for both, the
                                           # compute stream goes on (it meets the second stream again at the next attention)
    handoff(sfx, main)
    return dx0, dx1
