"""The loss heads of `LAP._loss_impl` (lap.py:209-301, 472-566): the language head (row selection, final norm, chunked cross
entropy over the f32 table as two bf16 planes, and its backward), the action head, and the per-sample weight mixing of VQA /
prediction / language-action samples.  `_loss_impl` keeps the schedule: streams, collectives and the hand-off to `joint_layers.llm_bwd`.
The weights are read through the model (`W`, `F`, `G`, `ps`); `mix_sample_weights` is plain torch and runs on any device.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from lap_amd import hip
from lap_amd.config import VQA_DATASET_ID_MAP
from lap_amd.joint_layers import mod_slot


def vocab_chunks(R: int, V: int, cap_cols: int | None = None) -> list[tuple[int, int]]:
    """(v0, vc) column ranges of the [R, V] logits.  One chunk while [R, vc] bf16 (the cotangent planes) stays below the 2 GiB
    buffer-descriptor range of the GEMM (B <= 32 at the LAP-3B shapes); 1024-column granularity.  `cap_cols`: test hook."""
    if cap_cols is None:
        cap_cols = max(1024, (int(1.5e9) // (2 * R)) // 1024 * 1024)
    return [(v0, min(cap_cols, V - v0)) for v0 in range(0, V, cap_cols)]


def lm_logits(model, pl, v0: int, vc: int, out=None):
    """Embedder.decode (gemma.py:153-154) on table rows v0 .. v0+vc: the bf16 pre-logits times the F32 table.  table = hi + lo,
    two bf16 planes (16 mantissa bits; the products are exact in the f32 accumulator) -> logits to ~2^-17 of the f32 product."""
    R, Dv = pl.shape
    if out is None:
        out = torch.empty((R, vc), dtype=torch.float32, device=pl.device)
    hip.gemm(pl, model.W("llm/embed")[v0:v0 + vc], out, M=R, N=vc, K=Dv, lda=Dv, ldb=Dv, ldc=vc)
    hip.gemm(pl, model.ps.w16lo("llm/embed")[v0:v0 + vc], out, M=R, N=vc, K=Dv, lda=Dv, ldb=Dv, ldc=vc, accum=True)
    return out


# ---- language head (lap.py:209-289): rows Pn-Lt .. Pn-2 predict tokens 1 .. Lt-1
class LangHead(NamedTuple):
    """The language loss, and what its backward reads.  With the language loss off: zeros and nothing else."""
    lang_loss: torch.Tensor             # [B] per-sample mean cross entropy over the loss mask
    lm: torch.Tensor = None             # [B, Lt-1] loss mask, f32
    lm_s: torch.Tensor = None           # [B, Ls] the same on the selected rows
    cnt: torch.Tensor = None            # [B] max(sum(lm), 1)
    sel: torch.Tensor = None            # [B, Ls] selected rows in 0 .. Lt-2, or None: all rows
    rowid: torch.Tensor = None          # [B, Ls] their rows in xf0 (with `sel`)
    rows: torch.Tensor = None           # [R, Dv] the head's input rows
    pl: torch.Tensor = None             # [R, Dv] pre-logits (final norm of `rows`)
    rstd_pl: torch.Tensor = None
    targets: torch.Tensor = None        # [R] int32
    m: torch.Tensor = None              # [R] running max / sum of the softmax
    lsum: torch.Tensor = None
    chunks: list = None                 # vocab_chunks(R, V)
    logit_chunks: list = None           # f32 logits per chunk (kept for the backward)
    Lt: int = 0
    verbose_metrics: dict = {}
    compact: bool = False               # `rows` IS the prefix stream's output (the last layer ran on the selected rows only)


class LossRows(NamedTuple):
    """Which rows the language head reads (`select_loss_rows`): chosen once per step, before the joint layers, so that the last
    layer's prefix stream can run on these rows alone (joint_layers.llm_fwd `last_rows`)."""
    lm: torch.Tensor                    # [B, Lt-1] loss mask, f32
    cnt: torch.Tensor                   # [B] max(sum(lm), 1)
    sel: torch.Tensor = None            # [B, Ls] selected rows in 0 .. Lt-2 (masked rows first, stable order, padded), or None: all
    hint_too_small: torch.Tensor = None  # 0-d bool (with `sel`)
    cls_masks: list = None              # verbose: the class masks on rows 0 .. Lt-2


def select_loss_rows(model, obs, observation, *, verbose: bool) -> LossRows:
    """`obs`: the preprocessed observation; `observation`: the caller's (its row hints win over the derived ones)."""
    dev = model.device
    Lt = obs.tokenized_prompt.shape[1]
    loss_mask = obs.tokenized_langact_mask[:, 1:] & obs.tokenized_prompt_mask[:, 1:]
    if obs.token_loss_mask is not None:
        loss_mask = loss_mask & obs.token_loss_mask[:, 1:]
    lm_bool = loss_mask if obs.sample_mask is None else loss_mask & obs.sample_mask[:, None]
    lm = lm_bool.to(torch.float32)
    cnt = torch.clamp(lm.sum(-1), min=1.0)
    # Only rows whose loss mask is set matter (the reference multiplies the other rows' cross entropy by 0): with the host
    # hint `loss_rows_max` the head runs on that many rows per sample — the masked ones first (stable order), padded with
    # rows of weight 0 — instead of all Lt - 1 (BASELINE shapes: 16 of 47).  A hint smaller than a sample's count would drop
    # tokens silently, so the device-side check turns the loss into NaN instead (no host sync).
    n_sel = observation.loss_rows_max if observation.loss_rows_max is not None else obs.loss_rows_max
    # verbose (lap.py:240-277): the class masks lie inside the reasoning mask but not inside token_loss_mask (reasoning
    # dropout), so the rows are chosen by loss mask | class masks and the hint is `metric_rows_max`, counted over that union
    # (no hint: all Lt - 1 rows).  The loss still weighs the rows by `lm` alone.
    row_mask = lm_bool
    if verbose:
        def prep(mk):       # prepare_mask, lap.py:241-247
            if mk is None:
                return None
            mk = mk[:, 1:].to(dev, torch.bool)
            return (mk & obs.sample_mask[:, None] if obs.sample_mask is not None else mk).contiguous()

        cls_masks = [prep(obs.critical_token_mask), prep(obs.number_token_mask), prep(obs.direction_token_mask)]
        for mk in cls_masks:
            if mk is not None:
                row_mask = row_mask | mk
        n_sel = observation.metric_rows_max if observation.metric_rows_max is not None else obs.metric_rows_max
    sel = hint_too_small = None
    if n_sel is not None and 0 < n_sel < Lt - 1:
        sel = torch.sort((~row_mask).to(torch.uint8), dim=1, stable=True).indices[:, :n_sel]          # [B, n_sel] in 0 .. Lt-2
        hint_too_small = ((row_mask.sum(-1) if verbose else lm.sum(-1)) > n_sel).any()
    return LossRows(lm, cnt, sel, hint_too_small, cls_masks if verbose else None)


def lang_head_fwd(model, xf0, obs, lr: LossRows, B, Pn, *, backward: bool, verbose: bool, collect, compact: bool = False) -> LangHead:
    """`lr`: select_loss_rows' choice.  `compact`: xf0 holds exactly the selected rows, [B * Ls, Dv] in `lr.sel`'s order (the last
    layer's row-subset path); else xf0 is the whole prefix stream [B * Pn, Dv] and the rows are gathered from it."""
    dev = model.device
    Dv, V = model.v.width, model.config.vocab_size
    Lt = obs.tokenized_prompt.shape[1]
    lm, cnt, sel, hint_too_small, cls_masks = lr
    rowid = None
    if sel is not None:
        Ls = sel.shape[1]
        rowid = (torch.arange(B, device=dev) * Pn + (Pn - Lt))[:, None] + sel
        rows = xf0 if compact else xf0.index_select(0, rowid.view(-1))
        targets = obs.tokenized_prompt[:, 1:].gather(1, sel).to(torch.int32).contiguous().view(-1)
        lm_s = lm.gather(1, sel)
    else:
        if compact:
            raise ValueError("lang_head_fwd: compact rows need a row selection")
        Ls = Lt - 1
        rows = torch.empty((B * Ls, Dv), dtype=torch.bfloat16, device=dev)
        hip.copy_rows_bf16(xf0, rows, B * Ls, Ls, Dv, Pn, Pn - Lt, Ls, 0)
        targets = obs.tokenized_prompt[:, 1:].to(torch.int32).contiguous().view(-1)
        lm_s = lm
    R = B * Ls
    pl, rstd_pl = hip.rmsnorm_fwd(rows, scale=model.F("llm/final_norm"), save_rstd=backward)
    chunks = vocab_chunks(R, V)
    m = torch.full((R,), -3.0e38, dtype=torch.float32, device=dev)
    lsum = torch.zeros(R, dtype=torch.float32, device=dev); tl = torch.zeros(R, dtype=torch.float32, device=dev)
    amax = torch.empty(R, dtype=torch.int32, device=dev) if verbose else None      # predictions from the same pass
    logit_chunks = []
    for v0, vc in chunks:
        lg = lm_logits(model, pl, v0, vc)
        if verbose:
            hip.ce_chunk_update_argmax(lg, targets, m, lsum, tl, amax, v0)
        else:
            hip.ce_chunk_update(lg, targets, m, lsum, tl, v0)
        logit_chunks.append(lg if backward else None)
    nll = (m + torch.log(lsum) - tl).view(B, Ls)
    lang_loss = (nll * lm_s).sum(-1) / cnt
    if sel is not None:
        lang_loss = torch.where(hint_too_small, torch.full_like(lang_loss, float("nan")), lang_loss)
    verbose_metrics = {}
    if verbose:
        verbose_metrics = _token_metrics(model, amax, targets, nll, lm, sel, cls_masks, obs.tokenized_prompt[:, 1:])
        if collect is not None:
            collect["predictions"], collect["sel"] = amax.view(B, Ls), sel
    return LangHead(lang_loss, lm, lm_s, cnt, sel, rowid, rows, pl, rstd_pl, targets, m, lsum, chunks, logit_chunks, Lt, verbose_metrics,
                    compact)


def _token_metrics(model, amax, targets, nll, lm, sel, cls_masks, labels):
    """compute_token_accuracy_metrics (metrics.py:7-45) from the LM head's argmax: per-token loss and per-sample (correct, total)
    counts in one kernel (lap_token_metrics); the batch accuracies from the counts' totals, all-reduced in one collective so that
    under FSDP they are the global values the reference computes."""
    crit, num, dirn = cls_masks
    ptl, counts = hip.token_metrics(amax, targets, nll.reshape(-1).contiguous(), lm.contiguous(),
                                    sel=sel.to(torch.int32).contiguous() if sel is not None else None,
                                    critical=crit, number=num, direction=dirn)
    tot = model.comm.all_reduce_sum(counts.sum(0).reshape(8)).view(4, 2)
    acc = tot[:, 0] / torch.clamp(tot[:, 1], min=1.0)
    out = {"token_accuracy": acc[0], "per_token_loss": ptl, "labels": labels}
    for k, (name, mk) in enumerate((("critical", crit), ("number", num), ("direction", dirn)), start=1):
        if mk is not None:
            out[f"{name}_token_accuracy"] = acc[k]
            out[f"per_sample_{name}_correct"] = counts[:, k, 0]
            out[f"per_sample_{name}_total"] = counts[:, k, 1]
    return out


def lang_head_bwd(model, head: LangHead, wl, n_active, B, Pn):
    """dlogits = w * (softmax - onehot); w = d loss / d nll.  The cotangent of the f32 logits stays f32 in the reference
    (d pre_logits = dlogits . table, d table = dlogits^T . pre_logits in f32): dlogits = dh + dl (two bf16 planes),
    table = hi + lo -> dh.hi + dl.hi + dh.lo (dl.lo is 2^-16 of the sum) and (dh + dl)^T . pre_logits.
    The planes are stacked along the rows, [dh; dl]: ONE weight-gradient product over 2R rows against [pl; pl] (the f32 [V, D]
    output is written once instead of accumulated onto), ONE data-gradient product [dh; dl] . hi (the table plane is read
    once), plus dh . lo onto its first half.  Returns dx0 [B*Pn, Dv]: zeros but for the head's rows — or, for a `compact` head, the
    cotangent of its rows alone [B*Ls, Dv]."""
    dev = model.device
    R, Dv = head.pl.shape
    w = (wl[:, None] * head.lm_s / head.cnt[:, None] / n_active).contiguous().view(-1)
    pl2 = torch.cat([head.pl, head.pl], 0)
    dpl32 = torch.empty((2 * R, Dv), dtype=torch.float32, device=dev)
    table16, table_lo, gE = model.W("llm/embed"), model.ps.w16lo("llm/embed"), model.G("llm/embed")
    for ci, (v0, vc) in enumerate(head.chunks):
        dlogits = torch.empty((2 * R, vc), dtype=torch.bfloat16, device=dev)
        hip.ce_chunk_grad(head.logit_chunks[ci], head.targets, head.m, head.lsum, w, dlogits[:R], v0, dlogits_lo=dlogits[R:])
        head.logit_chunks[ci] = None
        if model.ps.is_trainable("llm/embed"):
            hip.linear_wgrad(dlogits, pl2, gE[v0:v0 + vc])
        hip.linear_dgrad(dlogits, table16[v0:v0 + vc], out=dpl32, accum=ci > 0)
        hip.linear_dgrad(dlogits[:R], table_lo[v0:v0 + vc], out=dpl32[:R], accum=True)
        del dlogits
    dpl = hip.cast_f32_to_bf16(dpl32[:R] + dpl32[R:])
    drows = hip.rmsnorm_bwd(head.rows, dpl, head.rstd_pl, scale=model.F("llm/final_norm"), dscale=model.G("llm/final_norm"))
    if head.compact:
        return drows
    dx0 = torch.zeros((B * Pn, Dv), dtype=torch.bfloat16, device=dev)
    if head.sel is not None:
        dx0.index_copy_(0, head.rowid.view(-1), drows)
    else:
        hip.copy_rows_bf16(drows, dx0, R, head.Lt - 1, Dv, head.Lt - 1, 0, Pn, Pn - head.Lt)
    return dx0


# ---- action head (lap.py:291-301)
class ActionHead(NamedTuple):
    pre1: torch.Tensor = None           # [B*S, We] bf16 final norm of the action rows
    pre1f: torch.Tensor = None          # the same in f32 (input of action_out_proj)
    rstd_p1: torch.Tensor = None
    v_t: torch.Tensor = None            # [B*S, ad]


def action_head_fwd(model, xf1, mod, B, S, Sx, *, backward: bool) -> ActionHead:
    We = model.e.width
    if model.config.pi05:
        pre1, rstd_p1 = hip.rmsnorm_fwd(xf1, mod=mod_slot(model, mod, 2 * model.v.depth), rows_per_sample=S, save_rstd=backward)
    else:       # plain final norm; the action head reads the last S rows of each sample (`suffix_out[:, -ah:]`, lap.py:298)
        pre1_all, rstd_p1 = hip.rmsnorm_fwd(xf1, scale=model.F("llm/final_norm1"), save_rstd=backward)
        pre1 = pre1_all.view(B, Sx, We)[:, 1:].reshape(B * S, We).contiguous()
    pre1f = hip.cast_bf16_to_f32(pre1)
    return ActionHead(pre1, pre1f, rstd_p1, model._lin32(pre1f, "act/out_w", "act/out_b"))


def action_head_bwd(model, head: ActionHead, xf1, mod, dv, B, S, Sx):
    """Returns (dx1, dmod): dmod (pi05) is the f32 cotangent of every modulation slot, zero but for the final norm's."""
    dev, We = model.device, model.e.width
    dpre1f = model._lin32_bwd(head.pre1f, dv.view(B * S, -1), "act/out_w", "act/out_b")
    if model.config.pi05:
        dmod = torch.zeros(mod.shape, dtype=torch.float32, device=dev)
        dx1 = hip.rmsnorm_bwd(xf1, hip.cast_f32_to_bf16(dpre1f), head.rstd_p1, mod=mod_slot(model, mod, 2 * model.v.depth), rows_per_sample=S,
                              dmod=mod_slot(model, dmod, 2 * model.v.depth))
        return dx1, dmod
    dall = torch.zeros((B, Sx, We), dtype=torch.bfloat16, device=dev)      # (the state token's row of the final norm has no consumer)
    dall[:, 1:] = hip.cast_f32_to_bf16(dpre1f).view(B, S, We)
    return hip.rmsnorm_bwd(xf1, dall.view(B * Sx, We), head.rstd_p1, scale=model.F("llm/final_norm1"), dscale=model.G("llm/final_norm1")), None


# ---- combination (lap.py:472-566)
class Mix(NamedTuple):
    wl: torch.Tensor            # [B] f32 weight of every sample's language loss
    act_mask: torch.Tensor      # [B] bool: samples that carry the action loss
    mixing: bool                # per-kind weights and metrics are on
    extra_metrics: dict


class KindMasks(NamedTuple):
    sm: torch.Tensor            # [B] bool sample mask (all ones without one)
    vqa_m: torch.Tensor         # [B] bool active VQA / prediction / language-action samples (with `mixing`, else None)
    pred_m: torch.Tensor
    lang_m: torch.Tensor
    act_mask: torch.Tensor      # [B] bool: samples that carry the action loss
    mixing: bool


def sample_kind_masks(cfg, B: int, dev, sample_mask, is_vqa, is_pred, *, lang_on: bool) -> KindMasks:
    """The sample masks of the loss (lap.py:400-409,480-486,557-566) from the batch's flags alone: what `mix_sample_weights`
    weighs by and what the loss divides by (`global_denominators`)."""
    sm = sample_mask.to(dev, torch.bool) if sample_mask is not None else torch.ones(B, dtype=torch.bool, device=dev)
    vqa = is_vqa.to(dev, torch.bool) if is_vqa is not None else None
    pred = is_pred.to(dev, torch.bool) if is_pred is not None else None
    if not (lang_on and (cfg.enable_vqa_training or cfg.enable_prediction_training)):
        # (also the langact-off branch: the VQA / prediction masks reach the action loss as they came, lap.py:557-566)
        act_mask = torch.ones(B, dtype=torch.bool, device=dev)
        if vqa is not None:
            act_mask = act_mask & ~vqa
        if pred is not None:
            act_mask = act_mask & ~pred
        return KindMasks(sm, None, None, None, act_mask, False)
    vqa_m = (vqa if vqa is not None else torch.zeros(B, dtype=torch.bool, device=dev)) & sm      # lap.py:480-486
    pred_m = (pred if pred is not None else torch.zeros(B, dtype=torch.bool, device=dev)) & sm
    lang_m = ~((vqa if vqa is not None else vqa_m) | (pred if pred is not None else pred_m)) & sm
    act_mask = ~vqa_m & ~pred_m          # the masks were AND-ed with the sample mask before this point (lap.py:484-485,562-566)
    return KindMasks(sm, vqa_m, pred_m, lang_m, act_mask, True)


def global_denominators(cfg, observations, comm=None, device=None):
    """(n_active, n_action) of the K micro-batches `observations` taken together, as `LAP._loss_impl` counts them for one batch:
    active samples (the batch size without a sample mask) and samples that carry the action loss, each summed over the
    micro-batches and — one `comm.all_reduce_sum` for both — over the ranks, then clamped to >= 1.  f32 device scalars; n_action is
    None without action training.  Passed as `denominators=` to every micro-step, they make the micro-steps' losses and gradients
    sum to those of the whole batch."""
    lang_on, act_on = cfg.enable_langact_training, cfg.enable_action_training
    dev = torch.device(device) if device is not None else observations[0].tokenized_prompt.device
    tot = torch.zeros(2, dtype=torch.float32, device=dev)
    for obs in observations:
        B = obs.tokenized_prompt.shape[0]
        km = sample_kind_masks(cfg, B, dev, obs.sample_mask, obs.is_vqa_sample if cfg.enable_vqa_training else None,
                               obs.is_prediction_sample if cfg.enable_prediction_training else None, lang_on=lang_on)
        tot = tot + torch.stack([km.sm.to(torch.float32).sum(), km.act_mask.to(torch.float32).sum()])
    if comm is not None:
        tot = comm.all_reduce_sum(tot)
    tot = torch.clamp(tot, min=1.0)
    return tot[0], (tot[1] if act_on else None)


def mix_sample_weights(cfg, lang_loss, sample_mask, is_vqa, is_pred, vqa_dataset_id, *, lang_on: bool) -> Mix:
    """Per-sample weights: language loss x {language, VQA (optionally per dataset), prediction} weight by sample kind; action loss
    only on samples that are neither VQA nor prediction samples.  `is_vqa` / `is_pred` are the reference's `vqa_mask` /
    `pred_mask` (lap.py:400-409): None unless that kind of training is on and the observation marks its samples."""
    dev, B = lang_loss.device, lang_loss.shape[0]
    fb = lambda t: t.to(torch.float32)
    km = sample_kind_masks(cfg, B, dev, sample_mask, is_vqa, is_pred, lang_on=lang_on)
    sm, vqa_m, pred_m, lang_m, act_mask = km.sm, km.vqa_m, km.pred_m, km.lang_m, km.act_mask
    if not km.mixing:
        wl = torch.full((B,), cfg.language_loss_weight if lang_on else 0.0, dtype=torch.float32, device=dev)
        return Mix(wl, act_mask, False, {})
    extra_metrics = {}
    vqa_w = torch.full((B,), cfg.vqa_loss_weight, dtype=torch.float32, device=dev)               # lap.py:526-543
    if cfg.enable_vqa_training and cfg.vqa_loss_weights and vqa_dataset_id is not None:
        ids = vqa_dataset_id.to(dev)
        for name, wgt in cfg.vqa_loss_weights.items():
            if name in VQA_DATASET_ID_MAP:
                vqa_w = torch.where(ids == VQA_DATASET_ID_MAP[name], torch.full_like(vqa_w, float(wgt)), vqa_w)
    wl = vqa_w * fb(vqa_m) + cfg.prediction_loss_weight * fb(pred_m) + cfg.language_loss_weight * fb(lang_m)
    n_act_loc = fb(sm).sum()
    for pfx, msk in (("vqa_", vqa_m), ("pred_", pred_m), ("langact_", lang_m)):   # metrics.py:49-56 (per-rank values)
        if (pfx == "vqa_" and not cfg.enable_vqa_training) or (pfx == "pred_" and not cfg.enable_prediction_training):
            continue
        extra_metrics[pfx + "loss"] = (lang_loss * fb(msk)).sum() / torch.clamp(fb(msk).sum(), min=1.0)
        extra_metrics[pfx + "num_samples"] = fb(msk).sum()
        extra_metrics[pfx + "sample_portion"] = fb(msk).sum() / torch.clamp(n_act_loc, min=1.0)
    if cfg.enable_vqa_training and vqa_dataset_id is not None:
        # metrics.py:59-73 (lap.py:500-508): loss and sample count per VQA dataset, one [B, K] indicator for all K datasets
        names = list(VQA_DATASET_ID_MAP)
        idv = torch.tensor([VQA_DATASET_ID_MAP[n] for n in names], dtype=torch.int64, device=dev)
        ind = fb((vqa_dataset_id.to(dev).to(torch.int64).view(B, 1) == idv.view(1, -1)) & vqa_m.view(B, 1))
        ns = ind.sum(0)
        ls = (lang_loss.view(1, B) @ ind).view(-1) / torch.clamp(ns, min=1.0)
        for k, n in enumerate(names):
            extra_metrics[f"vqa_{n}_loss"] = ls[k]
            extra_metrics[f"vqa_{n}_num_samples"] = ns[k]
    extra_metrics["active_num_samples"] = n_act_loc
    extra_metrics["active_sample_portion"] = n_act_loc / max(B, 1)
    return Mix(wl, act_mask, True, extra_metrics)
