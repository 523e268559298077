"""LAP_AR token decoding (lap.py:678-766) behind `LAP.sample_tokens` and `LAP.score_tokens`: the request checks, the VLM-only
prefill, the eager decode step on generic launches, the eager and the fused drivers, and the routing between them.  The fused step
and its device-side state are `decode_ctx.DecodeCtx` (the single-token kernels of csrc/decode*.hip), which the fused drivers here
and `serve.GraphedTokenDecoder` (`prefill` + `DecodeCtx.first_token` and `DecodeCtx.step` captured into two graphs) sequence.
The weights are read through the model (`W`, `F`, `_dec_fp8`), as `LAP._serving_weights` presents them.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import torch

from lap_amd import hip, prefill as serving_prefill
from lap_amd.decode_ctx import DecodeCtx, check_decode_weights
from lap_amd.grammar import check_grammar
from lap_amd.joint_layers import llm_fwd
from lap_amd.loss import lm_logits
from lap_amd.model import LAP, _gen
from lap_amd.observation import preprocess_observation
from lap_amd.score import check_score_args
from lap_amd.speculate import check_jump_forward, check_speculate

DECODE_STEPS_PER_CHECK = 8      # fused steps between two host reads of the device stop flag (eager `decode="fused"`)


def check_fused_decode(model: LAP, B: int):
    if model.comm.world_size != 1:
        raise ValueError("fused decode is a serving path: replicas only (world_size 1)")
    if not model.decode_supported(B):
        v = model.v
        raise ValueError(f"fused decode serves the Gemma-2B widths at 1 <= B <= 8 (D 2048, 8 / 1 heads of 256, MLP 16384); got "
                         f"B {B}, D {v.width}, heads {v.num_heads} / {v.num_kv_heads} of {v.head_dim}, MLP {v.mlp_dim}")


def check_allowed_tokens(ids, vocab_size: int, eos_token: int) -> torch.Tensor:
    """The allowed set of a constrained decode as the kernels take it: sorted unique int32 ids (on the CPU) from any integer
    sequence or tensor; duplicates and order are normalised.  ValueError for an empty set, a non-integer dtype, an id outside
    [0, vocab_size), or a set without the EOS token when that token is in the vocabulary (such a request could only end at its
    budget)."""
    if not isinstance(ids, torch.Tensor) and not hasattr(ids, "__array__"):
        ids = list(ids)
    t = torch.as_tensor(ids).detach().cpu()
    if t.numel() == 0:
        raise ValueError("allowed_tokens: the set is empty")
    if t.dtype == torch.bool or t.is_floating_point() or t.is_complex():
        raise ValueError(f"allowed_tokens: expected integer ids, got {t.dtype}")
    t = t.reshape(-1).to(torch.int64)
    lo, hi = int(t.min()), int(t.max())
    if lo < 0 or hi >= vocab_size:
        raise ValueError(f"allowed_tokens: ids must lie in [0, {vocab_size}), got {lo if lo < 0 else hi}")
    t = torch.unique(t)     # (sorted)
    if 0 <= eos_token < vocab_size and not bool((t == eos_token).any()):
        raise ValueError(f"allowed_tokens: the EOS token {eos_token} is not in the set, so no request could stop before its budget")
    return t.to(torch.int32)


class AllowedSet(NamedTuple):
    """A checked allowed set on the model's device, with what it was checked against (`allowed_set`)."""
    ids: torch.Tensor               # sorted unique int32 ids
    vocab_size: int
    eos_token: int


def allowed_set(model: LAP, allowed_tokens) -> AllowedSet:
    """`check_allowed_tokens` for `model`, once: an AllowedSet that was checked against this model's vocabulary, EOS token and
    device is handed back as it is, so a server normalises its set at start-up and not per request."""
    V, eos = model.config.vocab_size, model.EOS_TOKEN
    if isinstance(allowed_tokens, AllowedSet):
        if (allowed_tokens.vocab_size, allowed_tokens.eos_token) == (V, eos) and allowed_tokens.ids.device.type == model.device.type:
            return allowed_tokens
        allowed_tokens = allowed_tokens.ids
    return AllowedSet(check_allowed_tokens(allowed_tokens, V, eos).to(model.device), V, eos)


MAX_NUM_SAMPLES = 8     # best-of-N decodes its candidates as the rows of one fused batch (B <= 8)


def check_num_samples(num_samples, batch: int, *, decode: str, sampler: str, temperature: float) -> int:
    """`num_samples` of a best-of-N request as an int; ValueError naming the condition it breaks."""
    if isinstance(num_samples, bool) or int(num_samples) != num_samples:
        raise ValueError(f"num_samples must be an integer, got {num_samples!r}")
    N = int(num_samples)
    if not 1 <= N <= MAX_NUM_SAMPLES:
        raise ValueError(f"num_samples must lie in [1, {MAX_NUM_SAMPLES}] (the candidates are the rows of one fused batch), got {N}")
    if batch != 1:
        raise ValueError(f"num_samples needs an observation of batch 1 (its prefix is prefilled once), got batch {batch}")
    if decode != "fused":
        raise ValueError(f"num_samples needs decode=\"fused\" (the candidates decode as one fused batch), got decode={decode!r}")
    if sampler != "device":
        raise ValueError(f"num_samples needs sampler=\"device\" (row b draws with Philox row index b), got sampler={sampler!r}")
    if not temperature > 0.0:
        raise ValueError(f"num_samples needs temperature > 0 (greedy candidates are all the same), got {temperature!r}")
    return N


def check_filter(top_k, top_p, *, sampler: str, temperature: float):
    """(top_k, top_p) of a filtered request as the kernels take them, or None when both are neutral or the decode is greedy (the
    argmax is always kept); ValueError naming the value, or the sampler: the filters are on the device sampler only."""
    from lap_amd.sampling import check_filter as check_values

    k, p = check_values(top_k, top_p)
    if top_k is None and top_p is None:
        return None
    if sampler != "device" and temperature > 0.0:
        raise ValueError(f"top_k / top_p need sampler=\"device\" (the filters are part of the device sampler), got sampler={sampler!r}")
    if (k == 0 and p >= 1.0) or not temperature > 0.0:
        return None
    return k, p


def _on_device(t: torch.Tensor, device) -> bool:
    """Whether tensor `t` lives on `device`, index included ("cuda" names the current device)."""
    dev = torch.device(device)
    if t.device.type != dev.type:
        return False
    if dev.type != "cuda":
        return True
    return t.device.index == (torch.cuda.current_device() if dev.index is None else dev.index)


def grammar_on_device(model: LAP, grammar, host):
    """The automaton `grammar`, whose host form `check_grammar` returned as `host`, on the model's device: a DeviceAutomaton that
    is already there is handed back as it is, so a server copies its automaton at start-up and not per request; anything else is
    copied from `host` without a second `check_automaton`."""
    from lap_amd.grammar import DeviceAutomaton

    if isinstance(grammar, DeviceAutomaton) and _on_device(grammar.ids, model.device):
        return grammar
    return host.to_device(model.device, check=False)


def device_grammar(model: LAP, grammar, **combined):
    """`check_grammar` for `model` (one `check_automaton` of a host automaton), then `grammar_on_device`."""
    return grammar_on_device(model, grammar, check_grammar(grammar, model.config.vocab_size, model.EOS_TOKEN, **combined))


def sample_tokens(model: LAP, rng, observation, *, max_decoding_steps: int = 390, temperature: float = 0.0, collect=None,
                  decode: str = "eager", sampler: str = "host", decode_weights: str = "bf16", allowed_tokens=None,
                  return_logprobs: bool = False, num_samples=None, top_k=None, top_p=None, speculate=None, draft_tokens=None,
                  grammar=None, jump_forward=None, num_beams=None, early_stop: bool = True):
    """`LAP.sample_tokens` (documented there): every argument is checked before any device work."""
    if decode not in ("eager", "fused"):
        raise ValueError(f"sample_tokens: decode must be 'eager' or 'fused', got {decode!r}")
    if num_beams is not None:
        return _sample_beams(model, observation, num_beams, early_stop, max_decoding_steps=max_decoding_steps, temperature=temperature,
                             collect=collect, decode=decode, sampler=sampler, decode_weights=decode_weights, allowed_tokens=allowed_tokens,
                             return_logprobs=return_logprobs, num_samples=num_samples, top_k=top_k, top_p=top_p, speculate=speculate,
                             draft_tokens=draft_tokens, grammar=grammar, jump_forward=jump_forward)
    grammar_host = None
    if grammar is not None:
        grammar_host = check_grammar(grammar, model.config.vocab_size, model.EOS_TOKEN, allowed_tokens=allowed_tokens, top_k=top_k,
                                     top_p=top_p, speculate=speculate, sampler=sampler, temperature=temperature)
    S = None
    if speculate is not None:
        S = check_speculate(speculate, observation.tokenized_prompt.shape[0], decode=decode, temperature=temperature,
                            return_logprobs=return_logprobs, num_samples=num_samples, top_k=top_k, top_p=top_p, collect=collect)
    elif draft_tokens is not None and jump_forward is None:
        raise ValueError("sample_tokens: draft_tokens needs speculate=S")
    J = None
    if jump_forward is not None:
        J = check_jump_forward(jump_forward, observation.tokenized_prompt.shape[0], grammar=grammar, decode=decode, sampler=sampler,
                               temperature=temperature, num_samples=num_samples, collect=collect)
    check_decode_weights(decode_weights)
    if decode_weights != "bf16" and decode != "fused":
        raise ValueError(f"sample_tokens: decode_weights={decode_weights!r} runs on the fused decode kernels only: pass decode=\"fused\"")
    if sampler not in ("host", "device"):
        raise ValueError(f"sample_tokens: sampler must be 'host' or 'device', got {sampler!r}")
    filt = check_filter(top_k, top_p, sampler=sampler, temperature=temperature)
    N = None
    if num_samples is not None:
        N = check_num_samples(num_samples, observation.tokenized_prompt.shape[0], decode=decode, sampler=sampler, temperature=temperature)
    if decode == "fused":
        check_fused_decode(model, N or observation.tokenized_prompt.shape[0])
    if sampler == "device":
        hip.sampling_words(rng, temperature)        # (rejects a temperature whose inverse is not finite before any work)
    allowed = None
    if allowed_tokens is not None:
        allowed = allowed_set(model, allowed_tokens).ids
    if grammar is not None:
        grammar = grammar_on_device(model, grammar, grammar_host)
    with model._serving_weights():
        if decode == "fused" and (sampler == "device" or temperature <= 0.0):   # (the host sampler's noise cannot run on the device state)
            return _sample_fused(model, observation, max_decoding_steps=max_decoding_steps, collect=collect,
                                 sampling=(rng, temperature) if sampler == "device" else None, weights=decode_weights,
                                 allowed=allowed, logprobs=return_logprobs or N is not None, num_samples=N, filt=filt,
                                 speculate=S, draft=draft_tokens, grammar=grammar, jump=J)
        if decode_weights != "bf16":
            raise ValueError("sample_tokens: decode_weights other than 'bf16' with temperature > 0 needs sampler='device' (the "
                             "host sampler keeps the eager loop)")
        return _sample_eager(model, rng, observation, max_decoding_steps=max_decoding_steps, temperature=temperature, collect=collect,
                             device_sampler=sampler == "device", allowed=allowed, logprobs=return_logprobs, filt=filt, grammar=grammar)


def _sample_beams(model: LAP, observation, num_beams, early_stop, *, max_decoding_steps, temperature, collect, decode, sampler,
                  decode_weights, allowed_tokens, return_logprobs, num_samples, top_k, top_p, speculate, draft_tokens, grammar, jump_forward):
    """`sample_tokens(num_beams=N)`: the checks, then the fused or the eager beam decode; the rank-0 beam as [1, cap] tokens (and
    its token log-probabilities)."""
    from lap_amd.beam import check_num_beams

    N = check_num_beams(num_beams, observation.tokenized_prompt.shape[0], decode=decode, temperature=temperature, sampler=sampler,
                        num_samples=num_samples, top_k=top_k, top_p=top_p, speculate=speculate, grammar=grammar, jump_forward=jump_forward,
                        collect=collect)
    if draft_tokens is not None:
        raise ValueError("sample_tokens: draft_tokens needs speculate=S")
    grammar_host = None
    if grammar is not None:
        grammar_host = check_grammar(grammar, model.config.vocab_size, model.EOS_TOKEN, allowed_tokens=allowed_tokens)
    check_decode_weights(decode_weights)
    if decode_weights != "bf16" and decode != "fused":
        raise ValueError(f"sample_tokens: decode_weights={decode_weights!r} runs on the fused decode kernels only: pass decode=\"fused\"")
    if max_decoding_steps < 1:
        raise ValueError(f"sample_tokens: num_beams needs max_decoding_steps >= 1, got {max_decoding_steps}")
    if decode == "fused":
        check_fused_decode(model, N)
    allowed = allowed_set(model, allowed_tokens).ids if allowed_tokens is not None else None
    if grammar is not None:
        grammar = grammar_on_device(model, grammar, grammar_host)
    with model._serving_weights():
        if decode == "fused":
            tokens, logp, _ = beam_decode_fused(model, observation, N, max_decoding_steps=max_decoding_steps, early_stop=early_stop,
                                                weights=decode_weights, allowed=allowed, grammar=grammar)
        else:
            tokens, logp, _ = beam_decode_eager(model, observation, N, max_decoding_steps=max_decoding_steps, early_stop=early_stop,
                                                allowed=allowed, grammar=grammar)
    return (tokens[:1].contiguous(), logp[:1].contiguous()) if return_logprobs else tokens[:1].contiguous()


class Prefill(NamedTuple):
    """What the VLM-only prefill leaves for the decode steps."""
    B: int
    Pn: int
    cache: list                     # prefix K/V per layer
    kinfo_prefix: torch.Tensor      # [B, Pn]
    qinfo_d: torch.Tensor           # qinfo of the decode query
    plen: torch.Tensor              # [B] prefill_len
    x_last: torch.Tensor            # [B, D] the last valid residual row of every sample


def prefill(model: LAP, observation) -> Prefill:
    """The VLM-only prefill of sample_tokens (lap.py:693-716)."""
    cfg = model.config
    dev = model.device
    if model.comm.world_size != 1:
        raise NotImplementedError("sample_tokens is a serving path: replicas only (SURVEY.md §8e)")
    model.comm.wait_unit("small")
    obs = preprocess_observation(observation, train=False, image_keys=cfg.image_keys, image_resolution=cfg.image_resolution)
    B = obs.tokenized_prompt.shape[0]
    x0, Pn, _ = model._embed_prefix(obs, False, tower=serving_prefill.siglip_fwd_serve)
    qinfo_p, kinfo_p, ppos = model._serve_infos(obs, 1)[:3]
    prefix_mask, _ = model._prefix_masks(obs)
    ar = torch.arange(Pn, device=dev)
    seqlen = (prefix_mask.to(torch.int64) * ar).max(-1).values + 1          # left_to_right_align's roll amount
    plen = prefix_mask.sum(-1)                                               # prefill_len
    in_range = (ar[None] >= (seqlen - plen)[:, None]) & (ar[None] < seqlen[:, None])
    kinfo_prefix = (in_range.to(torch.int32) << 24).contiguous()
    qinfo_d = torch.full((B, 1), (1 << 24) | 0xFFFFFF, dtype=torch.int32, device=dev)
    cache = []
    if model.serve_fusions and model.gemm_dtype == "bf16":
        xf0 = serving_prefill.llm_prefill(model, x0, ppos, qinfo_p, kinfo_p, B, Pn, cache)
    else:
        xf0, _, _ = llm_fwd(model, x0, None, None, ppos, qinfo_p, kinfo_p, B, Pn, 0, False, cache_out=cache)
    last = (torch.arange(B, device=dev) * Pn + seqlen - 1)
    return Prefill(B, Pn, cache, kinfo_prefix, qinfo_d, plen, xf0.index_select(0, last).contiguous())


def replicate_prefill(pre: Prefill, N: int) -> Prefill:
    """The batch-1 prefill `pre` as N identical rows (best-of-N): plain copies of the prefix K / V of every layer, the key-info
    words, the prefill length and the last residual row, from which the LM head forms every row's first-token logits."""
    if pre.B != 1:
        raise ValueError(f"replicate_prefill: a prefill of batch 1, got {pre.B}")

    def rep(t):
        return t.repeat((N,) + (1,) * (t.dim() - 1))

    return Prefill(N, pre.Pn, [(rep(k), rep(v)) for k, v in pre.cache], rep(pre.kinfo_prefix), rep(pre.qinfo_d), rep(pre.plen),
                   rep(pre.x_last))


# ---- the eager step: generic launches
def _vlm_decode_step(model: LAP, token, pos, step, cache, gen, qinfo_d, kinfo_prefix, B, Pn):
    """One expert-0 decode step (lap.py:734-752): embed the sampled token, run the 18 VLM layers on that single row
    per sample with keys = [prefilled prefix cache | generated tokens incl. this one], return f32 logits [B, V].
    The reference appends into a fixed-size cache by index (gemma.py:597-605); here the generated keys are a second
    key segment that grows by one row per step."""
    v = model.v
    NH, HD, KV, Dv = v.num_heads, v.head_dim, v.num_kv_heads, v.width
    dev = model.device
    x = torch.empty((B, Dv), dtype=torch.bfloat16, device=dev)
    rows, lo, hi = model.ps.embed_rows()
    hip.embed_gather(rows, token.view(B, 1).contiguous(), x, B, 1, Dv, 1, 0, math.sqrt(Dv), lo, hi)
    kinfo = torch.cat([kinfo_prefix, torch.full((B, step + 1), 1 << 24, dtype=torch.int32, device=dev)], 1).contiguous()
    for l in range(v.depth):
        p = f"llm/{l}/"
        h, _ = hip.rmsnorm_fwd(x, scale=model.F(p + "n_attn"), save_rstd=False)
        qkv = hip.linear_fwd(h, model.W(p + "wqkv0"))
        q, k, vv = hip.rope_split_fwd(qkv, pos, B, 1, 1, 0, NH, HD, HD ** -0.5)
        gk, gv = gen[l]
        gk = k.view(B, 1, -1) if gk is None else torch.cat([gk, k.view(B, 1, -1)], 1)
        gv = vv.view(B, 1, -1) if gv is None else torch.cat([gv, vv.view(B, 1, -1)], 1)
        gen[l] = (gk, gv)
        ck, cv = cache[l]
        o, _ = hip.attention_fwd([None, q], [ck, gk.view(B * (step + 1), -1)], [cv, gv.view(B * (step + 1), -1)], [0, 1],
                                 [Pn, step + 1], B, NH, KV, HD, qinfo_d, kinfo, need_lse=False)
        xa = hip.linear_fwd(o[1], model.W(p + "wo0"), residual=x)
        hf, _ = hip.rmsnorm_fwd(xa, scale=model.F(p + "n_ffw"), save_rstd=False)
        act = hip.geglu_fwd(hip.linear_fwd(hf, model.W(p + "wgu0")))
        x = hip.linear_fwd(act, model.W(p + "wd0"), residual=xa)
    return _lm_logits(model, x)


def _lm_logits(model: LAP, rows):
    """final norm + Embedder.decode (gemma.py:153-154, 525-527): f32 logits [R, V]."""
    pl, _ = hip.rmsnorm_fwd(rows, scale=model.F("llm/final_norm"), save_rstd=False)
    return lm_logits(model, pl, 0, model.config.vocab_size)      # the f32 table as hi + lo, as in the training loss


def _grammar_mask(g, q, V: int):
    """bool [B, V]: the ids the state q[b] (int64 device [B]) of the device automaton `g` allows, per row."""
    counts = g.offsets[1:] - g.offsets[:-1]
    edge_state = torch.repeat_interleave(torch.arange(counts.numel(), device=q.device), counts.long())
    rows, cols = (edge_state[None, :] == q[:, None]).nonzero(as_tuple=True)
    mask = torch.zeros((q.numel(), V), dtype=torch.bool, device=q.device)
    mask[rows, g.ids[cols].long()] = True
    return mask


def _grammar_step(g, q, token):
    """The states after `token` [B]: a binary search (`torch.searchsorted`) for the token in the segment of q[b].  A segment's
    ids ascend and the segments follow in state order, so (state, id) ascends over the whole edge array; the search of
    (q[b], token[b]) in it lands inside the segment of q[b]."""
    lo, hi = g.offsets[q].long(), g.offsets[q + 1].long()
    counts = (g.offsets[1:] - g.offsets[:-1]).long()
    V = int(g.host.vocab_size)
    key = torch.repeat_interleave(torch.arange(counts.numel(), device=q.device), counts) * V + g.ids.long()
    pos = torch.searchsorted(key, q * V + token.long()).clamp_(max=key.numel() - 1)
    ok = (pos >= lo) & (pos < hi) & (g.ids[pos].long() == token.long())
    return torch.where(ok, g.next[pos].long(), q)       # (a token outside the segment: only from a row of -inf; the state stays)


def _outside_mask(model: LAP, allowed):
    """bool [V]: the ids outside the allowed set (int32 device ids), which the eager routes fill with -inf; None without a set."""
    if allowed is None:
        return None
    outside = torch.ones((model.config.vocab_size,), dtype=torch.bool, device=model.device)
    outside[allowed.long()] = False
    return outside


def _sample_eager(model: LAP, rng, observation, *, max_decoding_steps: int, temperature: float, collect, device_sampler: bool,
                  allowed=None, logprobs: bool = False, filt=None, grammar=None):
    """grammar: a DeviceAutomaton; the mask of every row's state is built with torch ops, the draw is the unconstrained one on the
    masked logits, the transition a `torch.searchsorted` (slow and simple: the second implementation beside the fused route).
    allowed: int32 device ids; the logits outside the set are -inf before the argmax or the noise.  logprobs: also the f32
    log_softmax of logits * inv_t (over the allowed set) at every token, returned beside the tokens: over all candidates, also
    when filt = (top_k, top_p) narrows the draw (lap_filter_gumbel_argmax_rows_f32)."""
    dev = model.device
    B, Pn, cache, kinfo_prefix, qinfo_d, plen, x_last = prefill(model, observation)
    logits = _lm_logits(model, x_last)                                      # decodes the first token (lap.py:716)
    out = torch.zeros((B, max_decoding_steps), dtype=torch.int32, device=dev)
    eos = torch.zeros((B,), dtype=torch.bool, device=dev)
    logp = torch.zeros((B, max_decoding_steps), dtype=torch.float32, device=dev) if logprobs else None
    inv_t = float(hip.sampling_words(0, temperature)[2]) if logprobs else 0.0      # float32(1 / temperature); 0: greedy, scored at tau = 1
    gen = [(None, None)] * model.v.depth
    g = _gen(rng, dev) if temperature > 0.0 and not device_sampler else None
    outside = _outside_mask(model, allowed)
    gq = torch.zeros((B,), dtype=torch.int64, device=dev) if grammar is not None else None
    step = 0
    while step < max_decoding_steps:
        if outside is not None:
            logits = logits.masked_fill(outside, float("-inf"))
        if gq is not None:
            logits = logits.masked_fill(~_grammar_mask(grammar, gq, model.config.vocab_size), float("-inf"))
        raw = logits
        if device_sampler and temperature > 0.0:      # one pass over the raw logits, no [B, V] temporaries
            if filt is not None:
                token = hip.filter_gumbel_argmax_rows(logits, temperature, rng, step, *filt)
            else:
                token = hip.gumbel_argmax_rows(logits, temperature, rng, step)
        else:
            if temperature > 0.0:
                u = torch.rand(logits.shape, generator=g, device=dev, dtype=torch.float32).clamp_(1e-20, 1.0)
                logits = logits / temperature - torch.log(-torch.log(u))
            token = hip.argmax_rows(logits)
        if collect is not None:
            collect[f"logit/{step}"] = logits.clone()
        out[:, step] = token
        if gq is not None:
            gq = _grammar_step(grammar, gq, token)
        if logp is not None:
            z = raw * inv_t if inv_t != 0.0 else raw
            logp[:, step] = torch.log_softmax(z, dim=-1).gather(1, token.view(B, 1).long()).view(B)
        eos |= token == model.EOS_TOKEN
        step += 1
        if step >= max_decoding_steps or bool(eos.all()):   # lap.py:754-756 loop condition (the unused last decode is skipped)
            break
        pos = (plen + (step - 1)).to(torch.int32).view(B, 1).contiguous()
        logits = _vlm_decode_step(model, token, pos, step - 1, cache, gen, qinfo_d, kinfo_prefix, B, Pn)
    return (out, logp) if logprobs else out


def beam_decode_eager(model: LAP, observation, N: int, *, max_decoding_steps: int, early_stop: bool = True, allowed=None, on_step=None,
                      grammar=None):
    """Beam search on the eager step, the second implementation beside `beam_decode_fused` (call it under `_serving_weights`): the
    batch-1 prefill replicated to N rows, per-step f32 logits from the generic launches, `beam.beam_step` on the host in float64,
    `index_select` by parent on the generated K / V.  allowed: int32 device ids.  on_step: `beam.beam_search`'s hook.
    grammar: a DeviceAutomaton (not with allowed): every row is masked to its state's set and stepped by `beam.grammar_beam_step`
    on the host (`beam.grammar_beam_search`; on_step then also receives the states before the step).
    Returns (tokens int32 [N, cap], logp f32 [N, cap], scores f32 [N]) on the device, in rank order."""
    import numpy as np

    from lap_amd import beam as bm

    dev = model.device
    B, Pn, cache, kinfo_prefix, qinfo_d, plen, x_last = replicate_prefill(prefill(model, observation), N)
    outside = _outside_mask(model, allowed)
    gen = [(None, None)] * model.v.depth
    state = {"gen": gen}

    def logits_fn(prefixes):
        t = prefixes.shape[1]
        if t == 0:
            lg = _lm_logits(model, x_last)
        else:
            token = torch.from_numpy(np.ascontiguousarray(prefixes[:, t - 1])).to(dev)
            pos = (plen + (t - 1)).to(torch.int32).view(B, 1).contiguous()
            lg = _vlm_decode_step(model, token, pos, t - 1, cache, state["gen"], qinfo_d, kinfo_prefix, B, Pn)
        if outside is not None:
            lg = lg.masked_fill(outside, float("-inf"))
        return lg.cpu().numpy()

    def reorder(t, logits, scores, finished, res, *states):
        if on_step is not None:
            on_step(t, logits, scores, finished, res, *states)
        par = torch.from_numpy(res[0]).to(dev).long()
        state["gen"] = [(gk, gv) if gk is None else (gk.index_select(0, par), gv.index_select(0, par)) for gk, gv in state["gen"]]

    if grammar is not None:
        if allowed is not None:
            raise ValueError("grammar does not combine with allowed_tokens: the union of the automaton's edges replaces the set")
        tokens, logp, scores, _ = bm.grammar_beam_search(logits_fn, N, max_decoding_steps, model.EOS_TOKEN, grammar.host, early_stop,
                                                         on_step=reorder)
    else:
        tokens, logp, scores = bm.beam_search(logits_fn, N, max_decoding_steps, model.EOS_TOKEN, early_stop, on_step=reorder)
    return (torch.from_numpy(tokens).to(dev), torch.from_numpy(logp.astype(np.float32)).to(dev),
            torch.from_numpy(scores.astype(np.float32)).to(dev))


def beam_decode_fused(model: LAP, observation, N: int, *, max_decoding_steps: int, early_stop: bool = True, weights: str = "bf16",
                      allowed=None, grammar=None):
    """Beam search on the fused step (call it under `_serving_weights`): `replicate_prefill` to N rows and a `DecodeCtx(beams=N)`.
    grammar: a DeviceAutomaton on the model's device (not with allowed): the beams stay inside the automaton.
    Returns `DecodeCtx.beam_result()`: (tokens int32 [N, cap], logp f32 [N, cap], scores f32 [N]) in rank order."""
    pre = replicate_prefill(prefill(model, observation), N)
    ctx = DecodeCtx(model, N, pre.Pn, max_decoding_steps, weights=weights, allowed=allowed, beams=N, early_stop=early_stop,
                    grammar=grammar)
    ctx.first_token(pre)
    _steps_until_done(ctx, max_decoding_steps)
    return ctx.beam_result()


# ---- the fused drivers: `decode_ctx.DecodeCtx` steps, state on the device
def _steps_until_done(ctx: DecodeCtx, max_decoding_steps: int):
    """The steps after `first_token`: DECODE_STEPS_PER_CHECK at a time, then one host read of the device stop flag `state[1]`."""
    n = DECODE_STEPS_PER_CHECK
    for _ in range((max_decoding_steps - 1 + n - 1) // n):
        if bool(ctx.state[1].item()):
            break
        for _ in range(n):
            ctx.step()


def _sample_fused(model: LAP, observation, *, max_decoding_steps: int, collect=None, sampling=None, weights: str = "bf16",
                  allowed=None, logprobs: bool = False, num_samples=None, filt=None, speculate=None, draft=None, grammar=None, jump=None):
    """grammar: None, or a DeviceAutomaton: a grammar context.  jump: None, or the rows S of a jump-forward step of that context
    (`check_jump_forward`), with `draft` as the reference sequence and `model.last_spec_stats` as under speculate.
    sampling: None (the greedy LM head) or (seed, temperature) for the sampling LM head.  weights: `decode_weights`.
    filt: None, or (top_k, top_p): a filtering context (it needs `sampling`).
    allowed: None or the int32 device ids of `check_allowed_tokens`.  logprobs: the context keeps the token log-probabilities
    and (tokens, logprobs) is returned.  num_samples: the batch-1 prefill is replicated to that many rows.
    speculate: None, or the rows S of a verify step (greedy, batch 1: `check_speculate`) with `draft` as the reference sequence;
    `model.last_spec_stats` then holds (verify_steps, accepted) of the request."""
    pre = prefill(model, observation)
    if num_samples is not None:
        pre = replicate_prefill(pre, num_samples)
    ctx = DecodeCtx(model, pre.B, pre.Pn, max_decoding_steps, sampling is not None, weights, allowed=allowed, logprobs=logprobs,
                    filtering=filt is not None, speculate=speculate, grammar=grammar, jump_forward=jump)
    if speculate is not None or jump is not None:
        ctx.set_draft(draft)
    if sampling is not None:
        ctx.set_sampling(*sampling)
    if filt is not None:
        ctx.set_filter(*filt)
    lg = None
    if collect is not None:     # (the constrained LM head writes the allowed columns only: the rest keeps the fill)
        lg = torch.empty((pre.B, model.config.vocab_size), dtype=torch.float32, device=model.device)
        if allowed is not None or grammar is not None:
            lg.fill_(float("-inf"))
    ctx.first_token(pre, lg)
    if collect is not None:     # debug: one host read per token
        collect["logit/0"] = lg.clone()
        while not bool(ctx.state[1].item()):
            ctx.step(lg)
            collect[f"logit/{int(ctx.state[0].item()) - 1}"] = lg.clone()
        return (ctx.out, ctx.logp) if logprobs else ctx.out
    _steps_until_done(ctx, max_decoding_steps)
    if speculate is not None or jump is not None:
        model.last_spec_stats = ctx.stats()
    return (ctx.out, ctx.logp) if logprobs else ctx.out


class ScoreResult(NamedTuple):
    """What `score_tokens` returns for N candidates."""
    logp: list                      # N f32 tensors: the log-probability of every given token
    total: torch.Tensor             # f32 [N]: their sums
    greedy: list                    # N int32 tensors: the argmax id at every position


def score_tokens(model: LAP, observation, tokens, *, rows: int = 8, temperature: float = 0.0, decode_weights: str = "bf16",
                 allowed_tokens=None, max_decoding_steps: int = 390) -> ScoreResult:
    """`LAP.score_tokens` (documented there): every argument is checked before any device work."""
    seqs, S, _ = check_score_args(tokens, rows, max_decoding_steps, batch=observation.tokenized_prompt.shape[0])
    check_decode_weights(decode_weights)
    check_fused_decode(model, S)
    hip.sampling_words(0, temperature)      # (rejects a temperature whose inverse is not finite before any work)
    allowed = allowed_set(model, allowed_tokens).ids if allowed_tokens is not None else None
    with model._serving_weights():
        pre = prefill(model, observation)
        ctx = DecodeCtx(model, 1, pre.Pn, max_decoding_steps, weights=decode_weights, allowed=allowed, score=S)
        ctx.set_score_temperature(temperature)
        logp, greedy = [], []
        for ids in seqs:                    # one prefill, one context: the state is reset and the generated cache overwritten
            ctx.set_candidate(ids)
            ctx.first_token(pre)
            for _ in range((len(ids) - 1 + S - 1) // S):
                ctx.step()
            lp, gr = ctx.score_result()
            if lp.numel() != len(ids):
                raise RuntimeError(f"score_tokens: scored {lp.numel()} of {len(ids)} tokens")
            logp.append(lp)
            greedy.append(gr)
    return ScoreResult(logp, torch.stack([lp.sum() for lp in logp]), greedy)
