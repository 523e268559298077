"""Flow-matching action sampling (lap.py:605-675) behind `LAP.sample_actions`: the serving prefill once, then the Euler steps of the
action expert against the cached prefix.  A denoise step runs on one of four routes, chosen once per call (`sample_actions`):
chain (the expert's layers as one persistent launch), skinny (five fused launches per layer), partials (split-K slabs + fused
consumers), generic (the layer loop of the train step; A/B tests); pi0 has a sampler of its own on the generic loop.
The weights are read through the model (`W`, `F`), as `LAP._serving_weights` presents them.
`inpaint=(known, mask)` (real-time chunking; the reference has no such option) holds the flagged action rows on a known trajectory:
every route then ends its steps on the inpainting form of its Euler tail, and nothing else changes.
`num_samples=N` (best-of-N; not in the reference either) draws N candidate chunks of ONE observation from one batch-1 prefill
(`_sample_candidates`): the steps run on N * S rows, and on the skinny route the attention reads the single prefix cache
(`hip.attention_serve_shared`); `select=` then picks one on the device (`hip.action_select`, specified by `action_select.py`).
"""
from __future__ import annotations

import contextlib
import functools
from typing import NamedTuple

import torch

from lap_amd import hip, prefill
from lap_amd.action_select import check_select
from lap_amd.joint_layers import llm_fwd, mod_slot
from lap_amd.model import LAP, _gen
from lap_amd.observation import preprocess_observation


class Denoise(NamedTuple):
    """What every Euler step of one `sample_actions` call works on."""
    x_t: torch.Tensor               # f32 [B, S, ad], updated in place by every step
    mods: torch.Tensor              # adaRMS modulations, one row per step (`serve_mods`)
    dt: float
    B: int
    S: int
    Pn: int
    cache: list                     # prefix K/V per layer
    rope_tab: torch.Tensor | None   # sin / cos of the action tokens' positions (the fused routes)
    qinfo: torch.Tensor             # info words of the suffix queries
    kinfo: torch.Tensor             # ... of the prefix and suffix keys
    pos: torch.Tensor
    collect: dict | None
    inp: "Inpaint | None" = None    # frozen rows (`sample_actions(inpaint=...)`): the steps then end on the inpainting tails
    shared: bool = False            # B candidates of ONE observation: `cache` holds the prefix once (`_sample_candidates`, skinny route)


class Inpaint(NamedTuple):
    """Action-chunk inpainting, as the Euler tails take it: rows are the B * S action rows."""
    noise: torch.Tensor             # f32 [B * S, ad]: the call's noise, kept beside its working copy x_t
    known: torch.Tensor             # f32 [B * S, ad], model space
    mask: torch.Tensor              # uint8 [B * S], 1 = frozen
    times: list                     # per step (t', 1 - t') of `inpaint_times`


def inpaint_times(nsteps: int):
    """Per Euler step k the flow time AFTER it, t' = (nsteps - 1 - k) / nsteps, and 1 - t', both in float64 (python floats); the
    kernels take them rounded to f32.  The last step's t' is 0 exactly: a frozen row of the result is `known` bit for bit."""
    return [((nsteps - 1 - k) / nsteps, 1.0 - (nsteps - 1 - k) / nsteps) for k in range(nsteps)]


def check_inpaint(inpaint, B: int, S: int, ad: int, device):
    """`inpaint=(known, mask)` of `sample_actions` -> (known f32 [B, S, ad], mask uint8 [B, S]) on `device`, or ValueError: wrong
    shapes (a batch mismatch included), non-finite `known`, mask values other than 0 / 1.  The values are not looked at while a
    stream is being captured (that would synchronise): `serve.GraphedSampler` checks every request before it copies it in."""
    try:
        known, mask = inpaint
    except (TypeError, ValueError):
        raise ValueError("inpaint: expected None or a pair (known, mask)") from None
    known, mask = torch.as_tensor(known), torch.as_tensor(mask)
    if tuple(known.shape) != (B, S, ad):
        raise ValueError(f"inpaint: known has shape {tuple(known.shape)}, expected [batch, action_horizon, action_dim] = {(B, S, ad)} (model space)")
    if tuple(mask.shape) != (B, S):
        raise ValueError(f"inpaint: mask has shape {tuple(mask.shape)}, expected [batch, action_horizon] = {(B, S)}")
    if known.is_complex() or mask.is_complex():
        raise ValueError(f"inpaint: known and mask must be real, got {known.dtype} / {mask.dtype}")
    capturing = torch.device(device).type == "cuda" and torch.cuda.is_current_stream_capturing()
    if not capturing:
        if not bool(torch.isfinite(known).all()):
            raise ValueError("inpaint: known has non-finite values")
        if not bool(((mask == 0) | (mask == 1)).all()):
            raise ValueError("inpaint: mask values must be 0 or 1")
    return known.to(device, torch.float32).contiguous(), mask.to(device, torch.uint8).contiguous()


def check_num_samples(num_samples, B: int, pi05: bool) -> int:
    """`num_samples=` of `sample_actions` -> N (None = 1), or ValueError: not an integer in 1 .. 8, or N > 1 with a batch of
    observations or with pi0 (whose suffix carries the state token: no shared-prefix route)."""
    if num_samples is None:
        return 1
    if isinstance(num_samples, bool) or not isinstance(num_samples, int) or not 1 <= num_samples <= 8:
        raise ValueError(f"num_samples: expected an integer in 1 .. 8, got {num_samples!r}")
    if num_samples > 1 and B != 1:
        raise ValueError(f"num_samples = {num_samples} draws candidates for ONE observation: got a batch of {B}")
    if num_samples > 1 and not pi05:
        raise ValueError("num_samples > 1 needs pi05=True (the pi0 sampler has no candidate route)")
    return num_samples


def sample_actions(model: LAP, rng, observation, *, num_steps: int = 10, noise=None, collect=None, fused=True, inpaint=None,
                   num_samples=None, select=None, coherence=None, share_prefix=True, _select_out=None):
    """`LAP.sample_actions` (documented there), with the weights as `_serving_weights` presents them (merged when the model has adapters)."""
    cfg, dev = model.config, model.device
    model.comm.wait_unit("small")
    obs = preprocess_observation(observation, train=False, image_keys=cfg.image_keys, image_resolution=cfg.image_resolution)
    B = obs.tokenized_prompt.shape[0]
    S, ad = model.action_horizon, model.action_dim
    N = check_num_samples(num_samples, B, cfg.pi05)
    mode, coh = check_select(select, coherence, S, ad)
    if N > 1:
        return _sample_candidates(model, rng, obs, N, num_steps, noise, collect, fused, inpaint, mode, coh, share_prefix, _select_out)
    if mode is not None:
        raise ValueError(f"select={select!r} chooses among candidates: it needs num_samples > 1")
    if fused is True:
        fused = "skinny" if hip.serve_supported(model.e.width, model.v.head_dim, model.e.mlp_dim, model.v.num_heads) else "partials"
    if fused not in (False, "skinny", "partials"):
        raise ValueError(f"fused={fused!r}")
    if noise is None:
        noise = torch.randn((B, S, ad), generator=_gen(rng, dev), device=dev, dtype=torch.float32)
    noise = noise.to(dev, torch.float32).contiguous()
    x_t = noise.clone()
    dt = -1.0 / num_steps
    nsteps, t = 0, 1.0
    while t >= -dt / 2:  # lap.py:669-674 loop condition, unrolled on the host (the time grid is data independent)
        nsteps += 1
        t += dt
    inp = None
    if inpaint is not None:     # (at t = 1 a frozen row IS its noise: step 0 reads x_t as it stands)
        known, mask = check_inpaint(inpaint, B, S, ad, dev)
        if tuple(noise.shape) != (B, S, ad):
            raise ValueError(f"inpaint: noise has shape {tuple(noise.shape)}, expected {(B, S, ad)}")
        inp = Inpaint(noise.view(B * S, ad), known.view(B * S, ad), mask.view(B * S), inpaint_times(nsteps))
    x0, Pn, _ = model._embed_prefix(obs, False, tower=prefill.siglip_fwd_serve)
    infos = model._serve_infos(obs, S)
    if not cfg.pi05:
        return _sample_actions_pi0(model, obs, x_t, x0, Pn, infos, num_steps, collect, inp)
    qinfo_p, kinfo_p, ppos, qinfo_s, kinfo_all, pos_all = infos
    # the adaRMS condition depends on the denoise time only: all steps' modulations in one pass over the adaRMS bank —
    # and on nothing else, so they are computed ONCE per (step count, parameter version) and kept: a captured sampler
    # (serve.GraphedSampler warms up before it captures) holds no time-MLP kernels at all (-0.25 ms per chunk)
    mods = serve_mods(model, nsteps, dt)
    # ... and so are the action tokens' positions: one sin / cos table serves the 10 x 18 fused RoPE kernels
    rope_tab = hip.rope_table(pos_all, B, S, pos_all.shape[1], pos_all.shape[1] - S, model.v.head_dim) if fused else None
    cache = []
    fast_prefill = model.serve_fusions and collect is None and model.gemm_dtype == "bf16"
    # The first denoise step needs layer l's K / V only when it reaches layer l: it is issued on a second stream and runs
    # beside the prefill's layers l+1 .. (whose big GEMMs leave CUs idle at their tails), joined before step 1.
    overlap = fast_prefill and fused == "skinny" and model.serve_overlap and dev.type == "cuda" and nsteps > 1
    kv_events = [] if overlap else None
    start = None
    if overlap:
        if model._den is None:
            model._den = torch.cuda.Stream(dev)
        start = torch.cuda.Event()
        start.record()
    if fast_prefill:
        prefill.llm_prefill(model, x0, ppos, qinfo_p, kinfo_p, B, Pn, cache, kv_events=kv_events)
    else:
        llm_fwd(model, x0, None, None, ppos, qinfo_p, kinfo_p, B, Pn, 0, False, cache_out=cache)
    d = Denoise(x_t, mods, dt, B, S, Pn, cache, rope_tab, qinfo_s, kinfo_all, pos_all, collect, inp)
    chain = (fused == "skinny" and model.serve_chain and not overlap and dev.type == "cuda" and model.v.depth <= hip.CHAIN_MAX_DEPTH
             and hip.serve_chain_ok(B, S, model.e.width, model.e.mlp_dim, model.v.num_heads, model.v.head_dim, model.v.num_kv_heads, Pn))
    if chain:
        route = functools.partial(_step_chain, chain=_chain_setup(model, d))
    elif fused == "skinny":
        route = functools.partial(_step_skinny, start=start, kv_events=kv_events)
    else:
        route = _step_partials if fused == "partials" else _step_generic
    x1 = None       # the next step's action tokens, where a step's tail has embedded them already (the chain)
    for step in range(nsteps):
        x1 = route(model, d, step, x1)
    return x_t


def _sample_candidates(model: LAP, rng, obs, N, num_steps, noise, collect, fused, inpaint, mode, coh, share_prefix, select_out):
    """`sample_actions(num_samples=N > 1)`: N candidate chunks of one observation.  The prefix is prefilled ONCE at batch 1 (the fast
    prefill and its K / V events as in the plain call); the Euler steps run on N * S rows with S rows per sample — the rope table, the
    info words and the positions are the batch-1 ones N times — on the skinny, partials or generic route, never on the chain.
    share_prefix (skinny route only): the attention reads the single cache (`hip.attention_serve_shared`); otherwise, and on the
    other routes, the cache is replicated N times behind the prefill and `hip.attention_fwd` runs at batch N: same bits.
    Returns [N, S, ad], or with `mode` the selected chunk [1, S, ad]."""
    dev = model.device
    S, ad = model.action_horizon, model.action_dim
    if fused is True:
        fused = "skinny" if hip.serve_supported(model.e.width, model.v.head_dim, model.e.mlp_dim, model.v.num_heads) else "partials"
    if fused not in (False, "skinny", "partials"):
        raise ValueError(f"fused={fused!r}")
    if noise is None:
        noise = torch.randn((N, S, ad), generator=_gen(rng, dev), device=dev, dtype=torch.float32)
    noise = torch.as_tensor(noise).to(dev, torch.float32).contiguous()
    if tuple(noise.shape) != (N, S, ad):
        raise ValueError(f"num_samples: noise has shape {tuple(noise.shape)}, expected [num_samples, action_horizon, action_dim] = {(N, S, ad)}")
    x_t = noise.clone()
    dt = -1.0 / num_steps
    nsteps, t = 0, 1.0
    while t >= -dt / 2:
        nsteps += 1
        t += dt
    inp = None
    if inpaint is not None:     # one (known, mask) for every candidate
        known, mask = check_inpaint(inpaint, 1, S, ad, dev)
        inp = Inpaint(noise.view(N * S, ad), known.expand(N, S, ad).reshape(N * S, ad), mask.expand(N, S).reshape(N * S), inpaint_times(nsteps))
    if coh is not None:
        coh = tuple(torch.as_tensor(c).to(dev, torch.float32).contiguous() for c in coh)
    x0, Pn, _ = model._embed_prefix(obs, False, tower=prefill.siglip_fwd_serve)
    qinfo_p, kinfo_p, ppos, qinfo_s, kinfo_all, pos_all = model._serve_infos(obs, S)
    rep = lambda w: w.expand(N, w.shape[1]).contiguous()
    qinfo_s, kinfo_all, pos_all = rep(qinfo_s), rep(kinfo_all), rep(pos_all)
    mods = serve_mods(model, nsteps, dt)
    rope_tab = hip.rope_table(pos_all, N, S, pos_all.shape[1], pos_all.shape[1] - S, model.v.head_dim) if fused else None
    shared = bool(share_prefix) and fused == "skinny"
    cache = []
    fast_prefill = model.serve_fusions and collect is None and model.gemm_dtype == "bf16"
    # step 0 beside the prefill, as in the plain call: only where the steps read the prefill's own cache tensors
    overlap = fast_prefill and shared and model.serve_overlap and dev.type == "cuda" and nsteps > 1
    kv_events = [] if overlap else None
    start = None
    if overlap:
        if model._den is None:
            model._den = torch.cuda.Stream(dev)
        start = torch.cuda.Event()
        start.record()
    if fast_prefill:
        prefill.llm_prefill(model, x0, ppos, qinfo_p, kinfo_p, 1, Pn, cache, kv_events=kv_events)
    else:
        llm_fwd(model, x0, None, None, ppos, qinfo_p, kinfo_p, 1, Pn, 0, False, cache_out=cache)
    if not shared:
        cache = [(k.repeat(N, 1), v.repeat(N, 1)) for k, v in cache]
    d = Denoise(x_t, mods, dt, N, S, Pn, cache, rope_tab, qinfo_s, kinfo_all, pos_all, collect, inp, shared)
    if fused == "skinny":
        route = functools.partial(_step_skinny, start=start, kv_events=kv_events)
    else:
        route = _step_partials if fused == "partials" else _step_generic
    for step in range(nsteps):
        route(model, d, step, None)
    if mode is None:
        return x_t
    scores, index, best = hip.action_select(x_t, mode, *(coh or ()))
    for out in (collect, select_out):
        if out is not None:
            out.update(candidates=x_t, scores=scores, index=index)
    return best.view(1, S, ad)


def _chain_setup(model: LAP, d: Denoise):
    """The one-launch chain's barrier counters, weights (packed images or the row-major ones) and scratch -> (weights, tp)."""
    v, e = model.v, model.e
    if model._chain_ctr is None:
        model._chain_ctr = hip.serve_chain_counters(model.device)
    for l in range(v.depth):
        model.comm.wait_unit(f"llm{l}")
    tp = (model.serve_packed and model.serve_tp
          and hip.serve_chain_tp_ok(d.B, d.S, e.width, e.mlp_dim, v.num_heads, v.head_dim, v.num_kv_heads, d.Pn))
    if not model.serve_packed:
        return [tuple(model.W(f"llm/{l}/{n}") for n in ("wqkv1", "wo1", "wgu1", "wd1")) for l in range(v.depth)], tp
    weights = serve_packed_weights(model)
    if model._chain_scratch is None or (tp and "tp_slabs" not in model._chain_scratch):
        model._chain_scratch = hip.serve_chain_scratch(model.device, e.width, e.mlp_dim, v.num_heads, v.head_dim, tp=tp)
    return weights, tp


def _step_chain(model: LAP, d: Denoise, step, x1, *, chain):
    """One launch for the expert's layers; the step's tail is `serve_final_euler`, or with `serve_euler_embed` (action_dim 7 / 8 at
    width 1024) one launch that also embeds the NEXT step's tokens: those are returned, and only step 0 embeds its own."""
    v, e = model.v, model.e
    B, S, ad = d.x_t.shape
    weights, tp = chain
    mod = d.mods[step:step + 1]
    fuse_tail = model.serve_euler_embed and ad in (7, 8) and e.width == 1024
    if not fuse_tail or step == 0:
        x1 = hip.serve_embed_actions(d.x_t.view(B * S, ad), model.F("act/in_w"), model.F("act/in_b"))
    xf1 = hip.serve_chain(x1, mod, 3 * e.width, weights, d.cache, d.rope_tab, d.qinfo, d.kinfo, B, S, v.num_heads, v.head_dim, e.mlp_dim,
                          d.Pn, v.head_dim ** -0.5, model._chain_ctr, packed_scratch=model._chain_scratch if model.serve_packed else None, tp=tp)
    v_t = torch.empty((B * S, ad), dtype=torch.float32, device=model.device) if d.collect is not None else None
    final = (xf1, mod_slot(model, mod, 2 * v.depth), 0, S, model.F("act/out_w"), model.F("act/out_b"), d.x_t.view(B * S, ad), d.dt, v_t)
    if fuse_tail:
        x1 = torch.empty((B * S, e.width), dtype=torch.bfloat16, device=model.device) if step + 1 < d.mods.shape[0] else None
        embed = dict(w_in=model.F("act/in_w"), b_in=model.F("act/in_b"), tokens=x1)
        if d.inp is None:
            hip.serve_final_euler_embed(*final, **embed)
        else:
            hip.serve_final_euler_embed_inpaint(*final[:-1], *_frozen(d, step), v_out=v_t, **embed)
    else:
        _final_euler(d, step, final)
    if d.collect is not None:
        d.collect[f"v_t/{step}"] = v_t.view(B, S, ad)
    return x1


def _step_skinny(model: LAP, d: Denoise, step, _x1, *, start, kv_events):
    """Five fused launches per layer (`expert_denoise_skinny`).  With `serve_overlap` (`start` is the event recorded in front of the
    prefill) step 0 is issued on the side stream, takes layer l's K / V at its event, and the current stream joins behind it."""
    B, S, ad = d.x_t.shape
    mod = d.mods[step:step + 1]
    side = start is not None and step == 0
    main = torch.cuda.current_stream() if side else None
    if side:
        model._den.wait_event(start)
        for tns in (d.x_t, d.mods, d.rope_tab, d.qinfo, d.kinfo, *(d.inp[:3] if d.inp is not None else ())):
            tns.record_stream(model._den)
    with (torch.cuda.stream(model._den) if side else contextlib.nullcontext()):
        x1 = hip.serve_embed_actions(d.x_t.view(B * S, ad), model.F("act/in_w"), model.F("act/in_b"))
        xf1 = expert_denoise_skinny(model, x1, mod, d.qinfo, d.kinfo, B, d.Pn, S, d.cache, d.rope_tab, kv_events=kv_events if side else None,
                                    shared=d.shared)
        v_t = torch.empty((B * S, ad), dtype=torch.float32, device=model.device) if d.collect is not None else None
        _final_euler(d, step, (xf1, mod_slot(model, mod, 2 * model.v.depth), 0, S, model.F("act/out_w"), model.F("act/out_b"),
                               d.x_t.view(B * S, ad), d.dt, v_t))
    if side:
        main.wait_stream(model._den)
    if d.collect is not None:
        d.collect[f"v_t/{step}"] = v_t.view(B, S, ad)


def _frozen(d: Denoise, step):
    """(noise, known, mask, (t', 1 - t')) of step `step` for the inpainting tails."""
    return d.inp.noise, d.inp.known, d.inp.mask, d.inp.times[step]


def _final_euler(d: Denoise, step, final):
    """`serve_final_euler` on `final` = (its arguments ..., v_out), or its inpainting form when rows are frozen."""
    if d.inp is None:
        hip.serve_final_euler(*final)
    else:
        hip.serve_final_euler_inpaint(*final[:-1], *_frozen(d, step), v_out=final[-1])


def _step_partials(model: LAP, d: Denoise, step, _x1):
    x1, _ = model._embed_actions(d.x_t)
    pre1 = expert_denoise_partials(model, x1, d.mods[step:step + 1], d.pos, d.qinfo, d.kinfo, d.B, d.Pn, d.S, d.cache, d.rope_tab)
    _euler_f32(model, d, step, pre1)


def _step_generic(model: LAP, d: Denoise, step, _x1):
    """The layer loop of the train step against the prefix cache (same numerics as the partials; kept for A/B tests)."""
    mod = d.mods[step:step + 1]
    x1, _ = model._embed_actions(d.x_t)
    _, xf1, _ = llm_fwd(model, None, x1, mod, d.pos, d.qinfo, d.kinfo, d.B, d.Pn, d.S, False, kv_cache=d.cache, mod_shared=True)
    pre1, _ = hip.rmsnorm_fwd(xf1, mod=mod_slot(model, mod, 2 * model.v.depth), rows_per_sample=d.S, save_rstd=False, mod_ld=0)
    _euler_f32(model, d, step, pre1)


def _euler_f32(model: LAP, d: Denoise, step, pre1):
    """The tail of the partials and generic routes: action_out_proj as an f32 nnx.Linear, then the Euler update of x_t."""
    v_t = model._lin32(hip.cast_bf16_to_f32(pre1), "act/out_w", "act/out_b")
    if d.collect is not None:
        d.collect[f"v_t/{step}"] = v_t.view(d.x_t.shape).clone()
    if d.inp is None:
        hip.axpy_f32(d.x_t, v_t, d.dt)
    else:
        hip.euler_inpaint_f32(d.x_t.view(v_t.shape), v_t, d.dt, *_frozen(d, step))


def _sample_actions_pi0(model: LAP, obs, x_t, x0, Pn, infos, num_steps, collect, inp=None):
    """`sample_actions` for pi0 (`pi05=False`): the suffix is [state token | action tokens mixed with the time embedding], embedded anew
    at every Euler step; the expert's layers run on the generic layer loop (plain norms and residuals) against the prefix cache.
    Functional path: no fused serving kernels, no hipGraph chain (no registry config of the reference is pi0)."""
    if obs.state is None:
        raise ValueError("pi05=False feeds the continuous state through state_proj: the observation has no `state`")
    qinfo_p, kinfo_p, ppos, qinfo_s, kinfo_all, pos_all = infos
    B, S, ad = x_t.shape
    Sx, We = S + 1, model.e.width
    cache = []
    llm_fwd(model, x0, None, None, ppos, qinfo_p, kinfo_p, B, Pn, 0, False, cache_out=cache)
    dt = -1.0 / num_steps
    t, step = 1.0, 0
    while t >= -dt / 2:      # lap.py:669-674
        x1, _ = model._embed_suffix_pi0(x_t, torch.full((B,), t, dtype=torch.float32, device=model.device), obs.state, False)
        _, xf1, _ = llm_fwd(model, None, x1, None, pos_all, qinfo_s, kinfo_all, B, Pn, Sx, False, kv_cache=cache)
        pre_all, _ = hip.rmsnorm_fwd(xf1, scale=model.F("llm/final_norm1"), save_rstd=False)
        pre1 = pre_all.view(B, Sx, We)[:, 1:].reshape(B * S, We).contiguous()
        v_t = model._lin32(hip.cast_bf16_to_f32(pre1), "act/out_w", "act/out_b")
        if collect is not None:
            collect[f"v_t/{step}"] = v_t.view(B, S, ad).clone()
        if inp is None:
            hip.axpy_f32(x_t, v_t, dt)
        else:
            hip.euler_inpaint_f32(x_t.view(B * S, ad), v_t, dt, inp.noise, inp.known, inp.mask, inp.times[step])
        t += dt
        step += 1
    return x_t


def expert_denoise_partials(model: LAP, x1, mod, pos, qinfo, kinfo, B, Pn, S, cache, rope_tab=None):
    """The 18 action-expert layers of one denoise step (gemma.py:336-387 with xs = [None, suffix], kv_cache given)
    on the fused serving kernels: every projection is a split-K GEMM that leaves f32 partials, and the reduction
    happens inside the consumer (RoPE+split / GeGLU / gated residual + next adaptive RMSNorm).  `mod` is the single
    modulation row of this step (shared by all samples).  Returns the final adaRMS-normed suffix activations."""
    v, e = model.v, model.e
    NH, HD, KV = v.num_heads, v.head_dim, v.num_kv_heads
    Ttot = pos.shape[1]
    We = e.width
    scratch = hip._gemm_scratch(model.device)
    slot = lambda j: mod_slot(model, mod, j)
    h, _ = hip.rmsnorm_fwd(x1, mod=slot(0), rows_per_sample=S, save_rstd=False, mod_ld=0)
    x = x1
    for l in range(v.depth):
        model.comm.wait_unit(f"llm{l}")
        p = f"llm/{l}/"
        part, ks = hip.linear_partials(h, model.W(p + "wqkv1"), scratch)
        q, k, vv = hip.fused_reduce_rope_split(part, ks, pos, B, S, Ttot, Ttot - S, NH, HD, HD ** -0.5, table=rope_tab)
        ck, cv = cache[l]
        o, _ = hip.attention_fwd([None, q], [ck, k], [cv, vv], [0, S], [Pn, S], B, NH, KV, HD, qinfo, kinfo, need_lse=False)
        part, ks = hip.linear_partials(o[1], model.W(p + "wo1"), scratch)
        xa, hf = hip.fused_reduce_residual_norm(part, ks, x, slot(2 * l)[:, 2 * We:], 0, slot(2 * l + 1), 0, S)
        part, ks = hip.linear_partials(hf, model.W(p + "wgu1"), scratch)
        act = hip.fused_reduce_geglu(part, ks, B * S, e.mlp_dim)
        part, ks = hip.linear_partials(act, model.W(p + "wd1"), scratch)
        x, h = hip.fused_reduce_residual_norm(part, ks, xa, slot(2 * l + 1)[:, 2 * We:], 0, slot(2 * l + 2), 0, S)
    return h   # slot 2L is final_norm_1: h == final adaRMS norm of the last layer's output


def expert_denoise_skinny(model: LAP, x1, mod, qinfo, kinfo, B, Pn, S, cache, rope_tab, kv_events=None, shared=False):
    """The same 18 layers on the skinny-M fused projections (csrc/serve_skinny.hip): five launches per layer —
    [adaRMS + qkv + RoPE/split] -> attention -> [out-proj + gated residual] -> [adaRMS + gate|up + GeGLU] ->
    [down-proj + gated residual] — with no f32 partial slabs in between.  Returns the last layer's residual stream
    (the final adaRMS norm is part of lap_serve_final_euler).  `shared`: the B samples are candidates of one observation and `cache`
    holds its prefix once."""
    v, e = model.v, model.e
    NH, HD, KV = v.num_heads, v.head_dim, v.num_kv_heads
    We = e.width
    slot = lambda j: mod_slot(model, mod, j)
    x = x1
    for l in range(v.depth):
        model.comm.wait_unit(f"llm{l}")
        p = f"llm/{l}/"
        q, k, vv = hip.serve_qkv_rope(x, slot(2 * l), 0, S, model.W(p + "wqkv1"), rope_tab, NH, HD, HD ** -0.5)
        ck, cv = cache[l]
        if kv_events is not None:     # running beside the prefill (first denoise step): layer l's cache is ready at its event
            torch.cuda.current_stream().wait_event(kv_events[l])
            ck.record_stream(torch.cuda.current_stream()); cv.record_stream(torch.cuda.current_stream())
        if shared:
            o1 = hip.attention_serve_shared(q, k, vv, ck, cv, B, S, Pn, NH, KV, HD, qinfo, kinfo)
        else:
            o1 = hip.attention_fwd([None, q], [ck, k], [cv, vv], [0, S], [Pn, S], B, NH, KV, HD, qinfo, kinfo, need_lse=False)[0][1]
        xa = hip.serve_proj_residual(o1, model.W(p + "wo1"), x, slot(2 * l)[:, 2 * We:], 0, S)
        act = hip.serve_gate_up(xa, slot(2 * l + 1), 0, S, model.W(p + "wgu1"))
        x = hip.serve_proj_residual(act, model.W(p + "wd1"), xa, slot(2 * l + 1)[:, 2 * We:], 0, S)
    return x


def serve_mods(model: LAP, nsteps: int, dt: float):
    """adaRMS modulations of the denoise time grid t_k = 1 + k dt (lap.py:655-660 through `_time_mod`), one PERSISTENT tensor
    per (nsteps, dt), refreshed IN PLACE when the parameters change: a captured sampler holds its address (ADVICE r3 — a
    cache that dropped the tensor on a version change left a replayed graph reading freed memory and stale modulations).
    `GraphedSampler.__call__` calls `refresh_serve_caches` before every replay; never refreshed during stream capture."""
    def build(old):
        tvec = 1.0 + dt * torch.arange(nsteps, dtype=torch.float32, device=model.device)
        new = model._time_mod(tvec, False)[0]
        return new if old is None else old.copy_(new)
    return model.serving_cache.get(("mods", nsteps, float(dt)), "ada", build)


def serve_packed_weights(model: LAP):
    """Fragment-packed images of the action expert's projections for the packed chain (csrc/serve_skinny_body.hpp PK),
    persistent like `serve_mods` and re-packed in place per parameter version (+0.62 GB for LAP-3B)."""
    def build(old):
        kinds = (("wqkv1", hip.PACK_QKV), ("wo1", hip.PACK_PLAIN), ("wgu1", hip.PACK_GATE_UP), ("wd1", hip.PACK_PLAIN))
        out = []
        for l in range(model.v.depth):
            model.comm.wait_unit(f"llm{l}")
            out.append(tuple(hip.serve_pack_weight(model.W(f"llm/{l}/{n}"), kind, model.v.head_dim, out=None if old is None else old[l][j])
                             for j, (n, kind) in enumerate(kinds)))
        return out
    return model.serving_cache.get(("chain",), None, build)
