"""Action-chunk inpainting restated on the oracle's own pieces (the reference has no such option, so neither has oracle/), and the
host replay of the Euler steps that the GPU tests hold the kernels to bit for bit.  Shared by test_inpaint_cpu / test_inpaint_gpu."""
import torch

from oracle import lap_oracle as O


def oracle_sample_inpaint(P, cfg, obs, noise, known, mask, num_steps=10, collect=None):
    """`O.sample_actions` (same pieces in the same order: embed_prefix, gemma_forward, embed_suffix) with the rows flagged in `mask`
    [B, S] held on t' noise + (1 - t') known after every Euler step, t' = (n - 1 - k) / n, the interpolation in float64.  With an
    all-zero mask every operation is `O.sample_actions`'s; the last step has t' = 0, so a frozen row of the result is `known`."""
    dt = -1.0 / num_steps
    B = noise.shape[0]
    frozen = mask.bool()[..., None]
    nsteps, t = 0, 1.0
    while t >= -dt / 2:
        nsteps, t = nsteps + 1, t + dt
    prefix_tokens, prefix_mask, prefix_ar = O.embed_prefix(P, cfg, obs)
    prefix_attn = O.make_attn_mask(prefix_mask, prefix_ar)
    positions = torch.cumsum(prefix_mask.long(), 1) - 1
    _, cache = O.gemma_forward(P, cfg, [prefix_tokens, None], positions, prefix_attn, [None, None])
    x_t, t = noise.clone(), 1.0
    for step in range(nsteps):
        suffix_tokens, suffix_mask, suffix_ar1, cond = O.embed_suffix(P, cfg, x_t, torch.full((B,), t, dtype=torch.float32), state=obs.get("state"))
        suffix_attn = O.make_attn_mask(suffix_mask, suffix_ar1[None].expand(B, -1))
        pmask = prefix_mask[:, None, :].expand(B, suffix_tokens.shape[1], -1)
        full = torch.cat([pmask, suffix_attn], dim=-1)
        pos = prefix_mask.long().sum(-1)[:, None] + torch.cumsum(suffix_mask.long(), -1) - 1
        (_, out1), _ = O.gemma_forward(P, cfg, [None, suffix_tokens], pos, full, [None, cond], kv_cache=cache)
        v_t = out1[:, -cfg.action_horizon:] @ P["action_out_proj/kernel"] + P["action_out_proj/bias"]
        if collect is not None:
            collect[f"v_t/{step}"] = v_t
        x_t = x_t + dt * v_t
        tp = (nsteps - 1 - step) / nsteps
        held = (tp * noise.double() + (1.0 - tp) * known.double()).to(x_t.dtype)
        x_t = torch.where(frozen, held, x_t)
        t = t + dt
    return x_t


def fma_f32(a: float, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """fl32(a * b + c) with ONE rounding, elementwise (a an f32-valued scalar; b, c f32 CPU tensors): what the kernels' free update
    x += dt * v_t compiles to.  The product of two f32 is exact in float64; the float64 sum is rounded to odd (its error term from
    TwoSum), after which rounding 53 bits to 24 is the rounding of the exact value."""
    p, c = b.double() * float(a), c.double()
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    bits = s.view(torch.int64)
    even = (bits & 1) == 0
    grow = (e > 0) == (s > 0)      # the exact value lies beyond s in magnitude
    bits = bits + torch.where((e != 0) & even, torch.where(grow, 1, -1), 0)
    return bits.view(torch.float64).float()


def replay_steps(noise, known, mask, v_ts, dt):
    """The sampler's x_t replayed on the host from the collected velocities `v_ts` (one [B, S, ad] per step): a free row takes
    x <- fl(x + dt v_t) (one fused multiply-add, dt rounded to f32, as in the plain sampler), a frozen row
    fl(fl(t' noise) + fl((1 - t') known)) in three f32 operations with t', 1 - t' rounded from float64 — `known` at t' = 0."""
    from lap_amd.flow_sample import inpaint_times

    noise, known = noise.float().cpu(), known.float().cpu()
    frozen = mask.bool().cpu()[..., None]
    dt32 = torch.tensor(dt, dtype=torch.float32).item()
    x = noise.clone()
    for v, (tp, omtp) in zip(v_ts, inpaint_times(len(v_ts))):
        free = fma_f32(dt32, v.float().cpu(), x)
        held = torch.tensor(tp, dtype=torch.float32) * noise + torch.tensor(omtp, dtype=torch.float32) * known
        x = torch.where(frozen, known if tp == 0 else held, free)
    return x
