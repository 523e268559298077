"""Candidate selection for best-of-N flow sampling (`LAP.sample_actions(num_samples=N, select=...)`): the specification, plain
torch in float64 (not in the reference, whose sampler draws one chunk).  The device kernel is `hip.action_select`
(csrc/action_select.hip): same scores in f32, same rule.

Lower is better, and `select` takes the lowest index on ties:
    medoid     score[n] = sum_m ||cand[n] - cand[m]||^2: the candidate closest to all the others (the mode of a multimodal sample
               set rather than its mean, which may lie between two modes);
    coherence  score[n] = sum_s w[s] ||cand[n, s] - known[s]||^2: the candidate that continues the chunk being executed
               (`known` = `chunking.shift_chunk(prev, executed, 0)`'s trajectory, `w` = `coherence_weights`).
"""
from __future__ import annotations

import torch

MODES = ("medoid", "coherence")


def _cand(cand):
    cand = torch.as_tensor(cand)
    if cand.dim() != 3 or cand.shape[0] < 1 or cand.is_complex():
        raise ValueError(f"select: candidates have shape {tuple(cand.shape)}, expected real [num_samples, action_horizon, action_dim]")
    return cand.detach().to("cpu", torch.float64)


def medoid_scores(cand) -> torch.Tensor:
    """cand [N, S, ad] -> float64 [N]: score[n] = sum_m ||cand[n] - cand[m]||^2 over all S * ad elements."""
    c = _cand(cand)
    d = c[:, None] - c[None]
    return (d * d).sum(dim=(1, 2, 3))


def check_coherence(known, weights, S: int, ad: int):
    """`coherence=(known [S, ad] or [1, S, ad], weights [S])` -> (known [S, ad], weights [S]) as given dtypes, or ValueError."""
    known, weights = torch.as_tensor(known), torch.as_tensor(weights)
    if known.dim() == 3 and known.shape[0] == 1:
        known = known[0]
    if tuple(known.shape) != (S, ad):
        raise ValueError(f"select: coherence known has shape {tuple(known.shape)}, expected [action_horizon, action_dim] = {(S, ad)} (model space)")
    if tuple(weights.shape) != (S,):
        raise ValueError(f"select: coherence weights have shape {tuple(weights.shape)}, expected [action_horizon] = {(S,)}")
    if known.is_complex() or weights.is_complex():
        raise ValueError(f"select: coherence known and weights must be real, got {known.dtype} / {weights.dtype}")
    return known, weights


def coherence_scores(cand, known, weights) -> torch.Tensor:
    """cand [N, S, ad], known [S, ad], weights [S] -> float64 [N]: score[n] = sum_s weights[s] ||cand[n, s] - known[s]||^2."""
    c = _cand(cand)
    known, weights = check_coherence(known, weights, c.shape[1], c.shape[2])
    d = c - known.detach().to("cpu", torch.float64)[None]
    return ((d * d).sum(-1) * weights.detach().to("cpu", torch.float64)[None]).sum(-1)


def coherence_weights(S: int, executed: int, rho: float = 0.5) -> torch.Tensor:
    """float32 [S]: w[s] = rho**s for s < S - executed (the rows of the new chunk the previous one still covers), else 0."""
    if isinstance(executed, bool) or not isinstance(executed, int) or isinstance(S, bool) or not isinstance(S, int):
        raise ValueError(f"coherence_weights: S and executed must be integers, got {S!r}, {executed!r}")
    if S < 1 or not 0 <= executed <= S:
        raise ValueError(f"coherence_weights: executed = {executed} outside [0, S = {S}]")
    if not 0.0 < float(rho) <= 1.0:
        raise ValueError(f"coherence_weights: rho = {rho!r} outside (0, 1]")
    s = torch.arange(S, dtype=torch.float64)
    return torch.where(s < S - executed, float(rho) ** s, torch.zeros_like(s)).to(torch.float32)


def select(scores) -> int:
    """The argmin of `scores` [N], the lowest index on ties."""
    scores = torch.as_tensor(scores)
    if scores.dim() != 1 or scores.numel() < 1:
        raise ValueError(f"select: scores have shape {tuple(scores.shape)}, expected [num_samples]")
    best = 0
    for n in range(1, scores.numel()):
        if bool(scores[n] < scores[best]):
            best = n
    return best


def check_select(select_mode, coherence, S: int, ad: int):
    """`select=` / `coherence=` of `sample_actions` -> (mode or None, (known, weights) or None), or ValueError: an unknown mode, a
    mode without its arguments, arguments without their mode, wrong shapes."""
    if select_mode is None:
        if coherence is not None:
            raise ValueError("select: coherence=(known, weights) needs select='coherence'")
        return None, None
    if select_mode not in MODES:
        raise ValueError(f"select: expected None, 'medoid' or 'coherence', got {select_mode!r}")
    if select_mode == "medoid":
        if coherence is not None:
            raise ValueError("select: coherence=(known, weights) needs select='coherence'")
        return "medoid", None
    try:
        known, weights = coherence
    except (TypeError, ValueError):
        raise ValueError("select: select='coherence' needs coherence=(known, weights)") from None
    return "coherence", check_coherence(known, weights, S, ad)
