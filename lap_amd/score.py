"""Teacher-forced scoring of a given LAP_AR answer: the quantity in numpy, and the checks of the surface.  This module is the
specification of csrc/decode_score.hip (lap_decode_score_finish) and of the TARGET LM heads (lap_decode_lm_head_score), as
sampling.py and speculate.py are of their kernels; tests/test_score_gpu.py compares the kernels with it.

`LAP.score_tokens(observation, tokens)` feeds the given tokens instead of the model's own and reports, for every position i,

    logp[i]   = z[tokens[i]] - logsumexp(z)          z = the logits row that follows tokens[:i] (the prefill's last row for i = 0)
    greedy[i] = argmax(z)                            lowest index among ties

with z = logit at temperature 0 (the convention of `return_logprobs=True` on a greedy decode) and z = float32(logit * inv_t), inv_t =
float32(1 / temperature), otherwise.  With an allowed set both run over the set only.  A score step of S rows (1 <= S <= 8) runs
the fused decode kernels on S consecutive positions of the one sequence, as a verify step of speculative decoding does; every row
is accumulated independently of S, so the numbers do not depend on it.
"""
from __future__ import annotations

import numpy as np

from lap_amd.sampling import inverse_temperature

MIN_ROWS, MAX_ROWS = 1, 8       # rows of a score step (the fused decode kernels serve 1 <= B <= 8 rows)


def score_reference(logits_rows, targets, *, temperature: float = 0.0, allowed=None):
    """(logp float64 [L], greedy int32 [L]) of the targets under the float32 `logits_rows` [L, V]: logp[i] = z[targets[i]] -
    logsumexp(z) with z = logit when temperature == 0 and z = float32(logit * float32(1 / temperature)) otherwise (everything after
    that product is float64); greedy[i] = argmax(z), lowest index among ties.  allowed: the log-sum-exp and the argmax run over
    these vocabulary ids only, and a target outside the set scores -inf.  A target outside [0, V) scores -inf."""
    lg = np.ascontiguousarray(np.asarray(logits_rows, dtype=np.float32))
    if lg.ndim != 2:
        raise ValueError("logits_rows: [L, vocab_size]")
    L, V = lg.shape
    tgt = np.asarray(targets).reshape(-1).astype(np.int64)
    if tgt.shape[0] != L:
        raise ValueError(f"targets: one per row of logits_rows, got {tgt.shape[0]} for {L} rows")
    inv_t = inverse_temperature(temperature)
    z = (lg * inv_t if inv_t != 0.0 else lg).astype(np.float64)
    inside = np.ones((V,), dtype=bool)
    if allowed is not None:
        ids = np.unique(np.asarray(allowed).reshape(-1).astype(np.int64))
        ids = ids[(ids >= 0) & (ids < V)]
        if ids.size == 0:
            raise ValueError("allowed: no id inside the vocabulary")
        inside[:] = False
        inside[ids] = True
    zs = np.where(inside[None, :], z, -np.inf)
    m = zs.max(axis=1)
    lse = m + np.log(np.exp(zs - m[:, None]).sum(axis=1))
    ok = (tgt >= 0) & (tgt < V)
    ok &= inside[np.where(ok, tgt, 0)]
    z_tgt = np.where(ok, z[np.arange(L), np.where(ok, tgt, 0)], -np.inf)
    with np.errstate(invalid="ignore"):
        logp = np.where(ok, z_tgt - lse, -np.inf)
    return logp, np.argmax(zs, axis=1).astype(np.int32)       # (np.argmax: the first of equal maxima)


def check_score_rows(rows) -> int:
    """`rows` of a scoring request (or `score` of a decode_ctx.DecodeCtx) as the number of rows S of a step; ValueError naming the value."""
    if isinstance(rows, bool) or not isinstance(rows, (int, np.integer)):
        raise ValueError(f"score rows must be an integer, got {rows!r}")
    S = int(rows)
    if not MIN_ROWS <= S <= MAX_ROWS:
        raise ValueError(f"score rows must lie in [{MIN_ROWS}, {MAX_ROWS}] (the rows of one fused step), got {S}")
    return S


def check_score_ctx(score, B: int, *, sampling: bool = False, filtering: bool = False, speculate=None, grammar=None, jump_forward=None,
                    beams=None) -> int:
    """`score=S` of a decode_ctx.DecodeCtx as S; ValueError naming what a scoring context does not combine with."""
    S = check_score_rows(score)
    if B != 1:
        raise ValueError(f"score needs B = 1 (the rows of a step are positions of one sequence), got B {B}")
    for name, on in (("sampling", sampling), ("filtering", filtering), ("speculate", speculate is not None),
                     ("grammar", grammar is not None), ("jump_forward", jump_forward is not None), ("beams", beams is not None)):
        if on:
            raise ValueError(f"score does not combine with {name}: a scoring context draws nothing (its temperature is set_temperature's)")
    return S


def _is_sequence_of_sequences(tokens) -> bool:
    if hasattr(tokens, "ndim"):                 # a tensor or an array: one sequence, or [N, L]
        return tokens.ndim == 2
    if isinstance(tokens, (list, tuple)) and len(tokens) > 0:
        return hasattr(tokens[0], "ndim") or isinstance(tokens[0], (list, tuple))
    return False


def _one_sequence(seq, i: int, cap: int) -> np.ndarray:
    if hasattr(seq, "detach"):                  # a torch tensor
        seq = seq.detach().cpu().numpy()
    a = np.asarray(seq)
    if a.size == 0:
        raise ValueError(f"score_tokens: sequence {i} is empty (length 0); every sequence needs 1 <= length <= {cap}")
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"score_tokens: sequence {i}: expected integer ids, got {a.dtype}")
    a = a.reshape(-1)
    if a.shape[0] > cap:
        raise ValueError(f"score_tokens: sequence {i} has length {a.shape[0]}; every sequence needs 1 <= length <= {cap}")
    if int(a.min()) < -(1 << 31) or int(a.max()) >= (1 << 31):
        raise ValueError(f"score_tokens: sequence {i}: an id does not fit int32")
    return a.astype(np.int32)


def check_score_args(tokens, rows, cap: int, *, batch: int = 1):
    """The arguments of a scoring request: (list of N int32 arrays, S, single), `single` telling that `tokens` was ONE sequence.
    ValueError, with the offending value, for an observation batch != 1, `rows` outside [1, 8] or not an integer, an empty
    sequence (or an empty list), a non-integer dtype, or a sequence longer than `cap` (max_decoding_steps)."""
    if batch != 1:
        raise ValueError(f"score_tokens needs an observation of batch 1 (its prefix is prefilled once), got batch {batch}")
    S = check_score_rows(rows)
    single = not _is_sequence_of_sequences(tokens)
    seqs = [tokens] if single else list(tokens)
    if len(seqs) == 0:
        raise ValueError("score_tokens: tokens is empty (0 sequences)")
    return [_one_sequence(s, i, int(cap)) for i, s in enumerate(seqs)], S, single
