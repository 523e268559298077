"""Beam search over the rows of one fused LAP_AR decode batch, in plain numpy: the specification of csrc/decode_beam.hip
(lap_decode_beam_topn / _select / _reorder and their grammar forms) and the host half of the eager route of `LAP.sample_tokens(num_beams=N)`.

The rules (every number float64 unless said otherwise):
* The N beams advance in lockstep, one token per step; `scores[b]` is the sum of beam b's token log-probabilities, `finished[b]`
  whether it has emitted EOS.  A decode starts from scores = [0, -inf, ...] and nothing finished (`initial`): the N prefilled rows
  are identical, so the first step fans out from row 0 alone.
* The log-probabilities of row b are logit - lse_b, lse_b the log-sum-exp over the entries greater than -inf (a NaN is not: it
  is left out of the sum and is no candidate).
* A row with score -inf contributes nothing, finished or not.  Otherwise a finished row contributes exactly one candidate
  (parent b, token 0, log-probability 0, its score unchanged).  Otherwise an alive row contributes its N best ids by
  log-probability (the lower id among equal logits), each with score scores[b] + logp; a row without an entry > -inf, or whose
  lse is not finite, contributes nothing.
* The new beams are the N best candidates by score, descending; ties go to the lower parent, then the lower id.  With fewer
  than N candidates the remaining beams are finished, with score -inf, parent = own index and token 0.
* A beam that emits `eos`, or whose parent was finished, is finished.
* done: every beam is finished, or t + 1 >= cap, or (early_stop) the rank-0 beam is finished: scores never rise, so no alive
  beam can pass it under the sum score.

Under a grammar (`grammar_beam_step` / `grammar_beam_search`; lap_decode_beam_grammar_topn / _grammar_select) beam b also carries the
state states[b] of a `grammar.TokenAutomaton`, and its row is read with -inf outside `automaton.allowed(states[b])`: the
log-probabilities are over that state's set, the rules above apply to the masked rows, and a beam's state moves along the edge of its
token (a finished parent's and a padding beam's state stays).  A state outside [0, Q), or a segment outside [0, E], offers nothing.
"""
from __future__ import annotations

import numpy as np

MAX_NUM_BEAMS = 8       # the beams are the rows of one fused batch (B <= 8)


def initial(N: int):
    """(scores float64 [N] = [0, -inf, ...], finished bool [N] = False) of a fresh decode."""
    scores = np.full((N,), -np.inf)
    scores[0] = 0.0
    return scores, np.zeros((N,), dtype=bool)


def row_topn(logits_row, n: int):
    """(ids int32 [<= n], logp float64 [<= n], lse): the n best entries of one f32 logits row by log-probability (the lower id
    among ties) and the row's log-sum-exp over its entries > -inf; empty when there is none or the lse is not finite."""
    x = np.asarray(logits_row, dtype=np.float32).astype(np.float64)
    valid = np.flatnonzero(x > -np.inf)         # (NaN > -inf is False)
    if valid.size == 0:
        return np.zeros((0,), np.int32), np.zeros((0,)), -np.inf
    v = x[valid]
    m = v.max()
    with np.errstate(invalid="ignore", over="ignore"):
        lse = m + np.log(np.exp(v - m).sum())
    if not np.isfinite(lse):
        return np.zeros((0,), np.int32), np.zeros((0,)), lse
    order = valid[np.lexsort((valid, -v))][:n]
    return order.astype(np.int32), x[order] - lse, lse


def candidates(logits, scores, finished, N: int):
    """The candidates of a step, unsorted: a list of (score, parent, token, logp)."""
    cands = []
    for b in range(N):
        if not scores[b] > -np.inf:
            continue
        if finished[b]:
            cands.append((float(scores[b]), b, 0, 0.0))
            continue
        ids, lp, _ = row_topn(logits[b], N)
        cands.extend((float(scores[b] + l), b, int(i), float(l)) for i, l in zip(ids, lp))
    return cands


def beam_step(logits, scores, finished, t: int, cap: int, eos: int, early_stop: bool = True):
    """One step of the N = len(scores) beams on their f32 logits [N, V] at step t: (parent int32 [N], token int32 [N],
    token_logp float64 [N], new_scores float64 [N], new_finished bool [N], done)."""
    scores = np.asarray(scores, dtype=np.float64)
    finished = np.asarray(finished, dtype=bool)
    N = scores.shape[0]
    logits = np.asarray(logits)
    if logits.ndim != 2 or logits.shape[0] != N or finished.shape != (N,):
        raise ValueError(f"beam_step: logits [N, V], scores [N], finished [N]; got {logits.shape}, {scores.shape}, {finished.shape}")
    cands = sorted(candidates(logits, scores, finished, N), key=lambda c: (-c[0], c[1], c[2]))[:N]
    parent = np.arange(N, dtype=np.int32)
    token = np.zeros((N,), dtype=np.int32)
    logp = np.zeros((N,))
    new_scores = np.full((N,), -np.inf)
    new_finished = np.ones((N,), dtype=bool)
    for r, (s, b, tok, lp) in enumerate(cands):
        parent[r], token[r], logp[r], new_scores[r] = b, tok, lp, s
        new_finished[r] = bool(finished[b]) or tok == eos
    done = bool(new_finished.all()) or t + 1 >= cap or (bool(early_stop) and bool(new_finished[0]))
    return parent, token, logp, new_scores, new_finished, done


def beam_search(logits_fn, N: int, cap: int, eos: int, early_stop: bool = True, on_step=None):
    """Drive `beam_step` with `logits_fn(prefixes)` -> f32 logits [N, V], prefixes the int32 [N, t] tokens of the beams so far
    (t = 0 first: all rows are the prompt alone).  The parent permutation is applied to the token and log-probability histories.
    Returns (tokens int32 [N, cap], token_logp float64 [N, cap], scores float64 [N]) in rank order, zeros after a stop.
    on_step(t, logits, scores, finished, result) is called after every step (tests measure their gap condition there)."""
    scores, finished = initial(N)
    tokens = np.zeros((N, cap), dtype=np.int32)
    logp = np.zeros((N, cap))
    t, done = 0, cap < 1
    while not done:
        logits = np.asarray(logits_fn(tokens[:, :t].copy()))
        res = beam_step(logits, scores, finished, t, cap, eos, early_stop)
        if on_step is not None:
            on_step(t, logits, scores, finished, res)
        parent, tok, lp, scores, finished, done = res
        tokens, logp = tokens[parent], logp[parent]
        tokens[:, t], logp[:, t] = tok, lp
        t += 1
    return tokens, logp, scores


def grammar_masked(logits, states, automaton):
    """f32 [N, V]: row b of `logits` with -inf outside `automaton.allowed(states[b])`; all -inf for a state outside [0, Q) or a
    segment outside [0, E]: what `grammar_beam_step` hands to `beam_step`."""
    lg = np.asarray(logits, dtype=np.float32)
    masked = np.full(lg.shape, -np.inf, dtype=np.float32)
    Q, E = automaton.num_states, automaton.num_edges
    for b, q in enumerate(np.asarray(states).reshape(-1).tolist()):
        if not 0 <= q < Q:
            continue
        lo, hi = int(automaton.offsets[q]), int(automaton.offsets[q + 1])
        if lo < 0 or hi > E or hi < lo:
            continue
        ids = automaton.ids[lo:hi]
        ids = ids[(ids >= 0) & (ids < lg.shape[1])]
        masked[b, ids] = lg[b, ids]
    return masked


def grammar_beam_step(logits, scores, finished, states, automaton, t: int, cap: int, eos: int, early_stop: bool = True):
    """`beam_step` of beams that are each in a state of `automaton` (states int [N]), on the rows of `grammar_masked`.  Returns
    `beam_step`'s tuple and new_states int32 [N]: states[parent[r]] when that parent was finished or beam r is padding (score -inf;
    its parent is its own index), else `automaton.step(states[parent[r]], token[r])`."""
    states = np.asarray(states).reshape(-1).astype(np.int64)
    finished = np.asarray(finished, dtype=bool)
    if states.shape != np.asarray(scores).shape:
        raise ValueError(f"grammar_beam_step: states [N] beside scores [N]; got {states.shape}, {np.asarray(scores).shape}")
    res = beam_step(grammar_masked(logits, states, automaton), scores, finished, t, cap, eos, early_stop)
    parent, token, _, new_scores = res[:4]
    new_states = np.zeros(states.shape, dtype=np.int32)
    for r in range(states.shape[0]):
        q = int(states[parent[r]])
        keep = bool(finished[parent[r]]) or not new_scores[r] > -np.inf
        new_states[r] = q if keep else automaton.step(q, int(token[r]))
    return res + (new_states,)


def grammar_beam_search(logits_fn, N: int, cap: int, eos: int, automaton, early_stop: bool = True, on_step=None):
    """`beam_search` under `automaton`: every beam starts in state 0 and `grammar_beam_step` moves them.  Returns (tokens int32
    [N, cap], token_logp float64 [N, cap], scores float64 [N], states int32 [N]) in rank order.
    on_step(t, masked_logits, scores, finished, result, states) is called after every step with the states before it."""
    scores, finished = initial(N)
    states = np.zeros((N,), dtype=np.int32)
    tokens = np.zeros((N, cap), dtype=np.int32)
    logp = np.zeros((N, cap))
    t, done = 0, cap < 1
    while not done:
        logits = np.asarray(logits_fn(tokens[:, :t].copy()))
        res = grammar_beam_step(logits, scores, finished, states, automaton, t, cap, eos, early_stop)
        if on_step is not None:
            on_step(t, grammar_masked(logits, states, automaton), scores, finished, res[:6], states)
        parent, tok, lp, scores, finished, done, states = res
        tokens, logp = tokens[parent], logp[parent]
        tokens[:, t], logp[:, t] = tok, lp
        t += 1
    return tokens, logp, scores, states


def step_gaps(logits, scores, finished):
    """(row_gap, select_gap) of a step in the float64 specification: the smallest distance, over the alive rows that contribute,
    between the N-th and the (N+1)-th log-probability of a row, and the distance between the N-th and the (N+1)-th candidate
    score when every contributing row offers N + 1 ids; inf where there is no (N+1)-th.  A kernel whose log-probabilities are
    within a quarter of both gaps of the float64 ones selects what `beam_step` selects."""
    scores = np.asarray(scores, dtype=np.float64)
    N = scores.shape[0]
    row_gap, pool = np.inf, []
    for b in range(N):
        if not scores[b] > -np.inf:
            continue
        if finished[b]:
            pool.append(float(scores[b]))
            continue
        _, lp, _ = row_topn(logits[b], N + 1)
        if lp.size > N:
            row_gap = min(row_gap, float(lp[N - 1] - lp[N]))
        pool.extend(float(scores[b] + l) for l in lp)
    pool.sort(reverse=True)
    return row_gap, (pool[N - 1] - pool[N]) if len(pool) > N else np.inf


def check_num_beams(num_beams, batch: int, *, decode: str = "fused", temperature: float = 0.0, sampler: str = "host", num_samples=None,
                    top_k=None, top_p=None, speculate=None, grammar=None, jump_forward=None, collect=None) -> int:
    """`num_beams` of a request as an int N, 1 <= N <= 8; ValueError naming the condition it breaks."""
    if isinstance(num_beams, bool) or not isinstance(num_beams, (int, np.integer)):
        raise ValueError(f"num_beams must be an integer, got {num_beams!r}")
    N = int(num_beams)
    if not 1 <= N <= MAX_NUM_BEAMS:
        raise ValueError(f"num_beams must lie in [1, {MAX_NUM_BEAMS}] (the beams are the rows of one fused batch), got {N}")
    if batch != 1:
        raise ValueError(f"num_beams needs an observation of batch 1 (its prefix is prefilled once), got batch {batch}")
    if decode not in ("fused", "eager"):
        raise ValueError(f"num_beams needs decode=\"fused\" or \"eager\", got decode={decode!r}")
    if temperature > 0.0:
        raise ValueError(f"num_beams is deterministic: temperature must be 0, got temperature={temperature!r}")
    if sampler == "device":
        raise ValueError("num_beams is deterministic: it does not combine with sampler=\"device\"")
    if num_samples is not None:
        raise ValueError(f"num_beams does not combine with best-of-N: num_samples must be None, got {num_samples!r}")
    if top_k is not None or top_p is not None:
        raise ValueError("num_beams is deterministic: top_k / top_p must be None")
    if speculate is not None:
        raise ValueError("num_beams does not combine with speculate")
    if grammar is not None:         # (the automaton itself is checked by `grammar.check_grammar`, which also rejects allowed_tokens)
        from lap_amd.grammar import DeviceAutomaton, TokenAutomaton

        if not isinstance(grammar.host if isinstance(grammar, DeviceAutomaton) else grammar, TokenAutomaton):
            raise ValueError(f"num_beams combines with grammar= only as a grammar.TokenAutomaton (or its to_device form), got "
                             f"{type(grammar).__name__}")
    if jump_forward is not None:
        raise ValueError("num_beams does not combine with jump_forward")
    if collect is not None:
        raise ValueError("num_beams does not hand out logits: collect must be None")
    return N
