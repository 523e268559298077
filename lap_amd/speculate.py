"""Greedy speculative decoding of one LAP_AR sequence: the draft rule and the accept rule in numpy, and the checks of the
surface.  This module is the specification of csrc/decode_spec.hip (lap_decode_spec_draft, lap_decode_spec_accept), as
sampling.py and fp8.py are of their kernels; tests/test_speculate_gpu.py compares the kernels with it exactly.

A verify step of S rows (2 <= S <= 8) runs the fused decode kernels on the consecutive positions t-1 .. t-1+S-1 of the sequence:
row 0 feeds the real last token out[t-1], row r the drafted token draft[r-1].  Row r computes what the single-token step at t + r
computes provided drafts 0 .. r-1 were right, so emitting tok[0] and then tok[r] while draft[r-1] == tok[r-1] reproduces the greedy
decode token for token; only the number of passes over the weights changes.
"""
from __future__ import annotations

import numpy as np

MIN_ROWS, MAX_ROWS = 2, 8       # rows of a verify step (the fused decode kernels serve 1 <= B <= 8 rows)


def draft_tokens(ref, out, t: int, S: int) -> np.ndarray:
    """The S - 1 drafted tokens after `t` tokens of `out` have been written (t >= 1), from the reference sequence `ref` (None or
    empty: no draft).  last = out[t-1], prev = out[t-2] (t >= 2).  An anchor is an index a < n with ref[a] == last; a 2-gram
    anchor also has a >= 1 and ref[a-1] == prev.  The 2-gram anchor that minimises |a - (t-1)| is taken (the lower a on a tie);
    without one, the 1-gram anchor by the same rule; without one, a = t-1.  draft[r] = ref[a+1+r] when a+1+r < n, else -1, which
    never equals a token."""
    ref = np.zeros((0,), np.int64) if ref is None else np.asarray(ref).reshape(-1).astype(np.int64)
    out = np.asarray(out).reshape(-1)
    n = ref.shape[0]
    if t < 1:
        raise ValueError(f"draft_tokens: t >= 1 (the first token comes from the prefill), got {t}")
    last = int(out[t - 1])
    best2 = best1 = None
    for a in range(n):
        if int(ref[a]) != last:
            continue
        key = (abs(a - (t - 1)), a)
        if best1 is None or key < best1:
            best1 = key
        if t >= 2 and a >= 1 and int(ref[a - 1]) == int(out[t - 2]) and (best2 is None or key < best2):
            best2 = key
    a = best2[1] if best2 is not None else best1[1] if best1 is not None else t - 1
    return np.array([int(ref[a + 1 + r]) if a + 1 + r < n else -1 for r in range(S - 1)], dtype=np.int32)


def accept(tok, draft, t: int, cap: int, eos: int) -> np.ndarray:
    """The tokens a verify step emits (out[t + i] = emitted[i]) from its S argmax tokens `tok` and S - 1 drafts: tok[0], and for
    r = 1 .. S-1 tok[r] while tok[r-1] != eos and draft[r-1] == tok[r-1] and t + r < cap.  Empty when t >= cap (the step then only
    sets done).  After n tokens: t + n tokens are written, the decode is done when t + n >= cap or an emitted token is the EOS,
    the step counts 1 verify step and n - 1 accepted drafts."""
    tok = np.asarray(tok).reshape(-1)
    draft = np.asarray(draft).reshape(-1)
    if t >= cap:
        return np.zeros((0,), np.int32)
    emitted = [int(tok[0])]
    for r in range(1, tok.shape[0]):
        if not (int(tok[r - 1]) != eos and int(draft[r - 1]) == int(tok[r - 1]) and t + r < cap):
            break
        emitted.append(int(tok[r]))
    return np.array(emitted, dtype=np.int32)


def replay(tokens, ref, S: int, cap: int, eos: int):
    """(verify_steps, accepted) of a speculative decode whose greedy answer is `tokens` (one row of `sample_tokens`, zeros after
    the stop) under the reference `ref`: the verify steps are replayed with `draft_tokens` and `accept`, row r's argmax being
    tokens[t + r] while the drafts before it are right (what a wrong row computes is never emitted)."""
    tokens = np.asarray(tokens).reshape(-1)
    t, steps, accepted, done = 1, 0, 0, cap <= 1 or int(tokens[0]) == eos
    while not done:
        d = draft_tokens(ref, tokens, t, S)
        tok = np.array([int(tokens[t + r]) if t + r < cap else -2 for r in range(S)])
        e = accept(tok, d, t, cap, eos)
        steps += 1
        accepted += len(e) - 1
        t += len(e)
        done = t >= cap or eos in e.tolist()
    return steps, accepted


def check_speculate(speculate, batch: int, *, decode: str = "fused", temperature: float = 0.0, return_logprobs: bool = False,
                    num_samples=None, top_k=None, top_p=None, collect=None) -> int:
    """`speculate` of a request as the number of rows S of a verify step; ValueError naming the condition it breaks."""
    if isinstance(speculate, bool) or not isinstance(speculate, (int, np.integer)):
        raise ValueError(f"speculate must be an integer, got {speculate!r}")
    S = int(speculate)
    if not MIN_ROWS <= S <= MAX_ROWS:
        raise ValueError(f"speculate must lie in [{MIN_ROWS}, {MAX_ROWS}] (the rows of one fused verify step), got {S}")
    if batch != 1:
        raise ValueError(f"speculate needs an observation of batch 1 (the rows of a step are positions of one sequence), got batch {batch}")
    if decode != "fused":
        raise ValueError(f"speculate needs decode=\"fused\" (a verify step runs on the fused decode kernels), got decode={decode!r}")
    if temperature > 0.0:
        raise ValueError(f"speculate is greedy: temperature > 0 needs sampling LM heads that take the step per row, got temperature={temperature!r}")
    if return_logprobs:
        raise ValueError("speculate does not return log-probabilities: return_logprobs must be False")
    if num_samples is not None:
        raise ValueError(f"speculate does not combine with best-of-N: num_samples must be None, got {num_samples!r}")
    if top_k is not None or top_p is not None:
        raise ValueError("speculate is greedy: top_k / top_p must be None")
    if collect is not None:
        raise ValueError("speculate does not store logits: collect must be None")
    return S
