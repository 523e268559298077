"""Greedy speculative decoding of one LAP_AR sequence: the draft rule and the accept rule in numpy, and the checks of the
surface.  This module is the specification of csrc/decode_spec.hip (lap_decode_spec_draft, lap_decode_spec_accept), as
sampling.py and fp8.py are of their kernels; tests/test_speculate_gpu.py compares the kernels with it exactly.

A verify step of S rows (2 <= S <= 8) runs the fused decode kernels on the consecutive positions t-1 .. t-1+S-1 of the sequence:
row 0 feeds the real last token out[t-1], row r the drafted token draft[r-1].  Row r computes what the single-token step at t + r
computes provided drafts 0 .. r-1 were right, so emitting tok[0] and then tok[r] while draft[r-1] == tok[r-1] reproduces the greedy
decode token for token; only the number of passes over the weights changes.

Jump-forward grammar decoding (`jump_forward=S`) runs a grammar-constrained decode (lap_amd/grammar.py) on the same S-row steps.  In
an automaton state with a single edge the next token is known before the model runs, at any temperature, so it is drafted;
elsewhere the reference may draft.  The constrained draw of row r is that of the single-row grammar step at step index t + r from
the state the rows before it led to, so the accepted run reproduces the plain grammar decode, sampled or greedy.
`grammar_drafts`, `grammar_verify` and `replay_grammar` are the specification of lap_decode_grammar_draft and
lap_decode_grammar_spec_finish (csrc/decode_grammar.hip).
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


def _segment(automaton, q: int):
    """The ids state q allows; None for a q outside the automaton (the kernels never use such a q as an address)."""
    return automaton.allowed(int(q)) if 0 <= int(q) < automaton.num_states else None


def grammar_drafts(automaton, q: int, refdraft) -> np.ndarray:
    """The S - 1 drafts of a jump-forward step from the automaton state `q` after the last written token; `refdraft` (int [S-1]) is
    what `draft_tokens(ref, out, t, S)` gives (all -1 without a reference).  For r = 0 .. S-2: a state with one edge drafts that id;
    otherwise refdraft[r] is drafted when the state allows it; otherwise this draft and every later one is -1.  After a drafted
    token q = step(q, draft); drafts after a drafted EOS are -1, as are all drafts from a q outside the automaton."""
    refdraft = np.asarray(refdraft).reshape(-1)
    out = np.full(refdraft.shape[0], -1, dtype=np.int32)
    q = int(q)
    for r in range(refdraft.shape[0]):
        seg = _segment(automaton, q)
        if seg is None:
            break
        d = int(seg[0]) if seg.shape[0] == 1 else int(refdraft[r])
        nq = automaton.step(q, d)
        if nq < 0:
            break
        out[r] = d
        if d == automaton.eos_token:
            break
        q = nq
    return out


def grammar_verify(logits, automaton, q: int, drafts, t: int, cap: int, temperature: float, seed: int):
    """What a jump-forward step emits from its float32 `logits` [S, V]: (emitted int32 [n], logp float64 [n], q_after), with
    out[t + i] = emitted[i].  Row r is the constrained draw of `grammar.decode_reference` for row index 0 at step index t + r from the
    state q_r (q_0 = q, q_{r+1} = step(q_r, tok[r])): `sampling.sample_from_logits` on the logits set to -inf outside allowed(q_r),
    and `sampling.token_logprobs` over that set.  A row whose q_r lies outside the automaton emits the EOS token with
    log-probability -inf and keeps its state.  The accept rule is `accept`'s: tok[0], then tok[r] while tok[r-1] != eos and
    drafts[r-1] == tok[r-1] and t + r < cap.  Empty when t >= cap.  q_after: the state after the last emitted token."""
    from lap_amd import sampling

    lg = np.asarray(logits, dtype=np.float32)
    drafts = np.asarray(drafts).reshape(-1)
    eos = automaton.eos_token
    q = int(q)
    if t >= cap:
        return np.zeros((0,), np.int32), np.zeros((0,), np.float64), q
    emitted, logp = [], []
    for r in range(lg.shape[0]):
        if r > 0 and not (emitted[-1] != eos and int(drafts[r - 1]) == emitted[-1] and t + r < cap):
            break
        seg = _segment(automaton, q)
        if seg is None:
            emitted.append(eos)
            logp.append(-np.inf)
            continue
        masked = np.full((1, lg.shape[1]), -np.inf, dtype=np.float32)
        masked[0, seg] = lg[r, seg]
        tok = sampling.sample_from_logits(masked, temperature, seed, t + r)
        emitted.append(int(tok[0]))
        logp.append(float(sampling.token_logprobs(lg[r:r + 1], tok, temperature, allowed=seg)[0]))
        nq = automaton.step(q, int(tok[0]))
        if nq < 0:
            raise ValueError(f"row {r}: token {int(tok[0])} is not allowed (every allowed logit is -inf or NaN)")
        q = nq
    return np.array(emitted, dtype=np.int32), np.array(logp, dtype=np.float64), q


def replay_grammar(tokens, automaton, ref, S: int, cap: int):
    """(verify_steps, accepted) of a jump-forward decode whose answer is `tokens` (one row of `sample_tokens`, zeros after the
    stop) under the reference `ref`, as `replay` gives them for `speculate`: the steps are replayed with `draft_tokens`,
    `grammar_drafts` and `accept`, row r's token being tokens[t + r] while the drafts before it are right."""
    tokens = np.asarray(tokens).reshape(-1)
    eos = automaton.eos_token
    q = automaton.step(0, int(tokens[0]))
    t, steps, accepted, done = 1, 0, 0, cap <= 1 or int(tokens[0]) == eos
    while not done:
        d = grammar_drafts(automaton, q, draft_tokens(ref, tokens, t, S))
        tok = np.array([int(tokens[t + r]) if t + r < cap else -2 for r in range(S)])
        e = accept(tok, d, t, cap, eos)
        for x in e.tolist():
            q = automaton.step(q, x) if q >= 0 else q
        steps += 1
        accepted += len(e) - 1
        t += len(e)
        done = t >= cap or eos in e.tolist()
    return steps, accepted


def check_jump_forward(jump_forward, batch: int, *, grammar, decode: str = "fused", sampler: str = "device", temperature: float = 0.0,
                       num_samples=None, collect=None) -> int:
    """`jump_forward` of a request as the number of rows S of a step; ValueError naming the condition it breaks."""
    if isinstance(jump_forward, bool) or not isinstance(jump_forward, (int, np.integer)):
        raise ValueError(f"jump_forward must be an integer, got {jump_forward!r}")
    S = int(jump_forward)
    if not MIN_ROWS <= S <= MAX_ROWS:
        raise ValueError(f"jump_forward must lie in [{MIN_ROWS}, {MAX_ROWS}] (the rows of one fused step), got {S}")
    if grammar is None:
        raise ValueError("jump_forward needs grammar= (the forced tokens are those of the automaton's single-edge states)")
    if decode != "fused":
        raise ValueError(f"jump_forward needs decode=\"fused\" (its steps run on the fused decode kernels), got decode={decode!r}")
    if batch != 1:
        raise ValueError(f"jump_forward needs an observation of batch 1 (the rows of a step are positions of one sequence), got batch {batch}")
    if num_samples is not None:
        raise ValueError(f"jump_forward does not combine with best-of-N: num_samples must be None, got {num_samples!r}")
    if collect is not None:
        raise ValueError("jump_forward does not hand out logits: collect must be None")
    if sampler != "device" and temperature > 0.0:
        raise ValueError(f"jump_forward at temperature > 0 needs sampler=\"device\" (the constrained draw is part of the device sampler), "
                         f"got sampler={sampler!r}")
    return S


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
