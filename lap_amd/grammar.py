"""Grammar-constrained LAP_AR decoding: the token automaton, its specification and its builders (numpy only; no GPU code).

A language-action format is a small regular language ("move forward 3 cm, tilt left 10 degrees, open gripper"; H * D integers).
`TokenAutomaton` is a deterministic automaton over token ids in CSR form: state q allows the ids of its segment and every edge
names the next state; the start state is 0.  `LAP.sample_tokens(grammar=automaton)` draws token t of row b among the edges of the
state that row is in, so every answer that ends before its budget is a sentence of the format; rows of one batch (best-of-N) may
be in different states.  The state lives on the device beside the step counter (csrc/decode_grammar.hip), and
`decode_reference` below is the specification of that kernel, as lap_amd/sampling.py is of the sampler.

`automaton_from_words` builds an automaton from a word-level graph (`WordGraph`) and a tokenizer's `encode`;
`lang_actions.word_graph` gives the word graphs of the registered formats and `policy_io.grammar_automaton` joins the two.
"""
from __future__ import annotations

import dataclasses
from collections import deque
from typing import Any, Callable, NamedTuple

import numpy as np

from lap_amd import sampling


@dataclasses.dataclass(frozen=True, eq=False)
class TokenAutomaton:
    """offsets int32 [Q+1], ids int32 [E] (strictly ascending inside every state's segment), next int32 [E]; state q allows
    ids[offsets[q] : offsets[q+1]] and edge e leads to next[e].  The start state is 0.  Every EOS edge leads to a sink state whose
    only edge is EOS -> sink, so a finished row of a batch keeps emitting EOS, as the plain decode lets finished rows run on.
    The constructor does not validate: `check_automaton` does (the builders, `to_device` and the serving surface call it)."""
    offsets: np.ndarray
    ids: np.ndarray
    next: np.ndarray
    vocab_size: int
    eos_token: int

    def __post_init__(self):
        for name in ("offsets", "ids", "next"):
            a = np.ascontiguousarray(np.asarray(getattr(self, name)).reshape(-1).astype(np.int32))
            a.setflags(write=False)
            object.__setattr__(self, name, a)
        object.__setattr__(self, "vocab_size", int(self.vocab_size))
        object.__setattr__(self, "eos_token", int(self.eos_token))

    @property
    def num_states(self) -> int:
        return int(self.offsets.shape[0]) - 1

    @property
    def num_edges(self) -> int:
        return int(self.ids.shape[0])

    def union(self) -> np.ndarray:
        """The sorted unique int32 ids of all edges: what the LM head of a constrained step streams."""
        return np.unique(self.ids).astype(np.int32)

    def allowed(self, q: int) -> np.ndarray:
        """The ids state q allows (ascending)."""
        if not 0 <= q < self.num_states:
            raise ValueError(f"state {q} outside [0, {self.num_states})")
        return self.ids[self.offsets[q]:self.offsets[q + 1]]

    def step(self, q: int, tok: int) -> int:
        """The state after token `tok` in state q (binary search in the segment); -1 when q does not allow it."""
        seg = self.allowed(q)
        i = int(np.searchsorted(seg, tok))
        if i >= seg.shape[0] or int(seg[i]) != int(tok):
            return -1
        return int(self.next[int(self.offsets[q]) + i])

    def accepts(self, tokens) -> bool:
        """True when the run over `tokens` from state 0 stays inside the automaton and ends with an EOS edge.  Tokens after the
        first EOS are not read (a decode's row holds EOS repeats or zeros there); a sequence without an EOS token is accepted when
        it ends in a state that allows EOS (a sentence given without its terminator)."""
        q = 0
        for tok in np.asarray(tokens).reshape(-1).tolist():
            q = self.step(q, tok)
            if q < 0:
                return False
            if tok == self.eos_token:
                return True
        return self.step(q, self.eos_token) >= 0

    def to_device(self, device, check: bool = True) -> "DeviceAutomaton":
        """The checked automaton as int32 tensors on `device` (with its union), for the kernels and the eager route.
        check=False: the caller has run `check_automaton` on this automaton already."""
        import torch

        if check:
            check_automaton(self)
        put = lambda a: torch.from_numpy(np.array(a, dtype=np.int32)).to(device)
        return DeviceAutomaton(put(self.offsets), put(self.ids), put(self.next), put(self.union()), self)


class DeviceAutomaton(NamedTuple):
    """`TokenAutomaton.to_device`: the CSR arrays and the union as int32 device tensors, beside the host automaton."""
    offsets: Any
    ids: Any
    next: Any
    union: Any
    host: TokenAutomaton


def check_automaton(a: TokenAutomaton) -> TokenAutomaton:
    """ValueError naming the condition for: Q < 1 (or offsets that do not delimit ids / next), an empty segment, an id outside
    [0, V), a segment that is not strictly sorted, a next outside [0, Q), an EOS edge that does not lead to a sink (a state whose
    only edge is EOS -> itself), a state from which no EOS edge is reachable.  Returns the automaton."""
    off, ids, nxt, V, eos = a.offsets.astype(np.int64), a.ids.astype(np.int64), a.next.astype(np.int64), a.vocab_size, a.eos_token
    Q, E = off.shape[0] - 1, ids.shape[0]
    if Q < 1:
        raise ValueError(f"automaton: Q < 1 (offsets holds {off.shape[0]} entries, Q + 1 are needed)")
    if nxt.shape[0] != E or off[0] != 0 or off[-1] != E or bool((np.diff(off) < 0).any()):
        raise ValueError(f"automaton: offsets must rise from 0 to E = {E} and next must hold E entries (got {nxt.shape[0]})")
    counts = np.diff(off)
    if bool((counts == 0).any()):
        raise ValueError(f"automaton: state {int(np.flatnonzero(counts == 0)[0])} has an empty segment (a row there could emit nothing)")
    if bool(((ids < 0) | (ids >= V)).any()):
        raise ValueError(f"automaton: ids must lie in [0, {V}), got {int(ids[(ids < 0) | (ids >= V)][0])}")
    src = np.repeat(np.arange(Q, dtype=np.int64), counts)
    inner = np.ones(E, dtype=bool)
    inner[off[:-1]] = False                                  # (the first entry of a segment has no predecessor in it)
    unsorted = inner & (np.concatenate([[0], np.diff(ids)]) <= 0)
    if bool(unsorted.any()):
        raise ValueError(f"automaton: the segment of state {int(src[np.flatnonzero(unsorted)[0]])} is not strictly sorted")
    if bool(((nxt < 0) | (nxt >= Q)).any()):
        raise ValueError(f"automaton: next must lie in [0, {Q}), got {int(nxt[(nxt < 0) | (nxt >= Q)][0])}")
    is_eos = ids == eos
    is_sink = np.zeros(Q, dtype=bool)
    single = np.flatnonzero(counts == 1)
    is_sink[single] = (ids[off[single]] == eos) & (nxt[off[single]] == single)
    if bool((is_eos & ~is_sink[nxt]).any()):
        e = int(np.flatnonzero(is_eos & ~is_sink[nxt])[0])
        raise ValueError(f"automaton: the EOS edge of state {int(src[e])} must lead to a sink (a state whose only edge is EOS -> itself)")
    # backwards from the states with an EOS edge
    reach = np.zeros(Q, dtype=bool)
    reach[src[is_eos]] = True
    order = np.argsort(nxt, kind="stable")
    into = np.searchsorted(nxt[order], np.arange(Q + 1))
    todo = deque(np.flatnonzero(reach).tolist())
    while todo:
        s = todo.popleft()
        for p in src[order[into[s]:into[s + 1]]].tolist():
            if not reach[p]:
                reach[p] = True
                todo.append(p)
    if not bool(reach.all()):
        raise ValueError(f"automaton: no EOS edge is reachable from state {int(np.flatnonzero(~reach)[0])} (a row there could never stop)")
    return a


def check_grammar(grammar, vocab_size: int, eos_token: int, *, allowed_tokens=None, top_k=None, top_p=None, speculate=None,
                  sampler: str = "device", temperature: float = 0.0):
    """The host automaton of a grammar-constrained request (`grammar`: a TokenAutomaton or its `to_device` form), checked
    (`check_automaton`) and compared with the model's vocabulary and EOS token; ValueError naming what it does not combine with:
    allowed_tokens (the automaton's union replaces the set), top_k / top_p, speculate, and the host sampler at temperature > 0
    (the constrained draw is part of the device sampler)."""
    host = grammar.host if isinstance(grammar, DeviceAutomaton) else grammar
    if not isinstance(host, TokenAutomaton):
        raise ValueError(f"grammar: expected a grammar.TokenAutomaton (or its to_device form), got {type(grammar).__name__}")
    if allowed_tokens is not None:
        raise ValueError("grammar does not combine with allowed_tokens: the union of the automaton's edges replaces the set")
    if top_k is not None or top_p is not None:
        raise ValueError("grammar does not combine with top_k / top_p")
    if speculate is not None:
        raise ValueError("grammar does not combine with speculate")
    if sampler != "device" and temperature > 0.0:
        raise ValueError(f"grammar at temperature > 0 needs sampler=\"device\" (the constrained draw is part of the device sampler), "
                         f"got sampler={sampler!r}")
    if (host.vocab_size, host.eos_token) != (vocab_size, eos_token):
        raise ValueError(f"grammar: the automaton was built for vocab_size {host.vocab_size} and EOS token {host.eos_token}, the model "
                         f"has vocab_size {vocab_size} and EOS token {eos_token}")
    if not isinstance(grammar, DeviceAutomaton):        # (`to_device` has checked the other form)
        check_automaton(host)
    return host


def decode_reference(logits_per_step, automaton: TokenAutomaton, temperature: float, seed: int, rows: int | None = None, start=None):
    """The specification of the grammar-constrained draw (csrc/decode_grammar.hip), on float32 logits [T, B, V] of T steps.
    At step t, row b in state q takes `sampling.sample_from_logits` of its logits set to -inf outside `allowed(q)`: the argmax of
    float32(logit * inv_t) + the noise of the VOCABULARY index, (j >> 1, b, t), as everywhere; the argmax with the lowest index
    among ties when temperature <= 0.  Then q = step(q, token).  The log-probability is `sampling.token_logprobs(...,
    allowed=allowed(q))`: the token's probability under the noise-free softmax over that state's set.
    rows: B (checked when given).  start: the state of every row before step 0 (default: the start state 0).
    Returns (tokens int32 [B, T], logprobs float64 [B, T], states int32 [B, T + 1])."""
    lg = np.asarray(logits_per_step, dtype=np.float32)
    if lg.ndim != 3:
        raise ValueError("logits_per_step: [T, B, V]")
    T, B, V = lg.shape
    if rows is not None and int(rows) != B:
        raise ValueError(f"rows = {rows} but logits_per_step holds {B} rows")
    if V != automaton.vocab_size:
        raise ValueError(f"logits of width {V} for an automaton over {automaton.vocab_size} ids")
    q = np.zeros(B, dtype=np.int64) if start is None else np.asarray(start, dtype=np.int64).reshape(B).copy()
    tokens = np.zeros((B, T), dtype=np.int32)
    logp = np.zeros((B, T), dtype=np.float64)
    states = np.zeros((B, T + 1), dtype=np.int32)
    states[:, 0] = q
    for t in range(T):
        masked = np.full((B, V), -np.inf, dtype=np.float32)
        sets = [automaton.allowed(int(q[b])) for b in range(B)]
        for b in range(B):
            masked[b, sets[b]] = lg[t, b, sets[b]]
        tok = sampling.sample_from_logits(masked, temperature, seed, t)
        for b in range(B):
            logp[b, t] = sampling.token_logprobs(lg[t, b:b + 1], tok[b:b + 1], temperature, allowed=sets[b])[0]
            q[b] = automaton.step(int(q[b]), int(tok[b]))
            if q[b] < 0:
                raise ValueError(f"step {t}, row {b}: token {int(tok[b])} is not allowed (every allowed logit is -inf or NaN)")
        tokens[:, t] = tok
        states[:, t + 1] = q
    return tokens, logp, states


# ------------------------------------------------------------------------------------------------ builders
class WordGraph(NamedTuple):
    """A word-level deterministic automaton: edges {state: [(word, next_state), ...]} (states are any hashable values), the start
    state and the accepting states.  A sentence is the words of a path from `start` to an accepting state, joined by blanks."""
    edges: dict
    start: Any
    accepting: frozenset


def sentences(graph: WordGraph, limit: int = 100000) -> list[str]:
    """Every sentence of an acyclic word graph (depth first, in edge order); ValueError beyond `limit` sentences."""
    out: list[str] = []

    def walk(s, words):
        if s in graph.accepting:
            out.append(" ".join(words))
            if len(out) > limit:
                raise ValueError(f"sentences: more than {limit}")
        for word, nxt in graph.edges.get(s, ()):
            walk(nxt, words + [word])

    walk(graph.start, [])
    return out


def random_sentences(graph: WordGraph, n: int, seed: int = 0, max_words: int = 4096) -> list[str]:
    """n sentences from random walks over the word graph (an accepting state that has edges stops with probability 1/2)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        s, words = graph.start, []
        while len(words) <= max_words:
            outs = graph.edges.get(s, ())
            if s in graph.accepting and (not outs or rng.random() < 0.5):
                out.append(" ".join(words))
                break
            if not outs:
                raise ValueError(f"word graph: state {s!r} has no edge and does not accept")
            word, s = outs[int(rng.integers(len(outs)))]
            words.append(word)
        else:
            raise ValueError(f"random_sentences: a walk of more than {max_words} words")
    return out


def automaton_from_words(encode: Callable[[str], Any], graph: WordGraph, eos_token: int, vocab_size: int) -> TokenAutomaton:
    """The token automaton of a word graph.  Each word becomes the chain `encode(word)` of token ids; the chains that leave one
    state are merged as a trie (two words that share a token prefix share those states), the end of a chain continues with the
    next state's trie, and accepting states get the EOS edge to the sink, which is the last state.  Where one word's chain is a
    prefix of another's ("1" and "10" under a digit tokenizer) the end of the shorter is both: the states are the sets of trie
    positions a token sequence can be in (the subset construction), so the result is deterministic for any `encode`.

    This rests on the tokenizer never merging across whitespace: the encoding of a sentence must be the concatenation of the
    encodings of its words, each as `encode` gives it for the word on its own (SentencePiece with its default whitespace split
    and dummy prefix: every word starts with a "▁" piece and no piece spans two words).  `policy_io.grammar_automaton` checks that
    on full sentences."""
    eos_token, vocab_size = int(eos_token), int(vocab_size)
    children: list[dict] = []           # trie position -> {token: position}
    ends: list[list] = []               # trie position -> the word states whose trie continues there
    root: dict = {}

    def new():
        children.append({})
        ends.append([])
        return len(children) - 1

    def root_of(s):
        if s not in root:
            root[s] = new()
        return root[s]

    root_of(graph.start)
    chains: dict = {}
    for s, outs in graph.edges.items():
        for word, nxt in outs:
            if word not in chains:
                chains[word] = [int(t) for t in encode(word)]
                if not chains[word]:
                    raise ValueError(f"automaton_from_words: {word!r} encodes to no token")
                if eos_token in chains[word]:
                    raise ValueError(f"automaton_from_words: {word!r} encodes to the EOS token {eos_token}")
            n = root_of(s)
            for tok in chains[word]:
                if tok not in children[n]:
                    children[n][tok] = new()
                n = children[n][tok]
            if root_of(nxt) not in ends[n]:
                ends[n].append(root_of(nxt))
    accepting = {root_of(s) for s in graph.accepting}

    start = frozenset([root[graph.start]])
    number = {start: 0}
    todo = deque([start])
    table: list[list] = []              # state -> [(token, next state)]
    accepts: list[bool] = []
    while todo:
        cur = todo.popleft()
        moves: dict = {}
        for n in cur:
            for tok, c in children[n].items():
                moves.setdefault(tok, set()).update([c, *ends[c]])
        row = []
        for tok in sorted(moves):
            tgt = frozenset(moves[tok])
            if tgt not in number:
                number[tgt] = len(number)
                todo.append(tgt)
            row.append((tok, number[tgt]))
        table.append(row)
        accepts.append(bool(cur & accepting))
    sink = len(table)
    offsets, ids, nxt = [0], [], []
    for row, acc in zip(table, accepts):
        if acc:
            row = sorted(row + [(eos_token, sink)])
        ids += [t for t, _ in row]
        nxt += [s for _, s in row]
        offsets.append(len(ids))
    ids.append(eos_token)
    nxt.append(sink)
    offsets.append(len(ids))
    return check_automaton(TokenAutomaton(np.array(offsets), np.array(ids), np.array(nxt), vocab_size, eos_token))


def single_state_automaton(ids, eos_token: int, vocab_size: int) -> TokenAutomaton:
    """The automaton of `allowed_tokens=ids`: one state that loops over the set (which must hold the EOS token), and the sink."""
    ids = np.unique(np.asarray(ids).reshape(-1).astype(np.int64))
    if not bool((ids == eos_token).any()):
        raise ValueError(f"single_state_automaton: the EOS token {eos_token} is not in the set")
    nxt = np.where(ids == eos_token, 1, 0)
    return check_automaton(TokenAutomaton(np.array([0, len(ids), len(ids) + 1]), np.concatenate([ids, [eos_token]]),
                                          np.concatenate([nxt, [1]]), vocab_size, eos_token))
