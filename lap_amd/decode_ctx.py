"""`DecodeCtx`: the device-side context of one fused LAP_AR decode on the single-token kernels of csrc/decode*.hip.  The core (state,
output, generated K/V cache, step activations, the layers of a step) is the class; what a decode MODE adds to it is one row of
`KINDS`: its buffers, what `first_token` resets, the head + finish of the first token, and a step's prologue / embed and head + finish.
The constructor picks the row once.  `ar_decode` builds the prefill, drives the context and routes requests to it;
`serve.GraphedTokenDecoder` captures `prefill` + `first_token` and `step` into two graphs.
"""
from __future__ import annotations

import math
from typing import Callable, NamedTuple

import torch

from lap_amd import hip
from lap_amd.grammar import check_grammar
from lap_amd.model import LAP
from lap_amd.score import check_score_ctx
from lap_amd.speculate import check_jump_forward, check_speculate


def check_decode_weights(weights):
    if weights not in LAP.DECODE_WEIGHTS:
        raise ValueError(f"decode_weights must be one of {LAP.DECODE_WEIGHTS}, got {weights!r}")


class Kind(NamedTuple):
    """What one kind of context adds to the core.  `c` is the DecodeCtx."""
    buffers: Callable       # (c): allocate what the kind owns beyond the core
    reset: Callable         # (c): the device ops of `first_token` after lap_decode_init (a captured prefill graph replays them)
    first: Callable         # (c, x, logits): head + finish of the first token, on the prefill's last rows
    embed: Callable         # (c, table, scale): a step's prologue and embed into c.x
    token: Callable         # (c, x, logits): a step's head + finish on the R rows of c.x


def _nothing(c):
    pass


def _reset_logp(c):
    if c.logp is not None:
        c.logp.zero_()


def _embed(c, table, scale):
    hip.decode_embed(c.state, *table, c.out, c.x, scale)


def _head_logits(c):
    """The f32 [B, V] logits a plain head stores for a finish that draws from them: -inf outside an allowed set, written once (the
    constrained head writes the allowed columns only)."""
    lg = torch.empty((c.B, c.model.config.vocab_size), dtype=torch.float32, device=c.model.device)
    if c.allowed is not None:
        lg.fill_(float("-inf"))
    return lg


# ---- plain: the greedy or the sampling head, then lap_decode_finish
def _plain_token(c, x, logits):
    """final norm + LM head over the hi / lo planes + argmax -> out[:, t], EOS mask, t + 1 (lap.py:716-724).  A context with sampling
    words runs the sampling LM head, which is the greedy one while the words hold inv_t = 0."""
    norm, hi, lo, kw = c._lm_head()
    if c.sampling is not None:
        hip.decode_lm_head_sample(c.state, c.sampling, x, norm, hi, lo, c.pval, c.pidx, logits, **kw)
    else:
        hip.decode_lm_head(c.state, x, norm, hi, lo, c.pval, c.pidx, logits, **kw)
    hip.decode_finish(c.state, c.pval, c.pidx, c.out, c.model.EOS_TOKEN)


# ---- logprob (logprobs=True): the same head with the log-sum-exp partials, and the finish that turns them into logp[:, t]
def _logprob_buffers(c):
    c.plp = hip.decode_lm_logp_partials(c.R, c.model.device)


def _logprob_token(c, x, logits):
    norm, hi, lo, kw = c._lm_head()
    hip.decode_lm_head_lp(c.state, c.sampling, x, norm, hi, lo, c.pval, c.pidx, c.plp, logits, **kw)
    hip.decode_finish_lp(c.state, c.pval, c.pidx, c.plp, c.out, c.logp, c.model.EOS_TOKEN)


# ---- filter (filtering=True; needs sampling=True)
def _filter_buffers(c):
    """The context draws through top-k / top-p filter words {top_k, bits of top_p, 0, 0} (neutral until `set_filter`): its LM head
    is the plain greedy one, which stores its f32 logits in a [B, V] buffer the context owns (its partials are not read), and
    lap_decode_filter_finish draws from that buffer and does the finish's bookkeeping."""
    c.filter = hip.decode_filter(c.model.device)
    c.logits = _head_logits(c)
    if c.logp is not None:      # (allocated beside `logp` as in every context without a grammar; the filter finish does not read it)
        _logprob_buffers(c)


def _filter_token(c, x, logits):
    norm, hi, lo, kw = c._lm_head()
    hip.decode_lm_head(c.state, x, norm, hi, lo, c.pval, c.pidx, c.logits, **kw)
    hip.decode_filter_finish(c.state, c.sampling, c.filter, c.logits, c.out, c.model.EOS_TOKEN, logp=c.logp)
    if logits is not None:      # (debug: the caller's copy of what the draw saw)
        logits.copy_(c.logits)


# ---- grammar (grammar=DeviceAutomaton; not with allowed, filtering or speculate)
def _grammar_buffers(c):
    """The context draws every row's token among the edges of the automaton state that row is in (lap_amd/grammar.py).  It owns
    `gstate` (int32 [B], zeroed by `first_token` with a device op that a captured prefill replays) and an [R, V] f32 logits buffer,
    written to -inf once; its LM head is the plain SUBSET head (bf16 or fp8) over the automaton's union, which stores its logits
    there, and lap_decode_grammar_finish draws from them, moves `gstate` and does the finish's bookkeeping, with the log-probability
    over the state's set when logprobs is on."""
    dev = c.model.device
    c.gstate = torch.zeros((c.B,), dtype=torch.int32, device=dev)
    c.logits = torch.full((c.R, c.model.config.vocab_size), float("-inf"), dtype=torch.float32, device=dev)


def _grammar_reset(c):          # every request starts in state 0
    _reset_logp(c)
    c.gstate.zero_()


def _grammar_token(c, x, logits):
    norm, hi, lo, kw = c._lm_head()
    g = c.grammar
    lg = c.logits[:c.B]         # (a jump-forward context's first token: row 0 of its S rows)
    hip.decode_lm_head(c.state, x, norm, hi, lo, c.pval, c.pidx, lg, **(kw | {"ids": g.union}))
    hip.decode_grammar_finish(c.state, c.sampling, c.gstate, g.offsets, g.ids, g.next, lg, c.out, c.model.EOS_TOKEN, logp=c.logp)
    if logits is not None:      # (debug: the caller's copy of what the draw saw)
        logits.copy_(lg)


# ---- speculate (speculate=S, 2 <= S <= 8; B = 1, greedy, no log-probabilities)
def _draft_buffers(c):
    """The context decodes ONE sequence on verify steps of S rows (lap_amd/speculate.py, csrc/decode_spec.hip).  The state, `out`,
    `plen` and the generated cache stay those of B = 1; the activations, the attention scratch and the LM partials hold S rows; a
    reference sequence {length, ids[cap]} lives in one device buffer at a fixed address (`set_draft`) beside the S - 1 drafted
    tokens of the step.  `first_token` runs the plain B = 1 head and finish; `step` drafts S - 1 tokens from the reference, runs
    the layers on the S positions t-1 .. t-1+S-1 and accepts the longest verified run; `stats` reads the counters.  The tokens
    are those of the context without it."""
    c.ref = hip.decode_spec_ref(c.cap, c.model.device)
    c.draft = torch.full((c.R - 1,), -1, dtype=torch.int32, device=c.model.device)


def _spec_embed(c, table, scale):
    hip.decode_spec_draft(c.state, c.ref, c.out, c.draft)
    hip.decode_spec_embed(c.state, *table, c.out, c.draft, c.x, scale)


def _spec_token(c, x, logits):
    norm, hi, lo, kw = c._lm_head()
    hip.decode_lm_head(c.state, x, norm, hi, lo, c.pval, c.pidx, None, **kw)
    hip.decode_spec_accept(c.state, c.pval, c.pidx, c.draft, c.out, c.model.EOS_TOKEN)


# ---- jump-forward (jump_forward=S, 2 <= S <= 8; needs grammar, B = 1; with or without sampling and logprobs)
def _jump_buffers(c):
    """The grammar context decodes ONE sequence on steps of S rows, in the arrangement of speculate=S (state, `out`, `logp`, `gstate`
    and the generated cache of B = 1; activations, attention scratch, LM partials and the logits buffer of S rows).  `first_token`
    runs the single-row grammar head and finish on logits[:B]; `step` drafts from the reference (`set_draft`), overwrites the
    drafts with the grammar's (lap_decode_grammar_draft: a state with one edge forces its token), runs the layers on the S
    positions, the plain SUBSET head over the union on the S rows, and lap_decode_grammar_spec_finish, which draws the rows in
    sequence with the single-row finish's bits and accepts the longest verified run.  Tokens and log-probabilities are those of
    the grammar context without it; `stats` reads the counters."""
    _grammar_buffers(c)
    _draft_buffers(c)


def _jump_embed(c, table, scale):
    g = c.grammar
    hip.decode_spec_draft(c.state, c.ref, c.out, c.draft)
    hip.decode_grammar_draft(c.state, c.gstate, g.offsets, g.ids, g.next, c.draft, c.out, c.model.config.vocab_size, c.model.EOS_TOKEN)
    hip.decode_spec_embed(c.state, *table, c.out, c.draft, c.x, scale)


def _jump_token(c, x, logits):
    norm, hi, lo, kw = c._lm_head()
    g = c.grammar
    hip.decode_lm_head(c.state, x, norm, hi, lo, c.pval, c.pidx, c.logits, **(kw | {"ids": g.union}))
    hip.decode_grammar_spec_finish(c.state, c.sampling, c.gstate, g.offsets, g.ids, g.next, c.logits, c.draft, c.out,
                                   c.model.EOS_TOKEN, logp=c.logp)


# ---- beam (beams=N, B = N; greedy, not with filtering, speculate or jump_forward; composes with weights and allowed)
def _beam_words(c):
    dev = c.model.device
    c.beam_init = hip.decode_beam_init_words(c.B, c.early_stop, dev)
    c.beam = c.beam_init.clone()
    c.cand_logp = torch.zeros((c.B, c.B), dtype=torch.float32, device=dev)
    c.cand_id = torch.full((c.B, c.B), -1, dtype=torch.int32, device=dev)


def _beam_buffers(c):
    """The rows are the beams of one beam search (lap_amd/beam.py, csrc/decode_beam.hip).  The context owns the beam buffer (scores,
    finished, parent, the `early_stop` flag; reset by `first_token` with a device copy of `beam_init` that a captured prefill
    replays), the [N, V] f32 logits of the step, the [N, N] best (log-probability, id) of every row and `logp`.  Its LM head is the
    plain greedy one (plain / SUBSET / fp8), which stores its logits; lap_decode_beam_topn and lap_decode_beam_select finish the
    step, and `step` starts with lap_decode_beam_reorder, which moves the generated K / V rows to the parents the last select
    chose.  `beam_result` hands out all beams."""
    _beam_words(c)
    c.logits = _head_logits(c)


def _beam_reset(c):             # every request starts from {0, -inf, ...}
    c.logp.zero_()
    c.beam.copy_(c.beam_init)


def _beam_embed(c, table, scale):
    hip.decode_beam_reorder(c.state, c.beam, c.gen)
    hip.decode_embed(c.state, *table, c.out, c.x, scale)


def _beam_token(c, x, logits):
    norm, hi, lo, kw = c._lm_head()
    m = c.model
    hip.decode_lm_head(c.state, x, norm, hi, lo, c.pval, c.pidx, c.logits, **kw)
    hip.decode_beam_topn(c.state, c.beam, c.logits, c.cand_logp, c.cand_id, c.cap)
    hip.decode_beam_select(c.state, c.beam, c.cand_logp, c.cand_id, c.out, c.logp, m.config.vocab_size, m.EOS_TOKEN)


# ---- grammar-beam (beams=N with grammar=DeviceAutomaton)
def _grammar_beam_buffers(c):
    """The beams are the most probable sentences of the automaton (`beam.grammar_beam_step`).  Beside the beam context's buffers the
    context owns `gstate` [N] (every beam's automaton state), the grammar context's logits (-inf outside the union) and
    `cand_next`; the head is the SUBSET head over the automaton's union, lap_decode_beam_grammar_topn reads only the edges of
    every row's state and lap_decode_beam_grammar_select carries the states along the parent permutation."""
    _grammar_buffers(c)
    _beam_words(c)
    c.cand_next = torch.full((c.B, c.B), -1, dtype=torch.int32, device=c.model.device)


def _grammar_beam_reset(c):
    c.logp.zero_()
    c.gstate.zero_()
    c.beam.copy_(c.beam_init)


def _grammar_beam_token(c, x, logits):
    norm, hi, lo, kw = c._lm_head()
    m, g = c.model, c.grammar
    hip.decode_lm_head(c.state, x, norm, hi, lo, c.pval, c.pidx, c.logits, **(kw | {"ids": g.union}))
    hip.decode_beam_grammar_topn(c.state, c.beam, c.gstate, g.offsets, g.ids, g.next, c.logits, c.cand_logp, c.cand_id, c.cand_next, c.cap)
    hip.decode_beam_grammar_select(c.state, c.beam, c.gstate, c.cand_logp, c.cand_id, c.cand_next, c.out, c.logp, m.config.vocab_size,
                                   m.EOS_TOKEN)


# ---- score (score=S, 1 <= S <= 8; B = 1; composes with weights and allowed, with nothing else)
def _score_buffers(c):
    """The context scores a GIVEN sequence instead of decoding one (lap_amd/score.py, csrc/decode_score.hip).  The arrangement is
    that of speculate=S (at S = 1: the plain B = 1 layers); the candidate lives in the reference buffer (`set_candidate`) and
    nothing is drafted, `logp` [1, cap] receives the log-probability of every given token and `greedy` [1, cap] the argmax id at
    its position; `out` stays zero.  `score_words` carry the temperature of z to the TARGET head (zeros: z = logit;
    `set_score_temperature`).  `first_token` scores token 0 from the prefill's last row, every `step` feeds row r the
    candidate's ids[t-1+r] and scores the next min(S, length - t) tokens on one pass over the weights; the context is done when
    all are scored.  `stats` reads the counters."""
    dev = c.model.device
    c.ref = hip.decode_spec_ref(c.cap, dev)
    _logprob_buffers(c)
    c.greedy = torch.zeros((c.B, c.cap), dtype=torch.int32, device=dev)
    c.score_words = hip.decode_sampling(dev)


def _score_reset(c):
    c.logp.zero_()
    c.greedy.zero_()


def _score_embed(c, table, scale):
    hip.decode_score_embed(c.state, *table, c.ref, c.x, scale)


def _score_token(c, x, logits):
    norm, hi, lo, kw = c._lm_head()
    hip.decode_lm_head_score(c.state, c.score_words, c.ref, x, norm, hi, lo, c.pval, c.pidx, c.plp, logits, **kw)
    hip.decode_score_finish(c.state, c.pval, c.pidx, c.plp, c.ref, c.logp.view(-1), c.greedy.view(-1), x.shape[0])


#                             buffers                reset                first           embed         token
KINDS = {
    "plain":        Kind(_nothing,              _nothing,            _plain_token,        _embed,       _plain_token),
    "logprob":      Kind(_logprob_buffers,      _reset_logp,         _logprob_token,      _embed,       _logprob_token),
    "filter":       Kind(_filter_buffers,       _reset_logp,         _filter_token,       _embed,       _filter_token),
    "grammar":      Kind(_grammar_buffers,      _grammar_reset,      _grammar_token,      _embed,       _grammar_token),
    "speculate":    Kind(_draft_buffers,        _nothing,            _plain_token,        _spec_embed,  _spec_token),
    "jump-forward": Kind(_jump_buffers,         _grammar_reset,      _grammar_token,      _jump_embed,  _jump_token),
    "beam":         Kind(_beam_buffers,         _beam_reset,         _beam_token,         _beam_embed,  _beam_token),
    "grammar-beam": Kind(_grammar_beam_buffers, _grammar_beam_reset, _grammar_beam_token, _beam_embed,  _grammar_beam_token),
    "score":        Kind(_score_buffers,        _score_reset,        _score_token,        _score_embed, _score_token),
}


class DecodeCtx:
    """One fused decode of `model` (B rows, `Pn` prefix keys, `cap` = max_decoding_steps).  The core: the device state, `plen`, the
    token output `out`, the fixed-capacity generated K/V cache of every layer (`gen` [depth, 2, B, cap, head_dim] bf16, 7.2 MB per
    sample at 390 steps for LAP-3B), the activations of a step's R rows (`x`, `xa`, `q`, `o`, `act`, the attention scratch and the
    LM partials `pval` / `pidx`; R = B, or the S positions of ONE sequence in a speculate / jump_forward / score context), and
    the layers of a step.  The prefix K/V cache and kinfo come from the prefill (`first_token` -> `bind`).
    `weights` ("bf16", "fp8": projections + LM head, "fp8_layers") and `allowed` (the int32 device ids of the allowed set of every
    token) change only the weights the layers stream and what the LM heads receive (`_w`, `_lm_head`); `sampling` gives the context
    the sampling words {seed low, seed high, bits of 1 / temperature, 0} (zeros: greedy; `set_sampling`) and `logprobs` (forced by
    beams and score) the log-probability of every token of `out` beside it (`logp` f32 [B, cap], zeros where nothing was written).
    Everything else is the context's `kind`, one row of `KINDS`, decided here and nowhere else: plain, logprob, filter, grammar,
    speculate, jump-forward, beam, grammar-beam or score; each is described at its functions above.  Attributes a kind does not
    own are None."""

    def __init__(self, model: LAP, B: int, Pn: int, cap: int, sampling: bool = False, weights: str = "bf16", allowed=None,
                 logprobs: bool = False, filtering: bool = False, speculate=None, grammar=None, jump_forward=None, beams=None,
                 early_stop: bool = True, score=None):
        check_decode_weights(weights)
        self.score = None
        if score is not None:
            self.score = check_score_ctx(score, B, sampling=sampling, filtering=filtering, speculate=speculate, grammar=grammar,
                                         jump_forward=jump_forward, beams=beams)
            logprobs = True
        self.beams = None
        if beams is not None:
            from lap_amd.beam import check_num_beams

            self.beams = check_num_beams(beams, 1, temperature=1.0 if sampling else 0.0, top_k=0 if filtering else None,
                                         speculate=speculate, grammar=grammar, jump_forward=jump_forward)
            if B != self.beams:
                raise ValueError(f"DecodeCtx: beams={self.beams} are the rows of the batch, got B {B}")
            logprobs = True
        self.J = None
        if jump_forward is not None:
            self.J = check_jump_forward(jump_forward, B, grammar=grammar)
        if grammar is not None:
            check_grammar(grammar, model.config.vocab_size, model.EOS_TOKEN, allowed_tokens=allowed, top_k=0 if filtering else None,
                          speculate=speculate)
            if not grammar.ids.is_cuda:
                raise ValueError("DecodeCtx: grammar must be the automaton on the device (TokenAutomaton.to_device)")
        self.grammar = grammar          # None, or the device automaton (captured graphs keep its buffers' addresses)
        self.S = None
        if speculate is not None:
            self.S = check_speculate(speculate, B, return_logprobs=logprobs, temperature=1.0 if sampling else 0.0)
        if filtering and not sampling:
            raise ValueError("DecodeCtx: filtering needs sampling=True (the filters are part of the device sampler)")
        if allowed is not None and (allowed.dtype != torch.int32 or not allowed.is_cuda or allowed.dim() != 1):
            raise ValueError("DecodeCtx: allowed must be the int32 device ids of check_allowed_tokens")
        self.allowed = allowed          # (captured graphs keep the buffer's address)
        self.kind = ("score" if self.score is not None else "grammar-beam" if self.beams is not None and grammar is not None else
                     "beam" if self.beams is not None else "jump-forward" if self.J is not None else
                     "speculate" if self.S is not None else "grammar" if grammar is not None else "filter" if filtering else
                     "logprob" if logprobs else "plain")
        self._kind = KINDS[self.kind]
        v = model.v
        self.model = model
        self.weights = weights
        self.early_stop = early_stop
        dev = model.device
        bf = torch.bfloat16
        self.B, self.Pn, self.cap = B, Pn, cap
        self.R = R = self.S or self.J or self.score or B        # rows of a step's activations
        self.rows_of_one = R != B       # the rows are S >= 2 positions of one sequence: the layers run the multi-row qkv / attention
        self.state = hip.decode_state(B, dev)
        self.plen = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.out = torch.zeros((B, cap), dtype=torch.int32, device=dev)
        self.gen = torch.zeros((v.depth, 2, B, cap, v.head_dim), dtype=bf, device=dev)
        self.x = torch.zeros((R, v.width), dtype=bf, device=dev)
        self.xa = torch.zeros((R, v.width), dtype=bf, device=dev)
        self.q = torch.zeros((R, v.num_heads * v.head_dim), dtype=bf, device=dev)
        self.o = torch.zeros((R, v.num_heads * v.head_dim), dtype=bf, device=dev)
        self.act = torch.zeros((R, v.mlp_dim), dtype=bf, device=dev)
        self.attn_scratch = hip.decode_attn_scratch(R, Pn, cap, dev)
        self.pval, self.pidx = hip.decode_lm_partials(R, dev)
        self.sampling = hip.decode_sampling(dev) if sampling else None
        self.logp = torch.zeros((B, cap), dtype=torch.float32, device=dev) if logprobs else None
        self.ref = self.draft = self.plp = self.greedy = self.score_words = self.filter = self.logits = self.gstate = None
        self.beam = self.beam_init = self.cand_logp = self.cand_id = self.cand_next = None
        self._kind.buffers(self)
        self.prefix = None
        self.kinfo = None

    def beam_result(self):
        """All beams of the decode so far, in rank order: (tokens int32 [N, cap], logp f32 [N, cap], scores f32 [N]), fresh
        tensors; `scores` is the device's running f32 sum of a beam's token log-probabilities (-inf: a padding beam)."""
        if self.beam is None:
            raise ValueError("this decode context was built without beams")
        return self.out.clone(), self.logp.clone(), self.beam[:self.B].clone().view(torch.float32)

    def beam_reorders(self) -> int:
        """The steps of the decode so far whose parent permutation was not the identity (a host read)."""
        if self.beam is None:
            raise ValueError("this decode context was built without beams")
        return int(self.beam[25].item())

    def set_filter(self, top_k, top_p):
        """top_k / top_p of the next decode (None: neutral; a host-to-device copy; captured graphs keep the buffer's address)."""
        if self.filter is None:
            raise ValueError("this decode context was built without filtering")
        hip.decode_set_filter(self.filter, top_k, top_p)

    def set_candidate(self, ids):
        """The sequence the next `first_token` + `step`s score (any integer sequence of 1 .. cap ids): a host-to-device copy."""
        if self.score is None:
            raise ValueError("this decode context was built without score")
        n = len(ids)
        if not 1 <= n <= self.cap:
            raise ValueError(f"set_candidate: a sequence of 1 <= length <= {self.cap} ids, got length {n}")
        hip.decode_set_spec_ref(self.ref, ids)

    def set_score_temperature(self, temperature: float):
        """The temperature the next candidates are scored at (0: z = logit): a host-to-device copy."""
        if self.score is None:
            raise ValueError("this decode context was built without score")
        hip.decode_set_sampling(self.score_words, 0, temperature)

    def score_result(self):
        """(logp f32 [n], greedy int32 [n]) of the n tokens scored so far (a host read of t): fresh tensors."""
        if self.score is None:
            raise ValueError("this decode context was built without score")
        n = int(self.state[0].item())
        return self.logp[0, :n].clone(), self.greedy[0, :n].clone()

    def set_draft(self, ids):
        """The reference sequence the next decode drafts from (any integer sequence, truncated to `cap`; None: no draft, every
        verify step then emits one token): a host-to-device copy; captured graphs keep the buffer's address."""
        if self.ref is None:
            raise ValueError("this decode context was built without speculate or jump_forward")
        hip.decode_set_spec_ref(self.ref, ids)

    def stats(self):
        """(verify_steps, accepted) of the decode so far: two words of the device state (a host read)."""
        if self.ref is None:
            raise ValueError("this decode context was built without speculate or jump_forward")
        a, b = self.state[24:26].tolist()
        return int(a), int(b)

    def set_sampling(self, seed: int, temperature: float):
        """Seed and temperature of the next decode (a host-to-device copy; captured graphs keep the buffer's address)."""
        if self.sampling is None:
            raise ValueError("this decode context was built without sampling")
        hip.decode_set_sampling(self.sampling, seed, temperature)

    def bind(self, cache, kinfo_prefix):
        if kinfo_prefix.shape != (self.B, self.Pn):
            raise ValueError(f"decode context for B {self.B}, {self.Pn} prefix keys; got kinfo {tuple(kinfo_prefix.shape)}")
        self.prefix = list(cache)
        self.kinfo = kinfo_prefix

    def first_token(self, pre, logits=None):
        """Reset the device state for the prefill `pre` (an `ar_decode.Prefill`) and decode the first token from its last rows."""
        self.bind(pre.cache, pre.kinfo_prefix)
        self.plen.copy_(pre.plen)
        hip.decode_init(self.state, self.plen, self.out)
        self._kind.reset(self)
        self._kind.first(self, pre.x_last, logits)

    def _w(self, name):
        """A layer projection as the fused step streams it: (weight, {}) or (e4m3 codes, {"wscale": row scales})."""
        if self.weights == "bf16":
            return self.model.W(name), {}
        codes, scales = self.model._dec_fp8(name)
        return codes, {"wscale": scales}

    def _lm_head(self):
        """What every LM head launch receives: (final norm scale, hi plane, lo plane, keywords)."""
        m = self.model
        if self.weights == "fp8":         # one e4m3 plane of the f32 table
            hi, scales = m._dec_fp8("llm/embed")
            lo, kw = None, {"wscale": scales}
        else:
            hi, lo, kw = m.W("llm/embed"), m.ps.w16lo("llm/embed"), {}
        if self.allowed is not None:      # the LM head streams the allowed rows only
            kw["ids"] = self.allowed
        return m.F("llm/final_norm"), hi, lo, kw

    def step(self, logits=None):
        """One decode step (lap.py:734-752) + its token, positions and stop condition from the device state: replays unchanged."""
        m = self.model
        v = m.v
        NH, HD, KV = v.num_heads, v.head_dim, v.num_kv_heads
        self._kind.embed(self, m.ps.embed_rows(), math.sqrt(v.width))
        qkv, attention = (hip.decode_spec_qkv, hip.decode_spec_attention) if self.rows_of_one else (hip.decode_qkv, hip.decode_attention)
        for l in range(v.depth):
            p = f"llm/{l}/"
            gk, gv = self.gen[l, 0], self.gen[l, 1]
            w, kw = self._w(p + "wqkv0")
            ck, cv = self.prefix[l]
            qkv(self.state, self.x, m.F(p + "n_attn"), w, self.q, gk, gv, NH, HD, HD ** -0.5, **kw)
            attention(self.state, self.q, ck, cv, self.kinfo, self.Pn, gk, gv, self.o, self.attn_scratch, NH, KV, HD)
            w, kw = self._w(p + "wo0")
            hip.decode_proj_residual(self.state, self.o, w, self.x, self.xa, **kw)
            w, kw = self._w(p + "wgu0")
            hip.decode_gate_up(self.state, self.xa, m.F(p + "n_ffw"), w, self.act, **kw)
            w, kw = self._w(p + "wd0")
            hip.decode_proj_residual(self.state, self.act, w, self.xa, self.x, kwaves=hip.DECODE_KWAVES_DOWN, **kw)
        self._kind.token(self, self.x, logits)
