"""Batch-1 action-chunk serving: hipGraph-captured `sample_actions` and a minimal `Policy.infer` surface.

Reference: scripts/serve_policy.py:69-107 -> policy_config_adapter.create_trained_policy (85-154) ->
openpi Policy.infer [UPSTREAM-RECALL]: add batch dim -> Observation.from_dict -> jit(sample_actions) -> strip batch
-> {"actions", "policy_timing": {"infer_ms"}}.  The request-level transforms (CoTInputs, Normalize, tokenizer,
Unnormalize, CoTOutputs) are SURVEY.md §8(f) rank-1 "next" items; this module takes model-level inputs.

The reference's jit turns the whole sampler (prefix prefill + lax.while_loop of 10 denoise steps, lap.py:605-675)
into one XLA executable.  Here the same region is captured once into a HIP graph (torch.cuda.CUDAGraph is the
capture plumbing; every node is one of our C-ABI kernel launches) and replayed per request: ~2,800 kernel launches
cost one graph launch on the host.
"""
from __future__ import annotations

import time

import numpy as np
import torch

from lap_amd import ar_decode
from lap_amd.chunking import RealTimeChunker
from lap_amd.model import LAP
from lap_amd.observation import CoTObservation


def _placeholder_obs(model: LAP, batch_size: int, prompt_len: int | None, langact_mask: bool = False) -> CoTObservation:
    """The observation a captured graph reads: requests are copied into its tensors (`_load`)."""
    cfg = model.config
    dev = model.device
    L = prompt_len or cfg.max_token_len
    H = cfg.image_size
    return CoTObservation(
        images={k: torch.zeros(batch_size, H, H, 3, device=dev) for k in cfg.image_keys},
        image_masks={k: torch.ones(batch_size, dtype=torch.bool, device=dev) for k in cfg.image_keys},
        state=torch.zeros(batch_size, cfg.action_dim, device=dev),
        tokenized_prompt=torch.zeros(batch_size, L, dtype=torch.int32, device=dev),
        tokenized_prompt_mask=torch.ones(batch_size, L, dtype=torch.bool, device=dev),
        tokenized_langact_mask=torch.zeros(batch_size, L, dtype=torch.bool, device=dev) if langact_mask else None)


def graph_compatible(captured: CoTObservation, obs: CoTObservation) -> bool:
    """A captured graph is tied to the batch size, image resolution and prompt length of the observation it was captured on."""
    return (all(k in obs.images and tuple(obs.images[k].shape) == tuple(captured.images[k].shape) for k in captured.images)
            and tuple(obs.tokenized_prompt.shape) == tuple(captured.tokenized_prompt.shape))


class GraphedSampler:
    """hipGraph-replayed `LAP.sample_actions`.  `inpaint=True` (not in the reference) captures on the inpainting Euler tails with
    persistent `known` / `mask` buffers: ONE graph then serves every mask, the all-zero one (no row frozen) included, and a call
    takes `inpaint=(known, mask)` or None.  Without the flag the sampler holds no such buffers and captures the plain launches.

    `num_samples=N` (2 .. 8, batch_size 1; best-of-N, not in the reference): one capture holds the batch-1 prefill, the denoising of
    N candidates and, with `select="medoid"` / `"coherence"`, the select launch.  A call takes noise [N, S, ad] and returns the
    candidates [N, S, ad], or with `select` the chosen chunk [1, S, ad]; `last_candidates`, `last_scores` and `last_index` are
    views of the captured outputs.  `select="coherence"` keeps persistent `known` [S, ad] / `weights` [S] buffers that
    `__call__(..., coherence=(known, weights))` checks and copies in before the replay: one graph serves every pair."""

    def __init__(self, model: LAP, batch_size: int = 1, num_steps: int = 10, prompt_len: int | None = None, inpaint: bool = False,
                 num_samples=None, select=None, share_prefix: bool = True):
        from lap_amd.action_select import MODES
        from lap_amd.flow_sample import check_num_samples

        self.model, self.B, self.num_steps = model, batch_size, num_steps
        cfg = model.config
        self.N = check_num_samples(num_samples, batch_size, cfg.pi05)
        if select is not None and (select not in MODES or self.N < 2):
            raise ValueError(f"GraphedSampler: select={select!r} needs 'medoid' or 'coherence' and num_samples > 1")
        self.select, self.share_prefix = select, share_prefix
        self.obs = _placeholder_obs(model, batch_size, prompt_len)
        self.noise = torch.zeros(max(batch_size, self.N), cfg.action_horizon, cfg.action_dim, device=model.device)
        self.inpaint = None
        if inpaint:
            self.inpaint = (torch.zeros(batch_size, cfg.action_horizon, cfg.action_dim, device=model.device),
                            torch.zeros(batch_size, cfg.action_horizon, dtype=torch.uint8, device=model.device))
        self.coherence = None
        if select == "coherence":
            self.coherence = (torch.zeros(cfg.action_horizon, cfg.action_dim, device=model.device), torch.zeros(cfg.action_horizon, device=model.device))
        self._sel = {}
        self.last_candidates = self.last_scores = self.last_index = None
        self.graph = None
        self.out = None

    def _load(self, obs: CoTObservation, noise: torch.Tensor, inpaint=None, coherence=None):     # (unlike GraphedTokenDecoder._load: absent image masks and `state` keep the last request's)
        if inpaint is not None and self.inpaint is None:
            raise ValueError("this GraphedSampler was built without inpaint=True")
        if (coherence is None) != (self.coherence is None):
            raise ValueError("coherence=(known, weights) goes with a GraphedSampler built with select='coherence', and is required there")
        if tuple(noise.shape) != tuple(self.noise.shape):
            raise ValueError(f"noise has shape {tuple(noise.shape)}, expected {tuple(self.noise.shape)}")
        new_coh = None
        if coherence is not None:       # (checked BEFORE anything is copied, like `inpaint`)
            from lap_amd.action_select import check_coherence

            new_coh = check_coherence(*coherence, *self.noise.shape[1:])
            if not all(bool(torch.isfinite(torch.as_tensor(c, dtype=torch.float32)).all()) for c in new_coh):
                raise ValueError("select: coherence known / weights have non-finite values")
        if self.inpaint is not None:
            from lap_amd.flow_sample import check_inpaint

            known, mask = self.inpaint
            if inpaint is None:
                mask.zero_()
            else:       # (checked BEFORE anything is copied: the capture itself cannot look at values)
                k, m = check_inpaint(inpaint, *known.shape, self.model.device)
                known.copy_(k)
                mask.copy_(m)
        if new_coh is not None:
            for buf, c in zip(self.coherence, new_coh):
                buf.copy_(torch.as_tensor(c).to(buf.device, torch.float32))
        for k in self.obs.images:
            self.obs.images[k].copy_(obs.images[k])
            if k in obs.image_masks and obs.image_masks[k] is not None:
                self.obs.image_masks[k].copy_(obs.image_masks[k])
        self.obs.tokenized_prompt.copy_(obs.tokenized_prompt)
        self.obs.tokenized_prompt_mask.copy_(obs.tokenized_prompt_mask)
        self.noise.copy_(noise)

    def capture(self):
        side = torch.cuda.Stream(device=self.model.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):  # warm-up outside capture (kernel attribute setup, allocator pools)
            for _ in range(2):
                self._sample()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self._sample()
        if self.N > 1:
            self.last_candidates = self._sel.get("candidates", self.out)
            self.last_scores, self.last_index = self._sel.get("scores"), self._sel.get("index")
        return self

    def _sample(self):
        kw = {} if self.inpaint is None else {"inpaint": self.inpaint}
        if self.N > 1:
            kw |= dict(num_samples=self.N, select=self.select, coherence=self.coherence, share_prefix=self.share_prefix, _select_out=self._sel)
        return self.model.sample_actions(0, self.obs, num_steps=self.num_steps, noise=self.noise, **kw)

    def __call__(self, obs: CoTObservation, noise: torch.Tensor, inpaint=None, coherence=None) -> torch.Tensor:
        if self.graph is None:
            self.capture()
        # parameter-derived caches the graph holds addresses of (adaRMS modulations, packed expert weights) follow the
        # parameters in place; a no-op unless a train step / restore / reload happened since the last call
        self.model.refresh_serve_caches(self.num_steps)
        self._load(obs, noise, inpaint, coherence)
        self.graph.replay()
        return self.out


class GraphedTokenDecoder:
    """hipGraph-replayed greedy `LAP.sample_tokens(decode="fused")` (the LAP_AR serving mode), the sibling of GraphedSampler.

    Two graphs: (1) the VLM prefill + the first token (state reset included) and (2) `steps_per_replay` fused decode steps
    (csrc/decode.hip), each of which reads its position, cache row and stop flag from the device state, so the same graph
    replays for every token and turns into no-ops once every sample has emitted EOS or the budget is spent.  The host reads
    the stop flag once per replay of (2).  Returns int32 [B, max_decoding_steps] like `sample_tokens` (a fresh tensor).
    The EOS token is the model's `EOS_TOKEN` when the graphs are captured.

    sampling=True captures both graphs on the sampling LM head (`sample_tokens(decode="fused", sampler="device")`): the seed and
    the temperature of a call are four device words that `__call__(obs, temperature=, seed=)` rewrites before the first replay,
    so one capture serves greedy and sampled requests of any seed and temperature, with no further host read.  A greedy call
    returns what the sampling=False decoder returns, bit for bit.

    weights: `sample_tokens`' `decode_weights` ("bf16", "fp8", "fp8_layers"): the step graph is captured on the fp8 kernels and
    holds the addresses of the model's fp8 weight cache, which `refresh_serve_caches` re-quantises in place before a replay
    when the parameters have changed.  Composes with sampling=True.

    allowed_tokens: `sample_tokens`' constrained decoding, fixed at construction (the graphs hold the address of the id buffer):
    every call decodes inside that set.  None: the whole vocabulary.  Composes with sampling= and weights=.

    logprobs=True: `sample_tokens`' `return_logprobs`: both graphs are captured on the LM head that also leaves the log-sum-exp
    partials (no further launch), the log-probability buffer lives beside the context's `out`, and a call returns
    (tokens, logprobs), both fresh tensors.  Composes with sampling=, weights= and allowed_tokens=.

    num_samples=N (1 <= N <= 8; batch_size 1, sampling=True): `sample_tokens`' best-of-N.  The prefill graph runs at B = 1 and
    ends with the copies of its prefix K / V, key-info words and last row to N rows; the step graph runs at B = N.  A call
    (temperature > 0) returns (tokens [N, steps], logprobs [N, steps]).

    filtering=True (needs sampling=True): `sample_tokens`' `top_k` / `top_p`.  Both graphs are captured on the filtering context
    (the plain LM head stores its f32 logits, lap_decode_filter_finish draws from them); `__call__(obs, temperature=, seed=,
    top_k=, top_p=)` rewrites four more device words before the first replay, so one capture serves any k and p, and a call with
    neither returns the filtering=False decoder's tokens.  Composes with weights=, allowed_tokens=, logprobs= (the log-probability
    stays the one over all candidates) and num_samples=.

    speculate=S (2 <= S <= 8; batch_size 1, greedy: sampling=, logprobs=, num_samples= and filtering= raise ValueError):
    `sample_tokens`' exact speculative decoding.  The step graph is captured on verify steps of S rows, and the reference sequence
    lives in one device buffer that `__call__(obs, draft_tokens=ids_or_None)` rewrites before the first replay, so one step graph
    serves any draft.  A call returns the tokens of the decoder without it; `last_stats` = (verify_steps, accepted) of the call.
    Composes with weights= and allowed_tokens=.

    grammar: `sample_tokens`' grammar-constrained decoding, a `grammar.TokenAutomaton` fixed at construction (the graphs hold the
    addresses of its device buffers).  The automaton state of every row lives in the context and is zeroed inside the prefill graph,
    so one capture serves every request and every request starts in state 0.  Composes with sampling=, weights=, logprobs= and
    num_samples=; allowed_tokens=, filtering= and speculate= raise ValueError.

    jump_forward=S (2 <= S <= 8; needs grammar=, batch_size 1 and no num_samples): `sample_tokens`' jump-forward grammar decoding.
    The step graph is captured on steps of S rows that are driven by device state alone (the automaton state, the reference
    buffer, the sampling words), so one capture serves greedy and sampled requests and any `draft_tokens`; a call returns what the
    decoder without it returns, log-probabilities included, and `last_stats` = (verify_steps, accepted).  Composes with sampling=,
    weights= and logprobs=.

    num_beams=N (1 <= N <= 8; batch_size 1, greedy: sampling=, num_samples=, filtering=, speculate= and jump_forward= raise
    ValueError from `beam.check_num_beams`), early_stop=: `sample_tokens`' beam search.  The prefill graph runs at B = 1, copies its
    prefix to N rows and resets the beam buffer with a device copy; the step graph runs the beam step at B = N, so one capture
    serves every request.  A call returns the rank-0 beam ([1, steps] tokens, with logprobs=True also its log-probabilities);
    `last_beams` = (tokens [N, steps], logprobs [N, steps], scores [N]) of the call.  Composes with weights=, allowed_tokens= and
    logprobs=, and with grammar= (not with allowed_tokens=): the beams are then the most probable sentences of the automaton, every
    beam's automaton state lives in the context and is zeroed inside the prefill graph, and one capture serves every request."""

    def __init__(self, model: LAP, batch_size: int = 1, max_decoding_steps: int = 390, prompt_len: int | None = None,
                 steps_per_replay: int = 8, sampling: bool = False, weights: str = "bf16", allowed_tokens=None,
                 logprobs: bool = False, num_samples=None, filtering: bool = False, speculate=None, grammar=None, jump_forward=None,
                 num_beams=None, early_stop: bool = True):
        self.NB = None
        self.early_stop = bool(early_stop)
        self.last_beams = None
        if num_beams is not None:
            from lap_amd.beam import check_num_beams

            self.NB = check_num_beams(num_beams, batch_size, temperature=1.0 if sampling else 0.0, num_samples=num_samples,
                                      top_k=0 if filtering else None, speculate=speculate, grammar=grammar, jump_forward=jump_forward)
            ar_decode.check_fused_decode(model, self.NB)
        self.grammar = None
        host = None
        if grammar is not None:
            host = ar_decode.check_grammar(grammar, model.config.vocab_size, model.EOS_TOKEN, allowed_tokens=allowed_tokens,
                                           top_k=0 if filtering else None, speculate=speculate)
        self.J = None
        if jump_forward is not None:
            from lap_amd.speculate import check_jump_forward

            self.J = check_jump_forward(jump_forward, batch_size, grammar=grammar, num_samples=num_samples)
        if grammar is not None:
            self.grammar = ar_decode.grammar_on_device(model, grammar, host)
        self.S = None
        self.last_stats = None
        if speculate is not None:
            from lap_amd.speculate import check_speculate

            self.S = check_speculate(speculate, batch_size, return_logprobs=logprobs, num_samples=num_samples,
                                     temperature=1.0 if sampling else 0.0, top_k=0 if filtering else None)
        if filtering and not sampling:
            raise ValueError("GraphedTokenDecoder: filtering needs a decoder built with sampling=True")
        self.filtering = bool(filtering)
        self.N = None
        if num_samples is not None:
            if not sampling:
                raise ValueError("GraphedTokenDecoder: num_samples needs a decoder built with sampling=True")
            self.N = ar_decode.check_num_samples(num_samples, batch_size, decode="fused", sampler="device", temperature=1.0)
            ar_decode.check_fused_decode(model, self.N)
        self.logprobs = bool(logprobs) or self.N is not None
        ar_decode.check_fused_decode(model, batch_size)
        ar_decode.check_decode_weights(weights)
        self.weights = weights
        self.allowed = None
        if allowed_tokens is not None:
            self.allowed = ar_decode.allowed_set(model, allowed_tokens).ids
        if max_decoding_steps < 1 or steps_per_replay < 1:
            raise ValueError("max_decoding_steps and steps_per_replay must be >= 1")
        self.model, self.B, self.max_steps, self.spr = model, batch_size, max_decoding_steps, steps_per_replay
        self.sampling = bool(sampling)
        self.obs = _placeholder_obs(model, batch_size, prompt_len, langact_mask=True)
        self.ctx = None
        self.g_prefill = self.g_step = None

    def _load(self, obs: CoTObservation):
        for k in self.obs.images:
            self.obs.images[k].copy_(obs.images[k])
            m = obs.image_masks.get(k) if obs.image_masks else None
            if m is not None:
                self.obs.image_masks[k].copy_(m)
            else:
                self.obs.image_masks[k].fill_(True)
        if obs.state is not None:
            self.obs.state.copy_(obs.state)
        self.obs.tokenized_prompt.copy_(obs.tokenized_prompt)
        self.obs.tokenized_prompt_mask.copy_(obs.tokenized_prompt_mask)
        if obs.tokenized_langact_mask is not None:      # (an all-false mask is the same prefix attention as none)
            self.obs.tokenized_langact_mask.copy_(obs.tokenized_langact_mask)
        else:
            self.obs.tokenized_langact_mask.zero_()

    def _prefill(self):
        pre = ar_decode.prefill(self.model, self.obs)
        if self.N is not None or self.NB is not None:
            pre = ar_decode.replicate_prefill(pre, self.N or self.NB)
        if self.ctx is None:
            self.ctx = ar_decode.DecodeCtx(self.model, pre.B, pre.Pn, self.max_steps, self.sampling, self.weights,
                                           allowed=self.allowed, logprobs=self.logprobs, filtering=self.filtering, speculate=self.S,
                                           grammar=self.grammar, jump_forward=self.J, beams=self.NB, early_stop=self.early_stop)
        self.ctx.first_token(pre)

    def _steps(self):
        for _ in range(self.spr):
            self.ctx.step()

    def capture(self):
        m = self.model
        m.refresh_serve_caches()
        with m._serving_weights():
            side = torch.cuda.Stream(device=m.device)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):   # warm-up outside capture (kernel attribute setup, allocator pools, serving caches)
                self._prefill()
                self._steps()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            self.g_prefill = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g_prefill):
                self._prefill()
            self.g_step = torch.cuda.CUDAGraph()      # (reads the prefix caches the first graph's pool holds)
            with torch.cuda.graph(self.g_step):
                self._steps()
        torch.cuda.synchronize()
        return self

    def __call__(self, obs: CoTObservation, *, temperature: float = 0.0, seed: int = 0, top_k=None, top_p=None, draft_tokens=None):
        if draft_tokens is not None and self.S is None and self.J is None:
            raise ValueError("GraphedTokenDecoder: draft_tokens needs a decoder built with speculate=S")
        if temperature > 0.0 and not self.sampling:
            raise ValueError("GraphedTokenDecoder: temperature > 0 needs a decoder built with sampling=True")
        filt = ar_decode.check_filter(top_k, top_p, sampler="device", temperature=temperature)
        if filt is not None and not self.filtering:
            raise ValueError("GraphedTokenDecoder: top_k / top_p need a decoder built with filtering=True")
        if self.N is not None and not temperature > 0.0:
            raise ValueError(f"GraphedTokenDecoder: num_samples needs temperature > 0 (greedy candidates are all the same), got {temperature!r}")
        if self.g_step is None:
            self.capture()
        # merged LoRA weights / fp8 decode weights / packed prefill images the graphs hold addresses of follow the parameters in place
        self.model.refresh_serve_caches()
        self._load(obs)
        if self.sampling:
            self.ctx.set_sampling(seed, temperature)
        if self.filtering:
            self.ctx.set_filter(*(filt or (None, None)))
        if self.S is not None or self.J is not None:
            self.ctx.set_draft(draft_tokens)
        self.g_prefill.replay()
        for _ in range((self.max_steps - 1 + self.spr - 1) // self.spr):
            if bool(self.ctx.state[1].item()):      # one host read per replay
                break
            self.g_step.replay()
        if self.S is not None or self.J is not None:
            self.last_stats = self.ctx.stats()
        if self.NB is not None:             # all beams are kept; the answer is the rank-0 beam, as a batch of 1
            self.last_beams = self.ctx.beam_result()
            tokens, logp, _ = self.last_beams
            return (tokens[:1].clone(), logp[:1].clone()) if self.logprobs else tokens[:1].clone()
        if self.logprobs:
            return self.ctx.out.clone(), self.ctx.logp.clone()
        return self.ctx.out.clone()


class Policy:
    """openpi's Policy surface: `infer(obs)` -> {"actions", ..., "policy_timing"}.

    With `transforms` / `output_transforms` (lap_amd/policy_io.py, assembled by `create_trained_policy`) `obs` is the raw
    client request ({"observation": {image keys, "state"}, "prompt", ...}) and the result carries un-normalised actions, as
    in policies/policy_config_adapter.py:139-153.  Without them `obs` is already model-level (un-batched numpy arrays).

    Real-time chunking (not in the reference): a request key `"inpaint"` freezes the head of the new chunk on committed actions
    (`LAP.sample_actions(inpaint=...)`), all in MODEL space.  `{"executed": s, "freeze": d}` uses the policy's OWN last chunk, kept
    as the sampler returned it — before unnormalisation and the output transforms, so no inverse transform is needed: s of its rows
    will have been executed when the new chunk starts, and the d rows after them come back unchanged as rows 0 .. d-1
    (`chunking.shift_chunk`).  On the first request, or after `reset()` / `"reset": True`, there is no previous chunk: the two
    numbers are ignored and `policy_timing["inpaint"]` says so.  `{"known": [S, action_dim], "mask": [S]}` passes the arrays
    explicitly.  Shifting a previous chunk is meaningful only when the action representation does not depend on the new
    observation's frame.  Such requests replay a second captured graph (one graph for every mask), built at the first of them;
    requests without the key take the path they always took."""

    def __init__(self, model: LAP, *, num_steps: int = 10, use_graph: bool = True, seed: int = 0, metadata: dict | None = None,
                 transforms=(), output_transforms=(), sample_kwargs: dict | None = None):
        from lap_amd.policy_io import compose

        self.model = model
        self.metadata = metadata or {}
        self._sample_kwargs = dict(sample_kwargs or {})
        self.num_steps = self._sample_kwargs.pop("num_steps", num_steps)
        # (pi0, `pi05=False`, runs on the generic layer loop with its suffix re-embedded by torch ops at every step: served eagerly)
        self._sampler = GraphedSampler(model, 1, self.num_steps) if (use_graph and model.config.pi05) else None
        self._inpaint_sampler = None        # GraphedSampler(inpaint=True), built at the first request with an "inpaint" key
        # best-of-N (sample_kwargs "num_samples", "select", "rho"): candidates of one prefill, one chosen on the device
        from lap_amd.action_select import MODES
        from lap_amd.flow_sample import check_num_samples

        self._N = check_num_samples(self._sample_kwargs.pop("num_samples", None), 1, model.config.pi05)
        self._select = self._sample_kwargs.pop("select", None)
        self._rho = float(self._sample_kwargs.pop("rho", 0.5))
        if self._N > 1 and self._select not in MODES:
            raise ValueError(f"Policy: num_samples = {self._N} needs sample_kwargs['select'] = 'medoid' or 'coherence', got {self._select!r}")
        if self._N == 1 and self._select is not None:
            raise ValueError("Policy: sample_kwargs['select'] needs num_samples > 1")
        self._cand_samplers = {}            # (select mode, inpaint) -> GraphedSampler(num_samples=N, ...), built on first use
        self.last_candidates = None         # [N, S, ad] of the last best-of-N request (device copy)
        self._chunker = RealTimeChunker()   # the last model-space chunk
        self._gen = torch.Generator(device=model.device).manual_seed(seed)
        self._has_transforms = bool(transforms) or bool(output_transforms)
        self._transforms = list(transforms)
        self._input_transform = compose(self._transforms)
        self._output_transform = compose(list(output_transforms))

    def _to_observation(self, inputs: dict) -> tuple[CoTObservation, dict]:
        batched = {k: ({kk: np.asarray(vv)[None] for kk, vv in v.items()} if isinstance(v, dict) else np.asarray(v)[None])
                   for k, v in inputs.items() if v is not None and not isinstance(v, str)}
        return CoTObservation.from_dict(batched, device=self.model.device), batched

    def reset(self):
        """Forget the previous chunk: the next `"inpaint": {"executed", "freeze"}` request samples freely."""
        self._chunker.reset()

    def _inpaint_request(self, req):
        """The request's "inpaint" value -> ((known [1, S, ad], mask [1, S]) or None, the note for `policy_timing`)."""
        if not isinstance(req, dict):
            raise ValueError('"inpaint": expected {"executed": s, "freeze": d} or {"known": ..., "mask": ...}')
        if req.get("reset"):
            self._chunker.reset()
        if "known" in req or "mask" in req:
            if "known" not in req or "mask" not in req:
                raise ValueError('"inpaint": "known" and "mask" go together')
            known, mask = np.asarray(req["known"], dtype=np.float32), np.asarray(req["mask"])
            known, mask = (known[None] if known.ndim == 2 else known), (mask[None] if mask.ndim == 1 else mask)
        else:
            if "executed" not in req or "freeze" not in req:
                raise ValueError('"inpaint": "executed" and "freeze" are both required')
            nxt = self._chunker.next(int(req["executed"]), int(req["freeze"]))
            if nxt is None:
                return None, {"applied": False, "reason": "no previous chunk: executed / freeze ignored"}
            known, mask = nxt[0][None], nxt[1][None]
        return (known, mask), {"applied": True, "frozen_rows": int(np.count_nonzero(mask))}

    def _infer_candidates(self, o, executed, inpaint, noise):
        """One best-of-N request -> (the chosen chunk [1, S, ad], the note for `policy_timing["select"]`)."""
        from lap_amd.action_select import coherence_weights
        from lap_amd.chunking import shift_chunk

        cfg, dev = self.model.config, self.model.device
        S, ad = cfg.action_horizon, cfg.action_dim
        if noise is None:
            noise = torch.randn((self._N, S, ad), generator=self._gen, device=dev)
        else:
            noise = torch.as_tensor(np.asarray(noise), dtype=torch.float32, device=dev).reshape(self._N, S, ad)
        mode, coh, fallback = self._select, None, False
        if mode == "coherence":
            if self._chunker.prev is None:      # nothing to be coherent with: the candidate closest to the others
                mode, fallback = "medoid", True
            else:
                ex = 0 if executed is None else int(executed)
                prev = self._chunker.prev if self._chunker.prev.ndim == 2 else self._chunker.prev[0]
                coh = (torch.from_numpy(shift_chunk(prev, ex, 0)[0]), coherence_weights(S, ex, self._rho))
        sel = {}
        if self._sampler is not None and graph_compatible(self._sampler.obs, o):
            key = (mode, inpaint is not None)
            if key not in self._cand_samplers:
                self._cand_samplers[key] = GraphedSampler(self.model, 1, self.num_steps, inpaint=key[1], num_samples=self._N, select=mode)
            sampler = self._cand_samplers[key]
            a = sampler(o, noise, inpaint, coh)
            sel = dict(candidates=sampler.last_candidates, scores=sampler.last_scores, index=sampler.last_index)
        else:
            kw = {} if inpaint is None else {"inpaint": inpaint}
            a = self.model.sample_actions(0, o, num_steps=self.num_steps, noise=noise, num_samples=self._N, select=mode, coherence=coh,
                                          _select_out=sel, **kw)
        self.last_candidates = sel["candidates"].clone()
        return a, {"mode": mode, "index": int(sel["index"].item()), "scores": sel["scores"].cpu().tolist(), "fallback": fallback}

    def infer(self, obs: dict, *, noise=None) -> dict:
        t0 = time.perf_counter()
        dev = self.model.device
        request = dict(obs)
        executed = request.pop("executed", None)        # (best-of-N coherence; an "inpaint" request's own "executed" comes first)
        if isinstance(request.get("inpaint"), dict) and "executed" in request["inpaint"]:
            executed = request["inpaint"]["executed"]
        inpaint, note = self._inpaint_request(request.pop("inpaint")) if "inpaint" in request else (None, None)
        inputs = self._input_transform(request)
        o, batched = self._to_observation(inputs)
        cfg = self.model.config
        select_note = None
        if self._N > 1:
            a, select_note = self._infer_candidates(o, executed, inpaint, noise)
            noise = torch.zeros(0) if noise is None else torch.as_tensor(np.asarray(noise))
        elif noise is None:
            noise = torch.randn((1, cfg.action_horizon, cfg.action_dim), generator=self._gen, device=dev)
        else:
            noise = torch.as_tensor(np.asarray(noise), dtype=torch.float32, device=dev).reshape(1, cfg.action_horizon, cfg.action_dim)
        if self._N > 1:
            pass
        elif inpaint is None:
            if self._sampler is not None and graph_compatible(self._sampler.obs, o):
                a = self._sampler(o, noise)
            else:
                a = self.model.sample_actions(0, o, num_steps=self.num_steps, noise=noise)
        elif self._sampler is not None and graph_compatible(self._sampler.obs, o):
            if self._inpaint_sampler is None:
                self._inpaint_sampler = GraphedSampler(self.model, 1, self.num_steps, inpaint=True)
            a = self._inpaint_sampler(o, noise, inpaint)
        else:
            a = self.model.sample_actions(0, o, num_steps=self.num_steps, noise=noise, inpaint=inpaint)
        actions = a[0].cpu().numpy()  # device sync
        if self.model.serve_chain_failed():
            # A block of the one-launch denoise step (csrc/serve_chain.hpp) was not scheduled within its bounded wait — the GPU is
            # shared with work that holds compute units — so this chunk is invalid: go back to the separate launches for good.
            self.model.disable_serve_chain()
            for sampler in (self._sampler, self._inpaint_sampler, *self._cand_samplers.values()):
                if sampler is not None:
                    sampler.graph = None
            return self.infer(obs, noise=noise.cpu().numpy() if noise.numel() else None)
        self._chunker.update(actions)       # model space: before Unnormalize and the output transforms (best-of-N: the chosen chunk)
        model_ms = (time.perf_counter() - t0) * 1e3
        timing = {"infer_ms": model_ms} | ({} if note is None else {"inpaint": note}) | ({} if select_note is None else {"select": select_note})
        if not self._has_transforms:
            return {"actions": actions, "policy_timing": timing}
        outputs = self._output_transform({"state": batched["state"][0], "actions": actions})
        outputs["policy_timing"] = timing
        return outputs


def create_trained_policy(train_config, checkpoint_dir, *, tokenizer_model_path=None, tokenizer=None, repack_transforms=(),
                          sample_kwargs: dict | None = None, default_prompt: str | None = None, norm_stats: dict | None = None,
                          device="cuda", use_graph: bool = True, deterministic: bool = False) -> Policy:
    """policies/policy_config_adapter.py:85-154: model from `<checkpoint_dir>/params`, norm stats from
    `<checkpoint_dir>/assets/<asset_id>/norm_stats.json`, and the standard transform stack
        [repack.inputs, InjectDefaultPrompt, CoTInputs (the data config's), Normalize, InjectDefaultPrompt, Tokenize, PadStatesAndActions]
        -> model -> [DetokenizeReasoning, Unnormalize, CoTOutputs, repack.outputs]  (VLA-0: [DetokenizeReasoning, CoTOutputs(norm stats)]).
    `repack_transforms` = (inputs, outputs) lists.  The PaliGemma SentencePiece model cannot be downloaded here: pass
    `tokenizer_model_path` (or a ready `tokenizer`).
    `deterministic` (not in the reference, which has no serving override): True switches off the training-time randomness the data /
    model config carries into the serving stack — wrist-image dropout, random un-masking of missing cameras, state dropout — so that
    equal requests give equal prompts and masks.  False keeps the reference's wiring and warns when any of the three is non-zero."""
    import pathlib

    from lap_amd import checkpoints as _ckpt
    from lap_amd import policy_io as pio

    checkpoint_dir = pathlib.Path(checkpoint_dir)
    mc = train_config.model
    model = mc.load(_ckpt.restore_params(checkpoint_dir), device=device, with_grads=False)
    if norm_stats is None:
        if getattr(train_config.data, "asset_id", None) is None:
            raise ValueError("Asset id is required to load norm stats.")
        norm_stats = _ckpt.load_norm_stats(checkpoint_dir / "assets")
    ntype = getattr(train_config.data, "action_proprio_normalization_type", "bounds_q99")
    if tokenizer is None:
        tokenizer = pio.PaligemmaTokenizer(tokenizer_model_path, mc.max_token_len, prompt_format=mc.prompt_format,
                                           reasoning_mask_prob=0.0)
    rin, rout = (list(repack_transforms[0]), list(repack_transforms[1])) if repack_transforms else ([], [])
    import dataclasses as _dc
    import warnings

    from lap_amd.data import data_transform_inputs
    dc = train_config.data
    state_dropout = getattr(mc, "state_dropout", 0.0)
    noisy = {k: v for k, v in (("data.wrist_image_dropout_prob", getattr(dc, "wrist_image_dropout_prob", 0.0)),
                               ("data.random_mask_prob", getattr(dc, "random_mask_prob", 0.0)), ("model.state_dropout", state_dropout)) if v}
    if deterministic:
        if _dc.is_dataclass(dc):
            dc = _dc.replace(dc, **{k: 0.0 for k in ("wrist_image_dropout_prob", "random_mask_prob") if hasattr(dc, k)})
        state_dropout = 0.0
    elif noisy:
        warnings.warn("create_trained_policy: the serving stack keeps the config's training-time randomness as the reference does "
                      f"({', '.join(f'{k}={v}' for k, v in noisy.items())}): images are blanked / un-masked and the state dropped at random "
                      "per request.  Pass deterministic=True (or zero these fields) for a deterministic server.", stacklevel=2)
    strategy = getattr(dc, "transform_strategy", "standard")
    fmt_name = getattr(dc, "language_action_format_name", "verbose_eef_with_rotation")
    # policy_config_adapter.py:137-150: the data config's OWN data-transform group serves too — the same `CoTInputs` as in training,
    # training-time image randomness included (wrist dropout / random un-masking are whatever the data config says: the reference has no
    # serving override; set them to 0 in the config a server is started with) — then Normalize, then the model transforms
    # (training/config.py:195-207: default prompt, tokenizer with the model's state dropout, padding).
    transforms = [*rin, pio.InjectDefaultPrompt(default_prompt), data_transform_inputs(dc, mc),
                  pio.Normalize(norm_stats, normalization_type=ntype), pio.InjectDefaultPrompt(None),
                  pio.TokenizePromptAndReasoning(tokenizer, discrete_state_input=mc.discrete_state_input, verbose_mode=mc.verbose_mode,
                                                 state_dropout=state_dropout),
                  pio.PadStatesAndActions(mc.action_dim)]
    detok = pio.DetokenizeReasoning(tokenizer)      # model_transforms.outputs (include_outputs, training/config.py:192-194)
    if strategy == "vla0":      # OutputTransformAssembler._build_vla0_outputs (:44-66): the decoder un-normalises, no Unnormalize
        outputs = [detok, pio.CoTOutputs(language_action_format=fmt_name, norm_stats=norm_stats, normalization_type=ntype, transform_strategy="vla0"), *rout]
    else:                       # _build_standard_outputs (:68-82)
        outputs = [detok, pio.Unnormalize(norm_stats, normalization_type=ntype),
                   pio.CoTOutputs(language_action_format=fmt_name, transform_strategy=strategy), *rout]
    return Policy(model, transforms=transforms, output_transforms=outputs, sample_kwargs=sample_kwargs, use_graph=use_graph,
                  metadata=getattr(train_config, "policy_metadata", None))


class ARPolicy:
    """policies/policy_adapter.py:13-61: the autoregressive serving mode (LAP_AR).  `infer` returns the generated token
    ids of `LAP.sample_tokens` (+ the model-level state) instead of an action chunk; decoding them to text / actions is
    the job of the output transforms, which take exactly this dict."""

    def __init__(self, base: Policy, *, sample_kwargs: dict | None = None, use_graph: bool = False, tokenizer=None):
        if not hasattr(base.model, "sample_tokens"):
            raise AssertionError("Model must have a sample_tokens method")
        self._base = base
        # the tokenizer `score` encodes answer strings with: the one given, else the input stack's (None: ids only)
        self._tokenizer = tokenizer
        self._sample_kwargs = dict(sample_kwargs or {})
        self._calls = 0
        # use_graph: greedy requests of the captured shapes replay a GraphedTokenDecoder (B = 1); anything else, and models whose
        # widths the fused decode kernels do not serve, go through sample_tokens.  With sample_kwargs["sampler"] == "device" the
        # decoder is captured on the sampling LM head and serves requests of any temperature; the seed of a request is the call
        # counter that sample_tokens gets as `rng`, so both routes (and a restarted server) draw the same tokens.
        self._decoder = None
        if self._sample_kwargs.get("sampler", "host") not in ("host", "device"):
            raise ValueError(f"ARPolicy: sampler must be 'host' or 'device', got {self._sample_kwargs['sampler']!r}")
        self._device_sampler = self._sample_kwargs.get("sampler", "host") == "device"
        # sample_kwargs["decode_weights"] ("fp8" / "fp8_layers") reaches both routes: the decoder is captured on those weights,
        # and sample_tokens gets decode="fused" with it (the fp8 kernels are fused decode kernels), so both decode on the same weights
        weights = self._sample_kwargs.get("decode_weights", "bf16")
        ar_decode.check_decode_weights(weights)
        if weights != "bf16":
            if self._sample_kwargs.setdefault("decode", "fused") != "fused":
                raise ValueError(f"ARPolicy: decode_weights={weights!r} needs decode=\"fused\", got {self._sample_kwargs['decode']!r}")
        # sample_kwargs["grammar"] (grammar-constrained decoding: a grammar.TokenAutomaton) reaches both routes: it is checked and
        # put on the device once, here; the decoder is captured with it and sample_tokens gets the device form on every call
        # sample_kwargs["jump_forward"] = S (jump-forward grammar decoding; needs "grammar", implies decode="fused") reaches both
        # routes and is checked between the grammar's own check and its copy to the device; like "speculate" it makes the policy
        # pass the previous answer as the draft of the next request and report "spec_steps" / "spec_accepted"
        kw = self._sample_kwargs
        self._jump = kw.get("jump_forward")
        host = None
        if kw.get("grammar") is not None:
            host = ar_decode.check_grammar(
                kw["grammar"], base.model.config.vocab_size, base.model.EOS_TOKEN, allowed_tokens=kw.get("allowed_tokens"),
                top_k=kw.get("top_k"), top_p=kw.get("top_p"), speculate=kw.get("speculate"), sampler=kw.get("sampler", "host"),
                temperature=kw.get("temperature", 0.0))
        if self._jump is not None:
            from lap_amd.speculate import check_jump_forward

            check_jump_forward(self._jump, 1, grammar=kw.get("grammar"), decode=kw.get("decode", "fused"), sampler=kw.get("sampler", "host"),
                               temperature=kw.get("temperature", 0.0), num_samples=kw.get("num_samples"), collect=kw.get("collect"))
            kw.setdefault("decode", "fused")
        if host is not None:
            kw["grammar"] = ar_decode.grammar_on_device(base.model, kw["grammar"], host)
        # sample_kwargs["allowed_tokens"] (constrained decoding) reaches both routes as well: the set is checked and put on the
        # device once, here; the decoder is captured with it and sample_tokens gets the checked set on every call
        if self._sample_kwargs.get("allowed_tokens") is not None:
            self._sample_kwargs["allowed_tokens"] = ar_decode.allowed_set(base.model, self._sample_kwargs["allowed_tokens"])
        # sample_kwargs["return_logprobs"] adds "token_logprobs" and "logprob" (the sum up to the EOS) to a result;
        # sample_kwargs["num_samples"] = N decodes N candidates per request (best-of-N: decode="fused", sampler="device",
        # temperature > 0), answers with the one sample_kwargs["select"] ("sum", the default, or "mean": sampling.select_best)
        # picks, and reports all of them under "candidates".  Both reach either route; "select" is ARPolicy's own key.
        self._select = self._sample_kwargs.pop("select", "sum")
        if self._select not in ("sum", "mean"):
            raise ValueError(f"ARPolicy: select must be 'sum' or 'mean', got {self._select!r}")
        self._num_samples = self._sample_kwargs.get("num_samples")
        # sample_kwargs["num_beams"] = N selects beam search (greedy; decode "fused", the default here, or "eager"): the policy
        # answers with the beam `sampling.select_best` picks under "select", reports all N under "candidates" in best-of-N's layout,
        # and searches with early_stop=False under "mean" (a longer beam may then win).  "allowed_tokens" and "decode_weights" compose,
        # and so does "grammar" (on the device by now; not with "allowed_tokens"): the beams are sentences of the automaton.
        self._num_beams = self._sample_kwargs.pop("num_beams", None)
        self._beam_scores = None        # the device scores of the last request's beams (-inf: a padding beam)
        if self._num_beams is not None:
            from lap_amd.beam import check_num_beams

            kw = self._sample_kwargs
            check_num_beams(self._num_beams, 1, decode=kw.setdefault("decode", "fused"), temperature=kw.get("temperature", 0.0),
                            sampler=kw.get("sampler", "host"), num_samples=self._num_samples, top_k=kw.get("top_k"), top_p=kw.get("top_p"),
                            speculate=kw.get("speculate"), grammar=kw.get("grammar"), jump_forward=kw.get("jump_forward"),
                            collect=kw.get("collect"))
            kw.pop("return_logprobs", None)
        self._logprobs = (bool(self._sample_kwargs.get("return_logprobs", False)) or self._num_samples is not None
                          or self._num_beams is not None)
        if self._num_samples is not None:
            self._sample_kwargs.setdefault("decode", "fused")
            ar_decode.check_num_samples(self._num_samples, 1, decode=self._sample_kwargs["decode"],
                                        sampler=self._sample_kwargs.get("sampler", "host"),
                                        temperature=self._sample_kwargs.get("temperature", 0.0))
        # sample_kwargs["top_k"] / ["top_p"] (filtering of a device-sampled draw) reach both routes: checked here, once; the decoder
        # is captured with filtering=True when either is present and gets them on every call
        self._filter = {k: self._sample_kwargs[k] for k in ("top_k", "top_p") if self._sample_kwargs.get(k) is not None}
        ar_decode.check_filter(self._filter.get("top_k"), self._filter.get("top_p"), sampler=self._sample_kwargs.get("sampler", "host"),
                               temperature=self._sample_kwargs.get("temperature", 0.0))
        # sample_kwargs["speculate"] = S (exact greedy speculative decoding; implies decode="fused") reaches both routes: the
        # policy keeps the previous answer's tokens, up to and including the EOS, and passes them as the draft of the next request
        # (the first request drafts nothing); "policy_timing" gains "spec_steps" and "spec_accepted"
        self._speculate = self._sample_kwargs.get("speculate")
        self._drafting = self._speculate is not None or self._jump is not None
        self._prev_tokens = None
        if self._speculate is not None:
            from lap_amd.speculate import check_speculate

            check_speculate(self._speculate, 1, decode=self._sample_kwargs.setdefault("decode", "fused"),
                            temperature=self._sample_kwargs.get("temperature", 0.0), return_logprobs=self._logprobs,
                            num_samples=self._num_samples, top_k=self._sample_kwargs.get("top_k"), top_p=self._sample_kwargs.get("top_p"),
                            collect=self._sample_kwargs.get("collect"))
        if use_graph and base.model.decode_supported(self._num_samples or self._num_beams or 1):
            self._decoder = GraphedTokenDecoder(base.model, 1, self._sample_kwargs.get("max_decoding_steps", 390),
                                                num_beams=self._num_beams, early_stop=self._select != "mean",
                                                sampling=self._device_sampler and self._speculate is None, weights=weights,
                                                allowed_tokens=self._sample_kwargs.get("allowed_tokens"),
                                                logprobs=self._logprobs, num_samples=self._num_samples,
                                                filtering=bool(self._filter) and self._device_sampler, speculate=self._speculate,
                                                grammar=self._sample_kwargs.get("grammar"), jump_forward=self._jump)

    def __getattr__(self, name):
        return getattr(self._base, name)

    def infer_reasoning(self, obs: dict) -> dict:
        t0 = time.perf_counter()
        base = self._base
        if base._has_transforms:   # raw client request (policy_adapter.py:25-31)
            raw_state = np.array(obs["observation"]["state"], copy=True)
            inputs = base._input_transform(dict(obs))
        else:
            raw_state = np.array(obs["state"], copy=True) if obs.get("state") is not None else None
            inputs = obs
        o, batched = base._to_observation(inputs)
        self._calls += 1
        temperature = self._sample_kwargs.get("temperature", 0.0)
        spec_stats = None
        if (self._decoder is not None and (temperature <= 0.0 or self._device_sampler)
                and self._sample_kwargs.get("decode", "eager") in ("eager", "fused") and graph_compatible(self._decoder.obs, o)):
            if self._num_beams is not None:
                self._decoder(o)
                tokens, self._beam_scores = self._decoder.last_beams[:2], self._decoder.last_beams[2].cpu().numpy()
            elif self._speculate is not None:
                tokens = self._decoder(o, draft_tokens=self._prev_tokens)
                spec_stats = self._decoder.last_stats
            elif self._jump is not None:
                tokens = (self._decoder(o, temperature=temperature, seed=self._calls, draft_tokens=self._prev_tokens)
                          if self._device_sampler else self._decoder(o, draft_tokens=self._prev_tokens))
                spec_stats = self._decoder.last_stats
            else:
                tokens = (self._decoder(o, temperature=temperature, seed=self._calls, **self._filter) if self._device_sampler
                          else self._decoder(o))
        elif self._num_beams is not None:
            tokens = self._beams(o)
        elif self._drafting:
            tokens = base.model.sample_tokens(self._calls, o, draft_tokens=self._prev_tokens, **self._sample_kwargs)
            spec_stats = base.model.last_spec_stats
        else:
            tokens = base.model.sample_tokens(self._calls, o, **self._sample_kwargs)
        if self._drafting:                  # the next request's draft: this answer up to and including its EOS
            row = (tokens[0] if self._logprobs else tokens)[0].cpu().numpy()
            stop = np.flatnonzero(row == base.model.EOS_TOKEN)
            self._prev_tokens = row[:int(stop[0]) + 1] if stop.size else row
        extra = {}
        if self._logprobs:
            from lap_amd import sampling

            tokens, logp = (t.cpu().numpy() for t in tokens)
            eos = base.model.EOS_TOKEN
            if self._num_beams is not None:       # a padding beam (fewer than N candidates ever existed) is no answer: -inf throughout
                logp = np.where(np.isfinite(self._beam_scores)[:, None], logp, -np.inf)
            seq = sampling.sequence_logprob(tokens, logp, eos)
            if self._num_samples is not None or self._num_beams is not None:     # the answer is one candidate, as a batch of 1; all of them are reported
                extra["candidates"] = {"tokens": tokens, "logprob": seq}
                best = sampling.select_best(tokens, logp, eos, self._select)
                tokens, logp, seq = tokens[best:best + 1], logp[best:best + 1], seq[best:best + 1]
            extra |= {"token_logprobs": logp, "logprob": seq}
            out = {"state": batched.get("state"), "tokens": tokens, "raw_state": raw_state} | extra
        else:
            out = {"state": batched.get("state"), "tokens": tokens.cpu().numpy(), "raw_state": raw_state}
        model_ms = (time.perf_counter() - t0) * 1e3
        if base._has_transforms:      # (the output stack keeps the keys it knows, CoTOutputs: actions and reasoning; the
            out = base._output_transform(out) | extra       # log-probabilities and the candidates go round it to the client)
        out["policy_timing"] = {"infer_ms": model_ms}
        if spec_stats is not None:
            out["policy_timing"] |= {"spec_steps": spec_stats[0], "spec_accepted": spec_stats[1]}
        return out

    def _beams(self, o):
        """All beams of a request off the graph: (tokens [N, steps], logprobs [N, steps]) through the route "decode" names."""
        kw, m = self._sample_kwargs, self._base.model
        N = self._num_beams
        m_kw = dict(max_decoding_steps=kw.get("max_decoding_steps", 390), early_stop=self._select != "mean")
        allowed = ar_decode.allowed_set(m, kw["allowed_tokens"]).ids if kw.get("allowed_tokens") is not None else None
        weights = kw.get("decode_weights", "bf16")
        with m._serving_weights():
            if kw.get("decode", "fused") == "fused":
                ar_decode.check_fused_decode(m, N)
                tok, logp, scores = ar_decode.beam_decode_fused(m, o, N, weights=weights, allowed=allowed, grammar=kw.get("grammar"), **m_kw)
            else:
                tok, logp, scores = ar_decode.beam_decode_eager(m, o, N, allowed=allowed, grammar=kw.get("grammar"), **m_kw)
        self._beam_scores = scores.cpu().numpy()
        return tok, logp

    def score(self, obs: dict, answers, *, select: str = "sum", rows: int = 8) -> dict:
        """Rank GIVEN answers for the request `obs` instead of generating one (`LAP.score_tokens`: the prefix is prefilled once,
        every answer is scored teacher-forced on the serving kernels, `rows` positions per pass over the weights).
        answers: strings, tokenised with the policy's tokenizer the way a training target is (cleaned, no BOS) and with the EOS
        appended, as a generated answer ends; or integer id sequences, taken as they are.  One answer or a list of them.
        sample_kwargs["decode_weights"], ["allowed_tokens"], ["temperature"] and ["max_decoding_steps"] apply; nothing else does.
        Returns {"logp_sum", "logp_mean", "token_accuracy"} (float64 [N]: the sum of an answer's token log-probabilities up to and
        including its first EOS (`sampling.sequence_logprob`), that sum per counted token, and the share of positions where the
        served model's argmax is the given token), "token_logprobs" (N arrays), "tokens" (N arrays: the ids that were scored),
        "best" (the index `sampling.select_best` picks under `select`: the largest sum or mean, the lowest index among ties) and
        "policy_timing".  The scoring steps are launched eagerly: they are not captured into the policy's graphs."""
        from lap_amd import policy_io as pio, sampling

        if select not in ("sum", "mean"):
            raise ValueError(f"ARPolicy.score: select must be 'sum' or 'mean', got {select!r}")
        t0 = time.perf_counter()
        base = self._base
        model = base.model
        if isinstance(answers, str) or (len(answers) > 0 and not isinstance(answers[0], str) and np.ndim(answers[0]) == 0):
            answers = [answers]
        if len(answers) == 0:
            raise ValueError("ARPolicy.score: answers is empty (0 answers)")
        seqs = []
        for a in answers:
            if isinstance(a, str):
                tok = self._tokenizer or next((t.tokenizer for t in base._transforms if isinstance(t, pio.TokenizePromptAndReasoning)), None)
                if tok is None:
                    raise ValueError("ARPolicy.score: an answer string needs the policy's tokenizer (a policy without transforms "
                                     "takes token id sequences)")
                a = list(tok.encode(a.strip().replace("_", " ").replace("\n", " "), add_bos=False, add_eos=False)) + [model.EOS_TOKEN]
            seqs.append(a)
        inputs = base._input_transform(dict(obs)) if base._has_transforms else obs
        o, _ = base._to_observation(inputs)
        kw = self._sample_kwargs
        res = model.score_tokens(o, seqs, rows=rows, temperature=kw.get("temperature", 0.0), decode_weights=kw.get("decode_weights", "bf16"),
                                 allowed_tokens=kw.get("allowed_tokens"), max_decoding_steps=kw.get("max_decoding_steps", 390))
        eos = model.EOS_TOKEN
        tokens = [np.asarray(s, dtype=np.int32).reshape(-1) for s in seqs]
        logp = [lp.cpu().numpy() for lp in res.logp]
        greedy = [g.cpu().numpy() for g in res.greedy]
        total = np.array([sampling.sequence_logprob(t[None], lp[None], eos)[0] for t, lp in zip(tokens, logp)])
        count = np.array([int(sampling._counted(t[None], eos).sum()) for t in tokens])
        mean = total / count
        acc = np.array([float((g == t).mean()) for g, t in zip(greedy, tokens)])
        best = int(np.argmax(total if select == "sum" else mean))       # (sampling.select_best's rule on rows of their own lengths)
        return {"logp_sum": total, "logp_mean": mean, "token_accuracy": acc, "token_logprobs": logp, "tokens": tokens, "best": best,
                "policy_timing": {"infer_ms": (time.perf_counter() - t0) * 1e3}}

    def infer(self, obs: dict, *, noise=None) -> dict:
        return self.infer_reasoning(obs)

    def vqa_infer(self, obs: dict) -> dict:
        return self.infer_reasoning(obs)


def create_trained_policy_ar(*args, sample_kwargs: dict | None = None, language_action_format="verbose_eef_with_rotation",
                             ar_graph: bool = False, grammar: bool = False, grammar_limits: dict | None = None, jump_forward=None,
                             num_beams=None, **kwargs) -> ARPolicy:
    """policy_config_adapter.py:157-160 with the AR output stack [DetokenizeReasoning, CoTOutputs(language_action_format)]:
    generated ids -> text -> [dx, dy, dz, droll, dpitch, dyaw, gripper] (the language action describes the whole chunk as
    one delta, output_transforms.py:75-104; `Unnormalize` has no `actions` statistics to apply to such deltas and is left out
    as in the reference's standard stack it would act on the normalised `state` only).
    ar_graph: serve greedy requests through a GraphedTokenDecoder (ARPolicy(use_graph=True)); off by default.  With
    sample_kwargs={"temperature": T, "sampler": "device"} the same graphs serve sampled requests too;
    sample_kwargs={"decode_weights": "fp8" | "fp8_layers"} decodes on fp8 weights (implies decode="fused") on either route;
    sample_kwargs={"allowed_tokens": ids} constrains every token to that set on either route (`policy_io.allowed_token_ids`);
    sample_kwargs={"return_logprobs": True} adds "token_logprobs" (f32 [1, steps]) and "logprob" (the sum up to the EOS) to the
    result; sample_kwargs={"num_samples": N, "select": "sum" | "mean"} (with "temperature" > 0 and "sampler": "device"; implies
    decode="fused") decodes N candidates per request, runs the output transforms on the one `sampling.select_best` picks and
    reports all N under "candidates": {"tokens" [N, steps], "logprob" [N]};
    sample_kwargs={"top_k": k, "top_p": p} (with "temperature" > 0 and "sampler": "device") draws every token among the k most
    likely candidates and, of those, the nucleus of mass p (`LAP.sample_tokens`; `sampling.filter_keep` restates the kept set) on
    either route: the decoder is captured with filtering=True when either is present; log-probabilities stay the model's (over
    all candidates), so best-of-N ranks as before;
    sample_kwargs={"speculate": S} (2 <= S <= 8, greedy; implies decode="fused") decodes every request on verify steps of S rows
    with the previous request's answer as the draft (`LAP.sample_tokens`): the tokens are unchanged, and "policy_timing" gains
    "spec_steps" and "spec_accepted".  These keys are added to what the output stack
    returns ({"actions", "reasoning"}), so a client of this policy and of the websocket server receives them.
    grammar=True: every answer is constrained to the grammar of `language_action_format` (`policy_io.grammar_automaton` under the
    policy's tokenizer, for the model's vocabulary; sample_kwargs["grammar"] may instead hold an automaton of one's own), so a
    sampled answer (best-of-N, temperature > 0) always parses; grammar_limits: the keywords of `lang_actions.word_graph`.
    jump_forward=S (2 <= S <= 8; with grammar=True or an automaton in sample_kwargs; the same as sample_kwargs={"jump_forward": S}):
    the constrained answer is decoded on steps of S rows on which the tokens the grammar forces, and what the previous request's
    answer drafts, ride along (`LAP.sample_tokens`); tokens and log-probabilities are unchanged, at any temperature, and
    "policy_timing" gains "spec_steps" and "spec_accepted".
    num_beams=N (the same as sample_kwargs={"num_beams": N}): beam search; with grammar=True the answer is the most probable sentence
    of the format among the N beams kept (`beam.grammar_beam_step`), so it always parses.
    The policy's `score(obs, answers)` ranks GIVEN answer strings (or id sequences) for a request with this tokenizer
    (`LAP.score_tokens`)."""
    from lap_amd import policy_io as pio

    base = create_trained_policy(*args, use_graph=False, **kwargs)
    tok = next(t.tokenizer for t in base._transforms if isinstance(t, pio.TokenizePromptAndReasoning))
    if grammar:
        sample_kwargs = dict(sample_kwargs or {})
        sample_kwargs["grammar"] = pio.grammar_automaton(tok, language_action_format, vocab_size=base.model.config.vocab_size,
                                                         **(grammar_limits or {}))
    if jump_forward is not None:
        sample_kwargs = dict(sample_kwargs or {}) | {"jump_forward": jump_forward}
    if num_beams is not None:
        sample_kwargs = dict(sample_kwargs or {}) | {"num_beams": num_beams}
    base._output_transform = pio.compose([pio.DetokenizeReasoning(tok), pio.CoTOutputs(language_action_format=language_action_format)])
    return ARPolicy(base, sample_kwargs=sample_kwargs, use_graph=ar_graph, tokenizer=tok)
