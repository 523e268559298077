"""LAP on MI355X: the model object behind `LAPConfig.create()` / `.load()`.

Keeps the reference's model surface (src/lap/models/lap.py):
    compute_loss(rng, observation, actions, *, train=False, ...) -> (loss, metrics)      lap.py:380-602
    sample_actions(rng, observation, *, num_steps=10, noise=None) -> [b, ah, ad]         lap.py:605-675
and adds `loss_and_grad(...)`, the fused forward + hand-written backward that the train step uses (the
reference gets it from nnx.value_and_grad, scripts/train.py:358-361).

Everything numeric is a call into liblap_hip.so (lap_amd/hip.py); torch only owns device memory, the stream,
and a few O(batch x tokens) integer tensors (masks -> per-token info words, positions).  There is no autograd
and no fallback path.  Activations needed by the backward are kept in HBM (288 GB per MI355X) instead of being
recomputed — the reference rematerialises every block (gemma.py:418-423 nothing_saveable), which costs a
fourth forward pass.

What is here: the switches (`LAP_*`, read in `__init__`), how the model reads a parameter and routes a product (`W` / `F` / `G`,
`_wgrad` / `_bgrad`, the fp8 and LoRA routes, merged serving weights), the per-token info words, the two streams' embeddings with
their backward, and `_loss_impl`, the schedule of the train step (streams, collectives, the order of the passes).  What it calls
are modules of functions on the model:
    joint_layers.py     the joint Gemma layers, forward and backward (both experts; the last layer's row subset)
    siglip.py           the SigLIP training tower
    streams.py          the suffix stream and its hand-offs, the weight-gradient stream (`model.wg`)
    loss.py             the language head, the action head, the sample-weight mixing
    flow_sample.py, ar_decode.py, prefill.py    the serving paths: action sampler, token decoding, their prefill
"""
from __future__ import annotations

import contextlib
import math
import os

import torch

from lap_amd import hip
from lap_amd.config import LAPConfig, get_gemma_config, get_siglip_config
from lap_amd.joint_layers import last_layer_rows, llm_bwd, llm_fwd
from lap_amd.loss import (ActionHead, LangHead, action_head_bwd, action_head_fwd, lang_head_bwd, lang_head_fwd, mix_sample_weights,
                          select_loss_rows)
from lap_amd.observation import CoTObservation, preprocess_observation
from lap_amd.params import LORA_PROJ, ParamStore, lora_geometry
from lap_amd.serve_cache import ServeCache
from lap_amd.siglip import siglip_bwd, siglip_fwd
from lap_amd.streams import OffPathStream, handoff, suffix_stream

SUFFIX_IDX_BASE = 0x800000  # suffix ar-indices live above every prefix index (see _train_infos)


class _NullComm:
    """world_size == 1: parameters are always resident, gradients stay where they are written."""
    world_size = 1

    def wait_unit(self, name, also=None): pass
    def pace(self, name): pass
    def grads_ready(self, name, also=None): pass
    def before_backward(self): pass
    def all_reduce_sum(self, t): return t


def _gen(rng, device):
    if isinstance(rng, torch.Generator):
        return rng
    g = torch.Generator(device=device)
    g.manual_seed(int(rng) if rng is not None else 0)
    return g


class LAP:
    EOS_TOKEN = 1   # PaliGemma <eos> (lap.py: self.EOS_TOKEN)

    def __init__(self, config: LAPConfig, seed: int = 0, params: dict | None = None, device="cuda", store: ParamStore | None = None,
                 comm=None, with_optimizer: bool = False, with_ema: bool = False, with_grads: bool = True, gemm_dtype: str = "bf16"):
        self.config = config
        if gemm_dtype not in ("bf16", "fp8"):
            raise ValueError(f"gemm_dtype {gemm_dtype!r}: 'bf16' or 'fp8'")
        self.gemm_dtype = gemm_dtype
        self._w8: dict = {}     # fp8 mirrors of the VLM projections: name -> (store version, W8, W8t, scale)
        self.device = torch.device(device)
        self.v = get_gemma_config(config.paligemma_variant)
        self.e = get_gemma_config(config.action_expert_variant)
        self.s = get_siglip_config(config.siglip_variant)
        self.action_dim, self.action_horizon, self.max_token_len = config.action_dim, config.action_horizon, config.max_token_len
        self.comm = comm if comm is not None else _NullComm()
        if store is None:
            store = ParamStore(config, device, with_optimizer=with_optimizer, with_ema=with_ema, with_grads=with_grads)
            if params is not None:
                store.load_reference_tree(params)
            else:
                store.init_random(seed)
        self.ps = store
        self.n_img_tok = (config.image_size // self.s.patch) ** 2
        self.deterministic = True
        self.dual_stream = os.environ.get("LAP_DUAL_STREAM", "1") != "0"
        # serving prefill on the fused consumers (lap_amd/prefill.py); "0": the generic layer loops (A/B, tests)
        self.serve_fusions = os.environ.get("LAP_SERVE_FUSIONS", "1") != "0"
        # prefix stream, bf16: d(act) of the down projection goes straight into the GeGLU backward inside the assembly GEMM's epilogue
        self.fuse_geglu_bwd = os.environ.get("LAP_FUSE_GEGLU_BWD", "1") != "0" and gemm_dtype != "fp8"
        self.fuse_geglu_fwd = os.environ.get("LAP_FUSE_GEGLU_FWD", "1") != "0" and gemm_dtype != "fp8"
        self.fuse_gelu = os.environ.get("LAP_FUSE_GELU", "1") != "0"      # SigLIP MLP: GELU forward / backward inside the Dense GEMMs
        # train step: the last joint layer's prefix stream keeps K / V of every row but runs everything behind them on the rows the
        # language head reads (`joint_layers.last_layer_rows`).  LAP_LAST_LAYER_ROWS=0: all rows, as every other layer (A/B runs, tests)
        self.last_layer_rows = os.environ.get("LAP_LAST_LAYER_ROWS", "1") != "0"
        self.last_rows_steps = 0      # passes that took the row-subset path (tests read it)
        # first denoise step on a second stream beside the prefill (it needs layer l's K / V only at its layer l).  Measured, hipGraph
        # replay, same box, interleaved: 15.65 -> 16.30 ms per chunk — the step's 110 short kernels take CUs from the prefill's
        # load-bound GEMMs for longer than they save.  Kept as a switch, OFF by default.
        self.serve_overlap = os.environ.get("LAP_SERVE_OVERLAP", "0") != "0"
        # the 18 action-expert layers of a denoise step as ONE persistent launch (csrc/serve_chain.hpp) instead of 6 launches per
        # layer; bitwise equal to them.  LAP_SERVE_CHAIN=0: the separate launches (A/B runs, tests).
        self.serve_chain = os.environ.get("LAP_SERVE_CHAIN", "1") != "0"
        # ... on fragment-packed operands (round 4: every operand load 1 KiB contiguous per wave instruction; same bits).
        # LAP_SERVE_PACKED=0: the row-major chain of round 3 (A/B runs, tests)
        self.serve_packed = os.environ.get("LAP_SERVE_PACKED", "1") != "0"
        # ... mapped onto the chip as 8-way tensor parallelism over the XCDs (csrc/serve_chain_tp.hpp: two chip-wide seams per layer
        # instead of five; bf16-rounding-noise equal to the flat chain, not bitwise).  LAP_SERVE_TP=0: the flat packed chain
        self.serve_tp = os.environ.get("LAP_SERVE_TP", "0") != "0"
        # an Euler step's tail (final adaRMS + action_out_proj + x_t update) and the next step's action_in_proj in one launch
        # (csrc/serve_skinny.hip final_euler_embed_kernel; same arithmetic).  LAP_SERVE_EULER_EMBED=0: the two launches
        self.serve_euler_embed = os.environ.get("LAP_SERVE_EULER_EMBED", "1") != "0"
        # the serving prefill's small projections (SigLIP qkv / out / fc1 / fc2; Gemma's qkv / out opt-in, see _panel_llm) on the row-panel kernel
        # (csrc/serve_panel.hip: the rows of A resident in LDS, packed weights streamed into MFMA fragments, no barrier in the k-loop)
        # against packed weight images kept per parameter version (+1.0 GB for LAP-3B).  qkv / out / fc1 are bitwise equal to the
        # unsplit tiles they replace.  LAP_SERVE_PANEL=0: the LDS-tiled kernels (A/B runs, tests)
        self.serve_panel = os.environ.get("LAP_SERVE_PANEL", "1") != "0"
        # the prefill's fused GELU / GeGLU epilogues (SigLIP fc1 on the panel kernel, Gemma's gate|up tile) through v_exp / v_rcp, the training
        # kernels' arithmetic; "bf16": tanhf (A/B)
        self._panel_gelu = os.environ.get("LAP_SERVE_PANEL_GELU", "exp2")
        # which Gemma prefill projections take the panel kernel (q, o): none by default — in the chunk the out projection takes 23 us there
        # against 19.6 on the LDS tile (14.6 on cache-warm weights), qkv as one f32 slab 25 against the split-K tile's 17 (12.06 / 12.14 / 12.22 ms)
        self._panel_llm = os.environ.get("LAP_SERVE_PANEL_LLM", "")
        # feature tiles of 16 per wave for SigLIP's qkv / out / fc1 / fc2 on the panel kernel (tuning knob; sweep in the chunk: docs/EXPERIMENTS.md K)
        self._panel_nt = tuple(int(v) for v in os.environ.get("LAP_SERVE_PANEL_NT", "2,1,3,3").split(","))
        # ... and every panel launch pulls the NEXT launch's weights into the Infinity Cache with a fifth wave per block (the chain's
        # launches otherwise meet their weights HBM-cold).  LAP_SERVE_PREFETCH=0: off (A/B runs)
        self.serve_prefetch = os.environ.get("LAP_SERVE_PREFETCH", "1") != "0"
        self._chain_ctr = self._chain_scratch = self._den = None     # the chain's barrier counters and scratch, the overlap's side stream
        # K splits of the prefill's qkv / out / down projections, down's tile.  Round 5 sweep incl. the consumer (tools/probes/
        # prefill_down_sweep.py, us per GEMM + reduce / residual / norm): 256 x 256 x 8 65.0 | 320 x 128 (tile 19) x 8 60.8 | 320 x 256 x 16 64.5
        ks = os.environ.get("LAP_PREFILL_KS", "4,1,8,19").split(",")
        self._prefill_ks = tuple(int(k) for k in ks)
        self.sfx = None         # the suffix stream's HIP stream (created on first use: streams.suffix_stream)
        # which gradients leave the data-gradient path for a third stream (lap_amd/streams.py): s SigLIP weights, b biases, q / g the
        # prefix stream's attention / MLP projections; "1" all, "0" none.  Measured (tools/ab3.sh, interleaved on one box): sb
        # -2.1 .. -3.3 ms per step in round 2 and -2.6 ms in round 3 (310.0 -> 307.4), s -1.3, q 0, all +12.6.  Default "sb":
        # step time is the decision variable (the compute stream's GEMMs then share the chip, so their EVENT-timed rate drops
        # by 4 % — bench.py's roofline figure is computed from isolated per-shape times for that reason).
        mode = os.environ.get("LAP_WGRAD_STREAM", "sb")
        self.wgrad_stream = "" if mode == "0" else mode
        self.wg = OffPathStream(self.device)
        # LoRA adapters (config.GemmaConfig.lora_attn / lora_ffn): projection key ("wgu0", ...) -> (G, nsum, s), see params.lora_geometry.
        # Training keeps base and adapters apart (csrc/lora.hip); the serving paths run on merged weights (`_serving_weights`)
        self._lora_geo = {}
        for i, c in enumerate((self.v, self.e)):
            for proj in LORA_PROJ:
                geo = lora_geometry(c, proj, self.v.num_heads, self.v.num_kv_heads, self.v.head_dim)
                if geo is not None:
                    self._lora_geo[f"{proj}{i}"] = (geo[0], geo[2], geo[3])
        self._merge_depth = 0
        # every parameter-derived tensor of the serving paths (`_merged`, `_dec_fp8`, `prefill.panel_weight`, `flow_sample.serve_packed_weights`, `serve_mods`)
        self.serving_cache = ServeCache(self.ps, self.device, lambda unit: self.comm.wait_unit(unit))
        if self._lora_geo and gemm_dtype == "fp8":
            raise ValueError("gemm_dtype='fp8' has no LoRA route: use gemm_dtype='bf16' with the LoRA Gemma variants")
        if gemm_dtype == "fp8":
            dims = (self.v.width, self.v.num_heads * self.v.head_dim, self.v.mlp_dim, (self.v.num_heads + 2 * self.v.num_kv_heads) * self.v.head_dim)
            if any(d % 128 for d in dims):
                raise ValueError(f"gemm_dtype='fp8' needs projection dimensions that are multiples of 128, got {dims}")

    # ------------------------------------------------------------------ small helpers
    def W(self, name):
        if self._merge_depth and name.rsplit("/", 1)[-1] in self._lora_geo:
            return self._merged(name)
        return self.ps.w16(name)

    def F(self, name):
        return self.ps.f32(name)

    def G(self, name):
        return self.ps.g(name)

    def _wgrad(self, dy, x, name, **kw):
        """Weight gradient dWt = dy^T x into the gradient buffer of `name` — skipped for frozen parameters
        (scripts/train.py:358-361 differentiates w.r.t. the trainable filter only)."""
        if self.ps.is_trainable(name):
            mode = self.wgrad_stream
            kind = "s" if name.startswith("img/") else ("q" if name.endswith(("wqkv0", "wo0")) else "g")
            fold = not kw and getattr(self.comm, "fold_sumsq", False) and dy.dtype == torch.bfloat16

            def run():
                if fold:    # the weight gradient and, where the assembly kernel takes it, its share of the gradient norm in one launch
                    if hip.linear_wgrad_sumsq(dy, x, self.G(name), self.comm.sumsq[0:1]):
                        self.comm.folded.add(name)
                else:
                    hip.linear_wgrad(dy, x, self.G(name), **kw)
            if mode == "1" or kind in mode:
                with self.wg.run(dy, x):
                    run()
            else:
                run()

    def _bgrad(self, dy, name):
        """Bias gradient = column sums of dy, next to the weight gradient."""
        mode = self.wgrad_stream
        if mode == "1" or "b" in mode:
            with self.wg.run(dy):
                hip.colsum(dy, self.G(name))
        else:
            hip.colsum(dy, self.G(name))

    # ---- LoRA adapters (lora.Einsum / lora.FeedForward, gemma.py:180-200,279-285,366-372; csrc/lora.hip)
    def _lora(self, name):
        """(A, B, G, nsum, s) of the adapters on projection `name` ("llm/{l}/wgu0", ...), or None: no adapters there, or the
        serving paths are running on merged weights."""
        if not self._lora_geo or self._merge_depth:
            return None
        _, l, key = name.split("/")
        geo = self._lora_geo.get(key)
        if geo is None:
            return None
        return (self.ps.w16(f"llm/{l}/lora_a_{key}"), self.ps.w16(f"llm/{l}/lora_b_{key}"), *geo)

    def _lora_fwd(self, x, y, name):
        """y += bf16(s * bf16(t B)) in place with t = bf16(x A^T), per group; returns t (kept for the backward) or None.
        Where the base projection has a fused residual, y already holds it: the LoRA term is added after."""
        lo = self._lora(name)
        if lo is None:
            return None
        A, Bm, G, nsum, s = lo
        t = hip.lora_down(x, A)
        hip.lora_up_add(y, t, Bm, G=G, nsum=nsum, s=s)
        return t

    def _lora_bwd(self, dy, x, t, dx, name):
        """The adapters' share of a projection's backward: dt = bf16(bf16(s dy) B^T) per group, dx += bf16(dt A) in place, and the
        adapter gradients dA = dt^T x, dB = t^T bf16(s dy) (every stacked copy of B gets dB) like `_wgrad` (off the path where the
        base projection's would be)."""
        lo = self._lora(name)
        if lo is None:
            return
        A, Bm, G, nsum, s = lo
        Ng = Bm.shape[1]
        dt = hip.lora_down(dy, Bm, G=G, nsum=nsum, xg=Ng if G > 1 else 0, s=s)
        _, l, key = name.split("/")
        na, nb = f"llm/{l}/lora_a_{key}", f"llm/{l}/lora_b_{key}"

        def run():
            if self.ps.is_trainable(na):
                hip.lora_wgrad(dt, x, self.G(na))
            if self.ps.is_trainable(nb):
                hip.lora_wgrad(t, dy, self.G(nb), G=G, bg=Ng if G > 1 else 0, ncopy=nsum, s=s)
        mode = self.wgrad_stream
        if mode == "1" or ("q" if key in ("wqkv0", "wo0") else "g") in mode:
            with self.wg.run(dy, x, t, dt):
                run()
        else:
            run()
        if dx is not None:
            hip.lora_up_add(dx, dt, A)

    def _merged(self, name):
        """bf16(W + s B^T A) of a LoRA'd projection from the f32 masters, rounded once (csrc/lora.hip lap_lora_merge): persistent
        like `flow_sample.serve_mods` and recomputed in place per parameter version."""
        def build(old):
            _, l, key = name.split("/")
            self.comm.wait_unit(f"llm{l}")
            G, nsum, s = self._lora_geo[key]
            out = old if old is not None else torch.empty(self.ps.tensor_spec[name].shape, dtype=torch.bfloat16, device=self.device)
            return hip.lora_merge(self.F(name), self.F(f"llm/{l}/lora_a_{key}"), self.F(f"llm/{l}/lora_b_{key}"), out, G=G, nsum=nsum, s=s)
        return self.serving_cache.get(("merged", name), None, build)

    @contextlib.contextmanager
    def _serving_weights(self):
        """The serving paths (sample_actions, sample_tokens, their caches) read every LoRA'd projection as ONE merged bf16 weight
        (`_merged`) instead of base + adapters: every fused serving kernel applies unchanged.  The reference serves unmerged."""
        if not self._lora_geo:
            yield
            return
        if self.comm.world_size != 1:
            raise NotImplementedError("LoRA serving merges the weights from the f32 masters: replicas only")
        self._merge_depth += 1
        try:
            yield
        finally:
            self._merge_depth -= 1

    # ---- fp8 routing of the VLM expert's projections (BASELINE.json config 5; csrc/gemm_fp8.hip)
    def _w8_of(self, name):
        """(W8 [out][in], W8t [in][out], scale) of a VLM projection, re-quantised when the parameters changed."""
        ent = self._w8.get(name)
        if ent is None or ent[0] != self.ps.version:
            ent = (self.ps.version, *hip.quantize_fp8_weight(self.W(name)))
            self._w8[name] = ent
        return ent[1:]

    def _lin0(self, x, name, residual=None, out=None, tile=-1):
        """y = x @ Wt^T (+ residual) for a prefix-stream projection: bf16 MFMA GEMM, or e4m3 x e4m3 when gemm_dtype == 'fp8'."""
        if self.gemm_dtype == "fp8":
            x8, sx = hip.quantize_fp8(x)
            w8, _, sw = self._w8_of(name)
            return hip.gemm_fp8(x8, sx, w8, sw, residual=residual)
        if residual is not None and os.environ.get("LAP_UNFUSED_RESIDUAL", "0") == "1":
            # measurement switch: the reference rounds the projection to bf16 and then the sum to bf16
            # (gemma.py:285,582-583); the fused epilogue adds in f32 and rounds once
            return hip.add_bf16(residual, hip.linear_fwd(x, self.W(name)))
        return hip.linear_fwd(x, self.W(name), out, residual=residual, tile=tile)

    def _dgrad0(self, dy, name):
        """dx = dy @ Wt for a prefix-stream projection (the fp8 route multiplies by the transposed fp8 copy)."""
        if self.gemm_dtype == "fp8":
            d8, sd = hip.quantize_fp8(dy)
            _, w8t, sw = self._w8_of(name)
            return hip.gemm_fp8(d8, sd, w8t, sw)
        return hip.linear_dgrad(dy, self.W(name))

    def _prefix_frozen(self) -> bool:
        """True when no parameter reached by the prefix stream's backward is trainable (e.g. `get_vlm_freeze_filter`):
        the language-head, VLM and SigLIP backward passes are then skipped altogether.  The VLM's adapters
        (`llm/{l}/lora_{a,b}_<proj>0`) end in "0" like its base weights: under `get_freeze_filter` they keep this False."""
        fr = self.ps.frozen
        if not fr:
            return False
        return all(v for k, v in fr.items() if k.startswith("img/") or k in ("llm/embed", "llm/final_norm")
                   or (k.startswith("llm/") and (k.endswith("0") or k.endswith("n_attn") or k.endswith("n_ffw"))))

    def _lin32(self, x, wname, bname):
        """nnx.Linear in f32: y = x @ W^T + b (W stored [out][in])."""
        w = self.F(wname)
        out = torch.empty((x.shape[0], w.shape[0]), dtype=torch.float32, device=x.device)
        return hip.gemm_f32(x, w, out, M=x.shape[0], N=w.shape[0], K=w.shape[1], lda=x.stride(0), ldb=w.stride(0), ldc=w.shape[0],
                            bias=self.F(bname))

    def _lin32_bwd(self, x, dy, wname, bname, need_dx=True):
        """Gradients of _lin32: dW += dy^T x, db += colsum(dy), returns dx = dy @ W."""
        w = self.F(wname)
        hip.gemm_f32(dy, x, self.G(wname), M=w.shape[0], N=w.shape[1], K=x.shape[0], lda=dy.stride(0), ldb=x.stride(0), ldc=w.shape[1],
                     a_kc=False, b_kc=False, accum=True)
        hip.colsum(dy, self.G(bname))
        if not need_dx:
            return None
        dx = torch.empty_like(x)
        return hip.gemm_f32(dy, w, dx, M=x.shape[0], N=w.shape[1], K=w.shape[0], lda=dy.stride(0), ldb=w.stride(0), ldc=w.shape[1],
                            a_kc=True, b_kc=False)

    # ================================================================== token info words / positions
    def _prefix_masks(self, obs: CoTObservation):
        """lap.py:118-170: input mask and ar mask over [image tokens ..., prompt tokens]."""
        B = obs.tokenized_prompt.shape[0]
        T = self.n_img_tok
        im = [obs.image_masks[k][:, None].expand(B, T) for k in self.config.image_keys]
        prefix_mask = torch.cat(im + [obs.tokenized_prompt_mask], 1)
        zeros = torch.zeros(B, T * len(im), dtype=torch.bool, device=prefix_mask.device)
        la = obs.tokenized_langact_mask if obs.tokenized_langact_mask is not None else torch.zeros_like(obs.tokenized_prompt_mask)
        return prefix_mask, torch.cat([zeros, la], 1)

    def _suffix_idx(self, B, S, dev):
        """Block indices of the suffix tokens ([B, S] for pi05; [B, S + 1] with pi0's state token in front, one block earlier)."""
        idx = torch.full((B, S), SUFFIX_IDX_BASE + 1, dtype=torch.int32, device=dev)
        if S and not self.config.pi05:
            idx = torch.cat([idx[:, :1], idx + 1], 1)
        return idx

    def _train_infos(self, obs: CoTObservation, S: int):
        """Per-token info words equivalent to _build_combined_attention_mask / make_attn_mask (lap.py:303-364):
        class bit 1: valid prefix token (seen by prefix queries);  bit 2: in prefix_mask_action (seen by action
        queries);  bit 4: suffix token.  Low 24 bits: cumulative ar index (suffix indices offset above all prefix
        ones).  Positions per lap.py:366-377."""
        prefix_mask, prefix_ar = self._prefix_masks(obs)
        B, Pn = prefix_mask.shape
        dev = prefix_mask.device
        pma = prefix_mask & ~prefix_ar if obs.tokenized_langact_mask is not None else prefix_mask  # lap.py:303-325
        cs = torch.cumsum(prefix_ar.to(torch.int32), 1)
        kcls = prefix_mask.to(torch.int32) | (pma.to(torch.int32) << 1)
        kinfo_p = (kcls << 24) | cs
        qinfo_p = (prefix_mask.to(torch.int32) << 24) | cs
        # suffix: mask all ones, ar = [1, 0, ...] (embed_suffix pi05) -> one block; pi0: a state token in front as a block of its
        # own (ar = [1, 1, 0, ...]): the action tokens see it, it does not see them
        s_idx = self._suffix_idx(B, S, dev)
        S = s_idx.shape[1]
        kinfo = torch.cat([kinfo_p, (4 << 24) | s_idx], 1).to(torch.int32).contiguous()  # cumsum promoted to int64
        qinfo = torch.cat([qinfo_p, (6 << 24) | s_idx], 1).to(torch.int32).contiguous()
        ppos = torch.cumsum(prefix_mask.to(torch.int32), 1) - 1
        spos = pma.sum(-1, keepdim=True).to(torch.int32) + torch.arange(S, dtype=torch.int32, device=dev)[None]
        pos = torch.cat([ppos, spos], 1).to(torch.int32).contiguous()
        return qinfo, kinfo, pos

    def _serve_infos(self, obs: CoTObservation, S: int):
        """sample_actions masks (lap.py:624-654): prefix attends per make_attn_mask(prefix_mask, prefix_ar); suffix
        queries see every valid prefix token and all suffix tokens; suffix positions follow sum(prefix_mask)."""
        keys = self.config.image_keys
        if (self.config.pi05 and self.serve_fusions and obs.tokenized_prompt_mask.is_cuda and len(keys) <= 4
                and all(obs.image_masks[k].dtype == torch.bool for k in keys) and obs.tokenized_prompt_mask.dtype == torch.bool):
            la = obs.tokenized_langact_mask
            return hip.serve_infos([obs.image_masks[k].contiguous() for k in keys], self.n_img_tok, obs.tokenized_prompt_mask.contiguous(),
                                   None if la is None else la.to(torch.bool).contiguous(), S, SUFFIX_IDX_BASE + 1)
        prefix_mask, prefix_ar = self._prefix_masks(obs)
        B, Pn = prefix_mask.shape
        dev = prefix_mask.device
        cs = torch.cumsum(prefix_ar.to(torch.int32), 1)
        pm = prefix_mask.to(torch.int32)
        kinfo_p = ((pm | (pm << 1)) << 24) | cs
        qinfo_p = (pm << 24) | cs
        s_idx = self._suffix_idx(B, S, dev)
        S = s_idx.shape[1]
        kinfo_s, qinfo_s = (4 << 24) | s_idx, (6 << 24) | s_idx
        ppos = (torch.cumsum(pm, 1) - 1).to(torch.int32).contiguous()
        spos = (pm.sum(-1, keepdim=True) + torch.arange(S, dtype=torch.int32, device=dev)[None]).to(torch.int32)
        i32 = lambda t: t.to(torch.int32).contiguous()
        return (i32(qinfo_p), i32(kinfo_p), ppos, i32(qinfo_s), i32(torch.cat([kinfo_p, kinfo_s], 1)), i32(torch.cat([ppos, spos], 1)))

    # ================================================================== embedding of the two streams
    def _embed_prefix(self, obs: CoTObservation, save: bool, collect=None, tower=None):
        """lap.py:118-170 -> x0 bf16 [B*Pn, Dv] with rows (b, [img0 | img1 | prompt]).  tower: the serving callers' (prefill.siglip_fwd_serve)."""
        B, Lt = obs.tokenized_prompt.shape
        T, Dv, keys = self.n_img_tok, self.v.width, self.config.image_keys
        Pn = T * len(keys) + Lt
        images = torch.cat([obs.images[k] for k in keys], 0)
        fused = tower is not None and self.serve_fusions and not save and collect is None
        tok, ictx = (tower(self, images), None) if fused else siglip_fwd(self, images, save, collect)
        x0 = torch.empty((B * Pn, Dv), dtype=torch.bfloat16, device=self.device)
        for i in range(len(keys)):
            hip.copy_rows_bf16(tok[i * B * T:(i + 1) * B * T], x0, B * T, T, Dv, T, 0, Pn, i * T)
        self.comm.wait_unit("embed")
        tokens = obs.tokenized_prompt.to(torch.int32).contiguous()
        rows, lo, hi = self.ps.embed_rows()
        if self.comm.world_size == 1:
            hip.embed_gather(rows, tokens, x0, B * Lt, Lt, Dv, Pn, T * len(keys), math.sqrt(Dv), lo, hi)
        else:
            self.comm.sharded_embed_gather(rows, lo, hi, tokens, x0, Lt, Dv, Pn, T * len(keys), math.sqrt(Dv))
        return x0, Pn, (ictx, tokens)

    def _embed_prefix_bwd(self, pctx, dx0, B, Pn):
        ictx, tokens = pctx
        keys = self.config.image_keys
        T, Lt, Dv = self.n_img_tok, tokens.shape[1], self.v.width
        hip.embed_scatter_add(self.G("llm/embed"), tokens, dx0, B * Lt, Lt, Dv, Pn, T * len(keys), math.sqrt(Dv))
        self.comm.grads_ready("embed")
        dtok = torch.empty((len(keys) * B * T, Dv), dtype=torch.bfloat16, device=self.device)
        for i in range(len(keys)):
            hip.copy_rows_bf16(dx0, dtok[i * B * T:(i + 1) * B * T], B * T, T, Dv, Pn, i * T, T, 0)
        siglip_bwd(self, ictx, dtok)

    def _time_mod(self, time: torch.Tensor, save: bool):
        """[UPSTREAM-RECALL] openpi Pi0.embed_suffix (pi05), time branch: posemb_sincos -> time_mlp_in -> swish ->
        time_mlp_out -> swish = adaRMS condition; then all 2L+1 adaRMS Dense layers (gemma.py:128) as ONE GEMM against the
        adaRMS bank.  time f32 [n] -> mod bf16 [n, nslots*3*We]."""
        We = self.e.width
        temb = hip.posemb_sincos(time.contiguous(), We, 4e-3, 4.0)
        h1 = self._lin32(temb, "act/time_in_w", "act/time_in_b")
        s1 = hip.swish_fwd(h1)
        h2 = self._lin32(s1, "act/time_out_w", "act/time_out_b")
        cond = hip.swish_fwd(h2)
        cond16 = hip.cast_f32_to_bf16(cond)
        mod = hip.linear_fwd(cond16, self.W("ada/w"), bias=self.F("ada/b"))
        return mod, ((temb, h1, s1, h2, cond16) if save else None)

    def _embed_actions(self, x_t: torch.Tensor):
        """action_in_proj (f32 nnx.Linear, lap.py:52) on the noisy actions -> bf16 suffix tokens."""
        B, S, ad = x_t.shape
        xt2 = x_t.reshape(B * S, ad).contiguous()
        return hip.cast_f32_to_bf16(self._lin32(xt2, "act/in_w", "act/in_b")), xt2

    def _embed_suffix_pi0(self, x_t: torch.Tensor, time: torch.Tensor, state: torch.Tensor, save: bool):
        """[UPSTREAM-RECALL] openpi Pi0.embed_suffix, pi0 branch (parameters: lap.py:56-61): a state token `state_proj(state)`, then the
        action tokens mixed with the time embedding: action_time_mlp_out(swish(action_time_mlp_in([action_in_proj(x_t) | posemb(t)]))).
        f32 nnx.Linear layers; -> bf16 suffix tokens [B * (S + 1), We], no adaRMS condition."""
        B, S, ad = x_t.shape
        We = self.e.width
        xt2 = x_t.reshape(B * S, ad).contiguous()
        a = self._lin32(xt2, "act/in_w", "act/in_b")
        temb = hip.posemb_sincos(time.contiguous(), We, 4e-3, 4.0)
        cat = torch.cat([a.view(B, S, We), temb[:, None, :].expand(B, S, We)], -1).reshape(B * S, 2 * We).contiguous()
        h1 = self._lin32(cat, "act/atime_in_w", "act/atime_in_b")
        s1 = hip.swish_fwd(h1)
        at = self._lin32(s1, "act/atime_out_w", "act/atime_out_b")
        st2 = state.to(self.device, torch.float32).reshape(B, ad).contiguous()
        st = self._lin32(st2, "act/state_w", "act/state_b")
        tok = torch.cat([st[:, None, :], at.view(B, S, We)], 1).reshape(B * (S + 1), We).contiguous()
        return hip.cast_f32_to_bf16(tok), ((xt2, cat, h1, s1, st2) if save else None)

    def _embed_suffix_pi0_bwd(self, sctx, dx1, B, S):
        xt2, cat, h1, s1, st2 = sctx
        We = self.e.width
        d = hip.cast_bf16_to_f32(dx1).view(B, S + 1, We)
        self._lin32_bwd(st2, d[:, 0].contiguous(), "act/state_w", "act/state_b", need_dx=False)
        ds1 = self._lin32_bwd(s1, d[:, 1:].reshape(B * S, We).contiguous(), "act/atime_out_w", "act/atime_out_b")
        dh1 = hip.swish_bwd(h1, ds1)
        dcat = self._lin32_bwd(cat, dh1, "act/atime_in_w", "act/atime_in_b")
        self._lin32_bwd(xt2, dcat[:, :We].contiguous(), "act/in_w", "act/in_b", need_dx=False)      # (the time half has no parameters behind it)

    def _embed_suffix(self, x_t: torch.Tensor, time: torch.Tensor, save: bool, overlap: bool = False):
        """overlap (train step): the dozen small kernels go to the second HIP stream and run under whatever the current stream was
        given before (the SigLIP tower); their results are next touched by `joint_layers.llm_fwd`, which joins the streams."""
        sfx = suffix_stream(self, x_t, time) if overlap else None
        self.comm.wait_unit("ada", also=sfx)
        with (torch.cuda.stream(sfx) if sfx is not None else contextlib.nullcontext()):
            x1, xt2 = self._embed_actions(x_t)
            mod, tctx = self._time_mod(time, save)
        if sfx is not None:
            mod.record_stream(torch.cuda.current_stream()); x1.record_stream(torch.cuda.current_stream())
        return x1, mod, ((xt2, *tctx) if save else None)

    def _embed_suffix_bwd(self, sctx, dx1, dmod):
        """On the second HIP stream when there is one: it runs under the SigLIP backward that the caller issues next.  The
        caller joins the streams before it declares the "small" unit's gradients complete."""
        xt2, temb, h1, s1, h2, cond16 = sctx
        sfx = suffix_stream(self, dx1, dmod)
        with (torch.cuda.stream(sfx) if sfx is not None else contextlib.nullcontext()):
            dmod16 = hip.cast_f32_to_bf16(dmod)
            hip.colsum(dmod, self.G("ada/b"))
            self._wgrad(dmod16, cond16, "ada/w")
            dcond = hip.cast_bf16_to_f32(hip.linear_dgrad(dmod16, self.W("ada/w")))
            self.comm.grads_ready("ada")       # (its side stream starts behind the CURRENT stream: the one these gradients are on)
            dh2 = hip.swish_bwd(h2, dcond)
            ds1 = self._lin32_bwd(s1, dh2, "act/time_out_w", "act/time_out_b")
            dh1 = hip.swish_bwd(h1, ds1)
            self._lin32_bwd(temb, dh1, "act/time_in_w", "act/time_in_b", need_dx=False)
            self._lin32_bwd(xt2, hip.cast_bf16_to_f32(dx1), "act/in_w", "act/in_b", need_dx=False)
        return sfx

    # ================================================================== training forward (+ backward)
    def _loss_impl(self, rng, observation: CoTObservation, actions: torch.Tensor, *, train: bool, noise=None, time=None,
                   backward: bool, collect: dict | None = None, verbose: bool = False, denominators=None):
        cfg = self.config
        # lap.py:426-462,557-596: three branches — both losses (LAP-3B); enable_action_training=False: `llm([prefix])` and the
        # cross entropy only (VLA-0 style configs); enable_langact_training=False: both streams, flow matching only (pi0 style)
        act_on, lang_on = cfg.enable_action_training, cfg.enable_langact_training
        if not (act_on or lang_on):
            raise ValueError("LAPConfig with neither enable_action_training nor enable_langact_training has no loss")
        dev = self.device
        self.comm.wait_unit("small")
        g = _gen(rng, dev)
        obs = preprocess_observation(observation, train=train, image_keys=cfg.image_keys, image_resolution=cfg.image_resolution,
                                     enable_image_augmentation=cfg.enable_image_augmentation, rng=g)
        actions = actions.to(dev, torch.float32).contiguous()
        B, S, ad = actions.shape
        if S != self.action_horizon:
            raise ValueError(f"actions horizon {S} != action_horizon {self.action_horizon}")
        x1 = mod = sctx = u_t = None
        if act_on:
            # lap.py:185-207 prepare_suffix — noise ~ N(0,1), time ~ Beta(1.5, 1) * 0.999 + 0.001
            if noise is None:
                noise = torch.randn(actions.shape, generator=g, device=dev, dtype=torch.float32)
            if time is None:
                u1 = torch.rand(B, generator=g, device=dev, dtype=torch.float32)
                time = u1.pow(1.0 / 1.5) * 0.999 + 0.001  # Beta(a, 1) by inverse CDF
            noise = noise.to(dev, torch.float32).contiguous(); time = time.to(dev, torch.float32).contiguous()
            x_t, u_t = hip.fm_mix(noise, actions, time)
            if cfg.pi05:
                # suffix first: its small kernels go to the second HIP stream and run under the SigLIP tower issued next
                x1, mod, sctx = self._embed_suffix(x_t, time, backward, overlap=True)
            else:
                if obs.state is None:
                    raise ValueError("pi05=False feeds the continuous state through state_proj: the observation has no `state`")
                x1, sctx = self._embed_suffix_pi0(x_t, time, obs.state, backward)
        # suffix rows in the joint sequence: none without the action expert (lap.py:449-455); pi0 has its state token in front
        Sx = (S + (0 if cfg.pi05 else 1)) if act_on else 0
        x0, Pn, pctx = self._embed_prefix(obs, backward, collect)
        qinfo, kinfo, pos = self._train_infos(obs, S if act_on else 0)
        if collect is not None:
            collect["x0_in"], collect["x1_in"], collect["pos"], collect["mod"] = x0, x1, pos, mod
        # the language head's rows are chosen here, once: the last layer's prefix stream may run on them alone
        lrows = select_loss_rows(self, obs, observation, verbose=verbose) if lang_on else None
        last_rows = last_layer_rows(self, lrows, qinfo, B, Pn, obs.tokenized_prompt.shape[1], save=backward, x1=x1, collect=collect,
                                    verbose=verbose)
        xf0, xf1, lctx = llm_fwd(self, x0, x1, mod, pos, qinfo, kinfo, B, Pn, Sx, backward, collect=collect, last_rows=last_rows)
        if collect is not None:
            collect["x0_out"], collect["x1_out"] = xf0, xf1

        fb = lambda t: t.to(torch.float32)
        sm = obs.sample_mask if obs.sample_mask is not None else torch.ones(B, dtype=torch.bool, device=dev)
        head = lang_head_fwd(self, xf0, obs, lrows, B, Pn, backward=backward, verbose=verbose, collect=collect,
                             compact=last_rows is not None) if lang_on else LangHead(torch.zeros(B, dtype=torch.float32, device=dev))
        ah = action_head_fwd(self, xf1, mod, B, S, Sx, backward=backward) if act_on else ActionHead()
        lang_loss, v_t = head.lang_loss, ah.v_t
        # the reference's vqa_mask / pred_mask (lap.py:400-409): only where that kind of training is on
        wl, act_mask, mixing, extra_metrics = mix_sample_weights(
            cfg, lang_loss, sm, obs.is_vqa_sample if cfg.enable_vqa_training else None,
            obs.is_prediction_sample if cfg.enable_prediction_training else None, obs.vqa_dataset_id, lang_on=lang_on)
        # `denominators` (gradient accumulation, loss.global_denominators): the counts of the WHOLE batch of the optimizer step in place
        # of this micro-batch's, so that the micro-steps' losses and gradients sum to the big batch's
        if denominators is not None:
            n_active = denominators[0].to(dev, torch.float32).view(1)
        else:
            n_active = torch.clamp(self.comm.all_reduce_sum(fb(sm).sum().view(1)), min=1.0) if obs.sample_mask is not None else \
                self.comm.all_reduce_sum(torch.tensor([float(B)], device=dev))
        # lang_term: sum / active samples, or the batch mean without a sample mask (lap.py:579-596; the action-off branch's
        # `final_loss` is the same expression)
        lang_term = (wl * lang_loss).sum() / n_active
        act_loss = torch.zeros(B, dtype=torch.float32, device=dev)
        action_term = 0.0
        dv = None
        if act_on:
            if denominators is not None:
                n_action = denominators[1].to(dev, torch.float32).view(1)
            else:
                n_action = torch.clamp(self.comm.all_reduce_sum(fb(act_mask).sum().view(1)), min=1.0)
            coef = cfg.action_loss_weight * fb(act_mask) / n_action
            act_loss, dv = hip.mse_fwd_bwd(v_t.view(B, S * ad), u_t.view(B, S * ad), coef, need_grad=backward)
            action_term = (cfg.action_loss_weight * act_loss * fb(act_mask)).sum() / n_action
        loss = self.comm.all_reduce_sum((lang_term + action_term).view(1)).view(())
        metrics = {"lang_loss": lang_loss.mean(), "action_loss": (act_loss * fb(act_mask)).sum() / torch.clamp(fb(act_mask).sum(), min=1.0),
                   "langact_loss": (lang_loss * fb(sm)).sum() / torch.clamp(fb(sm).sum(), min=1.0) if not mixing else extra_metrics["langact_loss"],
                   **{k: v for k, v in extra_metrics.items() if k != "langact_loss"}, **head.verbose_metrics}
        if verbose:     # lap.py:569-577: weighted language term plus the weighted, masked action term of each sample
            metrics["per_sample_loss"] = wl * lang_loss + (cfg.action_loss_weight * act_loss * fb(act_mask) if act_on else 0.0)
        if collect is not None:
            collect.update(pl=head.pl, pre1=ah.pre1, v_t=v_t.view(B, S, ad) if v_t is not None else None, u_t=u_t, per_sample_lang=lang_loss,
                           per_sample_action=act_loss)
        if not backward:
            return loss, metrics

        # =============================== backward ===============================
        self.comm.before_backward()
        self.wg.begin(self.wgrad_stream)
        dx1, dmod = action_head_bwd(self, ah, xf1, mod, dv, B, S, Sx) if act_on else (None, None)
        skip_prefix = self._prefix_frozen()
        dx0 = None
        if not skip_prefix and lang_on:
            dx0 = lang_head_bwd(self, head, wl, n_active, B, Pn)
        elif not skip_prefix:
            # no language loss: the prefix stream's only cotangents are those of its keys / values under the action queries
            dx0 = torch.zeros((B * Pn, self.v.width), dtype=torch.bfloat16, device=dev)
            # the LM-head weight-gradient product is what overwrites (beta = 0) the embedding table's f32 gradient buffer; without it the
            # scatter-add of _embed_prefix_bwd would accumulate onto the previous step's values
            if self.ps.is_trainable("llm/embed"):
                self.G("llm/embed").zero_()
        dx0, dx1 = llm_bwd(self, lctx, dx0, dx1, mod, dmod, pos, qinfo, kinfo, B, Pn, Sx, last_rows=last_rows)
        sfx = None
        if act_on and cfg.pi05:
            sfx = self._embed_suffix_bwd(sctx, dx1, dmod)
        elif act_on:
            self._embed_suffix_pi0_bwd(sctx, dx1, B, S)
        elif "ada" in self.ps.unit_by_name:   # the action expert's units saw no gradient (zeros): still declared complete for the optimizer's pipeline
            self.comm.grads_ready("ada")
        if not skip_prefix:
            self._embed_prefix_bwd(pctx, dx0, B, Pn)
        handoff(sfx, torch.cuda.current_stream() if sfx is not None else None)
        self.wg.end()
        self.comm.grads_ready("small")
        return loss, metrics

    def compute_loss(self, rng, observation, actions, *, train: bool = False, stage_config=None, verbose_mode=None,
                     return_augmented_images: bool = False, noise=None, time=None, collect=None, denominators=None):
        """lap.py:380-602.  rng: int seed or torch.Generator.  `noise` / `time` may be given explicitly (parity tests).
        verbose_mode (None: the config's, lap.py:393-394) adds the token-accuracy metrics and `per_sample_loss` (loss._token_metrics).
        `denominators`: see `loss_and_grad`."""
        verbose = bool(self.config.verbose_mode if verbose_mode is None else verbose_mode)
        return self._loss_impl(rng, observation, actions, train=train, noise=noise, time=time, backward=False, collect=collect,
                               verbose=verbose, denominators=denominators)

    def loss_and_grad(self, rng, observation, actions, *, train: bool = True, noise=None, time=None, collect=None, denominators=None):
        """Forward + backward; gradients land in self.ps.grad (engine layout; bf16 for the GEMM-weight units, f32 for the embedding table and
        the small unit: ParamStore.grad_dtype).  The caller zeroes the accumulated (f32) units first.  Verbose metrics follow the
        config's `verbose_mode` (the reference's train step runs with the class attribute, scripts/train.py:351).
        `denominators=(n_active, n_action)`: f32 device scalars (n_action None where the action loss is off) that replace the two
        counts the loss divides by — taken from this batch's masks and all-reduced when absent — in the loss and in both cotangents
        (gradient accumulation: `loss.global_denominators` over the micro-batches of one optimizer step)."""
        return self._loss_impl(rng, observation, actions, train=train, noise=noise, time=time, backward=True, collect=collect,
                               verbose=bool(self.config.verbose_mode), denominators=denominators)

    # ================================================================== serving
    @torch.no_grad()
    def sample_actions(self, rng, observation, *, num_steps: int = 10, noise=None, collect=None, fused=True, inpaint=None,
                       num_samples=None, select=None, coherence=None, share_prefix=True, **internal):
        """lap.py:605-675: prefix prefill once -> per-layer K/V kept in HBM -> `num_steps` Euler steps of the action
        expert attending to [cached prefix | fresh suffix] as two key segments (the reference concatenates, gemma.py:228-230).
        `fused`: True = the fastest denoise-step kernels the shapes allow ("skinny" fused projections for the LAP-3B action
        expert, else "partials" = split-K partial slabs + fused consumers); False = the generic layer path (A/B tests).
        `inpaint` (NOT in the reference, whose sampler has no such option): None, or `(known, mask)` for real-time chunking by
        inpainting — `known` f32 [B, S, action_dim] in MODEL space (normalised, padded to action_dim) and `mask` [B, S] of 0 / 1, one
        flag per action row, 1 = frozen.  With t = 1 noise, t = 0 data, a frozen row is set after Euler step k of n to
        t' noise + (1 - t') known, t' = (n - 1 - k) / n (float64 on the host, passed as two f32; evaluated as two rounded products and
        a rounded sum), so it stays on the known trajectory while the free rows, which update as always, attend to it; the last
        step has t' = 0 and a frozen row of the result is `known` bit for bit.  Frozen rows stay in the sequence as action tokens: no
        attention kernel changes.  `collect` still records the model's v_t for every row.  Wrong shapes, a batch mismatch, non-finite
        `known` or mask values other than 0 / 1 raise ValueError.  `lap_amd.chunking.shift_chunk` builds the pair from the previous
        chunk; that is meaningful only when the action representation does not depend on the new observation's frame.
        `num_samples=N` (1 .. 8; NOT in the reference either): N candidate chunks of ONE observation (batch 1, pi05) from ONE prefill —
        `noise` is [N, S, action_dim], drawn from `rng` when absent, `inpaint=(known [1, S, ad], mask [1, S])` applies to every
        candidate; the steps run on N * S rows and, on the skinny route, the attention reads the single prefix cache
        (`share_prefix=False`, and the other routes, replicate it: same bits); the one-launch chain is not used.  Returns [N, S, ad].
        `select="medoid"` or `select="coherence"` with `coherence=(known [S, ad], weights [S])` picks one candidate on the device
        (`lap_amd/action_select.py` is the specification) and returns it as [1, S, ad]; `collect` then also receives `candidates`,
        `scores` and `index`.  `num_samples` absent or 1 is the plain call.  ValueError: N outside 1 .. 8, N > 1 with a batch or with
        pi0, `select` without candidates or without its arguments, wrong shapes."""
        with self._serving_weights():
            kw = {} if inpaint is None else {"inpaint": inpaint}
            if num_samples is not None or select is not None or coherence is not None:
                kw |= dict(num_samples=num_samples, select=select, coherence=coherence, share_prefix=share_prefix, **internal)
            return self._sample_actions(rng, observation, num_steps=num_steps, noise=noise, collect=collect, fused=fused, **kw)

    def _sample_actions(self, rng, observation, **kw):      # on the weights as they are (outside `_serving_weights`: base + adapters)
        from lap_amd import flow_sample     # (it imports this module)
        return flow_sample.sample_actions(self, rng, observation, **kw)

    def serve_chain_failed(self) -> bool:
        """True if a launch of the one-launch denoise step gave up at a grid barrier since the last check (synchronises)."""
        return self._chain_ctr is not None and hip.serve_chain_failed(self._chain_ctr)

    def disable_serve_chain(self):
        """After a launch that gave up at a barrier: one step back — the tensor-parallel chain (which needs 32 blocks on each of 8
        XCDs) falls back to the flat chain, the flat chain to the separate launches."""
        if self.serve_chain and self.serve_packed and self.serve_tp:
            self.serve_tp = False
        else:
            self.serve_chain = False
        if self._chain_ctr is not None:
            torch.cuda.synchronize(self.device)
            self._chain_ctr.zero_()

    def _dec_fp8(self, name):
        """(e4m3 codes [N, K], f32 row scales [N]) of a weight of the fused decoder in the format of lap_amd/fp8.py: persistent
        like `flow_sample.serve_packed_weights`, built on first use and re-quantised IN PLACE per parameter version (a captured decoder
        holds both addresses).  The layer projections are quantised from the bf16 weight `W(name)` the bf16 decoder reads (the
        merged one under `_serving_weights`), the LM head from the f32 embedding table.  +1 byte per weight on top of the bf16
        copies the prefill keeps: 2.0 GB for LAP-3B's 18 layers, 0.53 GB for the table."""
        def build(old):
            self.comm.wait_unit("embed" if name == "llm/embed" else "llm" + name.split("/")[1])
            return hip.quantize_fp8_rows(self.F(name) if name == "llm/embed" else self.W(name), *(old or ()))
        return self.serving_cache.get(("dec8", name), None, build)

    def refresh_serve_caches(self, num_steps=None):
        """Bring every parameter-derived serving tensor there is (`lap_amd/serve_cache.py`: merged LoRA weights, the fused decoder's
        fp8 weights, packed weight images, adaRMS modulations) up to the current parameter version, in place.  The eager paths do
        this on use; a captured graph cannot — call it before a replay.  `num_steps` is accepted and ignored: what a sampler
        needs exists since its warm-up."""
        with self._serving_weights():
            self.serving_cache.refresh()

    def sample_tokens(self, rng, observation, *, max_decoding_steps: int = 390, temperature: float = 0.0, collect=None,
                      decode: str = "eager", sampler: str = "host", decode_weights: str = "bf16", allowed_tokens=None,
                      return_logprobs: bool = False, num_samples=None, top_k=None, top_p=None, speculate=None, draft_tokens=None,
                      grammar=None, jump_forward=None, num_beams=None, early_stop: bool = True):
        """lap.py:678-766 (LAP_AR serving mode): VLM-only prefill, then single-token decode until every sample has emitted
        EOS or `max_decoding_steps` tokens; returns int32 [B, max_decoding_steps] (zeros after the stop).

        The reference right-aligns the prefix (`left_to_right_align`) so that a fixed-size cache can be addressed by
        `prefix_start`; rolling changes neither the attention pattern nor `cumsum(mask) - 1` positions of valid tokens,
        so the engine keeps the tokens in place and expresses the decode mask `[prefix_start, prefill_size + step]` in
        un-rolled coordinates: prefix keys `seqlen - prefill_len <= j < seqlen` (seqlen = last valid index + 1) plus every
        generated key.  Known deviation: with a hole inside the prefix (a masked-out image followed by valid tokens) the
        reference's range mask covers the hole's tokens, whose prefill activations above layer 0 are softmax outputs of
        fully masked rows (uniform averages, "never consumed" elsewhere); the engine's attention writes zeros for such
        rows, so decode logits differ from the reference in that case only (prefill logits still agree; tested).
        temperature > 0 samples with the Gumbel-max trick from a torch generator seeded by `rng` (the JAX PRNG stream of
        `jax.random.categorical` cannot be reproduced).

        decode: "eager" (default) runs each decode step as generic launches; "fused" runs it on the single-token kernels of
        csrc/decode.hip (Gemma-2B widths, 1 <= B <= 8, one replica; anything else raises ValueError) with a fixed-capacity
        generated K/V cache and the step / EOS / stop state on the device, checked by the host once per 8 steps.
        The two paths differ in the summation order of their dot products only.

        sampler: where the noise of a temperature > 0 draw comes from.  "host" (default) is the torch-generator Gumbel stream
        above; it cannot run inside a captured graph, so `decode="fused"` with temperature > 0 keeps the eager loop.
        "device" draws token t of row b as the argmax of logit * float32(1 / temperature) + g, g the counter-based Gumbel noise
        of (seed = `rng` as a 64-bit integer, t, b, vocabulary index) that lap_amd/sampling.py defines and restates on the host:
        `decode="eager"` applies it to its stored logits in one pass (lap_gumbel_argmax_rows_f32), `decode="fused"` as the
        epilogue of the fused LM head (lap_decode_lm_head_sample), where no logit is stored.  The two decode modes then draw
        from the same noise and differ in summation order only, and `sampling.sample_from_logits(collect["logit/<t>"],
        temperature, rng, t)` reproduces a draw offline.  temperature <= 0 is greedy under either sampler, bit for bit the same.
        `collect` keeps the raw logits under sampler="device" (under "host" it holds what the argmax saw, as before).

        decode_weights: what the fused decode steps stream.  "bf16" (default): the bf16 weights, as before.  "fp8": e4m3 codes
        with one power-of-two scale per output feature (lap_amd/fp8.py) for the four projections of every layer and for the LM
        head, half and a quarter of the bytes; "fp8_layers": the projections only, the LM head stays on the hi / lo bf16 planes
        of the f32 table (its precision decides greedy near-ties).  The kernels compute what the bf16 ones compute on the
        dequantised weights; the prefill and the embedding gather are unchanged.  The fp8 copies are cached on the model and
        follow the parameters (`refresh_serve_caches`).  Needs decode="fused".

        allowed_tokens: constrained decoding.  None (default): the whole vocabulary, as before.  Any integer sequence or tensor
        of token ids, one set for all rows (duplicates and order do not matter; it must hold the EOS token, ids outside the
        vocabulary and an empty set raise ValueError): every token is the argmax over the set of the score the unconstrained
        decode gives that vocabulary index, lowest index among ties, i.e. what the unconstrained rule picks on logits set to
        -inf outside the set; under sampler="device" the noise of index j stays that of j.  decode="fused" streams only the
        set's rows of the LM head (lap_decode_lm_head_subset*), with logits equal to the unconstrained kernel's bit for bit;
        decode="eager" masks its stored logits.  `collect["logit/<t>"]` is full width with -inf outside the set.
        `policy_io.allowed_token_ids` builds a set from example language actions.

        return_logprobs: False (default): the tokens alone, on the launches of before.  True: (tokens, logprobs), logprobs f32
        [B, max_decoding_steps] beside the tokens (column 0, the token of the prefill's logits, included; zeros where nothing
        was written): the log-probability of each token under the noise-free softmax of z = float32(logit * inv_t) (tau = 1 for
        a greedy decode) over the vocabulary, or over the allowed set.  decode="eager" takes a float32 log_softmax of its stored
        logits; decode="fused" folds the log-sum-exp into the LM-head pass (lap_decode_lm_head_lp / lap_decode_finish_lp: no
        logit is stored, no launch is added).  `sampling.token_logprobs` restates it, `sampling.sequence_logprob` sums a row up
        to its EOS.  The reference has no such output.

        num_samples: best-of-N.  None (default): one decode per observation row.  1 <= N <= 8 (observation of batch 1,
        decode="fused", sampler="device", temperature > 0; anything else raises ValueError): the prefix is prefilled once, its
        K / V, key-info words and last row are copied to N rows, and the N rows decode as one fused batch under `rng`, row b
        drawing with Philox row index b as any batch row does.  Returns (tokens [N, steps], logprobs [N, steps]);
        `sampling.select_best` picks the answer.

        top_k, top_p: top-k and nucleus filtering of a sampled draw (sampler="device"; with sampler="host" and temperature > 0
        they raise ValueError; None, the default, is the neutral value of either and leaves every request as it was).  top_k: an
        integer >= 0, the draw runs over the k candidates of largest z = float32(logit * inv_t) (ties at the cut go to the lower
        indices; 0 or k >= the number of candidates keeps all).  top_p in (0, 1]: of what top_k kept, in that order, the entries
        whose preceding cumulative softmax mass is below top_p times the kept mass (the first always).  The candidates are the
        allowed set of a constrained decode.  The token is the argmax of the unfiltered sampler's score over the kept entries, so
        `sampling.sample_from_logits(collect["logit/<t>"], temperature, rng, t, top_k, top_p)` reproduces it and
        `sampling.filter_keep` gives the kept set.  A greedy decode ignores both.  decode="eager" draws with
        lap_filter_gumbel_argmax_rows_f32; decode="fused" lets the plain LM head store its f32 logits and draws with
        lap_decode_filter_finish (one more launch per token than the unfiltered fused step).  `return_logprobs` and best-of-N keep
        their meaning: a log-probability is the log-softmax over ALL candidates at tau = inv_t, the model's probability of the
        token, not its probability inside the kept set; `select_best` ranks by it.  The reference has no such option.

        speculate, draft_tokens: exact greedy speculative decoding.  None (default): one token per pass over the weights, as
        before.  speculate=S, 2 <= S <= 8 (observation of batch 1, decode="fused", greedy; temperature > 0, return_logprobs,
        num_samples, top_k / top_p and collect raise ValueError): every fused step verifies S consecutive positions of the sequence
        at once, row 0 the real next position and rows 1 .. S-1 the tokens drafted from `draft_tokens`, an integer sequence that is
        expected to resemble the answer (in a control loop: the previous request's answer; None drafts nothing).  The draft is
        the continuation of the reference after the nearest match of the last two generated tokens (`speculate.draft_tokens`);
        the step emits the first row's token and every following row's while the drafts before it were right
        (`speculate.accept`).  Every row of the fused kernels is accumulated independently of the batch width, so the returned
        tokens are those of the call without `speculate`, whatever the draft; only the number of passes over the weights changes
        (`last_spec_stats` = (verify steps, drafts accepted) of the request).  Composes with decode_weights and allowed_tokens.
        The reference has no such option.

        grammar: grammar-constrained decoding.  None (default): as before.  A `grammar.TokenAutomaton` (or its `to_device` form),
        a deterministic automaton over token ids built for this model's vocabulary and EOS token
        (`policy_io.grammar_automaton` builds one from a language-action format and the tokenizer): every row starts in state 0,
        token t of row b is drawn among the ids its state allows, by the rule of `allowed_tokens` on that state's set (the
        argmax of the unconstrained score, lowest index among ties; under sampler="device" the noise of index j stays that of j),
        and the row moves along the edge of its token, so an answer that ends before its budget is a sentence of the format.  After
        its EOS a row stays in a sink state and keeps emitting EOS.  decode="fused" keeps the state of every row on the device:
        the SUBSET LM head streams the union of all edges and stores its f32 logits, lap_decode_grammar_finish draws from the
        state's segment and moves the state (rows of a best-of-N batch diverge); decode="eager" masks its stored logits per row and
        steps with a `torch.searchsorted`.  `grammar.decode_reference` restates the draw on `collect`ed logits.  With
        return_logprobs / num_samples a log-probability is the one over the state's set.  Composes with temperature > 0 under
        sampler="device", return_logprobs, num_samples and decode_weights; allowed_tokens, top_k / top_p, speculate and the host
        sampler at temperature > 0 raise ValueError, as does an automaton built for another vocabulary size or EOS token.  The
        reference has no such option.

        jump_forward: jump-forward grammar decoding.  None (default): a grammar decode emits one token per pass over the weights,
        as before.  jump_forward=S, 2 <= S <= 8 (needs grammar=, decode="fused", an observation of batch 1, num_samples None,
        collect None, and sampler="device" when temperature > 0; anything else raises ValueError): the constrained decode runs on
        steps of S rows, as `speculate` does.  Whenever the automaton state has a single edge the next token is known before the
        model runs, at any temperature, so it is drafted, and a run of such tokens rides along one pass; in the other states
        `draft_tokens` (optional, as under `speculate`) may draft (`speculate.grammar_drafts`).  Row r draws with the noise of step
        t + r from the state the rows before it led to (lap_decode_grammar_spec_finish: the single-row finish's bits, row after
        row), so tokens and log-probabilities are those of the call without `jump_forward`, sampled or greedy, whatever the draft;
        `last_spec_stats` = (steps, drafts accepted).  Composes with return_logprobs, decode_weights and temperature > 0.  The
        reference has no such option.

        num_beams: beam search.  None (default): everything above, unchanged.  num_beams=N, 1 <= N <= 8 (an observation of batch 1,
        temperature 0, decode "fused" or "eager"; sampler="device", num_samples, top_k / top_p, speculate, jump_forward
        and collect raise ValueError from `beam.check_num_beams`): the deterministic search for the most probable answer.  The
        prefix is prefilled once and shared by N rows that advance in lockstep; at every step each alive beam offers its N most
        probable tokens, and the N candidates with the largest sum of token log-probabilities become the beams, in rank order
        (lap_amd/beam.py states the rules; csrc/decode_beam.hip runs them on the fused route, `decode="eager"` is a second
        implementation on the host).  early_stop (default True): the search ends when the rank-0 beam has finished, which no alive
        beam can pass under the sum score; False: it runs until every beam has finished or the budget is spent.  Returns the
        rank-0 beam as int32 [1, max_decoding_steps] (with return_logprobs also its token log-probabilities);
        `ar_decode.beam_decode_fused` / `beam_decode_eager` return all beams.  num_beams=1 is the greedy decode.  Composes with
        allowed_tokens, decode_weights and return_logprobs, and with `grammar` (not with allowed_tokens): every beam is then in a state
        of the automaton and offers its N most probable edges, with log-probabilities over that state's set, so the answer is the most
        probable sentence of the format among the beams kept (`beam.grammar_beam_step`; lap_decode_beam_grammar_topn / _select).  The
        reference has no such option."""
        from lap_amd import ar_decode       # (it imports this module)
        return ar_decode.sample_tokens(self, rng, observation, max_decoding_steps=max_decoding_steps, temperature=temperature,
                                       collect=collect, decode=decode, sampler=sampler, decode_weights=decode_weights,
                                       allowed_tokens=allowed_tokens, return_logprobs=return_logprobs, num_samples=num_samples,
                                       top_k=top_k, top_p=top_p, speculate=speculate, draft_tokens=draft_tokens, grammar=grammar,
                                       jump_forward=jump_forward, num_beams=num_beams, early_stop=early_stop)

    def score_tokens(self, observation, tokens, *, rows: int = 8, temperature: float = 0.0, decode_weights: str = "bf16",
                     allowed_tokens=None, max_decoding_steps: int = 390):
        """Teacher-forced scoring: the log-probability of GIVEN answers under the serving kernels, instead of a decode.

        tokens: one integer sequence, or a list of N sequences, each with 1 <= length <= max_decoding_steps (they need not end
        with the EOS token; every given token is scored).  The observation (batch 1) is prefilled once and every candidate is
        scored against that prefix.  Returns `ar_decode.ScoreResult(logp, total, greedy)`: per candidate the f32 log-probability
        of every token, logp[i] = z[tokens[i]] - logsumexp(z) over the logits that follow tokens[:i], their sum in `total` (f32
        [N]), and the argmax id at every position (`greedy[i] == tokens[i]` is the token accuracy of the answer as served).
        temperature 0: z = logit, the convention of `sample_tokens(return_logprobs=True)` on a greedy decode, whose numbers this
        reproduces bit for bit for its own answer; otherwise z = float32(logit * float32(1 / temperature)).  allowed_tokens: the
        softmax and the argmax run over that set, as in a constrained decode; a token outside it scores -inf.  decode_weights as
        in `sample_tokens`, so the same answer can be scored under "bf16", "fp8_layers" and "fp8".
        rows = S, 1 <= S <= 8: a step scores S consecutive positions on one pass over the weights (the verify step of
        `speculate=S` with a draft that is always right: csrc/decode_score.hip, the TARGET LM heads of csrc/decode.hip), so L tokens
        cost 1 + ceil((L - 1) / S) passes; the numbers do not depend on S.  The steps are launched eagerly (no graph capture).
        lap_amd/score.py states the quantity and the argument checks (ValueError).  The reference has no such entry point."""
        from lap_amd import ar_decode       # (it imports this module)
        return ar_decode.score_tokens(self, observation, tokens, rows=rows, temperature=temperature, decode_weights=decode_weights,
                                      allowed_tokens=allowed_tokens, max_decoding_steps=max_decoding_steps)

    DECODE_WEIGHTS = ("bf16", "fp8", "fp8_layers")
    last_spec_stats = None      # (verify steps, drafts accepted) of the last `sample_tokens(speculate=S)` or `(jump_forward=S)` request

    def decode_supported(self, B: int) -> bool:
        """Whether `sample_tokens(decode="fused")` / `GraphedTokenDecoder` serve `B` rows of this model."""
        v = self.v
        return self.comm.world_size == 1 and hip.decode_ok(B, v.width, v.num_heads, v.num_kv_heads, v.head_dim, v.mlp_dim,
                                                            self.config.vocab_size)
