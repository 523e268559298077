"""LAP on MI355X: the model object behind `LAPConfig.create()` / `.load()`.

Keeps the reference's model surface (src/lap/models/lap.py):
    compute_loss(rng, observation, actions, *, train=False, ...) -> (loss, metrics)      lap.py:380-602
    sample_actions(rng, observation, *, num_steps=10, noise=None) -> [b, ah, ad]         lap.py:605-675
and adds `loss_and_grad(...)`, the fused forward + hand-written backward that the train step uses (the
reference gets it from nnx.value_and_grad, scripts/train.py:358-361).  `_loss_impl` is the schedule of that step (streams, collectives,
the order of the passes); the language head, the action head and the sample-weight mixing it calls are in lap_amd/loss.py.  The serving
paths are modules of functions on the model: the action sampler in flow_sample.py, token decoding in ar_decode.py, their prefill in prefill.py.

Everything numeric is a call into liblap_hip.so (lap_amd/hip.py); torch only owns device memory, the stream,
and a few O(batch x tokens) integer tensors (masks -> per-token info words, positions).  There is no autograd
and no fallback path.  Activations needed by the backward are kept in HBM (288 GB per MI355X) instead of being
recomputed — the reference rematerialises every block (gemma.py:418-423 nothing_saveable), which costs a
fourth forward pass.

Joint two-expert transformer (gemma.py:455-531): the prefix stream (SigLIP tokens + prompt, width of the VLM)
and the suffix stream (action tokens, width of the action expert) keep separate activations and weights and
meet only inside the attention kernel, which takes both as segments.  In the train step the suffix stream's kernels (1,600 rows:
poorly filled grids, launch-latency bound) are issued on a second HIP stream and run under the prefix stream's GEMMs; the two
streams synchronise before and after each layer's attention (`LAP_DUAL_STREAM=0`: everything on one stream).
"""
from __future__ import annotations

import contextlib
import dataclasses
import math
import os

import torch

from lap_amd import hip
from lap_amd.config import LAPConfig, get_gemma_config, get_siglip_config
from lap_amd.loss import (ActionHead, LangHead, action_head_bwd, action_head_fwd, lang_head_bwd, lang_head_fwd, mix_sample_weights,
                          select_loss_rows)
from lap_amd.observation import CoTObservation, preprocess_observation
from lap_amd.params import LORA_PROJ, ParamStore, lora_geometry
from lap_amd.serve_cache import ServeCache

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


class LastRows:
    """The prefix rows the LAST joint layer keeps in a train step (`LAP._last_layer_rows`): those the language head reads."""

    def __init__(self, sel, qinfo, B, n0, Lt):
        dev, n_sel = sel.device, sel.shape[1]
        self.n_sel = n_sel
        idx = sel + (n0 - Lt)                                                       # [B, n_sel] prefix positions, the head's order
        self.rowid = (torch.arange(B, device=dev)[:, None] * n0 + idx).to(torch.int32).reshape(-1).contiguous()   # rows of x0
        self.inv = torch.full((B * n0,), -1, dtype=torch.int32, device=dev)         # row of x0 -> its compact row, or -1
        self.inv[self.rowid.long()] = torch.arange(B * n_sel, dtype=torch.int32, device=dev)
        # info words of the kept queries, then the suffix queries': class bits and ar index travel with the row, so every kept
        # row meets the keys under the mask it had
        self.qinfo = torch.cat([qinfo[:, :n0].gather(1, idx), qinfo[:, n0:]], 1).to(torch.int32).contiguous()


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
        # language head reads (`_last_layer_rows`).  LAP_LAST_LAYER_ROWS=0: all rows, as every other layer (A/B runs, tests)
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
        self._sfx = None        # the suffix stream's HIP stream (created on first use)
        # which gradients leave the data-gradient path for a third stream (see _off_path): s SigLIP weights, b biases, q / g the
        # prefix stream's attention / MLP projections; "1" all, "0" none.  Measured (tools/ab3.sh, interleaved on one box): sb
        # -2.1 .. -3.3 ms per step in round 2 and -2.6 ms in round 3 (310.0 -> 307.4), s -1.3, q 0, all +12.6.  Default "sb":
        # step time is the decision variable (the compute stream's GEMMs then share the chip, so their EVENT-timed rate drops
        # by 4 % — bench.py's roofline figure is computed from isolated per-shape times for that reason).
        mode = os.environ.get("LAP_WGRAD_STREAM", "sb")
        self.wgrad_stream = "" if mode == "0" else mode
        self._wg = self._wg_obj = self._wg_main = None
        self._wg_dirty = False
        self._wg_ev: dict = {}
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
    def _suffix_stream(self, *tensors):
        """The second HIP stream for the suffix (action-expert) side of a joint layer loop, or None when both streams of
        activations go down the current one (one of them absent, CPU tensors, stream capture, LAP_DUAL_STREAM=0).  It starts
        behind everything the current stream has been given so far; `tensors` are marked as used on it."""
        if not self.dual_stream or any(t is None or not t.is_cuda for t in tensors) or torch.cuda.is_current_stream_capturing():
            return None
        if self._sfx is None:
            self._sfx = torch.cuda.Stream(self.device, priority=-1)   # short kernels: never let them queue behind a full grid
        self._sfx.wait_stream(torch.cuda.current_stream())
        for t in tensors:
            t.record_stream(self._sfx)
        return self._sfx

    @staticmethod
    def _handoff(src, dst, *tensors):
        """`dst` waits for what `src` has been given so far; `tensors` (allocated on src) are about to be used on dst."""
        if src is not None and dst is not None:
            dst.wait_stream(src)
            for t in tensors:
                if t is not None:
                    t.record_stream(dst)

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
                with self._off_path(dy, x):
                    run()
            else:
                run()

    def _bgrad(self, dy, name):
        """Bias gradient = column sums of dy, next to the weight gradient."""
        mode = self.wgrad_stream
        if mode == "1" or "b" in mode:
            with self._off_path(dy):
                hip.colsum(dy, self.G(name))
        else:
            hip.colsum(dy, self.G(name))

    # Nothing in the backward waits for a weight / bias gradient except the optimizer, so the prefix stream's and SigLIP's are
    # issued on a third HIP stream: the data-gradient chain (the critical path) keeps the compute stream, and the weight-gradient
    # GEMMs fill the CUs its poorly filled last rounds leave idle.  The compute stream joins before it updates a dy in place and
    # before a unit's gradients are declared complete.  (LAP_WGRAD_STREAM=0: inline.)
    @contextlib.contextmanager
    def _off_path(self, *tensors):
        wg = self._wg
        cur = torch.cuda.current_stream()
        if wg is None or cur != self._wg_main:
            yield
            return
        wg.wait_stream(self._wg_main)
        for t in tensors:
            t.record_stream(wg)
        with torch.cuda.stream(wg):
            yield
        ev = torch.cuda.Event()
        ev.record(wg)
        self._wg_ev.setdefault(tensors[0].data_ptr(), []).append(ev)     # keyed by dy: the tensor the path may rewrite
        self._wg_dirty = True

    def _wg_join(self, dy=None):
        """The compute stream waits for the off-path readers of `dy` (about to be updated in place), or for all of them."""
        if self._wg is None or not self._wg_dirty or torch.cuda.current_stream() != self._wg_main:
            return
        if dy is not None:
            for ev in self._wg_ev.pop(dy.data_ptr(), ()):
                self._wg_main.wait_event(ev)
        else:
            self._wg_main.wait_stream(self._wg)
            self._wg_ev.clear()
            self._wg_dirty = False

    def _unit_done(self, name, sfx=None):
        """comm.grads_ready for a unit whose gradients may still be in flight on the second (`sfx`) or third stream: the
        communication / optimizer stream waits for those too, the compute stream does not."""
        also = [sfx] if sfx is not None else []
        if self._wg is not None and self._wg_dirty and torch.cuda.current_stream() == self._wg_main:
            also.append(self._wg)
        self.comm.grads_ready(name, also=also or None)

    def _wg_begin(self):
        """Start of a backward pass on the current stream: weight gradients go off the path from here on."""
        if self.wgrad_stream and self.device.type == "cuda" and not torch.cuda.is_current_stream_capturing():
            if self._wg_obj is None:
                self._wg_obj = torch.cuda.Stream(self.device)
            self._wg, self._wg_main, self._wg_dirty = self._wg_obj, torch.cuda.current_stream(), False

    def _wg_end(self):
        self._wg_join()
        self._wg = None

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
            with self._off_path(dy, x, t, dt):
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

    def _rows_res_tile(self, x, name):
        """Tile request for the out / down projection (+ residual) of the last layer's row subset: 14, the assembly residual kernel
        the other layers' out / down products run on, where the library takes the shape (M a multiple of 256) and no A/B switch has
        the assembly routes off; else -1, the planner's choice.  Left to itself the planner's fill rule sends the 16 tiles of
        512 x 2048 to the HIP tiles: the step's out / down products would no longer all be the one kernel."""
        if os.environ.get("LAP_GEMM_NO_ASM") is not None or os.environ.get("LAP_GEMM_NO_ASM_RES") is not None or \
                os.environ.get("LAP_UNFUSED_RESIDUAL", "0") == "1":
            return -1
        w = self.W(name)
        ok = hip._lib.lap_gemm_asm_res_ok(0, x.shape[0], w.shape[0], x.shape[1], x.stride(0), w.stride(0), w.shape[0])
        return 14 if ok and x.stride(1) == 1 else -1

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

    # ================================================================== SigLIP
    def _siglip_fwd(self, images: torch.Tensor, save: bool, collect=None, x_in=None, blocks=None):
        """images f32 [N,H,W,3] -> tokens bf16 [N*T, Dv].  openpi siglip (missing) restated in
        siglip_gemma3.py:382-545 minus :432, plus head bias.
        Test hook (teacher-forced per-block parity): with `x_in` (bf16 [N*T, W]) the stem is skipped, only `blocks` run
        and the block output is returned instead of the projected tokens."""
        s, T = self.s, self.n_img_tok
        W = s.width
        hd = W // s.num_heads
        ctx = {"blocks": []} if save else None
        if x_in is not None:
            x, N = x_in, x_in.shape[0] // T
            for l in blocks:
                x = self._siglip_block(l, x, N, T, W, hd, None, False)
            return x, None
        N = images.shape[0]
        x, patches = self._siglip_stem(images)
        if collect is not None:
            collect["img/stem"] = x
        if save:
            ctx["patches"] = patches
        for l in range(s.depth):
            x = self._siglip_block(l, x, N, T, W, hd, ctx, save)
            if collect is not None:
                collect[f"img/block{l:02d}"] = x
        self.comm.wait_unit("img_head")
        enc, mean, rstd = hip.layernorm_fwd(x, self.F("img/norm_g"), self.F("img/norm_b"))
        tok = hip.linear_fwd(enc, self.W("img/head_w"), bias=self.F("img/head_b"))
        if save:
            ctx["final"] = (x, enc, mean, rstd)
        if collect is not None:
            collect["img/out"] = tok
        return tok, ctx

    def _siglip_stem(self, images: torch.Tensor):
        """f32 stem (siglip_gemma3.py:398-408) on the MFMA path -> (x bf16 [N*T, W], the (hi, lo) patches its weight gradient reads):
        x = hi + lo (2 x bf16, 16 mantissa bits), products exact in the f32 accumulator, the lo.lo term (2^-18 relative) dropped."""
        p_hi, p_lo = hip.split_f32_hilo(hip.im2col_patch(images.contiguous(), self.s.patch))
        w_hi, w_lo = hip.split_f32_hilo(self.F("img/stem_w"))
        (R, Kp), W = p_hi.shape, self.s.width
        stem = torch.empty((R, W), dtype=torch.float32, device=p_hi.device)
        hip.gemm(p_hi, w_hi, stem, M=R, N=W, K=Kp, lda=Kp, ldb=Kp, ldc=W, bias=self.F("img/stem_b"))
        hip.gemm(p_hi, w_lo, stem, M=R, N=W, K=Kp, lda=Kp, ldb=Kp, ldc=W, accum=True)
        hip.gemm(p_lo, w_hi, stem, M=R, N=W, K=Kp, lda=Kp, ldb=Kp, ldc=W, accum=True)
        return hip.add_posemb_cast(stem, self.F("img/pos"), self.n_img_tok), (p_hi, p_lo)

    def _siglip_block(self, l, x, N, T, W, hd, ctx, save):
        """One pre-LN encoder block (siglip_gemma3.py:59-167): x + MHA(LN(x)), then + MLP(LN(.))."""
        s = self.s
        self.comm.wait_unit(f"img{l}")
        p = f"img/{l}/"
        y, mean1, rstd1 = hip.layernorm_fwd(x, self.F(p + "ln1_g"), self.F(p + "ln1_b"))
        qkv = hip.linear_fwd(y, self.W(p + "wqkv"), bias=self.F(p + "bqkv"))
        (o, _), lse = hip.attention_fwd([qkv[:, :W]], [qkv[:, W:2 * W]], [qkv[:, 2 * W:]], [T], [T], N, s.num_heads, s.num_heads, hd,
                                        scale=hd ** -0.5, q_rs=(3 * W, 0), kv_rs=(3 * W, 0), need_lse=save)
        x1 = hip.linear_fwd(o, self.W(p + "wo"), bias=self.F(p + "bo"), residual=x)
        y2, mean2, rstd2 = hip.layernorm_fwd(x1, self.F(p + "ln2_g"), self.F(p + "ln2_b"))
        self.comm.pace(f"img{l}")
        if save:
            if self.fuse_gelu and hip.linear_bias_gelu_train_ok(y2, self.W(p + "w1"), self.F(p + "b1")):
                h, a = hip.linear_bias_gelu_train(y2, self.W(p + "w1"), self.F(p + "b1"))     # fc1 + bias with the GELU in its epilogue
            else:
                h = hip.linear_fwd(y2, self.W(p + "w1"), bias=self.F(p + "b1"))
                a = hip.gelu_fwd(h)
        else:   # nothing keeps the pre-activation: GELU in the GEMM epilogue, after the bf16 rounding of the Dense output (same bits)
            h, a = None, hip.linear_fwd(y2, self.W(p + "w1"), bias=self.F(p + "b1"), gelu="bf16")
        x2 = hip.linear_fwd(a, self.W(p + "w2"), bias=self.F(p + "b2"), residual=x1)
        if save:
            ctx["blocks"].append((x, y, mean1, rstd1, qkv, o, lse, x1, y2, mean2, rstd2, h, a))
        return x2

    def _siglip_bwd(self, ctx, dtok: torch.Tensor):
        s, T = self.s, self.n_img_tok
        W = s.width
        hd = W // s.num_heads
        x, enc, mean, rstd = ctx["final"]
        N = x.shape[0] // T
        self._bgrad(dtok, "img/head_b")
        self._wgrad(dtok, enc, "img/head_w")
        denc = hip.linear_dgrad(dtok, self.W("img/head_w"))
        self._unit_done("img_head")
        # Bias gradients = column sums of a dy.  Two of a block's four (fc2's and the out projection's) come out of the LayerNorm
        # backward that PRODUCES that dy instead of a pass of their own over 38 MB (+1.8 us in that kernel against a 15.5 us
        # column-sum launch; a GELU backward that sums its columns was 2.3 x slower than the two kernels it replaced).
        fuse_b = os.environ.get("LAP_FUSE_BGRAD", "1") != "0"
        last = s.depth - 1
        dx = hip.layernorm_bwd(x, denc, self.F("img/norm_g"), mean, rstd, self.G("img/norm_g"), self.G("img/norm_b"),
                               dxsum=self.G(f"img/{last}/b2") if fuse_b else None)
        for l in reversed(range(s.depth)):
            p = f"img/{l}/"
            x, y, mean1, rstd1, qkv, o, lse, x1, y2, mean2, rstd2, h, a = ctx["blocks"][l]
            if not fuse_b:
                self._bgrad(dx, p + "b2")
            self._wgrad(dx, a, p + "w2")
            if self.fuse_gelu and hip.dgrad_gelu_bwd_ok(dx, self.W(p + "w2"), h):
                dh = hip.linear_dgrad_gelu_bwd(dx, self.W(p + "w2"), h)      # fc2's data gradient with the GELU backward as its epilogue
            else:
                da = hip.linear_dgrad(dx, self.W(p + "w2"))
                dh = hip.gelu_bwd(h, da)
                del da
            self._bgrad(dh, p + "b1")
            self._wgrad(dh, y2, p + "w1")
            dy2 = hip.linear_dgrad(dh, self.W(p + "w1"))
            del dh
            self._wg_join(dx)    # (the fc2 weight / bias gradients read dx)
            hip.layernorm_bwd(x1, dy2, self.F(p + "ln2_g"), mean2, rstd2, self.G(p + "ln2_g"), self.G(p + "ln2_b"), dx=dx, accum_dx=True,
                              dxsum=self.G(p + "bo") if fuse_b else None)
            if not fuse_b:
                self._bgrad(dx, p + "bo")
            self._wgrad(dx, o, p + "wo")
            do = hip.linear_dgrad(dx, self.W(p + "wo"))
            dqkv = torch.empty_like(qkv)
            hip.attention_bwd([qkv[:, :W]], [qkv[:, W:2 * W]], [qkv[:, 2 * W:]], [o], [do], lse, [T], [T], N, s.num_heads, s.num_heads, hd,
                              scale=hd ** -0.5, q_rs=(3 * W, 0), kv_rs=(3 * W, 0),
                              dq_out=[dqkv[:, :W]], dk_out=[dqkv[:, W:2 * W]], dv_out=[dqkv[:, 2 * W:]])
            self._bgrad(dqkv, p + "bqkv")
            self._wgrad(dqkv, y, p + "wqkv")
            dy = hip.linear_dgrad(dqkv, self.W(p + "wqkv"))
            self._wg_join(dx)    # (the out-projection's read dx)
            hip.layernorm_bwd(x, dy, self.F(p + "ln1_g"), mean1, rstd1, self.G(p + "ln1_g"), self.G(p + "ln1_b"), dx=dx, accum_dx=True,
                              dxsum=self.G(f"img/{l - 1}/b2") if (fuse_b and l > 0) else None)
            ctx["blocks"][l] = None
            self._unit_done(f"img{l}")
        dstem = hip.add_posemb_cast_bwd(dx, self.G("img/pos"), T)     # f32 copy of a bf16 gradient: exact in bf16
        p_hi, p_lo = ctx["patches"]
        gw = self.G("img/stem_w")
        tmp = torch.empty((gw.shape[0], p_hi.shape[1]), dtype=torch.float32, device=gw.device)   # [W, 592]
        hip.linear_wgrad(dx, p_hi, tmp)
        hip.linear_wgrad(dx, p_lo, tmp, accum=True)
        gw.add_(tmp[:, :gw.shape[1]])
        hip.colsum(dstem, self.G("img/stem_b"))

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
        tok, ictx = (tower(self, images), None) if fused else self._siglip_fwd(images, save, collect)
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
        self._siglip_bwd(ictx, dtok)

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
        given before (the SigLIP tower); their results are next touched by `_llm_fwd`, which joins the streams."""
        sfx = self._suffix_stream(x_t, time) if overlap else None
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
        sfx = self._suffix_stream(dx1, dmod)
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

    # ================================================================== joint Gemma layers
    def _mod_slot(self, mod, slot):
        W3 = 3 * self.e.width
        return mod[:, slot * W3:(slot + 1) * W3]

    def _last_layer_rows(self, lr, qinfo, B, n0, Lt, *, save, x1, collect, verbose):
        """The row subset of the last layer's prefix stream, or None: every row.  Nothing behind the last layer's K / V reads a
        prefix row but the language head, and it reads `lr.sel`'s rows only (16 of 560 per sample at the benchmark's shapes), so
        in a train step Q, the attention output, the out projection, the FFN and their backward run on those rows alone.
        Anything that looks at the layer's other rows (`collect`, the per-layer hooks, eval, serving) or runs products this
        path has no route for (fp8, LoRA) keeps all rows; so does a step without a row selection or with a frozen prefix."""
        if not (self.last_layer_rows and save and x1 is not None and collect is None and not verbose and lr is not None
                and lr.sel is not None and self.gemm_dtype == "bf16" and not self._prefix_frozen()):
            return None
        p = f"llm/{self.v.depth - 1}/"
        if any(self._lora(p + k) is not None for k in ("wqkv0", "wo0", "wgu0", "wd0")):
            return None
        return LastRows(lr.sel, qinfo, B, n0, Lt)

    def _llm_fwd(self, x0, x1, mod, pos, qinfo, kinfo, B, n0, n1, save: bool, kv_cache=None, cache_out=None, collect=None,
                 mod_shared: bool = False, layers=None, last_rows=None):
        """gemma.Module.__call__ layers (gemma.py:336-387,167-290).  x0 [B*n0, Dv] or None, x1 [B*n1, De] or None.
        kv_cache: per-layer (k, v) of the prefix used as key segment 0 when x0 is None (serving).
        last_rows (`_last_layer_rows`): the last layer's prefix stream is compact behind K / V, and so is the x0 returned.
        Returns final pre-norm activations and the saved context."""
        v, e = self.v, self.e
        NH, HD, KV = v.num_heads, v.head_dim, v.num_kv_heads
        Ttot = pos.shape[1]
        ctx = [] if save else None
        mld = 0 if mod_shared else (mod.stride(0) if mod is not None else 0)  # 0: one modulation row for every sample
        sfx = self._suffix_stream(*([x1, mod] if mod is not None else [x1])) if (x0 is not None and x1 is not None) else None
        main = torch.cuda.current_stream() if sfx is not None else None
        on_sfx = (lambda: torch.cuda.stream(sfx)) if sfx is not None else contextlib.nullcontext
        if last_rows is not None and not (save and x0 is not None and x1 is not None and layers is None and collect is None):
            raise ValueError("_llm_fwd: last_rows goes with a saved two-stream pass over all layers without `collect`")
        for l in (range(v.depth) if layers is None else layers):    # `layers`: test hook (teacher-forced per-layer parity)
            self.comm.wait_unit(f"llm{l}", also=sfx)
            p = f"llm/{l}/"
            rows0 = last_rows if l == v.depth - 1 else None
            q = [None, None]; k = [None, None]; vv = [None, None]; h = [None, None]; rstd_a = [None, None]
            lt = [{}, {}]       # LoRA down products t per stream and projection (kept for the backward)
            if x0 is not None:
                h[0], rstd_a[0] = hip.rmsnorm_fwd(x0, scale=self.F(p + "n_attn"), save_rstd=save)
                qkv = self._lin0(h[0], p + "wqkv0")
                lt[0]["wqkv"] = self._lora_fwd(h[0], qkv, p + "wqkv0")
                if rows0 is None:
                    q[0], k[0], vv[0] = hip.rope_split_fwd(qkv, pos, B, n0, Ttot, 0, NH, HD, HD ** -0.5)
                else:   # K / V of every row, Q of the kept rows
                    q[0], k[0], vv[0] = hip.rope_split_fwd(qkv, pos, B, n0, Ttot, 0, NH, HD, HD ** -0.5, q_row=rows0.inv,
                                                           q_rows=B * rows0.n_sel)
                del qkv
            elif kv_cache is not None:
                k[0], vv[0] = kv_cache[l]
            if x1 is not None:
                with on_sfx():
                    if mod is None:     # pi0: plain RMSNorm in the expert (`use_adarms=[False, False]`, lap.py:51)
                        h[1], rstd_a[1] = hip.rmsnorm_fwd(x1, scale=self.F(p + "n_attn1"), save_rstd=save)
                    else:
                        h[1], rstd_a[1] = hip.rmsnorm_fwd(x1, mod=self._mod_slot(mod, 2 * l), rows_per_sample=n1, save_rstd=save, mod_ld=mld)
                    qkv = hip.linear_fwd(h[1], self.W(p + "wqkv1"))
                    lt[1]["wqkv"] = self._lora_fwd(h[1], qkv, p + "wqkv1")
                    q[1], k[1], vv[1] = hip.rope_split_fwd(qkv, pos, B, n1, Ttot, Ttot - n1, NH, HD, HD ** -0.5)
                    del qkv
                self._handoff(sfx, main, q[1], k[1], vv[1])
            if cache_out is not None:
                cache_out.append((k[0], vv[0]))
            qlen = [n0 if x0 is not None else 0, n1 if x1 is not None else 0]
            klen = [k[0].shape[0] // B if k[0] is not None else 0, n1 if x1 is not None else 0]
            xfull = x0
            if rows0 is not None:     # a query segment shorter than its key segment, as serving runs it against a cached prefix
                qlen[0] = rows0.n_sel
                x0 = hip.gather_rows_bf16(x0, rows0.rowid)      # the residual operand of the out projection, its only other reader
                self.last_rows_steps += 1
            o, lse = hip.attention_fwd(q, k, vv, qlen, klen, B, NH, KV, HD, qinfo if rows0 is None else rows0.qinfo, kinfo, need_lse=save)
            self._handoff(main, sfx, o[1])
            xa = [None, None]; y1 = None; hf = [None, None]; rstd_f = [None, None]; gu = [None, None]; act = [None, None]; y1f = None
            xn = [None, None]
            if x1 is not None and mod is None:       # pi0: plain residuals (gemma.py:577-583 with gate None)
                with on_sfx():
                    xa[1] = hip.linear_fwd(o[1], self.W(p + "wo1"), residual=x1)
                    lt[1]["wo"] = self._lora_fwd(o[1], xa[1], p + "wo1")
                    hf[1], rstd_f[1] = hip.rmsnorm_fwd(xa[1], scale=self.F(p + "n_ffw1"), save_rstd=save)
                    gu[1] = hip.linear_fwd(hf[1], self.W(p + "wgu1"))
                    lt[1]["wgu"] = self._lora_fwd(hf[1], gu[1], p + "wgu1")
                    act[1] = hip.geglu_fwd(gu[1])
                    xn[1] = hip.linear_fwd(act[1], self.W(p + "wd1"), residual=xa[1])
                    lt[1]["wd"] = self._lora_fwd(act[1], xn[1], p + "wd1")
            elif x1 is not None:     # (issued first: 8 short kernels that then run under the prefix stream's GEMMs)
                with on_sfx():
                    y1 = hip.linear_fwd(o[1], self.W(p + "wo1"))
                    lt[1]["wo"] = self._lora_fwd(o[1], y1, p + "wo1")
                    xa[1] = hip.gated_residual_fwd(x1, y1, self._mod_slot(mod, 2 * l)[:, 2 * e.width:], n1, mld)
                    hf[1], rstd_f[1] = hip.rmsnorm_fwd(xa[1], mod=self._mod_slot(mod, 2 * l + 1), rows_per_sample=n1, save_rstd=save, mod_ld=mld)
                    gu[1] = hip.linear_fwd(hf[1], self.W(p + "wgu1"))
                    lt[1]["wgu"] = self._lora_fwd(hf[1], gu[1], p + "wgu1")
                    act[1] = hip.geglu_fwd(gu[1])
                    y1f = hip.linear_fwd(act[1], self.W(p + "wd1"))
                    lt[1]["wd"] = self._lora_fwd(act[1], y1f, p + "wd1")
                    xn[1] = hip.gated_residual_fwd(xa[1], y1f, self._mod_slot(mod, 2 * l + 1)[:, 2 * e.width:], n1, mld)
            if x0 is not None:
                xa[0] = self._lin0(o[0], p + "wo0", residual=x0, tile=-1 if rows0 is None else self._rows_res_tile(o[0], p + "wo0"))
                lt[0]["wo"] = self._lora_fwd(o[0], xa[0], p + "wo0")
                hf[0], rstd_f[0] = hip.rmsnorm_fwd(xa[0], scale=self.F(p + "n_ffw"), save_rstd=save)
                self.comm.pace(f"llm{l}")     # optimizer units released here start under the longest MFMA-bound GEMM of the layer
                if save and self.fuse_geglu_fwd and self._lora(p + "wgu0") is None and hip.linear_geglu_train_ok(hf[0], self.W(p + "wgu0")):
                    # gate | up projection with the GeGLU in its epilogue: gu (kept for the backward pass) and act leave one launch
                    gu[0], act[0] = hip.linear_geglu_train(hf[0], self.W(p + "wgu0"))
                else:
                    gu_out = None
                    if save and self.fuse_geglu_bwd:    # rows padded like d(gate | up): the fused backward kernel shares one row stride
                        gu_out = hip._padded_rows(hf[0].shape[0], 2 * v.mlp_dim, hf[0].device, hip._row_pad(2 * v.mlp_dim))
                    gu[0] = self._lin0(hf[0], p + "wgu0", out=gu_out)
                    lt[0]["wgu"] = self._lora_fwd(hf[0], gu[0], p + "wgu0")   # (before the GeGLU: lora.FeedForward's _dot)
                    act[0] = hip.geglu_fwd(gu[0], pad=self.gemm_dtype != "fp8")
                xn[0] = self._lin0(act[0], p + "wd0", residual=xa[0], tile=-1 if rows0 is None else self._rows_res_tile(act[0], p + "wd0"))
                lt[0]["wd"] = self._lora_fwd(act[0], xn[0], p + "wd0")
            if save:
                ctx.append(dict(x=[xfull, x1], h=h, rstd_a=rstd_a, q=q, k=k, v=vv, o=o, lse=lse, xa=xa, y1=y1, hf=hf, rstd_f=rstd_f,
                                gu=gu, act=act, y1f=y1f, lt=lt))
            x0, x1 = xn
            if collect is not None:
                collect[f"llm/layer{l:02d}/x0"], collect[f"llm/layer{l:02d}/x1"] = x0, x1
        self._handoff(sfx, main, x1)
        return x0, x1, ctx

    def _llm_bwd(self, ctx, dx0, dx1, mod, dmod, pos, qinfo, kinfo, B, n0, n1, last_rows=None):
        """last_rows: as in `_llm_fwd` — dx0 arrives with the kept rows only and leaves the last layer with all of them."""
        v, e = self.v, self.e
        NH, HD, KV = v.num_heads, v.head_dim, v.num_kv_heads
        Ttot = pos.shape[1]
        has_sfx = dx1 is not None         # False: prefix-only backward (enable_action_training=False, lap.py:449-455)
        ada = has_sfx and mod is not None  # False with a suffix stream: pi0 (plain norms and residuals in the expert)
        ldm = mod.stride(0) if ada else 0
        zero_do0 = None
        sfx = self._suffix_stream(*([dx1, dmod, mod] if ada else [dx1]))
        main = torch.cuda.current_stream() if sfx is not None else None
        on_sfx = (lambda: torch.cuda.stream(sfx)) if sfx is not None else contextlib.nullcontext
        for l in reversed(range(v.depth)):
            p = f"llm/{l}/"
            c = ctx[l]
            d_o = [None, None]
            rows0 = last_rows if l == v.depth - 1 else None
            # ---- FFN + attention output, suffix stream: xn = xa + y1f * gate_f  (on the second HIP stream, see the module doc)
            slot_f, slot_a = 2 * l + 1, 2 * l
            if has_sfx and not ada:
                with on_sfx():      # xn = xa + act wd^T, xa = x + o wo^T: the residuals pass dx1 through, the norms add onto it in place
                    self._wgrad(dx1, c["act"][1], p + "wd1")
                    dact = hip.linear_dgrad(dx1, self.W(p + "wd1"))
                    self._lora_bwd(dx1, c["act"][1], c["lt"][1].get("wd"), dact, p + "wd1")
                    dgu = hip.geglu_bwd(c["gu"][1], dact)
                    self._wgrad(dgu, c["hf"][1], p + "wgu1")
                    dhf = hip.linear_dgrad(dgu, self.W(p + "wgu1"))
                    self._lora_bwd(dgu, c["hf"][1], c["lt"][1].get("wgu"), dhf, p + "wgu1")
                    hip.rmsnorm_bwd(c["xa"][1], dhf, c["rstd_f"][1], scale=self.F(p + "n_ffw1"), dx=dx1, dscale=self.G(p + "n_ffw1"), accum_dx=True)
                    self._wgrad(dx1, c["o"][1], p + "wo1")
                    d_o[1] = hip.linear_dgrad(dx1, self.W(p + "wo1"))
                    self._lora_bwd(dx1, c["o"][1], c["lt"][1].get("wo"), d_o[1], p + "wo1")
                    del dact, dgu, dhf
            elif has_sfx:
                with on_sfx():
                    gate_f = self._mod_slot(mod, slot_f)[:, 2 * e.width:]
                    dy1f = hip.gated_residual_bwd(dx1, c["y1f"], gate_f, n1, ldm, self._mod_slot(dmod, slot_f)[:, 2 * e.width:], dmod.stride(0))
                    self._wgrad(dy1f, c["act"][1], p + "wd1")
                    dact = hip.linear_dgrad(dy1f, self.W(p + "wd1"))
                    self._lora_bwd(dy1f, c["act"][1], c["lt"][1].get("wd"), dact, p + "wd1")
                    dgu = hip.geglu_bwd(c["gu"][1], dact)
                    self._wgrad(dgu, c["hf"][1], p + "wgu1")
                    dhf = hip.linear_dgrad(dgu, self.W(p + "wgu1"))
                    self._lora_bwd(dgu, c["hf"][1], c["lt"][1].get("wgu"), dhf, p + "wgu1")
                    hip.rmsnorm_bwd(c["xa"][1], dhf, c["rstd_f"][1], mod=self._mod_slot(mod, slot_f), rows_per_sample=n1, dx=dx1,
                                    dmod=self._mod_slot(dmod, slot_f), accum_dx=True)
                    gate_a = self._mod_slot(mod, slot_a)[:, 2 * e.width:]
                    dy1 = hip.gated_residual_bwd(dx1, c["y1"], gate_a, n1, ldm, self._mod_slot(dmod, slot_a)[:, 2 * e.width:], dmod.stride(0))
                    self._wgrad(dy1, c["o"][1], p + "wo1")
                    d_o[1] = hip.linear_dgrad(dy1, self.W(p + "wo1"))
                    self._lora_bwd(dy1, c["o"][1], c["lt"][1].get("wo"), d_o[1], p + "wo1")
                    del dy1f, dact, dgu, dhf, dy1
            # ---- FFN, prefix stream: xn = xa + act @ wd^T   (dx0 is None: the whole prefix side is frozen)
            if dx0 is not None:
                self._wgrad(dx0, c["act"][0], p + "wd0")
                if self.fuse_geglu_bwd and self._lora(p + "wd0") is None and hip.dgrad_geglu_bwd_ok(dx0, self.W(p + "wd0"), c["gu"][0]):
                    # the down projection's data gradient with the GeGLU backward as its epilogue: d(act) never reaches memory
                    dgu = hip.linear_dgrad_geglu_bwd(dx0, self.W(p + "wd0"), c["gu"][0])
                else:
                    dact = self._dgrad0(dx0, p + "wd0")
                    self._lora_bwd(dx0, c["act"][0], c["lt"][0].get("wd"), dact, p + "wd0")
                    dgu = hip.geglu_bwd(c["gu"][0], dact, pad=self.gemm_dtype != "fp8")
                    del dact
                self._wgrad(dgu, c["hf"][0], p + "wgu0")
                dhf = self._dgrad0(dgu, p + "wgu0")
                self._lora_bwd(dgu, c["hf"][0], c["lt"][0].get("wgu"), dhf, p + "wgu0")
                del dgu
                self._wg_join(dx0)   # (the down projection's weight gradient reads dx0)
                hip.rmsnorm_bwd(c["xa"][0], dhf, c["rstd_f"][0], scale=self.F(p + "n_ffw"), dx=dx0, dscale=self.G(p + "n_ffw"), accum_dx=True)
                del dhf
                self._wgrad(dx0, c["o"][0], p + "wo0")
                d_o[0] = self._dgrad0(dx0, p + "wo0")
                self._lora_bwd(dx0, c["o"][0], c["lt"][0].get("wo"), d_o[0], p + "wo0")
            else:   # the attention backward still needs a dO for the prefix queries: zero (their dq / dk / dv are discarded)
                if zero_do0 is None:
                    zero_do0 = torch.zeros_like(c["o"][0])
                d_o[0] = zero_do0
            # ---- attention
            self._handoff(sfx, main, d_o[1])
            dq, dk, dv = hip.attention_bwd(c["q"], c["k"], c["v"], c["o"], d_o, c["lse"], [n0 if rows0 is None else rows0.n_sel, n1], [n0, n1],
                                           B, NH, KV, HD, qinfo if rows0 is None else rows0.qinfo, kinfo,
                                           stop_q1_to_k0=self.config.stop_action_to_vlm_grad)
            self._handoff(main, sfx, dq[1], dk[1], dv[1])
            if has_sfx:
                with on_sfx():
                    dqkv = hip.rope_split_bwd(dq[1], dk[1], dv[1], pos, B, n1, Ttot, Ttot - n1, NH, HD, HD ** -0.5)
                    self._wgrad(dqkv, c["h"][1], p + "wqkv1")
                    dh = hip.linear_dgrad(dqkv, self.W(p + "wqkv1"))
                    self._lora_bwd(dqkv, c["h"][1], c["lt"][1].get("wqkv"), dh, p + "wqkv1")
                    if ada:
                        hip.rmsnorm_bwd(c["x"][1], dh, c["rstd_a"][1], mod=self._mod_slot(mod, slot_a), rows_per_sample=n1, dx=dx1,
                                        dmod=self._mod_slot(dmod, slot_a), accum_dx=True)
                    else:
                        hip.rmsnorm_bwd(c["x"][1], dh, c["rstd_a"][1], scale=self.F(p + "n_attn1"), dx=dx1, dscale=self.G(p + "n_attn1"), accum_dx=True)
                    del dqkv, dh
            if dx0 is not None:
                dqkv = hip.rope_split_bwd(dq[0], dk[0], dv[0], pos, B, n0, Ttot, 0, NH, HD, HD ** -0.5,
                                          q_row=None if rows0 is None else rows0.inv)      # (compact dq: zeros in the other rows' q columns)
                self._wgrad(dqkv, c["h"][0], p + "wqkv0")
                dh = self._dgrad0(dqkv, p + "wqkv0")
                self._lora_bwd(dqkv, c["h"][0], c["lt"][0].get("wqkv"), dh, p + "wqkv0")
                if rows0 is None:
                    self._wg_join(dx0)   # (the out projection's reads dx0)
                    hip.rmsnorm_bwd(c["x"][0], dh, c["rstd_a"][0], scale=self.F(p + "n_attn"), dx=dx0, dscale=self.G(p + "n_attn"), accum_dx=True)
                else:   # all rows from here on: the norm's backward of every row, the compact residual cotangent added at its rows
                    dx0 = hip.rmsnorm_bwd(c["x"][0], dh, c["rstd_a"][0], scale=self.F(p + "n_attn"), dscale=self.G(p + "n_attn"),
                                          add_row=rows0.inv, addend=dx0)
                del dqkv, dh
            ctx[l] = None
            self._unit_done(f"llm{l}", sfx)   # complete once both streams are through: the optimizer's stream waits for both, the
                                             # compute stream goes on (it meets the second stream again at the next attention)
        self._handoff(sfx, main)
        return dx0, dx1

    # ================================================================== training forward (+ backward)
    def _loss_impl(self, rng, observation: CoTObservation, actions: torch.Tensor, *, train: bool, noise=None, time=None,
                   backward: bool, collect: dict | None = None, verbose: bool = False):
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
        last_rows = self._last_layer_rows(lrows, qinfo, B, Pn, obs.tokenized_prompt.shape[1], save=backward, x1=x1, collect=collect,
                                          verbose=verbose)
        xf0, xf1, lctx = self._llm_fwd(x0, x1, mod, pos, qinfo, kinfo, B, Pn, Sx, backward, collect=collect, last_rows=last_rows)
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
        n_active = torch.clamp(self.comm.all_reduce_sum(fb(sm).sum().view(1)), min=1.0) if obs.sample_mask is not None else \
            self.comm.all_reduce_sum(torch.tensor([float(B)], device=dev))
        # lang_term: sum / active samples, or the batch mean without a sample mask (lap.py:579-596; the action-off branch's
        # `final_loss` is the same expression)
        lang_term = (wl * lang_loss).sum() / n_active
        act_loss = torch.zeros(B, dtype=torch.float32, device=dev)
        action_term = 0.0
        dv = None
        if act_on:
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
        self._wg_begin()
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
        dx0, dx1 = self._llm_bwd(lctx, dx0, dx1, mod, dmod, pos, qinfo, kinfo, B, Pn, Sx, last_rows=last_rows)
        sfx = None
        if act_on and cfg.pi05:
            sfx = self._embed_suffix_bwd(sctx, dx1, dmod)
        elif act_on:
            self._embed_suffix_pi0_bwd(sctx, dx1, B, S)
        elif "ada" in self.ps.unit_by_name:   # the action expert's units saw no gradient (zeros): still declared complete for the optimizer's pipeline
            self.comm.grads_ready("ada")
        if not skip_prefix:
            self._embed_prefix_bwd(pctx, dx0, B, Pn)
        self._handoff(sfx, torch.cuda.current_stream() if sfx is not None else None)
        self._wg_end()
        self.comm.grads_ready("small")
        return loss, metrics

    def compute_loss(self, rng, observation, actions, *, train: bool = False, stage_config=None, verbose_mode=None,
                     return_augmented_images: bool = False, noise=None, time=None, collect=None):
        """lap.py:380-602.  rng: int seed or torch.Generator.  `noise` / `time` may be given explicitly (parity tests).
        verbose_mode (None: the config's, lap.py:393-394) adds the token-accuracy metrics and `per_sample_loss` (loss._token_metrics)."""
        verbose = bool(self.config.verbose_mode if verbose_mode is None else verbose_mode)
        return self._loss_impl(rng, observation, actions, train=train, noise=noise, time=time, backward=False, collect=collect,
                               verbose=verbose)

    def loss_and_grad(self, rng, observation, actions, *, train: bool = True, noise=None, time=None, collect=None):
        """Forward + backward; gradients land in self.ps.grad (engine layout; bf16 for the GEMM-weight units, f32 for the embedding table and
        the small unit: ParamStore.grad_dtype).  The caller zeroes the accumulated (f32) units first.  Verbose metrics follow the
        config's `verbose_mode` (the reference's train step runs with the class attribute, scripts/train.py:351)."""
        return self._loss_impl(rng, observation, actions, train=train, noise=noise, time=time, backward=True, collect=collect,
                               verbose=bool(self.config.verbose_mode))

    # ================================================================== serving
    @torch.no_grad()
    def sample_actions(self, rng, observation, *, num_steps: int = 10, noise=None, collect=None, fused=True):
        """lap.py:605-675: prefix prefill once -> per-layer K/V kept in HBM -> `num_steps` Euler steps of the action
        expert attending to [cached prefix | fresh suffix] as two key segments (the reference concatenates, gemma.py:228-230).
        `fused`: True = the fastest denoise-step kernels the shapes allow ("skinny" fused projections for the LAP-3B action
        expert, else "partials" = split-K partial slabs + fused consumers); False = the generic layer path (A/B tests)."""
        with self._serving_weights():
            return self._sample_actions(rng, observation, num_steps=num_steps, noise=noise, collect=collect, fused=fused)

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
                      decode: str = "eager", sampler: str = "host", decode_weights: str = "bf16", allowed_tokens=None):
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
        `policy_io.allowed_token_ids` builds a set from example language actions."""
        from lap_amd import ar_decode       # (it imports this module)
        return ar_decode.sample_tokens(self, rng, observation, max_decoding_steps=max_decoding_steps, temperature=temperature,
                                       collect=collect, decode=decode, sampler=sampler, decode_weights=decode_weights,
                                       allowed_tokens=allowed_tokens)

    DECODE_WEIGHTS = ("bf16", "fp8", "fp8_layers")

    def decode_supported(self, B: int) -> bool:
        """Whether `sample_tokens(decode="fused")` / `GraphedTokenDecoder` serve `B` rows of this model."""
        v = self.v
        return self.comm.world_size == 1 and hip.decode_ok(B, v.width, v.num_heads, v.num_kv_heads, v.head_dim, v.mlp_dim,
                                                            self.config.vocab_size)
