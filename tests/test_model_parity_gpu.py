"""Model-level parity (GPU): the HIP engine (through the C ABI) against the CPU oracle on identical seeded
inputs and parameters — loss, activations at valid positions, every parameter gradient, the sampler.

Tolerances.  The engine computes in bf16 with f32 accumulation like the reference; the oracle's f32 mode is the
mathematical function and its bf16 mode rounds where the reference's dtype flow rounds.  We require the engine's
distance to the f32 oracle to be within a small factor of the bf16 oracle's own distance to it (i.e. our
rounding noise is the reference's rounding noise), plus absolute caps stated inline.
"""
import dataclasses
import os

import pytest
import torch

from oracle import lap_oracle as O
from tests.common import debug_model_cfg, make_inputs, oracle_cfg, rel, to_observation

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _engine(cfg, P):
    from lap_amd.model import LAP

    return LAP(cfg, params=P, device=DEV)


@pytest.mark.parametrize("B,ragged,stop", [(2, False, False), (3, True, False), (3, True, True)])
def test_loss_activations_and_grads(hip, B, ragged, stop):
    _check_loss_activations_and_grads(debug_model_cfg(stop_action_to_vlm_grad=stop), B, ragged)


def _full_width_cfg(monkeypatch, **kw):
    """LAP-3B WIDTHS (Gemma-2B 2048 / 16384, expert 1024 / 4096, SigLIP So400m 1152 / 4304, head sizes 256 and 72, 224 x 224
    images, 48-token prompt, 50-step chunk, action_dim 32) with 2 layers per tower and a 16k-word vocabulary, so that the
    oracle finishes in seconds."""
    from lap_amd import config as C
    from lap_amd.config import LAPConfig

    monkeypatch.setitem(C._GEMMA, "gemma_2b_x2", C.GemmaConfig(2048, 2, 16384, 8, 1, 256))
    monkeypatch.setitem(C._GEMMA, "gemma_300m_x2", C.GemmaConfig(1024, 2, 4096, 8, 1, 256))
    monkeypatch.setitem(C._SIGLIP, "So400m/14_x2", C.SiglipConfig(1152, 2, 4304, 16))
    monkeypatch.setitem(O.GEMMA, "gemma_2b_x2", O.GemmaCfg(2048, 2, 16384, 8, 1, 256))
    monkeypatch.setitem(O.GEMMA, "gemma_300m_x2", O.GemmaCfg(1024, 2, 4096, 8, 1, 256))
    monkeypatch.setitem(O.SIGLIP, "So400m/14_x2", O.SiglipCfg(1152, 2, 4304, 16))
    base = dict(paligemma_variant="gemma_2b_x2", action_expert_variant="gemma_300m_x2", siglip_variant="So400m/14_x2",
                image_size=224, vocab_size=16384, action_dim=32, action_horizon=50, max_token_len=48,
                language_loss_weight=0.4, enable_image_augmentation=False, enable_action_training=True)
    return LAPConfig(**(base | kw))


def test_full_width_two_layer_slice_matches_oracle(hip, monkeypatch):
    """Loss, activations and every gradient at the LAP-3B widths: this drives the production code paths the tiny debug model
    never reaches (256x256 tiles with staged epilogue and tail split, LDS-DMA attention for both head sizes, the hi/lo f32
    stem, vocabulary-chunked cross entropy at width 2048)."""
    _check_loss_activations_and_grads(_full_width_cfg(monkeypatch), B=2, ragged=True)


def _is_bf16_gemm_weight(key):
    """Reference-tree arrays whose cotangent reaches the f32 master through `w.astype(bf16)` of a bf16 dot (gemma.py:307,318; lora.Einsum;
    Flax Dense with dtype=bf16) = the tensors of the engine's bf16 gradient buffers (ParamStore.grad_dtype)."""
    return (key.endswith(("/w", "gating_einsum", "mlp/linear", "mlp_1/linear", "Dense_0/kernel", "Dense_1/kernel", "img/head/kernel"))
            or "MultiHeadDotProductAttention_0" in key and key.endswith("/kernel"))


@pytest.mark.parametrize("width", ["debug", "full"])
def test_weight_gradients_carry_the_reference_bf16_rounding_point(hip, monkeypatch, width):
    """the engine's weight-gradient GEMMs round once to bf16 in their epilogue (ParamStore.grad_dtype) on the argument that
    the reference's f32 masters receive a bf16-rounded cotangent through `w.astype(bf16)`.  The oracle's bf16 mode now has that rounding point
    (`_RoundWeightSTE`: the weight cast's backward rounds), so the claim is measured: every GEMM-weight gradient of the engine against the
    bf16-emulating oracle's autograd.  Two free-running bf16 backward passes decorrelate like the forward ones do, so the bound is stated
    relative to the bf16 oracle's own distance from the f32 oracle, tensor by tensor: the engine must be no further from the bf16 oracle than
    1.5 x that distance (floor 1e-2), and every stored gradient must be a bf16 value in both."""
    from lap_amd.params import engine_to_reference

    cfg = debug_model_cfg() if width == "debug" else _full_width_cfg(monkeypatch, action_dim=7)
    oc = oracle_cfg(cfg)
    P = O.init_params(oc, seed=7)
    obs, actions, noise, time = make_inputs(cfg, B=2, ragged=True)
    grads = {}
    for mode, c in (("f32", oc), ("bf16", dataclasses.replace(oc, emulate_bf16=True))):
        Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
        loss, _ = O.compute_loss(Pg, c, obs, actions, noise, time)
        loss.backward()
        grads[mode] = {k: v.grad for k, v in Pg.items()}
    model = _engine(cfg, P)
    for g in model.ps.grad.values():
        g.zero_()
    model.loss_and_grad(0, to_observation(obs, DEV), actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV))
    torch.cuda.synchronize()
    gref = engine_to_reference(cfg, {name: model.ps.g(name).detach().float().cpu() for name in model.ps.names()})
    checked, worst = 0, (0.0, None, 0.0)
    for k, g16 in grads["bf16"].items():
        if g16 is None or not _is_bf16_gemm_weight(k):
            continue
        # the oracle's rounding point is where the reference has it (SigLIP runs once per image key, lap.py embed_prefix: its masters receive
        # the f32 sum of two bf16-rounded cotangents; the engine batches both keys into one product and rounds once)
        assert "/img/" in k or torch.equal(g16, g16.to(torch.bfloat16).float()), k
        assert torch.equal(gref[k], gref[k].to(torch.bfloat16).float()), k  # ... and the engine's buffer holds bf16 values
        base = rel(g16, grads["f32"][k])
        r = rel(gref[k], g16)
        checked += 1
        if r > worst[0]:
            worst = (r, k, base)
        assert r < max(1.5 * base, 1e-2) or (gref[k] - g16).abs().max() < 1e-4, (k, r, base)
    print(f"weight-gradient rounding point [{width}]: {checked} GEMM-weight tensors, worst engine-vs-bf16-oracle {worst[0]:.2e} ({worst[1]}; "
          f"bf16 oracle vs f32 there {worst[2]:.2e})")
    assert checked >= 14


@pytest.mark.parametrize("name,kw", [
    # training/config.py:752-785 lap_libero: P = 180, S = 10, action_dim 7, language weight 0.4, no stop-grad
    ("lap_libero", dict(max_token_len=180, action_horizon=10, action_dim=7, language_loss_weight=0.4, stop_action_to_vlm_grad=False)),
    # training/config.py:608-619 lap: P = 180, S = 16, action_dim 7, language weight 1.0, stop_action_to_vlm_grad=True
    ("lap", dict(max_token_len=180, action_horizon=16, action_dim=7, language_loss_weight=1.0, stop_action_to_vlm_grad=True)),
    # BASELINE.json synthetic shapes with the benchmark's action_dim 7 (bench.py / lap_bench)
    ("lap_bench", dict(max_token_len=48, action_horizon=50, action_dim=7, language_loss_weight=0.4)),
])
def test_full_width_reference_config_shapes_match_oracle(hip, monkeypatch, name, kw):
    """The shapes of the reference's own TrainConfigs (parity at both prompt budgets) at the LAP-3B widths:
    692-token joint sequences (2 x 256 image tokens + 180 prompt + S), the stop-gradient split of the `lap` config at
    full width, action_dim 7 (ragged K = 7 f32 action projections)."""
    _check_loss_activations_and_grads(_full_width_cfg(monkeypatch, **kw), B=2, ragged=True)


def test_full_width_b16_benchmark_gemm_route_matches_oracle(hip, monkeypatch):
    """The route that runs the benchmark step, under the oracle.  At B = 2 the prefix stream has 1120 rows:
    not a multiple of 256, so gate|up + GeGLU, the down projection's data gradient + GeGLU backward, the residual-epilogue kernels,
    the M cut and the ring weight-gradient kernels all fall back to the HIP tiles there.  B = 16 at the LAP-3B widths (2 layers per
    tower, benchmark shapes) gives the prefix stream 8960 = 35 x 256 rows and SigLIP 8192: every assembly kernel of the B = 32 step
    takes its products, and loss, every layer (free running and teacher forced) and every gradient are held to the bounds of the
    B = 2 slices against the f32 oracle's autograd.  The test asserts that the kernels really ran."""
    import collections

    cfg = _full_width_cfg(monkeypatch, max_token_len=48, action_horizon=50, action_dim=7, language_loss_weight=0.4)
    calls = collections.Counter()
    for name in ("linear_geglu_train", "linear_dgrad_geglu_bwd", "linear_bias_gelu_train", "linear_dgrad_gelu_bwd"):
        def wrap(fn, name):
            def counted(*a, **k):
                calls[name] += 1
                return fn(*a, **k)
            return counted
        monkeypatch.setattr(hip, name, wrap(getattr(hip, name), name))
    before = hip.gemm_asm_launch_counts()
    _check_loss_activations_and_grads(cfg, B=16, ragged=True)
    ran = {k: v - before[k] for k, v in hip.gemm_asm_launch_counts().items()}
    L = 2       # layers per tower (free-running pass; the teacher-forced sweeps add forward launches on top)
    assert calls["linear_geglu_train"] >= L and ran["nt_geglu"] >= L, (calls, ran)              # gate|up + GeGLU, one launch
    assert calls["linear_dgrad_geglu_bwd"] >= L and ran["nn_geglu_bwd"] >= L, (calls, ran)      # down dgrad + GeGLU backward
    assert calls["linear_bias_gelu_train"] >= L and ran["nt_bias_gelu"] >= L, (calls, ran)      # SigLIP fc1 + bias + GELU
    assert calls["linear_dgrad_gelu_bwd"] >= L and ran["nn_gelu_bwd"] >= L, (calls, ran)        # SigLIP fc2 dgrad + GELU backward
    assert ran["nt_res"] + ran["nt_bias_res"] >= 4 * L, ran       # out / down (+ residual) of both towers: whole products or the M cut's full rounds
    # ring weight-gradient kernels of gate|up and down (K = 8960 rows): bf16 stores (round 5, ParamStore.grad_dtype) or f32 (LAP_GRAD_BF16=0)
    assert ran["tn"] + ran["tn_b16"] >= L and ran["tn_t"] + ran["tn_t_b16"] >= L, ran
    assert ran["nt"] >= 2 * L and ran["nn"] >= 2 * L, ran         # plain forward / data-gradient products (qkv, out, gate|up dgrad)


def test_full_width_sample_actions_matches_oracle(hip, monkeypatch):
    """Batch-1 serving at the LAP-3B widths: prefill + 10 denoise steps through the fused split-K consumers, the hoisted
    sin / cos table and the key-split attention, against the oracle and against the generic layer path (bit for bit)."""
    cfg = _full_width_cfg(monkeypatch)
    oc = oracle_cfg(cfg)
    P = O.init_params(oc, seed=5)
    obs, _, noise, _ = make_inputs(cfg, B=1, ragged=False)
    so = {k: v for k, v in obs.items() if k != "tokenized_langact_mask"}
    ref = O.sample_actions(P, oc, so, noise, num_steps=10)
    ref16 = O.sample_actions(P, dataclasses.replace(oc, emulate_bf16=True), so, noise, num_steps=10)
    model = _engine(cfg, P)
    o = to_observation(so | {"tokenized_langact_mask": None}, DEV)
    out = model.sample_actions(0, o, num_steps=10, noise=noise.to(DEV))                     # skinny fused projections, one launch per step
    assert model.serve_chain and model._chain_ctr is not None and not model.serve_chain_failed()
    model.serve_chain = False                                                               # ... as six launches per layer: same bits
    assert torch.equal(out, model.sample_actions(0, o, num_steps=10, noise=noise.to(DEV)))
    model.serve_chain = True
    # a barrier that timed out is reported, and the fallback (serve.Policy.infer does this after its device sync) is permanent
    model._chain_ctr[10 * 64] = 1                                                           # CH_CTR_ERR (csrc/serve_chain.hpp)
    assert model.serve_chain_failed()
    model.disable_serve_chain()
    assert not model.serve_chain and not model.serve_chain_failed()
    assert torch.equal(out, model.sample_actions(0, o, num_steps=10, noise=noise.to(DEV)))
    model.serve_chain = True
    generic = model.sample_actions(0, o, num_steps=10, noise=noise.to(DEV), fused=False)
    assert torch.equal(generic, model.sample_actions(0, o, num_steps=10, noise=noise.to(DEV), fused="partials"))
    err, base = rel(out, ref), rel(ref16, ref)
    assert out.shape == (1, 50, 32) and err < max(FREE_RUN_RATIO * base, 5e-3), (err, base)
    assert rel(generic, ref) < max(FREE_RUN_RATIO * base, 5e-3)
    assert rel(out, generic) < max(FREE_RUN_RATIO * base, 5e-3)    # same rounding points, different K summation order


def _serve_launch_traces(hip, monkeypatch):
    """The library entry points that take a stream, in the order ONE fresh model issues them, for `sample_actions` (3 Euler steps)
    on each denoise route and for `sample_tokens(decode="eager")`, run-length encoded as [[name, count], ...].  `_full_width_cfg`
    with action_dim 7: at the LAP-3B widths the skinny projections, the one-launch chain and the panel prefill are live, and with
    7 action dimensions so is the chain's fused Euler / embed tail (it takes 7 or 8), whose first, middle and last step differ.
    The routes run in a fixed order on one model: what a call finds cached (packed weight images, modulations) is part of the trace."""
    import ctypes

    cfg = _full_width_cfg(monkeypatch, action_dim=7)
    P = O.init_params(oracle_cfg(cfg), seed=5)
    obs, _, noise, _ = make_inputs(cfg, B=1, ragged=False)
    o = to_observation({k: v for k, v in obs.items() if k != "tokenized_langact_mask"} | {"tokenized_langact_mask": None}, DEV)
    model = _engine(cfg, P)
    trace = []

    def traced(name, fn):
        def call(*a):
            trace.append(name)
            return fn(*a)
        return call
    for name, fn in list(hip._fn.items()):
        sig = hip.SIGNATURES[name]
        if sig and sig[-1] is ctypes.c_void_p:      # (include/lap_hip.h: the stream is the last argument, a void*)
            monkeypatch.setitem(hip._fn, name, traced(name, fn))

    def record(run):
        del trace[:]
        run()
        torch.cuda.synchronize()
        rle = []
        for name in trace:
            if rle and rle[-1][0] == name:
                rle[-1][1] += 1
            else:
                rle.append([name, 1])
        return rle
    sample = lambda **kw: model.sample_actions(0, o, num_steps=3, noise=noise.to(DEV), **kw)
    out = {"chain": record(sample)}
    monkeypatch.setattr(model, "serve_euler_embed", False)
    out["chain_plain_tail"] = record(sample)
    monkeypatch.setattr(model, "serve_euler_embed", True)
    monkeypatch.setattr(model, "serve_chain", False)
    out["skinny"] = record(sample)
    out["partials"] = record(lambda: sample(fused="partials"))
    out["generic"] = record(lambda: sample(fused=False))
    out["tokens_eager"] = record(lambda: model.sample_tokens(0, o, max_decoding_steps=2, decode="eager"))
    assert not model.serve_chain_failed()
    return out


def test_serving_launch_trace_matches_fixture(hip, monkeypatch):
    """What a tolerance cannot see: a dropped, duplicated or reordered launch in the serving paths.  The ordered entry points of
    every denoise route and of the shared prefill equal tests/golden/serve_launch_trace.json, recorded with `_serve_launch_traces`
    on the commit before the sampler and the prefill moved out of model.py (a change that alters the launches on purpose records
    the fixture anew, with the reason)."""
    import json

    with open(os.path.join(os.path.dirname(__file__), "golden", "serve_launch_trace.json")) as f:
        want = json.load(f)
    got = _serve_launch_traces(hip, monkeypatch)
    assert set(got) == set(want)
    for route in want:
        assert got[route] == want[route], route
    names = lambda route: {n for n, _ in want[route]}
    assert "lap_serve_chain" in names("chain") and "lap_serve_final_euler_embed" in names("chain")      # the fixture holds the routes it names
    assert "lap_serve_final_euler" in names("chain_plain_tail") and "lap_serve_qkv_rope" in names("skinny")
    assert "lap_fused_reduce_geglu" in names("partials") and "lap_gated_residual_fwd" in names("generic")
    assert "lap_panel_gemm_pf" in names("tokens_eager") | names("chain")


def _train_launch_traces(hip, monkeypatch):
    """One `loss_and_grad` per route of the train step on a fresh model (`_full_width_cfg`, B = 2, ragged prompts, fixed noise and
    time, the loaders' `loss_rows_max` hint): every library entry point that takes a stream as [name, stream number, run length]
    (streams numbered by first appearance within the run: normally 0 the compute stream, 1 the suffix stream, 2 the weight-gradient
    stream; consecutive equal (name, stream) pairs run-length encoded) and, between them in issue order, the collective hooks as
    ["comm.<hook>", unit, streams in `also`].  Uses the public surface only (LAP(...), loss_and_grad, model.comm, model.ps, hip._fn):
    the recorder runs unchanged on the commit the fixture was recorded on."""
    import ctypes

    from lap_amd import config as C
    from lap_amd.model import LAP, _NullComm

    trace = []

    class RecordingComm(_NullComm):
        @staticmethod
        def _n(also):
            return 0 if also is None else (len(also) if isinstance(also, (list, tuple)) else 1)

        def wait_unit(self, name, also=None): trace.append(("comm.wait_unit", name, self._n(also)))
        def pace(self, name): trace.append(("comm.pace", name, 0))
        def grads_ready(self, name, also=None): trace.append(("comm.grads_ready", name, self._n(also)))
        def before_backward(self): trace.append(("comm.before_backward", "", 0))

    def traced(name, fn):
        def call(*a):
            s = a[-1]
            trace.append((name, int(getattr(s, "value", s) or 0)))
            return fn(*a)
        return call
    for name, fn in list(hip._fn.items()):
        sig = hip.SIGNATURES[name]
        if sig and sig[-1] is ctypes.c_void_p:      # (include/lap_hip.h: the stream is the last argument, a void*)
            monkeypatch.setitem(hip._fn, name, traced(name, fn))

    cfg = _full_width_cfg(monkeypatch)
    obs, actions, noise, time = make_inputs(cfg, B=2, ragged=True)
    # (the host-side hint the data loaders attach: with it the language head, and the last layer's prefix stream, run on the loss rows)
    o = dataclasses.replace(to_observation(obs, DEV), loss_rows_max=int(obs["tokenized_langact_mask"][:, 1:].sum(-1).max()))

    def record(cfg, setup=None, **kw):
        model = LAP(cfg, seed=5, device=DEV, comm=RecordingComm(), **kw)
        if setup is not None:
            setup(model)
        torch.cuda.synchronize()
        del trace[:]
        model.loss_and_grad(0, o, actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV))
        torch.cuda.synchronize()
        streams, rle = {}, []
        for ent in trace:
            if len(ent) == 3:
                rle.append(list(ent))
                continue
            sid = streams.setdefault(ent[1], len(streams))
            if rle and rle[-1][0] == ent[0] and rle[-1][1] == sid and not rle[-1][0].startswith("comm."):
                rle[-1][2] += 1
            else:
                rle.append([ent[0], sid, 1])
        return model, rle

    def one_stream(m):
        m.dual_stream, m.wgrad_stream = False, ""

    def all_rows(m):
        m.last_layer_rows = False

    record(cfg)     # the process-wide warm-up step (not recorded)
    out = {}
    model, out["pi05"] = record(cfg)
    assert model.last_rows_steps > 0      # the row-subset path is in the trace
    _, out["pi05_one_stream"] = record(cfg, one_stream)
    _, out["pi05_all_rows"] = record(cfg, all_rows)
    _, out["pi0"] = record(dataclasses.replace(cfg, pi05=False))
    model, out["prefix_frozen"] = record(cfg, lambda m: m.ps.set_frozen(cfg.get_vlm_freeze_filter()))
    assert model._prefix_frozen()
    _, out["lang_off"] = record(dataclasses.replace(cfg, enable_langact_training=False))
    _, out["action_off"] = record(dataclasses.replace(cfg, enable_action_training=False))
    monkeypatch.setitem(C._GEMMA, "gemma_2b_lora_x2", C.GemmaConfig(2048, 2, 16384, 8, 1, 256, lora_attn=(16, 16.0), lora_ffn=(16, 16.0)))
    monkeypatch.setitem(C._GEMMA, "gemma_300m_lora_x2", C.GemmaConfig(1024, 2, 4096, 8, 1, 256, lora_attn=(32, 32.0), lora_ffn=(32, 32.0)))
    _, out["lora"] = record(dataclasses.replace(cfg, paligemma_variant="gemma_2b_lora_x2", action_expert_variant="gemma_300m_lora_x2"))
    _, out["fp8"] = record(cfg, gemm_dtype="fp8")
    del model
    return out


def test_train_launch_trace_matches_fixture(hip, monkeypatch):
    """What a tolerance cannot see in the train step: a dropped join with the weight-gradient stream, a `comm.pace` that moved behind
    a GEMM, a weight gradient that left its stream.  The launches of one step, the stream of each and the collective hooks between
    them equal tests/golden/train_launch_trace.json on every route, recorded with `_train_launch_traces` on the commit before the
    joint layers, the SigLIP tower and the side streams moved out of model.py (a change that alters the launches on purpose records
    the fixture anew, with the reason)."""
    import json

    with open(os.path.join(os.path.dirname(__file__), "golden", "train_launch_trace.json")) as f:
        want = json.load(f)
    got = _train_launch_traces(hip, monkeypatch)
    assert set(got) == set(want)
    for route in want:
        assert got[route] == want[route], route
    launches = lambda route: [e for e in want[route] if not e[0].startswith("comm.")]
    names = lambda route: {e[0] for e in launches(route)}
    streams = lambda route: {e[1] for e in launches(route)}
    assert streams("pi05") == {0, 1, 2} and "lap_rope_split_fwd_rows" in names("pi05")      # the fixture holds the routes it names
    assert "lap_rope_split_fwd_rows" not in names("pi05_all_rows") and streams("pi05_one_stream") == {0}
    assert "lap_gated_residual_fwd" not in names("pi0") and "lap_gated_residual_fwd" in names("pi05")
    assert "lap_lora_down" in names("lora") and "lap_gemm_fp8" in names("fp8")
    ln_bwd = lambda route: {n for n in names(route) if n.startswith("lap_layernorm_bwd")}      # (SigLIP's: hip.layernorm_bwd)
    assert not ln_bwd("prefix_frozen") and ln_bwd("pi05")
    hooks = {e[0] for e in want["pi05"]} - names("pi05")
    assert hooks == {"comm.wait_unit", "comm.pace", "comm.grads_ready", "comm.before_backward"}


def _check_loss_activations_and_grads(cfg, B, ragged):
    oc = oracle_cfg(cfg)
    P = O.init_params(oc, seed=7)
    obs, actions, noise, time = make_inputs(cfg, B=B, ragged=ragged)
    # ---- oracle: f32 with autograd, and bf16-emulating forward
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    col32 = {}
    loss32, m32 = O.compute_loss(Pg, oc, obs, actions, noise, time, collect=col32)
    loss32.backward()
    col16 = {}
    loss16, _ = O.compute_loss(P, dataclasses.replace(oc, emulate_bf16=True), obs, actions, noise, time, collect=col16)
    # ---- engine
    model = _engine(cfg, P)
    col = {}
    for g in model.ps.grad.values():
        g.zero_()
    loss, metrics = model.loss_and_grad(0, to_observation(obs, DEV), actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV), collect=col)
    torch.cuda.synchronize()
    ref_noise = abs(loss16.item() - loss32.item()) / abs(loss32.item())
    assert abs(loss.item() - loss32.item()) / abs(loss32.item()) < max(3 * ref_noise, 5e-3), (loss.item(), loss32.item(), loss16.item())
    assert rel(col["per_sample_action"], m32["per_sample_action"]) < 2e-2
    assert rel(col["per_sample_lang"], m32["per_sample_lang"]) < 2e-2
    # activations at valid positions (padding rows are never consumed: SURVEY §8 a-bis)
    L = cfg.max_token_len
    Pn = model.n_img_tok * len(cfg.image_keys) + L
    pm = torch.cat([obs["image_masks"][k][:, None].expand(B, model.n_img_tok) for k in cfg.image_keys] + [obs["tokenized_prompt_mask"]], 1)
    last = oc.vlm.depth - 1
    x0 = col["x0_out"].view(B, Pn, -1).float().cpu()
    e32, e16 = col32[f"llm/layer{last:02d}/x0"], col16[f"llm/layer{last:02d}/x0"]
    err, base = rel(x0[pm], e32[pm]), rel(e16[pm], e32[pm])
    assert err < max(3 * base, 1e-2), (err, base)
    x1 = col["x1_out"].view(B, cfg.action_horizon, -1).float().cpu()
    err1, base1 = rel(x1, col32[f"llm/layer{last:02d}/x1"]), rel(col16[f"llm/layer{last:02d}/x1"], col32[f"llm/layer{last:02d}/x1"])
    assert err1 < max(3 * base1, 1e-2), (err1, base1)
    assert rel(col["v_t"], m32["v_t"]) < 2e-2
    _per_layer_sweep(cfg, oc, col, col32, col16, B, pm)
    _teacher_forced_sweep(model, cfg, oc, obs, col, col16, B, pm)
    # ---- every parameter gradient, mapped back to the reference's tree layout
    from lap_amd.params import engine_to_reference

    eng = {name: model.ps.g(name).detach().float().cpu() for name in model.ps.names()}
    gref = engine_to_reference(cfg, eng)
    worst = {}
    for k, g32 in ((k, v.grad) for k, v in Pg.items()):
        if g32 is None:
            continue
        r = rel(gref[k], g32)
        worst[k] = r
        # bf16 backward: 5e-2 relative L2 per tensor; tiny-norm tensors compared absolutely
        assert r < 5e-2 or (gref[k] - g32).abs().max() < 1e-4, (k, r)
    assert len(worst) == len(P)


def _check_loss_branch(cfg, B, ragged, min_untouched=1):
    """compute_loss with one of the two losses switched off (lap.py:426-462,557-596) against the f32 oracle's autograd: loss,
    per-sample losses, the last layer's activations, every gradient.  Parameters the branch never touches (the action expert,
    the action / time projections and the adaRMS bank without action training; the final norm without the language loss) have
    no gradient in the oracle: the engine must leave exactly zeros there (the optimizer then applies weight decay only, as optax
    does with a zero gradient)."""
    oc = oracle_cfg(cfg)
    P = O.init_params(oc, seed=11)
    obs, actions, noise, time = make_inputs(cfg, B=B, ragged=ragged)
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    col32 = {}
    loss32, m32 = O.compute_loss(Pg, oc, obs, actions, noise, time, collect=col32)
    loss32.backward()
    loss16, _ = O.compute_loss(P, dataclasses.replace(oc, emulate_bf16=True), obs, actions, noise, time)
    model = _engine(cfg, P)
    col = {}
    for g in model.ps.grad.values():
        g.zero_()
    loss, metrics = model.loss_and_grad(0, to_observation(obs, DEV), actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV), collect=col)
    torch.cuda.synchronize()
    ref_noise = abs(loss16.item() - loss32.item()) / abs(loss32.item())
    assert abs(loss.item() - loss32.item()) / abs(loss32.item()) < max(3 * ref_noise, 5e-3), (loss.item(), loss32.item(), loss16.item())
    # the forward-only entry point (nothing saved: the unfused GeGLU route, other rounding points than the training forward)
    loss_f, _ = model.compute_loss(0, to_observation(obs, DEV), actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV))
    assert abs(loss_f.item() - loss.item()) < 1e-3 * max(1.0, abs(loss.item())), (loss_f.item(), loss.item())
    if cfg.enable_langact_training:
        assert rel(col["per_sample_lang"], m32["per_sample_lang"]) < 2e-2
    else:
        assert float(col["per_sample_lang"].abs().max()) == 0.0 and float(metrics["lang_loss"]) == 0.0
    if cfg.enable_action_training:
        assert rel(col["per_sample_action"], m32["per_sample_action"]) < 2e-2
        assert rel(col["v_t"], m32["v_t"]) < 2e-2
    else:
        assert col["x1_out"] is None and float(col["per_sample_action"].abs().max()) == 0.0
    L = cfg.max_token_len
    Pn = model.n_img_tok * len(cfg.image_keys) + L
    pm = torch.cat([obs["image_masks"][k][:, None].expand(B, model.n_img_tok) for k in cfg.image_keys] + [obs["tokenized_prompt_mask"]], 1)
    last = oc.vlm.depth - 1
    x0 = col["x0_out"].view(B, Pn, -1).float().cpu()
    assert rel(x0[pm], col32[f"llm/layer{last:02d}/x0"][pm]) < 2e-2
    # (the full key map: without action training the reference's tree — and `engine_to_reference` — has no action expert at all,
    #  lap.py:64-74; the engine still holds its tensors, unused, and their gradients must stay exact zeros)
    from lap_amd.params import _engine_to_reference_full, engine_to_reference, _is_action_expert_key

    eng = {name: model.ps.g(name).detach().float().cpu() for name in model.ps.names()}
    gref = _engine_to_reference_full(cfg, eng)
    exported = engine_to_reference(cfg, eng)
    assert set(exported) == {k for k in gref if cfg.enable_action_training or not _is_action_expert_key(k)}
    checked = untouched = 0
    for k, v in Pg.items():
        if v.grad is None or float(v.grad.abs().max()) == 0.0:
            assert float(gref[k].abs().max()) == 0.0, (k, float(gref[k].abs().max()))      # untouched by this branch: exactly zero
            untouched += 1
            continue
        r = rel(gref[k], v.grad)
        # (SigLIP's key bias has an analytically zero gradient — softmax is shift invariant —: f32 rounding noise in the oracle, bf16 noise here)
        assert r < 5e-2 or (gref[k] - v.grad).abs().max() < (4e-4 if k.endswith("key/bias") else 1e-4), (k, r)
        checked += 1
    assert checked > 10 and untouched >= min_untouched, (checked, untouched)
    if cfg.enable_action_training:      # the action expert's residual stream behind the last layer (pi0: state token + action tokens)
        x1 = col["x1_out"].view(B, -1, oc.expert.width).float().cpu()
        assert x1.shape == col32[f"llm/layer{last:02d}/x1"].shape
        assert rel(x1, col32[f"llm/layer{last:02d}/x1"]) < 2e-2
    return checked, untouched


@pytest.mark.parametrize("act,lang", [(False, True), (True, False)])
def test_loss_branches_with_one_loss_off_match_oracle(hip, act, lang):
    """enable_action_training=False: `llm([prefix])`, cross entropy only (the vla0_* configs); enable_langact_training=False:
    both streams, flow matching only (pi0_replicated).  Debug model, ragged batch with an idle sample and an invalid image."""
    _check_loss_branch(debug_model_cfg(enable_action_training=act, enable_langact_training=lang), B=3, ragged=True)


@pytest.mark.parametrize("lang", [True, False])
def test_pi0_suffix_path_matches_oracle(hip, lang):
    """`pi05=False` (lap.py:46-61 + openpi Pi0.embed_suffix): a state token through `state_proj`, the action tokens mixed with the time
    embedding through `action_time_mlp_*`, plain RMSNorms and residuals in the action expert (`use_adarms=[False, False]`), the action
    head on the last S suffix rows.  Loss, per-sample losses, both residual streams and every gradient against the f32 oracle's
    autograd, with and without the language loss; then the sampler (state token re-embedded at every Euler step)."""
    cfg = debug_model_cfg(pi05=False, enable_action_training=True, enable_langact_training=lang)
    checked, untouched = _check_loss_branch(cfg, B=3, ragged=True, min_untouched=0 if lang else 1)
    assert checked > 25
    oc = oracle_cfg(cfg)
    P = O.init_params(oc, seed=11)
    assert "state_proj/kernel" in P and "time_mlp_in/kernel" not in P and "PaliGemma/llm/final_norm_1/scale" in P
    obs, _, noise, _ = make_inputs(cfg, B=2, ragged=True)
    so = {k: v for k, v in obs.items() if k != "tokenized_langact_mask"}
    col32, col = {}, {}
    ref = O.sample_actions(P, oc, so, noise, num_steps=10, collect=col32)
    ref16 = O.sample_actions(P, dataclasses.replace(oc, emulate_bf16=True), so, noise, num_steps=10)
    model = _engine(cfg, P)
    out = model.sample_actions(0, to_observation(so | {"tokenized_langact_mask": None}, DEV), num_steps=10, noise=noise.to(DEV), collect=col)
    assert out.shape == (2, cfg.action_horizon, cfg.action_dim)
    assert rel(col["v_t/0"], col32["v_t/0"]) < 2e-2
    err, base = rel(out, ref), rel(ref16, ref)
    assert err < max(3 * base, 1e-2), (err, base)


@pytest.mark.parametrize("act,lang,kw", [
    (False, True, dict(max_token_len=180, action_horizon=10, action_dim=7, language_loss_weight=1.0)),      # vla0_replicated_libero shapes
    (True, False, dict(max_token_len=48, action_horizon=16, action_dim=7)),                                 # pi0_replicated: S = 16
])
def test_full_width_loss_branches_match_oracle(hip, monkeypatch, act, lang, kw):
    """The same two branches at the LAP-3B widths (2 layers per tower): prefix-only attention backward on the LDS-DMA kernels
    with an empty suffix segment; prefix gradients that arrive through the action queries' keys / values only."""
    _check_loss_branch(_full_width_cfg(monkeypatch, enable_action_training=act, enable_langact_training=lang, **kw), B=2, ragged=True)


def test_full_width_pi0_matches_oracle(hip, monkeypatch):
    """pi0 at the LAP-3B widths (2 layers per tower; S + 1 = 51 suffix rows per sample at width 1024 / head size 256): the expert's plain
    norms, residual epilogues and the state token on the production kernels; loss, both streams, every gradient."""
    checked, _ = _check_loss_branch(_full_width_cfg(monkeypatch, pi05=False, action_dim=7), B=2, ragged=True, min_untouched=0)
    assert checked > 25


# Per-layer bounds (relative L2 over valid positions), stated once.  Measured on MI355X (round 2, LAP-3B
# full depth, gpurun_out/r2_par1.log): the bf16-emulating oracle itself sits 1.7e-3 (stem) ... 1.3e-2 (SigLIP block 26)
# ... 1.8e-2 (Gemma layer 17) from the f32 oracle, the engine 0.85-1.0x of that, and the two bf16 implementations are as
# far from each other as each is from f32: one bf16 rounding is 2^-9 relative, a flipped rounding is carried and amplified
# by every layer above it, so two FREE-RUNNING bf16 implementations decorrelate within a few layers.
#   * free-running, every layer, against the f32 oracle: the engine must not be further from it than 1.5x the bf16 oracle
#     is (floor 3e-3);  against the bf16 oracle: not further than 1.5x the bf16 oracle's own distance to f32 (same floor);
#   * TEACHER-FORCED, every layer (the tight per-layer statement): the engine's layer l is fed the bf16 oracle's
#     layer l-1 output and its result is compared with the bf16 oracle's layer l — only the rounding flips of ONE layer
#     remain.  Measured: joint Gemma layers 2.8-4.0e-3 (prefix stream) / 0.5-1.2e-3 (action stream), SigLIP blocks
#     4.3-5.6e-3 (the reference rounds the SigLIP attention logits and probabilities to bf16 [FLAX-RECALL]; the engine keeps
#     them in f32, i.e. it is closer to the f32 oracle there than the bf16 oracle is).  Bounds: TEACHER_FORCED_BOUND.
FREE_RUN_RATIO, FREE_RUN_FLOOR = 1.5, 3e-3
TEACHER_FORCED_BOUND = {"img": 7e-3, "llm": 5e-3}


def _sweep_keys(oc):
    keys = ["img/stem"] + [f"img/block{l:02d}" for l in range(oc.img.depth)] + ["img/out"]
    return keys + [f"llm/layer{l:02d}/x{i}" for l in range(oc.vlm.depth) for i in (0, 1)]


def _per_layer_sweep(cfg, oc, col, col32, col16, B, pm, report=None):
    """EVERY collected activation (SigLIP stem / blocks / output of the first image key, both streams of every joint
    Gemma layer) of the free-running engine against both oracle modes."""
    T = (cfg.image_size // oc.img.patch) ** 2
    S = cfg.action_horizon
    Pn = pm.shape[1]
    worst16 = worst32 = 0.0
    for k in _sweep_keys(oc):
        e = col[k].float().cpu()
        if k.startswith("img/"):
            e = e.view(-1, T, e.shape[-1])[:B]      # engine runs all image keys as one batch, key-major
            a32, a16 = col32[k], col16[k]           # SigLIP has no mask: every image is encoded
        elif k.endswith("x0"):
            e = e.view(B, Pn, -1)[pm]
            a32, a16 = col32[k][pm], col16[k][pm]
        else:
            e = e.view(B, S, -1)
            a32, a16 = col32[k], col16[k]
        err32, base, err16 = rel(e, a32), rel(a16, a32), rel(e, a16)
        if report is not None:
            report.append((k, err32, base, err16))
        if os.environ.get("LAP_PARITY_REPORT"):       # measurement mode (tools / DESIGN.md tables): print, do not judge
            print(f"  {k:22s} engine-f32 {err32:.2e}  bf16oracle-f32 {base:.2e}  engine-bf16oracle {err16:.2e}")
            continue
        lim = max(FREE_RUN_RATIO * base, FREE_RUN_FLOOR)
        assert err32 < lim, (k, err32, base)
        assert err16 < lim, (k, err16, base)
        worst16, worst32 = max(worst16, err16), max(worst32, err32)
    return worst16, worst32


def _teacher_forced_sweep(model, cfg, oc, obs, col, col16, B, pm, report=None):
    """Layer by layer: engine(layer l)(bf16 oracle's input of layer l) vs the bf16 oracle's output of layer l, for every
    SigLIP block (first image key) and every joint Gemma layer (both streams), at valid positions."""
    from lap_amd.joint_layers import llm_fwd
    from lap_amd.siglip import siglip_fwd

    T = (cfg.image_size // oc.img.patch) ** 2
    S = cfg.action_horizon
    Pn = pm.shape[1]
    dev = model.device
    bf = lambda t: t.to(torch.bfloat16).to(dev).contiguous()
    worst = 0.0

    def check(k, got, want):
        nonlocal worst
        err = rel(got, want)
        if report is not None:
            report.append((k, err))
        if os.environ.get("LAP_PARITY_REPORT"):
            print(f"  teacher-forced {k:22s} engine-bf16oracle {err:.2e}")
        else:
            assert err < TEACHER_FORCED_BOUND[k[:3]], (k, err)
        worst = max(worst, err)

    prev = col16["img/stem"]
    for l in range(oc.img.depth):
        out, _ = siglip_fwd(model, None, False, x_in=bf(prev).view(B * T, -1), blocks=[l])
        want = col16[f"img/block{l:02d}"]
        check(f"img/block{l:02d}", out.float().cpu().view(B, T, -1), want)
        prev = want
    qinfo, kinfo, pos = model._train_infos(to_observation(obs, dev), S)
    mod = col["mod"]
    x0p, x1p = col16["llm/in0"], col16["llm/in1"]
    for l in range(oc.vlm.depth):
        x0, x1, _ = llm_fwd(model, bf(x0p).view(B * Pn, -1), bf(x1p).view(B * S, -1), mod, pos, qinfo, kinfo, B, Pn, S, False, layers=[l])
        w0, w1 = col16[f"llm/layer{l:02d}/x0"], col16[f"llm/layer{l:02d}/x1"]
        check(f"llm/layer{l:02d}/x0", x0.float().cpu().view(B, Pn, -1)[pm], w0[pm])
        check(f"llm/layer{l:02d}/x1", x1.float().cpu().view(B, S, -1), w1)
        x0p, x1p = w0, w1
    return worst


def test_full_depth_lap3b_forward_and_sampler_match_oracle(hip):
    """The real LAP-3B: SigLIP So400m/14 (27 blocks) + Gemma-2B / Gemma-300M (18 joint layers), 257,152-word vocabulary,
    action_dim 7, BASELINE.json shapes (2 x 224 x 224 images, 48-token prompt, 50-step chunk), batch 1, random-init
    weights in the reference's tree layout.  Forward loss with EVERY layer's activations and the batch-1 sampler
    (prefill + 10 denoise steps) against both oracle modes.  CPU oracle time: a few minutes."""
    import time as _t

    from lap_amd.config import get_config

    cfg = get_config("lap_bench").model
    oc = oracle_cfg(cfg)
    nthr = torch.get_num_threads()
    torch.set_num_threads(min(32, nthr))    # torch-CPU matmuls stop scaling (and get slower) far beyond that
    try:
        t0 = _t.perf_counter()
        P = O.init_params(oc, seed=21)
        obs, actions, noise, time = make_inputs(cfg, B=1, ragged=True)
        col32, col16 = {}, {}
        with torch.no_grad():
            loss32, m32 = O.compute_loss(P, oc, obs, actions, noise, time, collect=col32)
            oc16 = dataclasses.replace(oc, emulate_bf16=True)
            loss16, _ = O.compute_loss(P, oc16, obs, actions, noise, time, collect=col16)
            so = {k: v for k, v in obs.items() if k != "tokenized_langact_mask"}
            ref = O.sample_actions(P, oc, so, noise, num_steps=10)
            ref16 = O.sample_actions(P, oc16, so, noise, num_steps=10)
        t_oracle = _t.perf_counter() - t0
    finally:
        torch.set_num_threads(nthr)
    from lap_amd.model import LAP

    model = LAP(cfg, params=P, device=DEV, with_grads=False)
    del P
    col = {}
    loss, _ = model.compute_loss(0, to_observation(obs, DEV), actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV), collect=col)
    torch.cuda.synchronize()
    ref_noise = abs(loss16.item() - loss32.item()) / abs(loss32.item())
    assert abs(loss.item() - loss32.item()) / abs(loss32.item()) < max(3 * ref_noise, 5e-3), (loss.item(), loss32.item(), loss16.item())
    pm = torch.cat([obs["image_masks"][k][:, None].expand(1, model.n_img_tok) for k in cfg.image_keys] + [obs["tokenized_prompt_mask"]], 1)
    report = []
    w16, w32 = _per_layer_sweep(cfg, oc, col, col32, col16, 1, pm, report=report)
    wtf = _teacher_forced_sweep(model, cfg, oc, obs, col, col16, 1, pm)
    assert rel(col["per_sample_lang"], m32["per_sample_lang"]) < 2e-2 and rel(col["per_sample_action"], m32["per_sample_action"]) < 2e-2
    o = to_observation(so | {"tokenized_langact_mask": None}, DEV)
    out = model.sample_actions(0, o, num_steps=10, noise=noise.to(DEV))
    assert model.serve_chain and model._chain_ctr is not None       # the 18 expert layers of a step ran as ONE launch (serve_chain.hpp) ...
    model.serve_chain = False
    assert torch.equal(out, model.sample_actions(0, o, num_steps=10, noise=noise.to(DEV)))     # ... bit-equal to 6 launches per layer
    model.serve_chain = True
    assert not model.serve_chain_failed()
    generic = model.sample_actions(0, o, num_steps=10, noise=noise.to(DEV), fused=False)
    assert torch.equal(generic, model.sample_actions(0, o, num_steps=10, noise=noise.to(DEV), fused="partials"))
    err, base = rel(out, ref), rel(ref16, ref)
    assert rel(generic, ref) < max(FREE_RUN_RATIO * base, 5e-3) and rel(out, generic) < max(FREE_RUN_RATIO * base, 5e-3)
    # BASELINE config 4 at the real size: the hipGraph-captured sampler replays to the eager sampler's bits (twice: no state leak)
    from lap_amd.serve import GraphedSampler

    gs = GraphedSampler(model, 1, 10).capture()
    g1 = gs(o, noise.to(DEV)).clone()
    g2 = gs(o, noise.to(DEV)).clone()
    assert torch.equal(g1, out) and torch.equal(g2, out)
    del gs
    print(f"full depth: oracle {t_oracle:.0f} s; loss {loss.item():.5f} / f32 {loss32.item():.5f} / bf16 {loss16.item():.5f}; "
          f"free-running worst layer vs bf16 oracle {w16:.2e}, vs f32 {w32:.2e}; teacher-forced worst layer {wtf:.2e}; "
          f"sampler {err:.2e} (bf16 oracle {base:.2e})")
    for k, e32, b, e16 in report[::6]:
        print(f"  {k:22s} engine-f32 {e32:.2e}  bf16oracle-f32 {b:.2e}  engine-bf16oracle {e16:.2e}")
    assert out.shape == (1, 50, 7) and err < max(FREE_RUN_RATIO * base, 5e-3), (err, base)


# the reference's own TrainConfig shapes at FULL depth (VERDICT r5 next #4a): training/config.py:752-785 `lap_libero` (P = 180, S = 10) and
# :608-619 `lap` (P = 180, S = 16, language weight 1.0, stop_action_to_vlm_grad=True) next to the benchmark's synthetic shapes
_FULL_DEPTH_SHAPES = {
    "lap_bench": {},
    "lap_libero": dict(max_token_len=180, action_horizon=10, action_dim=7, language_loss_weight=0.4, stop_action_to_vlm_grad=False),
    "lap": dict(max_token_len=180, action_horizon=16, action_dim=7, language_loss_weight=1.0, stop_action_to_vlm_grad=True),
}


@pytest.mark.parametrize("shapes", list(_FULL_DEPTH_SHAPES))
def test_full_depth_lap3b_training_gradients_match_oracle(hip, shapes):
    """The real LAP-3B (27 + 18 layers, 257,152-word vocabulary), B = 2, `loss_and_grad` on the DEFAULT schedule (action expert
    on the second stream, SigLIP weight / bias gradients on the third) against the f32 oracle's autograd: the loss, both
    per-sample losses and EVERY gradient tensor of the reference's tree (scripts/train.py:329-361).  The 2-layer slices cover
    every kernel shape; this covers the full-depth backward — the activation stash of 45 layers, the stream schedule and the
    accumulation of 18 + 27 layers of rounding noise into the early layers' gradients (bound: the slices' 5e-2 per tensor)."""
    import time as _t

    from lap_amd.config import get_config
    from lap_amd.model import LAP
    from lap_amd.params import engine_to_reference

    cfg = dataclasses.replace(get_config("lap_bench").model, **_FULL_DEPTH_SHAPES[shapes])
    oc = oracle_cfg(cfg)
    B = 2
    nthr = torch.get_num_threads()
    torch.set_num_threads(min(32, nthr))
    try:
        t0 = _t.perf_counter()
        P = O.init_params(oc, seed=23)
        obs, actions, noise, time = make_inputs(cfg, B=B, ragged=True)
        Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
        loss32, m32 = O.compute_loss(Pg, oc, obs, actions, noise, time)
        loss32.backward()
        g32 = {k: v.grad for k, v in Pg.items()}
        del Pg
        t_oracle = _t.perf_counter() - t0
    finally:
        torch.set_num_threads(nthr)
    model = LAP(cfg, params=P, device=DEV)
    del P
    assert model.dual_stream and model.wgrad_stream == "sb"          # the defaults bench.py runs with
    for g in model.ps.grad.values():
        g.zero_()
    col = {}
    loss, _ = model.loss_and_grad(0, to_observation(obs, DEV), actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV), collect=col)
    torch.cuda.synchronize()
    assert abs(loss.item() - loss32.item()) / abs(loss32.item()) < 5e-3, (loss.item(), loss32.item())
    assert rel(col["per_sample_action"], m32["per_sample_action"]) < 2e-2 and rel(col["per_sample_lang"], m32["per_sample_lang"]) < 2e-2
    gref = engine_to_reference(cfg, {name: model.ps.g(name).detach().float().cpu() for name in model.ps.names()})
    worst = []
    for k, g in g32.items():
        if g is None:
            continue
        r = rel(gref[k], g)
        worst.append((r, k))
        assert r < 5e-2 or (gref[k] - g).abs().max() < 1e-4, (k, r)
    worst.sort(reverse=True)
    assert len(worst) == len(g32)
    print(f"full-depth training parity [{shapes}]: oracle {t_oracle:.0f} s; loss {loss.item():.5f} vs f32 {loss32.item():.5f}; {len(worst)} gradient "
          f"tensors, worst relative L2: " + ", ".join(f"{k.split('PaliGemma/')[-1]} {r:.1e}" for r, k in worst[:4]))


def test_full_size_train_steps_do_not_depend_on_the_stream_schedule(hip, monkeypatch):
    """Three consecutive LAP-3B train steps at B = 32 (the benchmark's step: forward, backward, clip, AdamW, EMA) on the default
    schedule — second stream, third stream, optimizer paced under the next forward's GEMMs — against everything on one stream
    with the whole optimizer pass enqueued at once.  Step 0's loss is bit-equal (the forward does not depend on the schedule);
    later losses see parameters whose gradients carried f32-atomics-order noise in a handful of small tensors (norm scales,
    modulation, biases: free in BOTH schedules, `test_two_stream_schedule_equals_one_stream`), so they are compared to the
    spread two identical one-stream runs show between themselves."""
    import dataclasses as dc

    from lap_amd.config import get_config
    from lap_amd.train import SyntheticDataLoader, TrainingStepRunner, init_train_state

    tc = dc.replace(get_config("lap_bench"), batch_size=32, seed=3)

    def run(env):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        state = init_train_state(tc, device=DEV)
        runner = TrainingStepRunner(tc)
        it = iter(SyntheticDataLoader(tc.model, 32, DEV, seed=5))
        losses = []
        for step in range(3):
            state, info = runner(tc.seed, state, next(it), step)
            losses.append(info["loss"].item())
        torch.cuda.synchronize()
        del state
        torch.cuda.empty_cache()
        return losses

    one = {"LAP_DUAL_STREAM": "0", "LAP_WGRAD_STREAM": "0", "LAP_OPT_PACE": "top", "LAP_OPT_LOOKAHEAD": "0"}
    dflt = {"LAP_DUAL_STREAM": "1", "LAP_WGRAD_STREAM": "sb", "LAP_OPT_PACE": "gemm", "LAP_OPT_LOOKAHEAD": "9"}
    a, a2, b = run(one), run(one), run(dflt)
    assert a[0] == a2[0] == b[0], (a, a2, b)
    spread = max(abs(x - y) / abs(x) for x, y in zip(a[1:], a2[1:]))
    for x, y in zip(a[1:], b[1:]):
        # (floor: two identical one-stream runs differ by up to ~1e-5 of the step-2 loss — f32 atomics order in the small tensors'
        # gradients and in the gradient norm's partial sums — but sometimes by nothing at all, which must not turn that into the bound)
        assert abs(x - y) / abs(x) <= max(4 * spread, 4e-5), (a, a2, b)
    print(f"3 steps at B=32: one stream {a} / again {a2} / default schedule {b}")


def test_language_head_on_loss_rows_only_equals_all_rows(hip):
    """`CoTObservation.loss_rows_max` (host hint): the language head runs on the loss-carrying rows only (lap.py:221-260 computes
    every row and multiplies by the mask).  Every kept row's logits are the same GEMM rows, so losses and metrics agree to the
    f32 summation order of the per-sample sums (1e-6), gradients to that of the head's weight gradient (fewer zero rows in
    its contraction); a hint below a sample's count poisons the loss with NaN instead of dropping tokens."""
    import dataclasses as dc

    cfg = debug_model_cfg()
    oc = oracle_cfg(cfg)
    P = O.init_params(oc, seed=19)
    obs, actions, noise, time = make_inputs(cfg, B=3, ragged=True)
    model = _engine(cfg, P)
    o = to_observation(obs, DEV)
    lmask = (obs["tokenized_langact_mask"] & obs["tokenized_prompt_mask"] & obs["token_loss_mask"])[:, 1:]
    n_max = int(lmask.sum(-1).max())
    assert 0 < n_max < cfg.max_token_len - 1

    def run(ob):
        for g in model.ps.grad.values():
            g.zero_()
        col = {}
        loss, met = model.loss_and_grad(0, ob, actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV), collect=col)
        torch.cuda.synchronize()
        return loss.clone(), {k: v.clone() for k, v in met.items()}, col["per_sample_lang"].clone(), {n: model.ps.g(n).detach().clone() for n in model.ps.names()}

    l_all, m_all, ps_all, g_all = run(o)
    for hint in (n_max, n_max + 3):
        l_sel, m_sel, ps_sel, g_sel = run(dc.replace(o, loss_rows_max=hint))
        close = lambda a, b: torch.allclose(a, b, rtol=2e-6, atol=1e-7)
        assert close(l_sel, l_all) and close(ps_sel, ps_all) and all(close(m_sel[k], m_all[k]) for k in m_all)
        for n in g_all:
            assert torch.equal(g_sel[n], g_all[n]) or rel(g_sel[n], g_all[n]) < 2e-5, n
    l_bad, _, _, _ = run(dc.replace(o, loss_rows_max=n_max - 1))
    assert torch.isnan(l_bad)
    # from_dict derives the hint from host-side masks
    from lap_amd.observation import CoTObservation

    d = {"image": {k: v.numpy() for k, v in obs["images"].items()}, "image_mask": {k: v.numpy() for k, v in obs["image_masks"].items()},
         "tokenized_prompt": obs["tokenized_prompt"].numpy(), "tokenized_prompt_mask": obs["tokenized_prompt_mask"].numpy(),
         "tokenized_langact_mask": obs["tokenized_langact_mask"].numpy(), "token_loss_mask": obs["token_loss_mask"].numpy()}
    assert CoTObservation.from_dict(d, device="cpu").loss_rows_max == n_max


def test_language_head_in_several_vocab_chunks_equals_one_chunk(hip, monkeypatch):
    """The language head over two vocabulary chunks (`loss.vocab_chunks` capped at 1024 of 2048 columns) against one chunk, forward
    and backward, with the verbose argmax carried across the chunks.  The logits are the same GEMM columns and the cross-entropy
    kernel's running max, sum and argmax are exact across column splits, so predictions and integer metrics are equal; losses agree
    to the f32 summation order (the bound of the rows-only test); the table's gradient is exact (each row lies in one chunk), the
    data gradient sums two products in f32 instead of one."""
    from lap_amd import loss as loss_mod

    cfg = debug_model_cfg(vocab_size=2048, verbose_mode=True)
    P = O.init_params(oracle_cfg(cfg), seed=29)
    obs, actions, noise, time = make_inputs(cfg, B=3, ragged=True)
    model = _engine(cfg, P)
    o = to_observation(obs, DEV)
    seen = []

    def run():
        for g in model.ps.grad.values():
            g.zero_()
        col = {}
        loss, met = model.loss_and_grad(0, o, actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV), collect=col)
        torch.cuda.synchronize()
        return (loss.clone(), {k: v.clone() for k, v in met.items()}, {k: col[k].clone() for k in ("per_sample_lang", "predictions")},
                {n: model.ps.g(n).detach().clone() for n in model.ps.names()})

    one_chunk = loss_mod.vocab_chunks

    def two_chunks(R, V):
        seen.append(one_chunk(R, V, cap_cols=1024))
        return seen[-1]

    l1, m1, c1, g1 = run()
    assert len(one_chunk(3 * (cfg.max_token_len - 1), cfg.vocab_size)) == 1
    monkeypatch.setattr(loss_mod, "vocab_chunks", two_chunks)
    l2, m2, c2, g2 = run()
    assert seen == [[(0, 1024), (1024, 1024)]]
    assert torch.equal(c2["predictions"], c1["predictions"])
    close = lambda a, b: torch.allclose(a, b, rtol=2e-6, atol=1e-7)
    print(f"loss {l1.item()!r} / {l2.item()!r}; per_sample_lang diff {(c2['per_sample_lang'] - c1['per_sample_lang']).abs().max().item():.3e}")
    assert close(l2, l1) and close(c2["per_sample_lang"], c1["per_sample_lang"])
    assert set(m1) == set(m2)
    for k in m1:
        if not m1[k].dtype.is_floating_point or k.startswith("per_sample_") and k.endswith(("_correct", "_total")) or k == "labels":
            assert torch.equal(m2[k], m1[k]), k       # counts and labels
        else:
            assert close(m2[k], m1[k]), k
    for n in g1:
        print(f"grad {n}: equal {torch.equal(g2[n], g1[n])} rel {rel(g2[n], g1[n]):.3e}")
        assert torch.equal(g2[n], g1[n]) or rel(g2[n], g1[n]) < 2e-5, n


def test_graphed_sampler_replay_equals_eager_and_oracle(hip):
    """BASELINE config 4: the hipGraph-captured batch-1 sampler (serve.GraphedSampler).  Capture once, replay for two
    DIFFERENT requests: every replay must equal the eager sampler bit for bit (same kernels, same order) and agree
    with the oracle; a second replay of the first request must reproduce the first result (no state leaks between replays)."""
    from lap_amd.serve import GraphedSampler

    cfg = debug_model_cfg()
    oc = oracle_cfg(cfg)
    P = O.init_params(oc, seed=17)
    model = _engine(cfg, P)
    sampler = GraphedSampler(model, 1, 10).capture()
    outs = []
    for seed in (1, 2, 1):
        obs, _, noise, _ = make_inputs(cfg, B=1, ragged=False, seed=seed)
        so = {k: v for k, v in obs.items() if k != "tokenized_langact_mask"}
        o = to_observation(so | {"tokenized_langact_mask": None}, DEV)
        got = sampler(o, noise.to(DEV)).clone()
        eager = model.sample_actions(0, o, num_steps=10, noise=noise.to(DEV))
        assert torch.equal(got, eager), seed
        ref = O.sample_actions(P, oc, so, noise, num_steps=10)
        ref16 = O.sample_actions(P, dataclasses.replace(oc, emulate_bf16=True), so, noise, num_steps=10)
        err, base = rel(got, ref), rel(ref16, ref)
        assert err < max(3 * base, 1e-2), (seed, err, base)
        outs.append(got)
    assert torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[1])


def test_graphed_sampler_follows_parameter_updates_at_full_width(hip, monkeypatch):
    """The captured sampler holds the ADDRESSES of parameter-derived images: the adaRMS modulations, the packed expert weights of the
    denoise chain and (round 6) the packed SigLIP weights of the row-panel prefill kernels.  After the parameters change they must be
    rebuilt in place before the next replay (GraphedSampler.__call__ -> refresh_serve_caches): replay == eager before and after an
    update, at the LAP-3B widths (where the panel kernels, the one-launch denoise step and — action_dim 7 — the fused Euler tail run)."""
    from lap_amd.serve import GraphedSampler

    cfg = _full_width_cfg(monkeypatch, action_dim=7)
    oc = oracle_cfg(cfg)
    P = O.init_params(oc, seed=5)
    obs, _, noise, _ = make_inputs(cfg, B=1, ragged=False)
    so = {k: v for k, v in obs.items() if k != "tokenized_langact_mask"}
    o = to_observation(so | {"tokenized_langact_mask": None}, DEV)
    model = _engine(cfg, P)
    sampler = GraphedSampler(model, 1, 10).capture()
    assert model.serving_cache.entries("panel") and model.serving_cache.entries("chain") and model.serve_euler_embed      # the paths this test is about are live
    out1 = sampler(o, noise.to(DEV)).clone()
    assert torch.equal(out1, model.sample_actions(0, o, num_steps=10, noise=noise.to(DEV)))
    with torch.no_grad():
        for name in model.ps.master:
            model.ps.master[name].mul_(1.03)
    model.ps.refresh_mirror_local()                      # bf16 mirrors follow the masters; ParamStore.version moves
    out2 = sampler(o, noise.to(DEV)).clone()
    eager2 = model.sample_actions(0, o, num_steps=10, noise=noise.to(DEV))
    assert torch.equal(out2, eager2)
    assert not torch.equal(out1, out2) and bool(torch.isfinite(out2).all())
    # ... and against a model that held the new parameters from the start (nothing stale survives anywhere)
    fresh = _engine(cfg, P)
    with torch.no_grad():
        for name in fresh.ps.master:
            fresh.ps.master[name].mul_(1.03)
    fresh.ps.refresh_mirror_local()
    assert torch.equal(out2, fresh.sample_actions(0, o, num_steps=10, noise=noise.to(DEV)))


def test_refresh_serve_caches_rebuilds_every_record_in_place(hip):
    """After a parameter update `refresh_serve_caches()` leaves the store (lap_amd/serve_cache.py) with the same keys at the same
    addresses, every record at the new version, and the serving paths compute what a model built on the new parameters computes."""
    from lap_amd.serve_cache import _tensors

    cfg = debug_model_cfg()
    P = O.init_params(oracle_cfg(cfg), seed=19)
    obs, _, noise, _ = make_inputs(cfg, B=2, ragged=True)
    so = {k: v for k, v in obs.items() if k != "tokenized_langact_mask"}
    o = to_observation(so | {"tokenized_langact_mask": None}, DEV)

    def serve(m):
        return m.sample_actions(0, o, num_steps=10, noise=noise.to(DEV)), m.sample_tokens(0, o, max_decoding_steps=3)

    def updated(m):
        with torch.no_grad():
            for name in m.ps.master:
                m.ps.master[name].mul_(1.03)
        m.ps.refresh_mirror_local()
        return m

    def ptrs(m):
        return {k: [t.data_ptr() for t in _tensors(v)] for k, v in m.serving_cache.entries().items()}

    model = _engine(cfg, P)
    a1, t1 = serve(model)
    before = ptrs(model)
    assert before and not model.serving_cache.stale()
    updated(model)
    assert sorted(model.serving_cache.stale(), key=repr) == sorted(before, key=repr)
    model.refresh_serve_caches()
    assert ptrs(model) == before and list(ptrs(model)) == list(before) and not model.serving_cache.stale()
    a2, t2 = serve(model)
    assert ptrs(model) == before
    fa, ft = serve(updated(_engine(cfg, P)))
    assert torch.equal(a2, fa) and torch.equal(t2, ft)
    assert not torch.equal(a1, a2) and bool(torch.isfinite(a2).all())


def test_sample_actions_matches_oracle(hip):
    cfg = debug_model_cfg()
    oc = oracle_cfg(cfg)
    P = O.init_params(oc, seed=11)
    obs, _, noise, _ = make_inputs(cfg, B=2, ragged=True)
    so = {k: v for k, v in obs.items() if k != "tokenized_langact_mask"}  # serving observations carry no langact mask
    ref = O.sample_actions(P, oc, so, noise, num_steps=10)
    ref16 = O.sample_actions(P, dataclasses.replace(oc, emulate_bf16=True), so, noise, num_steps=10)
    model = _engine(cfg, P)
    o = to_observation(so | {"tokenized_langact_mask": None}, DEV)
    out = model.sample_actions(0, o, num_steps=10, noise=noise.to(DEV))
    # the fused serving kernels (split-K partial consumers) are bit-identical to the generic layer path
    assert torch.equal(out, model.sample_actions(0, o, num_steps=10, noise=noise.to(DEV), fused=False))
    err, base = rel(out, ref), rel(ref16, ref)
    assert out.shape == (2, cfg.action_horizon, cfg.action_dim)
    assert err < max(3 * base, 1e-2), (err, base)


@pytest.mark.parametrize("case", ["ragged", "masked_image", "langact"])
def test_sample_tokens_matches_oracle(hip, case):
    """AR decode (lap.py:678-766): prefill + single-token steps against the oracle's literal restatement
    (which physically right-aligns the prefix); logits per step and the greedy token sequence."""
    cfg = debug_model_cfg()
    oc = oracle_cfg(cfg)
    P = O.init_params(oc, seed=13)
    obs, _, _, _ = make_inputs(cfg, B=3, ragged=True)
    so = dict(obs)
    if case != "langact":
        so.pop("tokenized_langact_mask")          # serving observations carry no langact mask
    so["image_masks"] = {k: torch.ones_like(m) for k, m in so["image_masks"].items()}
    if case == "masked_image":
        # Hole in the middle of the prefix.  The reference's decode mask [prefix_start, ...) then covers the masked
        # image's tokens, whose prefill activations above layer 0 are the softmax of a fully masked row (uniform
        # "garbage", SURVEY 8 a-bis) - the engine writes zeros for such rows, so only the prefill logits and the
        # layer-0 visible mask arithmetic are comparable here; see the strict cases for everything else.
        so["image_masks"][cfg.image_keys[-1]][1] = False
    steps = 5
    c32, c16 = {}, {}
    ref = O.sample_tokens(P, oc, so, max_decoding_steps=steps, collect=c32)
    ref16 = O.sample_tokens(P, dataclasses.replace(oc, emulate_bf16=True), so, max_decoding_steps=steps, collect=c16)
    model = _engine(cfg, P)
    o = to_observation(so if "tokenized_langact_mask" in so else so | {"tokenized_langact_mask": None}, DEV)
    col = {}
    out = model.sample_tokens(0, o, max_decoding_steps=steps, collect=col)
    assert out.shape == (3, steps) and out.dtype == torch.int32
    agree = 0
    for s in range(steps):
        if not (torch.equal(ref[:, :s], ref16[:, :s]) and torch.equal(out[:, :s].cpu(), ref[:, :s])):
            break                                  # the contexts diverged (bf16 tie flip): later logits are not comparable
        err, base = rel(col[f"logit/{s}"], c32[f"logit/{s}"]), rel(c16[f"logit/{s}"], c32[f"logit/{s}"])
        assert err < max(3 * base, 1e-2), (s, err, base)
        agree += 1
        if case == "masked_image":
            break
    assert agree >= (1 if case == "masked_image" else 2)   # prefill logits (+ at least one true decode step) compared
    if torch.equal(ref, ref16) and case != "masked_image":
        assert torch.equal(out.cpu(), ref)
    # stop logic: a one-sample batch whose first token is declared EOS stops after one step, the rest stays zero
    def first(x):
        return {k: first(v) for k, v in x.items()} if isinstance(x, dict) else (None if x is None else x[:1])
    so1 = first(so)
    eos = int(ref[0, 0])
    model.EOS_TOKEN = eos
    ref_e = O.sample_tokens(P, oc, so1, max_decoding_steps=steps, eos_token=eos)
    o1 = to_observation(so1 if "tokenized_langact_mask" in so1 else so1 | {"tokenized_langact_mask": None}, DEV)
    out_e = model.sample_tokens(0, o1, max_decoding_steps=steps)
    assert ref_e[0, 0] == eos and int(ref_e[0, 1:].abs().sum()) == 0
    assert torch.equal(out_e.cpu(), ref_e)
    assert int(out.min()) >= 0 and int(out.max()) < cfg.vocab_size
    # temperature sampling draws valid, seed-reproducible tokens
    model.EOS_TOKEN = 1
    t1 = model.sample_tokens(7, o, max_decoding_steps=3, temperature=1.0)
    t2 = model.sample_tokens(7, o, max_decoding_steps=3, temperature=1.0)
    assert torch.equal(t1, t2) and int(t1.min()) >= 0 and int(t1.max()) < cfg.vocab_size


def test_compute_loss_is_forward_of_loss_and_grad(hip):
    cfg = debug_model_cfg()
    P = O.init_params(oracle_cfg(cfg), seed=3)
    obs, actions, noise, time = make_inputs(cfg, B=2, ragged=False)
    model = _engine(cfg, P)
    o = to_observation(obs, DEV)
    l1, _ = model.compute_loss(0, o, actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV))
    l2, _ = model.loss_and_grad(0, o, actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV))
    assert l1.item() == l2.item()
    # rng-driven draws are reproducible and differ across seeds
    a, _ = model.compute_loss(5, o, actions.to(DEV)); b, _ = model.compute_loss(5, o, actions.to(DEV)); c, _ = model.compute_loss(6, o, actions.to(DEV))
    assert a.item() == b.item() and a.item() != c.item()


def test_two_stream_schedule_equals_one_stream(hip, monkeypatch):
    """The action expert's kernels on a second HIP stream (streams.py: suffix_stream) against everything on one stream, LAP-3B
    widths: same loss bits, same activations, and gradients equal up to the order of the f32 atomics that the norm / modulation
    backward kernels add with (free in both schedules; what follows them inherits the last-bit noise: 1e-5 relative, and no more
    tensors affected than between two one-stream runs + 2).  Run five times: a missing join between the streams would show up
    as a flaky mismatch."""
    cfg = _full_width_cfg(monkeypatch)
    P = O.init_params(oracle_cfg(cfg), seed=11)
    obs, actions, noise, time = make_inputs(cfg, B=3, ragged=True)
    model = _engine(cfg, P)
    o = to_observation(obs, DEV)

    def run(dual):
        model.dual_stream, model.wgrad_stream = dual, ("1" if dual else "")   # second stream: action expert; third: weight / bias gradients (all of them)
        for g in model.ps.grad.values():
            g.zero_()
        col = {}
        loss, _ = model.loss_and_grad(0, o, actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV), collect=col)
        torch.cuda.synchronize()
        return loss.item(), {k: col[k].clone() for k in ("x0_out", "x1_out", "v_t")}, {n: model.ps.g(n).detach().clone() for n in model.ps.names()}

    l1, a1, g1 = run(False)
    assert model.sfx is None
    _, _, g1b = run(False)
    noisy = sum(not torch.equal(g1[n], g1b[n]) for n in g1)
    for _ in range(5):
        l2, a2, g2 = run(True)
        assert model.sfx is not None and model.wg.stream is not None
        assert l1 == l2
        for k in a1:
            assert torch.equal(a1[k], a2[k]), k
        loose = 0
        for n in g1:
            if torch.equal(g1[n], g2[n]):
                continue
            loose += 1
            assert rel(g2[n].float().cpu(), g1[n].float().cpu()) < 1e-5, n
        assert loose <= noisy + 2, (loose, noisy)


@pytest.mark.parametrize("pi05", [True, False])
def test_train_step_matches_oracle_adamw(hip, pi05):
    """One full train step (scripts/train.py:329-419): clip -> AdamW -> EMA, against the oracle's autograd + optax restatement
    (pi05=False: the pi0 suffix path — no adaRMS unit in the optimizer's schedule)."""
    from lap_amd.config import get_config
    from lap_amd.params import engine_to_reference
    from lap_amd.train import TrainingStepRunner, init_train_state

    tc = get_config("debug")
    if not pi05:
        tc = dataclasses.replace(tc, model=dataclasses.replace(tc.model, pi05=False))
    cfg = tc.model
    oc = oracle_cfg(cfg)
    P = O.init_params(oc, seed=5)
    obs, actions, noise, time = make_inputs(cfg, B=2, ragged=True)
    state = init_train_state(tc, params=P, device=DEV)
    runner = TrainingStepRunner(tc)
    state2, info = runner(0, state, (to_observation(obs, DEV), actions.to(DEV)), 0, noise=noise.to(DEV), time=time.to(DEV))
    torch.cuda.synchronize()
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    loss32, _ = O.compute_loss(Pg, oc, obs, actions, noise, time)
    loss32.backward()
    gn = torch.sqrt(sum((v.grad ** 2).sum() for v in Pg.values()))
    assert abs(info["grad_norm"].item() - gn.item()) / gn.item() < 3e-2
    cs = O.clip_scale(gn.item(), tc.optimizer.clip_gradient_norm)
    lr = tc.lr_schedule(0)
    new = state2.model.ps.to_reference_tree("master")
    ema = state2.model.ps.to_reference_tree("ema")
    d, on = tc.get_ema_decay_for_step(0)
    # (1) The optimizer arithmetic, EVERY tensor, tight: clip -> AdamW -> EMA applied to the ENGINE's own gradients must be the
    # oracle's optax restatement of the same gradients (f32 kernel with 1-ulp rcp / sqrt vs torch f32: 2e-5 on the update).
    # The gradients themselves are held to 5e-2 per tensor by the gradient tests above; comparing the END-TO-END update against
    # the oracle's gradients is inherently loose on the first Adam step (update = lr * g / (|g| + eps) ~ lr * sign(g): every
    # element whose gradient is bf16 noise flips by 2 lr), which is what the old 15 % bound on four tensors absorbed.
    ps = state2.model.ps
    g_eng = engine_to_reference(cfg, {name: ps.g(name).detach().float().cpu() for name in ps.names()})
    gn_eng = torch.sqrt(sum((g.double() ** 2).sum() for g in g_eng.values())).item()
    assert abs(info["grad_norm"].item() - gn_eng) / gn_eng < 1e-5
    cs_e = O.clip_scale(gn_eng, tc.optimizer.clip_gradient_norm)
    m_eng, v_eng = ps.to_reference_tree("m"), ps.to_reference_tree("v")
    worst = 0.0
    for k in P:
        p1, m1, v1 = O.adamw_step(P[k], g_eng[k], torch.zeros_like(P[k]), torch.zeros_like(P[k]), 1, lr, tc.optimizer.b1,
                                  tc.optimizer.b2, tc.optimizer.eps, tc.optimizer.weight_decay, cs_e)
        du, dr = new[k] - P[k], p1 - P[k]
        if dr.norm() > 0:
            # elements with |g| ~ eps * sqrt(1 - b2) sit on the knee of g / (|g| + eps): compare where the update is well conditioned
            big = g_eng[k].abs() * cs_e > 1e-5
            e = rel(du[big], dr[big]) if big.any() else 0.0
            worst = max(worst, e)
            assert e < 2e-5, (k, e)
        assert rel(m_eng[k], m1) < 1e-6 and rel(v_eng[k], v1) < 1e-6, k
        assert on and rel(ema[k], d * P[k] + (1 - d) * new[k]) < 1e-6, k
    # (2) end to end against the oracle's own gradients: a sanity bound only (see above)
    for k in ("PaliGemma/llm/layers/mlp/linear", "PaliGemma/img/head/kernel", "action_out_proj/kernel", "PaliGemma/llm/layers/pre_ffw_norm/scale"):
        p1, _, _ = O.adamw_step(P[k], Pg[k].grad, torch.zeros_like(P[k]), torch.zeros_like(P[k]), 1, lr, tc.optimizer.b1,
                                tc.optimizer.b2, tc.optimizer.eps, tc.optimizer.weight_decay, cs)
        assert rel(new[k] - P[k], p1 - P[k]) < 0.25, k
    assert state2.step == 1


@pytest.mark.parametrize("pi05", [True, False])
def test_second_train_step_without_language_loss_starts_from_clean_gradients(hip, pi05):
    """with enable_langact_training=False the LM-head weight-gradient product — the only writer (beta = 0) of the
    embedding table's f32 gradient buffer — is not run, and the prefix embedding's scatter-add would accumulate across steps.  Two train
    steps at learning rate 0 on the same batch: step 2's embedding gradient and gradient norm must be step 1's, and the oracle's."""
    from lap_amd.config import CosineDecaySchedule, get_config
    from lap_amd.params import engine_to_reference
    from lap_amd.train import TrainingStepRunner, init_train_state

    tc = get_config("debug")
    tc = dataclasses.replace(tc, model=dataclasses.replace(tc.model, pi05=pi05, enable_langact_training=False),
                             lr_schedule=CosineDecaySchedule(warmup_steps=0, peak_lr=0.0, decay_steps=10, decay_lr=0.0))
    cfg = tc.model
    oc = oracle_cfg(cfg)
    P = O.init_params(oc, seed=7)
    obs, actions, noise, time = make_inputs(cfg, B=2, ragged=True)
    state = init_train_state(tc, params=P, device=DEV)
    runner = TrainingStepRunner(tc)
    batch = (to_observation(obs, DEV), actions.to(DEV))
    norms, grads = [], []
    for step in range(2):
        state, info = runner(0, state, batch, step, noise=noise.to(DEV), time=time.to(DEV))
        torch.cuda.synchronize()
        ps = state.model.ps
        norms.append(info["grad_norm"].item())
        grads.append(engine_to_reference(cfg, {n: ps.g(n).detach().float().cpu() for n in ps.names()}))
    key = "PaliGemma/llm/embedder/input_embedding"
    assert grads[0][key].abs().max() > 0
    assert rel(grads[1][key], grads[0][key]) < 1e-5, rel(grads[1][key], grads[0][key])
    assert abs(norms[1] - norms[0]) / norms[0] < 1e-5, norms
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    loss32, _ = O.compute_loss(Pg, oc, obs, actions, noise, time)
    loss32.backward()
    gn = torch.sqrt(sum((v.grad ** 2).sum() for v in Pg.values() if v.grad is not None)).item()
    assert abs(norms[1] - gn) / gn < 3e-2, (norms, gn)
    assert rel(grads[1][key], Pg[key].grad) < 5e-2


# ------------------------------------------------------------------------------ fp8 GEMM path (BASELINE.json config 5)
# Tolerances re-stated for fp8 (north_star): the VLM expert's projections multiply e4m3 operands (3 mantissa bits: 2^-4
# relative rounding per element, per-tensor scale 448 / amax).  Measured on MI355X at the LAP-3B widths (2 layers):
#   * the fp8-EMULATING oracle sits FP8_NOISE ~ 2-4e-2 (relative L2, last layer) from the f32 oracle — that is the price of
#     the format, the engine must not add to it: engine-vs-f32 <= 1.5 x (fp8 oracle-vs-f32);
#   * engine vs the fp8-emulating oracle (same quantiser, same scales, different f32 summation order): the two free-running
#     fp8 implementations decorrelate like the bf16 pair does (a flipped e4m3 rounding is 2^-4): <= 1.5 x (fp8 oracle-vs-f32)
#     (measured 4.0e-2 / 5.0e-2 against a base of 4.2e-2 / 5.6e-2 for layers 0 / 1; action stream 1.4-2.2e-3);
#   * gradients (the data-gradient GEMMs quantise dy as well; weight gradients are bf16): relative L2 per tensor vs the f32
#     oracle <= FP8_GRAD_BOUND (measured worst 1.0e-1: q_einsum).
FP8_GRAD_BOUND = 0.25


def test_fp8_gemm_path_matches_fp8_emulating_oracle(hip, monkeypatch):
    cfg = _full_width_cfg(monkeypatch, action_dim=7)
    oc = oracle_cfg(cfg)
    P = O.init_params(oc, seed=7)
    B = 2
    obs, actions, noise, time = make_inputs(cfg, B=B, ragged=True)
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    col32, col8 = {}, {}
    loss32, _ = O.compute_loss(Pg, oc, obs, actions, noise, time, collect=col32)
    loss32.backward()
    with torch.no_grad():
        loss8, _ = O.compute_loss(P, dataclasses.replace(oc, emulate_fp8=True), obs, actions, noise, time, collect=col8)
    from lap_amd.model import LAP

    model = LAP(cfg, params=P, device=DEV, gemm_dtype="fp8")
    for g in model.ps.grad.values():
        g.zero_()
    col = {}
    loss, _ = model.loss_and_grad(0, to_observation(obs, DEV), actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV), collect=col)
    torch.cuda.synchronize()
    fp8_noise = abs(loss8.item() - loss32.item()) / abs(loss32.item())
    assert abs(loss.item() - loss32.item()) / abs(loss32.item()) < max(3 * fp8_noise, 2e-2), (loss.item(), loss32.item(), loss8.item())
    L = cfg.max_token_len
    Pn = model.n_img_tok * len(cfg.image_keys) + L
    pm = torch.cat([obs["image_masks"][k][:, None].expand(B, model.n_img_tok) for k in cfg.image_keys] + [obs["tokenized_prompt_mask"]], 1)
    rows = []
    for l in range(oc.vlm.depth):
        for i, (sel, shape) in enumerate(((pm, (B, Pn, -1)), (None, (B, cfg.action_horizon, -1)))):
            k = f"llm/layer{l:02d}/x{i}"
            e = col[k].float().cpu().view(*shape)
            a32, a8 = col32[k].detach(), col8[k]
            if sel is not None:
                e, a32, a8 = e[sel], a32[sel], a8[sel]
            err32, base, pair = rel(e, a32), rel(a8, a32), rel(e, a8)
            rows.append((k, err32, base, pair))
            if os.environ.get("LAP_PARITY_REPORT"):
                print(f"  fp8 {k:20s} engine-f32 {err32:.2e}  fp8oracle-f32 {base:.2e}  engine-fp8oracle {pair:.2e}")
                continue
            assert err32 < max(1.5 * base, 1e-2), (k, err32, base)
            assert pair < max(1.5 * base, 1e-2), (k, pair, base)
    # gradients: every tensor vs the f32 oracle
    from lap_amd.params import engine_to_reference

    gref = engine_to_reference(cfg, {name: model.ps.g(name).detach().float().cpu() for name in model.ps.names()})
    worst = max(((rel(gref[k], v.grad), k) for k, v in Pg.items() if v.grad is not None and v.grad.abs().max() > 1e-6), key=lambda t: t[0])
    if os.environ.get("LAP_PARITY_REPORT"):
        print(f"  fp8 worst gradient {worst[1]} {worst[0]:.2e}; loss {loss.item():.5f} f32 {loss32.item():.5f} fp8-oracle {loss8.item():.5f}")
    else:
        assert worst[0] < FP8_GRAD_BOUND, worst
    # the bf16 engine on the same inputs is closer to f32 than the fp8 one (sanity: the switch does something)
    model16 = LAP(cfg, params=P, device=DEV)
    l16, _ = model16.compute_loss(0, to_observation(obs, DEV), actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV))
    assert l16.item() != loss.item()
    with pytest.raises(ValueError, match="multiples of 128"):
        LAP(debug_model_cfg(), seed=0, device=DEV, gemm_dtype="fp8")


def test_fp8_weight_mirrors_follow_a_restore(hip, monkeypatch, tmp_path):
    """`restore_state` writes masters / bf16 mirrors directly; the e4m3 weight copies cached by `LAP._w8_of` are keyed
    on `ParamStore.version` and must be re-quantised after it — forward, restore, forward equals a model that always held the
    restored parameters, bit for bit."""
    from lap_amd import checkpoints as ck
    from lap_amd.config import get_config
    from lap_amd.train import init_train_state

    cfg = _full_width_cfg(monkeypatch, action_dim=7)
    tc = dataclasses.replace(get_config("debug"), model=cfg, gemm_dtype="fp8", checkpoint_base_dir=str(tmp_path), exp_name="r")
    obs, actions, noise, time = make_inputs(cfg, B=2, ragged=True)
    args = (to_observation(obs, DEV), actions.to(DEV))
    kw = dict(noise=noise.to(DEV), time=time.to(DEV))
    a = init_train_state(tc, seed=1, device=DEV)
    mngr, _ = ck.initialize_checkpoint_dir(tc.checkpoint_dir, keep_period=None, overwrite=False, resume=True)
    ck.save_state(mngr, a, None, 1)
    la, _ = a.model.compute_loss(0, *args, **kw)
    b = init_train_state(tc, seed=2, device=DEV)
    lb, _ = b.model.compute_loss(0, *args, **kw)          # caches the fp8 mirrors of the seed-2 weights
    b = ck.restore_state(mngr, b, None)
    lr, _ = b.model.compute_loss(0, *args, **kw)
    torch.cuda.synchronize()
    assert lb.item() != la.item() and torch.equal(lr, la), (la.item(), lb.item(), lr.item())


def test_vqa_and_prediction_loss_mixing_matches_oracle(hip):
    """lap.py:401-413,472-596: VQA / prediction samples carry their own language-loss weights (per-dataset VQA weights through
    the registry ids) and are excluded from the action loss, whose normaliser becomes the number of action samples; idle
    samples (`sample_mask` False) drop out of every language term.  Loss, per-kind metrics and every gradient vs the oracle."""
    cfg = debug_model_cfg(enable_vqa_training=True, enable_prediction_training=True, vqa_loss_weight=0.1, prediction_loss_weight=0.7,
                          vqa_loss_weights={"lvis": 0.3, "not_registered": 9.0})
    oc = oracle_cfg(cfg)
    P = O.init_params(oc, seed=23)
    B = 6
    obs, actions, noise, time = make_inputs(cfg, B=B, ragged=True)
    obs["is_vqa_sample"] = torch.tensor([True, False, False, True, False, True])
    obs["is_prediction_sample"] = torch.tensor([False, False, True, False, False, False])
    obs["vqa_dataset_id"] = torch.tensor([2, 0, 0, 7, 0, 2])                # lvis, -, -, vqa, -, lvis
    obs["sample_mask"] = torch.tensor([True, False, True, True, True, False])   # an idle robot sample and an idle VQA sample
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    loss32, m32 = O.compute_loss(Pg, oc, obs, actions, noise, time)
    loss32.backward()
    loss16, _ = O.compute_loss(P, dataclasses.replace(oc, emulate_bf16=True), obs, actions, noise, time)
    model = _engine(cfg, P)
    for g in model.ps.grad.values():
        g.zero_()
    loss, metrics = model.loss_and_grad(0, to_observation(obs, DEV), actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV))
    torch.cuda.synchronize()
    ref_noise = abs(loss16.item() - loss32.item()) / abs(loss32.item())
    assert abs(loss.item() - loss32.item()) / abs(loss32.item()) < max(3 * ref_noise, 5e-3), (loss.item(), loss32.item(), loss16.item())
    # the same inputs without the sample kinds give a different loss (the switch does something)
    plain = debug_model_cfg()
    l0, _ = _engine(plain, P).compute_loss(0, to_observation(obs, DEV), actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV))
    assert abs(l0.item() - loss.item()) > 1e-2
    # per-kind bookkeeping (metrics.py:49-56): 2 active VQA samples, 1 prediction sample, 1 language-action sample of 4 active
    assert metrics["vqa_num_samples"].item() == 2 and metrics["pred_num_samples"].item() == 1 and metrics["langact_num_samples"].item() == 1
    assert metrics["active_num_samples"].item() == 4 and abs(metrics["vqa_sample_portion"].item() - 0.5) < 1e-6
    pl = m32["per_sample_lang"]
    assert abs(metrics["vqa_loss"].item() - (pl[0] + pl[3]).item() / 2) < 2e-2 * abs((pl[0] + pl[3]).item() / 2) + 1e-3
    from lap_amd.params import engine_to_reference

    gref = engine_to_reference(cfg, {name: model.ps.g(name).detach().float().cpu() for name in model.ps.names()})
    for k, v in Pg.items():
        if v.grad is None:
            continue
        assert rel(gref[k], v.grad) < 5e-2 or (gref[k] - v.grad).abs().max() < 1e-4, (k, rel(gref[k], v.grad))


@pytest.mark.parametrize("case", ["all_idle", "no_langact_tokens", "no_valid_image", "batch_of_one", "max_padding"])
def test_degenerate_batches_match_oracle(hip, case):
    """Edge cases of the loss assembly (lap.py:209-289,472-596) and the masks (lap.py:118-170,303-377): every sample idle (sample_mask all
    False: the language term is 0 / max(0, 1)), a sample without language-action tokens (its cross entropy is 0 / max(0, 1)), a sample whose
    images are all invalid (its prefix keys are the prompt alone), a batch of one, and a prompt that is padding except for three tokens.
    Loss, per-sample losses and a handful of gradients against the f32 oracle."""
    cfg = debug_model_cfg()
    oc = oracle_cfg(cfg)
    P = O.init_params(oc, seed=21)
    B = 1 if case == "batch_of_one" else 3
    obs, actions, noise, time = make_inputs(cfg, B=B, ragged=True)
    L = cfg.max_token_len
    if case == "all_idle":
        obs["sample_mask"][:] = False
    elif case == "no_langact_tokens":
        obs["tokenized_langact_mask"][0] = False
    elif case == "no_valid_image":
        for k in cfg.image_keys:
            obs["image_masks"][k][0] = False
    elif case == "max_padding":
        obs["tokenized_prompt_mask"][0] = False
        obs["tokenized_prompt_mask"][0, :3] = True
        obs["tokenized_langact_mask"][0] = False
        obs["tokenized_langact_mask"][0, 1:3] = True
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    loss32, m32 = O.compute_loss(Pg, oc, obs, actions, noise, time)
    loss32.backward()
    model = _engine(cfg, P)
    for g in model.ps.grad.values():
        g.zero_()
    col = {}
    loss, metrics = model.loss_and_grad(0, to_observation(obs, DEV), actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV), collect=col)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and abs(loss.item() - loss32.item()) <= 1e-2 * abs(loss32.item()) + 1e-6, (loss.item(), loss32.item())
    assert rel(col["per_sample_action"], m32["per_sample_action"]) < 2e-2
    ps_lang = m32["per_sample_lang"].detach()
    if float(ps_lang.abs().max()) > 0:
        assert rel(col["per_sample_lang"], ps_lang) < 2e-2
    else:
        assert float(col["per_sample_lang"].abs().max()) == 0.0
    if case == "no_langact_tokens" or case == "all_idle":
        assert float(col["per_sample_lang"][0]) == 0.0 and float(ps_lang[0]) == 0.0
    from lap_amd.params import engine_to_reference

    gref = engine_to_reference(cfg, {name: model.ps.g(name).detach().float().cpu() for name in model.ps.names()})
    for k in ("PaliGemma/llm/layers/mlp_1/linear", "action_out_proj/kernel", "PaliGemma/llm/layers/attn/kv_einsum/w", "PaliGemma/img/head/kernel",
              "PaliGemma/llm/embedder/input_embedding"):
        g32 = Pg[k].grad
        if g32 is None or float(g32.abs().max()) == 0.0:
            assert float(gref[k].abs().max()) == 0.0, k
        else:
            assert rel(gref[k], g32) < 5e-2 or (gref[k] - g32).abs().max() < 1e-4, (k, rel(gref[k], g32))
