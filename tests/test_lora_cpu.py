"""LoRA Gemma variants without a GPU: the variant table, the reference's freeze filter, the parameter tree of the adapters and its
engine layout, and the weight loader's handling of a base checkpoint.

[UPSTREAM-RECALL] openpi's lora.py is not vendored: LoRAConfig(rank, alpha, init_fn=normal(0.01), rslora=False), scaling = alpha / rank
on lora.Einsum, no scaling in lora.FeedForward; lora_a takes w's shape with the last axis replaced by r, lora_b with the second-to-last."""
import re

import pytest
import torch

from lap_amd.config import LAPConfig, TrainConfig, get_gemma_config
from lap_amd.params import ParamStore, engine_sources, engine_to_reference, reference_shapes, reference_to_engine


def _cfg(vlm="dummy_lora", expert="dummy_lora", **kw):
    base = dict(paligemma_variant=vlm, action_expert_variant=expert, siglip_variant="mu/14", image_size=56, vocab_size=512,
                max_token_len=24, action_horizon=10, enable_action_training=True)
    return LAPConfig(**(base | kw))


def test_variant_table_and_ranks():
    assert get_gemma_config("gemma_2b_lora").lora_attn == (16, 16.0) and get_gemma_config("gemma_2b_lora").lora_ffn == (16, 16.0)
    assert get_gemma_config("gemma_300m_lora").lora_attn == (32, 32.0) and get_gemma_config("gemma_300m_lora").lora_ffn == (32, 32.0)
    for name, base in (("gemma_2b_lora", "gemma_2b"), ("gemma_300m_lora", "gemma_300m"), ("dummy_lora", "dummy")):
        a, b = get_gemma_config(name), get_gemma_config(base)
        assert (a.width, a.depth, a.mlp_dim, a.num_heads, a.num_kv_heads, a.head_dim) == \
               (b.width, b.depth, b.mlp_dim, b.num_heads, b.num_kv_heads, b.head_dim)
        assert a.has_lora and not b.has_lora
    assert get_gemma_config("gemma_2b_lora").reference and not get_gemma_config("dummy_lora").reference
    with pytest.raises(ValueError):
        get_gemma_config("gemma_2b_lora_x")


def _reference_freeze_filter(vlm: str, expert: str):
    """lap_config.py:132-169 restated literally: nnx.All over PathRegex filters, nnx.Nothing without LoRA."""
    filters, has_lora = [], False
    gemma, action_expert = ".*llm.*", ".*llm.*_1.*"
    if "lora" in vlm:
        filters.append(lambda p: re.fullmatch(gemma, p) is not None)
        if "lora" not in expert:
            filters.append(lambda p: re.fullmatch(action_expert, p) is None)
        has_lora = True
    elif "lora" in expert:
        filters.append(lambda p: re.fullmatch(action_expert, p) is not None)
        has_lora = True
    if has_lora:
        filters.append(lambda p: re.fullmatch(".*lora.*", p) is None)
    if not filters:
        return None
    return lambda p: all(f(p) for f in filters)


@pytest.mark.parametrize("vlm,expert", [("dummy", "dummy"), ("dummy_lora", "dummy"), ("dummy", "dummy_lora"), ("dummy_lora", "dummy_lora")])
def test_freeze_filter_truth_table(vlm, expert):
    cfg = _cfg(vlm, expert)
    got, ref = cfg.get_freeze_filter(), _reference_freeze_filter(vlm, expert)
    if ref is None:
        assert got is None
        return
    paths = list(reference_shapes(_cfg("dummy_lora", "dummy_lora")))
    assert len(paths) > 60
    for p in paths:
        assert bool(got(p)) == bool(ref(p)), p
    if "lora" in vlm:      # SigLIP trainable, embedder and final norm frozen with the VLM, adapters never frozen
        assert not got("PaliGemma/img/embedding/kernel") and got("PaliGemma/llm/embedder/input_embedding")
        assert got("PaliGemma/llm/final_norm/scale") and not got("PaliGemma/llm/layers/attn/q_einsum/lora_a")
    assert not got("action_out_proj/kernel")


def test_reference_shapes_of_the_adapters():
    cfg = LAPConfig(paligemma_variant="gemma_2b_lora", action_expert_variant="gemma_300m_lora", enable_action_training=True)
    sh = reference_shapes(cfg)
    lay = "PaliGemma/llm/layers"
    for sfx, D, F, r in (("", 2048, 16384, 16), ("_1", 1024, 4096, 32)):
        assert sh[f"{lay}/attn/q_einsum{sfx}/lora_a"] == (18, 8, D, r)
        assert sh[f"{lay}/attn/q_einsum{sfx}/lora_b"] == (18, 8, r, 256)
        assert sh[f"{lay}/attn/kv_einsum{sfx}/lora_a"] == (18, 2, 1, D, r)
        assert sh[f"{lay}/attn/kv_einsum{sfx}/lora_b"] == (18, 2, 1, r, 256)
        assert sh[f"{lay}/attn/attn_vec_einsum{sfx}/lora_a"] == (18, 8, 256, r)
        assert sh[f"{lay}/attn/attn_vec_einsum{sfx}/lora_b"] == (18, 8, r, D)
        assert sh[f"{lay}/mlp{sfx}/gating_einsum_lora_a"] == (18, 2, D, r)
        assert sh[f"{lay}/mlp{sfx}/gating_einsum_lora_b"] == (18, 2, r, F)
        assert sh[f"{lay}/mlp{sfx}/linear_lora_a"] == (18, F, r)
        assert sh[f"{lay}/mlp{sfx}/linear_lora_b"] == (18, r, D)
    assert sum("lora" in k for k in sh) == 20
    assert not any("lora" in k for k in reference_shapes(LAPConfig(enable_action_training=True)))
    one = reference_shapes(LAPConfig(paligemma_variant="gemma_2b_lora", enable_action_training=True))
    assert sum("lora" in k for k in one) == 10 and not any("lora" in k and "_1" in k for k in one)


@pytest.mark.parametrize("vlm,expert", [("dummy_lora", "dummy_lora"), ("dummy_lora", "dummy"), ("dummy", "dummy_lora")])
def test_engine_layout_round_trip_is_exact(vlm, expert):
    cfg = _cfg(vlm, expert)
    g = torch.Generator().manual_seed(3)
    P = {k: torch.randn(s, generator=g) for k, s in reference_shapes(cfg).items()}
    E = reference_to_engine(cfg, P)
    back = engine_to_reference(cfg, E)
    assert set(back) == set(P)
    for k in P:
        assert torch.equal(back[k], P[k]), k
    assert set(engine_sources(cfg)) == set(E)


def test_engine_layout_matches_the_einsums():
    """The engine's A / B blocks compute the reference's einsums: q|k|v heads, the gate|up pair and the N-summed attn_vec lora_b."""
    cfg = _cfg()
    g = torch.Generator().manual_seed(4)
    P = {k: torch.randn(s, generator=g, dtype=torch.float64) for k, s in reference_shapes(cfg).items()}
    E = reference_to_engine(cfg, {k: v.float() for k, v in P.items()})
    lay, l = "PaliGemma/llm/layers", 1
    x = torch.randn(5, 64, generator=g)
    r, HD, NH = 16, 16, 8
    qa, qb = P[f"{lay}/attn/q_einsum/lora_a"][l].float(), P[f"{lay}/attn/q_einsum/lora_b"][l].float()
    ref_q = torch.einsum("btnl,nlh->btnh", torch.einsum("btd,ndl->btnl", x[None], qa), qb)[0].reshape(5, NH * HD)
    A, Bm = E[f"llm/{l}/lora_a_wqkv0"], E[f"llm/{l}/lora_b_wqkv0"]
    t = x @ A.t()
    eng = torch.cat([t[:, gi * r:(gi + 1) * r] @ Bm[gi * r:(gi + 1) * r] for gi in range(NH + 2)], 1)
    assert torch.allclose(eng[:, :NH * HD], ref_q, atol=1e-4)
    o = torch.randn(5, NH * HD, generator=g)
    va, vb = P[f"{lay}/attn/attn_vec_einsum/lora_a"][l].float(), P[f"{lay}/attn/attn_vec_einsum/lora_b"][l].float()
    ref_o = torch.einsum("btl,nld->btd", torch.einsum("btnh,nhl->btl", o.view(1, 5, NH, HD), va), vb)[0]
    Ao, Bo = E[f"llm/{l}/lora_a_wo0"], E[f"llm/{l}/lora_b_wo0"]
    assert torch.allclose((o @ Ao.t()) @ Bo.view(NH, r, 64).sum(0), ref_o, atol=1e-4)


def test_set_frozen_splits_no_tensor_and_keeps_adapters_trainable():
    for vlm, expert in (("dummy_lora", "dummy_lora"), ("dummy_lora", "dummy"), ("dummy", "dummy_lora")):
        cfg = _cfg(vlm, expert)
        ps = ParamStore(cfg, "cpu", with_optimizer=False, with_ema=False, with_grads=False)
        ps.set_frozen(TrainConfig(model=cfg, freeze_filter=cfg.get_freeze_filter()).is_frozen)     # raises on a split tensor
        lora = [n for n in ps.names() if "/lora_" in n]
        assert lora and all(ps.is_trainable(n) for n in lora)
        assert ps.is_trainable("img/0/wqkv") and ps.is_trainable("act/out_w")
        if "lora" in vlm:
            assert not ps.is_trainable("llm/0/wqkv0") and not ps.is_trainable("llm/embed")
            assert ps.is_trainable("llm/0/wqkv1") == ("lora" not in expert)
        else:
            assert ps.is_trainable("llm/0/wqkv0") and not ps.is_trainable("llm/0/wqkv1")


def test_adapters_are_initialised_like_the_reference():
    cfg = _cfg()
    ps = ParamStore(cfg, "cpu", with_optimizer=False, with_ema=False, with_grads=False)
    ps.init_random(0)
    P = ps.to_reference_tree()
    a = torch.cat([v.reshape(-1) for k, v in P.items() if k.endswith(("lora_a", "lora_b"))])
    assert a.numel() > 10000 and abs(a.std().item() - 0.01) < 5e-4 and abs(a.mean().item()) < 5e-4


def test_base_checkpoint_loads_into_a_lora_model(tmp_path):
    """CheckpointWeightLoader (weight_loaders.py:105): missing `.*lora.*` keys come from the init even without allow_partial_weights;
    any other missing key and every unknown key still fail validation."""
    import dataclasses

    from lap_amd import checkpoints as ck
    from lap_amd.config import WeightLoaderChoice
    from lap_amd.train import load_weights, validate_loaded_params

    base_cfg, lora_cfg = _cfg("dummy", "dummy"), _cfg("dummy_lora", "dummy_lora")
    src = ParamStore(base_cfg, "cpu", with_optimizer=False, with_ema=False, with_grads=False)
    src.init_random(1)
    tree = src.to_reference_tree()
    def save(t, name):
        path = tmp_path / f"{name}.safetensors"
        ck._save_tensors(path, t)
        return str(path)

    tc = TrainConfig(model=lora_cfg, weight_loader=WeightLoaderChoice(kind="checkpoint", params_path=save(tree, "params")),
                     allow_partial_weights=False)
    ps = ParamStore(lora_cfg, "cpu", with_optimizer=False, with_ema=False, with_grads=False)
    ps.init_random(2)
    init = ps.to_reference_tree()
    assert load_weights(tc, ps)
    got = ps.to_reference_tree()
    for k, v in got.items():
        assert torch.equal(v, tree[k] if k in tree else init[k]), k
    bad = dict(tree)
    bad["PaliGemma/llm/layers/attn/q_einsum/unknown"] = torch.zeros(1)
    with pytest.raises(ValueError, match="unexpected"):
        validate_loaded_params(reference_shapes(lora_cfg), bad, allow_partial=True)
    part = {k: v for k, v in tree.items() if not k.endswith("mlp/linear")}
    with pytest.raises(ValueError, match="missing"):
        load_weights(dataclasses.replace(tc, weight_loader=WeightLoaderChoice(kind="checkpoint", params_path=save(part, "part"))), ps)


def test_fp8_is_rejected_with_lora():
    from lap_amd.model import LAP

    with pytest.raises(ValueError, match="LoRA"):
        LAP(_cfg(), device="cpu", gemm_dtype="fp8", store=ParamStore(_cfg(), "cpu", with_optimizer=False, with_ema=False, with_grads=False))
