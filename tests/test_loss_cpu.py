"""The sample-weight mixer and the vocabulary chunking of lap_amd/loss.py without a GPU: the expected values are written out by hand
from lap.py:472-566 (the masks are AND-ed with the sample mask first; VQA weight per dataset through the registry ids)."""
import dataclasses

import torch

from lap_amd.config import VQA_DATASET_ID_MAP, get_config
from lap_amd.loss import mix_sample_weights, vocab_chunks

T, F = True, False


def _cfg(**kw):
    return dataclasses.replace(get_config("debug").model, **kw)


def test_mixer_on_the_vqa_and_prediction_batch():
    """The batch of test_vqa_and_prediction_loss_mixing_matches_oracle: two active VQA samples (one with a per-dataset weight),
    one prediction sample, one language-action sample, an idle robot sample and an idle VQA sample."""
    cfg = _cfg(enable_vqa_training=True, enable_prediction_training=True, vqa_loss_weight=0.1, prediction_loss_weight=0.7,
               vqa_loss_weights={"lvis": 0.3, "not_registered": 9.0})
    i_lvis = VQA_DATASET_ID_MAP["lvis"]
    i_other = VQA_DATASET_ID_MAP["vqa"]          # registered, no per-dataset weight
    assert "vqa" not in cfg.vqa_loss_weights
    is_vqa = torch.tensor([T, F, F, T, F, T])
    is_pred = torch.tensor([F, F, T, F, F, F])
    sm = torch.tensor([T, F, T, T, T, F])
    ids = torch.tensor([i_lvis, 0, 0, i_other, 0, i_lvis])
    lang_loss = torch.tensor([1.25, 7.0, 0.5, 2.75, 3.0, 11.0])
    wl, act_mask, mixing, met = mix_sample_weights(cfg, lang_loss, sm, is_vqa, is_pred, ids, lang_on=True)
    assert mixing
    assert torch.equal(wl, torch.tensor([0.3, 0.0, 0.7, 0.1, cfg.language_loss_weight, 0.0], dtype=torch.float32))
    # the idle robot sample and the idle VQA sample stay in the action mask: the kind masks were AND-ed with the sample mask
    assert act_mask.tolist() == [F, T, F, F, T, T]
    assert met["vqa_num_samples"].item() == 2 and met["pred_num_samples"].item() == 1 and met["langact_num_samples"].item() == 1
    assert met["active_num_samples"].item() == 4 and abs(met["vqa_sample_portion"].item() - 0.5) < 1e-6
    assert abs(met["vqa_loss"].item() - lang_loss[[0, 3]].mean().item()) < 1e-6
    assert met["vqa_lvis_loss"].item() == lang_loss[0].item()


def test_mixer_without_mixing_with_language_loss_off_and_without_a_sample_mask():
    lang_loss = torch.tensor([1.0, 2.0, 3.0, 4.0])
    is_vqa = torch.tensor([F, T, F, T])
    is_pred = torch.tensor([F, F, T, F])
    sm = torch.tensor([T, T, F, T])
    # no mixing configured: every sample weighs language_loss_weight; a VQA mask that is given still keeps its samples out of the
    # action loss (lap.py:560-564), and there are no per-kind metrics
    cfg = _cfg()
    assert not (cfg.enable_vqa_training or cfg.enable_prediction_training)
    wl, act_mask, mixing, met = mix_sample_weights(cfg, lang_loss, sm, is_vqa, None, None, lang_on=True)
    assert not mixing and met == {}
    assert torch.equal(wl, torch.full((4,), cfg.language_loss_weight, dtype=torch.float32))
    assert torch.equal(act_mask, ~is_vqa)
    # language loss off: weight 0, and the VQA / prediction masks reach the action mask as they came (not AND-ed with the sample mask)
    cfg = _cfg(enable_vqa_training=True, enable_prediction_training=True, enable_langact_training=False)
    wl, act_mask, mixing, met = mix_sample_weights(cfg, torch.zeros(4), sm, is_vqa, is_pred, None, lang_on=False)
    assert not mixing and met == {}
    assert torch.equal(wl, torch.zeros(4)) and act_mask.tolist() == [T, F, F, F]
    # no sample mask: every sample is active
    cfg = _cfg(enable_vqa_training=True, enable_prediction_training=True, vqa_loss_weight=0.25, prediction_loss_weight=0.5)
    wl, act_mask, mixing, met = mix_sample_weights(cfg, lang_loss, None, is_vqa, is_pred, None, lang_on=True)
    assert mixing
    assert torch.equal(wl, torch.tensor([cfg.language_loss_weight, 0.25, 0.5, 0.25], dtype=torch.float32))
    assert act_mask.tolist() == [T, F, F, F]
    assert met["active_num_samples"].item() == 4 and met["vqa_num_samples"].item() == 2 and met["langact_num_samples"].item() == 1
    assert abs(met["vqa_loss"].item() - 3.0) < 1e-6 and abs(met["pred_loss"].item() - 3.0) < 1e-6 and abs(met["langact_loss"].item() - 1.0) < 1e-6


def test_vocab_chunks_tile_the_vocabulary():
    for R, V in ((32 * 47, 257_152), (64 * 47, 257_152), (256 * 47, 257_152), (1, 512), (10 ** 6, 5120), (3, 1024), (7, 1025)):
        chunks = vocab_chunks(R, V)
        assert chunks[0][0] == 0 and sum(vc for _, vc in chunks) == V
        assert all(a[0] + a[1] == b[0] for a, b in zip(chunks, chunks[1:]))         # ascending, no gap
        assert all(vc % 1024 == 0 for _, vc in chunks[:-1]) and all(vc > 0 for _, vc in chunks)
        assert all(2 * R * vc <= 1.5e9 or vc == 1024 for _, vc in chunks)
    assert len(vocab_chunks(32 * 47, 257_152)) == 1 and len(vocab_chunks(64 * 47, 257_152)) == 2
    assert vocab_chunks(141, 2048, cap_cols=1024) == [(0, 1024), (1024, 1024)]
