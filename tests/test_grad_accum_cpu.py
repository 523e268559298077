"""Gradient accumulation, the host side (no GPU): config validation, the global loss denominators, the micro-step seeds, the train
loop's loader arithmetic and resume, the parameter store's accumulators, and the kernel's entry in the C ABI."""
import ctypes
import dataclasses
import pathlib
import re
import types

import pytest
import torch

from lap_amd.config import TrainConfig, get_config

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_config_validation():
    tc = get_config("debug")
    assert tc.grad_accum_steps == 1 and TrainConfig().grad_accum_steps == 1
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="grad_accum_steps"):
            dataclasses.replace(tc, grad_accum_steps=bad)
    with pytest.raises(ValueError, match="divisible"):
        dataclasses.replace(tc, batch_size=8, grad_accum_steps=3)
    ok = dataclasses.replace(tc, batch_size=16, grad_accum_steps=4)
    assert ok.micro_batch_size(1) == 4 and ok.micro_batch_size(2) == 2
    with pytest.raises(ValueError, match="divisible"):
        ok.micro_batch_size(8)           # 16 samples over 8 ranks x 4 micro-steps
    for name in ("lap", "lap_libero"):   # the recipes' batch sizes on one 8-GPU box at 32 samples per GPU and micro-step
        rc = get_config(name)
        K = rc.batch_size // (8 * 32)
        assert dataclasses.replace(rc, grad_accum_steps=K).micro_batch_size(8) == 32


def _obs(sample_mask=None, vqa=None, pred=None, B=None):
    B = B if B is not None else len(sample_mask)
    t = lambda v: None if v is None else torch.tensor(v, dtype=torch.bool)      # noqa: E731
    return types.SimpleNamespace(tokenized_prompt=torch.zeros(B, 4, dtype=torch.int32), sample_mask=t(sample_mask), is_vqa_sample=t(vqa),
                                 is_prediction_sample=t(pred))


def test_global_denominators_against_hand_counted_masks():
    from lap_amd.loss import global_denominators, mix_sample_weights
    from tests.common import debug_model_cfg

    T, F = True, False
    mix = debug_model_cfg(enable_vqa_training=True, enable_prediction_training=True)
    micro = [_obs([T, F, T], [F, F, T], [F, F, F]),      # active 2; action samples: not (vqa & active), not (pred & active) -> 0, 1 -> 2
             _obs([F, F, F], [T, F, F], [F, T, F]),      # all masked: active 0; the masked flags do not count -> action samples 3
             _obs([T, T, T], [T, F, F], [F, T, F])]      # active 3; action samples 1
    na, nact = global_denominators(mix, micro)
    assert (na.item(), nact.item()) == (5.0, 6.0) and na.dtype == torch.float32 and na.dim() == 0
    # the per-batch counts are those of mix_sample_weights' masks (one piece of logic, not a copy)
    for o in micro:
        m = mix_sample_weights(mix, torch.zeros(3), o.sample_mask, o.is_vqa_sample, o.is_prediction_sample, None, lang_on=True)
        assert global_denominators(mix, [o])[1].item() == max(float(m.act_mask.sum()), 1.0)
    # an all-masked micro-batch alone: both clamped at 1, as the loss clamps them
    na, nact = global_denominators(mix, [_obs([F, F], [T, T], [F, F])])
    assert (na.item(), nact.item()) == (1.0, 2.0)
    na, nact = global_denominators(mix, [_obs([F, F], None, None)])
    assert (na.item(), nact.item()) == (1.0, 2.0)
    # without VQA / prediction training the flags are not read; without a sample mask every sample is active
    plain = debug_model_cfg()
    na, nact = global_denominators(plain, [_obs(None, [T, T], [T, F], B=2), _obs([T, F, F], None, None)])
    assert (na.item(), nact.item()) == (3.0, 5.0)
    # language-action training off (pi0 style): the flags reach the action mask as they came, masked or not
    pi0 = debug_model_cfg(enable_langact_training=False, enable_vqa_training=True)
    na, nact = global_denominators(pi0, [_obs([F, T, T], [T, F, F], None)])
    assert (na.item(), nact.item()) == (2.0, 2.0)
    # no action training: no action denominator
    assert global_denominators(debug_model_cfg(enable_action_training=False), [_obs([T, T])])[1] is None

    class Comm:      # one collective for both counts
        calls = 0

        def all_reduce_sum(self, t):
            Comm.calls += 1
            assert t.shape == (2,)
            return t * 2      # two ranks with the same counts

    na, nact = global_denominators(mix, micro, Comm())
    assert Comm.calls == 1 and (na.item(), nact.item()) == (10.0, 12.0)


def test_micro_step_seeds():
    from lap_amd.train import TrainingStepRunner as R

    assert R.micro_seed(7, 5, 0, 1) == 7 * 1_000_003 + 5          # K = 1: the seed as it always was
    base = 7 * 1_000_003 + 5
    assert [R.micro_seed(7, 5, k, 3) for k in range(3)] == [base * 1_000_003 + k for k in range(3)]
    assert len({R.micro_seed(7, s, k, 2) for s in range(4) for k in range(2)}) == 8
    g = torch.Generator()
    assert R.micro_seed(g, 5, 1, 2) is g


class _Loader:
    """Counts draws; state = the number of batches drawn (the protocol of train.SyntheticDataLoader)."""

    def __init__(self):
        self.index = 0

    def __iter__(self):
        return self

    def __next__(self):
        self.index += 1
        return ("obs", self.index - 1), ("actions", self.index - 1)

    def get_state(self):
        return {"index": self.index}

    def set_state(self, s):
        self.index = int(s["index"])


def _run_main(monkeypatch, tmp_path, K, steps, saved, resume_from=None, batch_size=8):
    """train.main with a stub step runner, a stub train state and stub checkpoint I/O: which batches does every step get?"""
    from lap_amd import checkpoints as ck
    from lap_amd import train

    seen = []

    class Runner:
        def __init__(self, config):
            assert config.grad_accum_steps == K

        def __call__(self, rng, state, batch, step):
            seen.append((step, batch))
            return dataclasses.replace(state, step=state.step + 1), {"loss": torch.tensor(0.0)}

        def param_norm(self, state):
            return torch.tensor(0.0)

    loaders = []

    def synthetic(cfg, per_rank, device, **kw):
        loaders.append(per_rank)
        return _Loader()

    monkeypatch.setattr(train, "TrainingStepRunner", Runner)
    monkeypatch.setattr(train, "SyntheticDataLoader", synthetic)
    monkeypatch.setattr(train, "init_train_state", lambda config, **kw: train.TrainState(step=0, model=None, ema_decay=None))
    monkeypatch.setattr(ck, "initialize_checkpoint_dir", lambda d, **kw: (ck.CheckpointManager(pathlib.Path(d)), resume_from is not None))
    monkeypatch.setattr(ck, "save_state", lambda mngr, state, loader, step, **kw: saved.__setitem__(step, loader.get_state()))

    def restore(mngr, state, loader):
        loader.set_state(saved[resume_from])
        return dataclasses.replace(state, step=resume_from)

    monkeypatch.setattr(ck, "restore_state", restore)
    tc = dataclasses.replace(get_config("debug"), batch_size=batch_size, grad_accum_steps=K, num_train_steps=steps, save_interval=2, log_interval=100,
                             exp_name="t", checkpoint_base_dir=str(tmp_path))
    lines = []
    train.main(tc, device="cpu", log=lines.append)
    return seen, loaders, lines


def test_train_loop_draws_k_batches_per_step_and_resumes_on_whole_steps(monkeypatch, tmp_path):
    K = 4
    saved = {}
    seen, loaders, lines = _run_main(monkeypatch, tmp_path, K, 4, saved)
    assert loaders == [8 // K]                                            # batch_size // (world * K) per rank and micro-step
    assert [s for s, _ in seen] == [0, 1, 2, 3]
    for step, batch in seen:                                              # K draws per optimizer step, in order
        assert isinstance(batch, list) and [b[0][1] for b in batch] == list(range(step * K, (step + 1) * K))
    assert saved == {2: {"index": 2 * K}, 4: {"index": 4 * K}}            # the loader's state after whole steps only
    assert any("samples/s" in ln for ln in lines)
    # a run interrupted after step 2 continues with the batches the uninterrupted run drew
    seen2, _, _ = _run_main(monkeypatch, tmp_path, K, 4, saved, resume_from=2)
    assert seen2 == seen[2:]
    # K = 1: one pair per step, not a list — the call as it always was
    seen1, loaders1, _ = _run_main(monkeypatch, tmp_path, 1, 2, {})
    assert loaders1 == [8] and [b for _, b in seen1] == [(("obs", 0), ("actions", 0)), (("obs", 1), ("actions", 1))]
    with pytest.raises(ValueError, match="divisible"):
        _run_main(monkeypatch, tmp_path, 3, 1, {}, batch_size=8)


def test_param_store_has_no_accumulator_until_asked():
    from lap_amd.fsdp import UnitPipeline
    from lap_amd.params import ParamStore

    cfg = get_config("debug").model
    ps = ParamStore(cfg, "cpu")
    pipe = UnitPipeline(ps)
    assert ps.gacc == {} and pipe.accum == (0, 1)
    pipe.begin_step(); pipe.before_backward()
    for u in ps.units:
        pipe.grads_ready(u.name)
    assert ps.gacc == {}                                                  # K = 1: nothing allocated
    big = next(u for u in ps.units if u.big)
    acc = ps.grad_accumulator(big.name)
    assert acc.dtype == torch.float32 and acc.shape == ps.gshard[big.name].shape and ps.grad_accumulator(big.name) is acc
    assert set(ps.gacc) == {big.name}
    with pytest.raises(ValueError):
        ps.grad_accumulator("small")                                      # the replicated unit accumulates in its own f32 buffer
    # sharded: the accumulator is shard-sized
    ps2 = ParamStore(cfg, "cpu", world_size=2, rank=1)
    assert ps2.grad_accumulator(big.name).numel() == ps2.shard_numel(big) == ps2.gshard[big.name].numel()
    # a fully frozen unit has none
    ps.set_frozen(lambda path: "/img/" in path)
    with pytest.raises(ValueError):
        ps.grad_accumulator("img_head")


def test_pipeline_accumulation_state():
    from lap_amd.fsdp import UnitPipeline
    from lap_amd.params import ParamStore

    pipe = UnitPipeline(ParamStore(get_config("debug").model, "cpu"))
    pipe.fold_sumsq = True                # (off on the CPU: pretend)
    pipe.set_accum(0, 3)
    assert pipe.accum == (0, 3) and pipe.fold_sumsq is False
    pipe.sumsq[0] = 5.0
    pipe._bwd_open = True
    pipe.set_accum(1, 3)
    pipe.before_backward()                # between micro-steps of one optimizer step: the open partial sums stay
    assert pipe.sumsq[0].item() == 5.0 and pipe.fold_sumsq is False
    pipe.set_accum(0, 1)
    assert pipe.fold_sumsq is True
    pipe.before_backward()                # a new step over a stale partial sum: cleared, as always
    assert pipe.sumsq[0].item() == 0.0
    with pytest.raises(ValueError):
        pipe.set_accum(2, 2)


def test_grad_fold_is_in_the_abi_table():
    from lap_amd.build import build

    header = (ROOT / "include" / "lap_hip.h").read_text()
    m = re.search(r"\bint lap_grad_fold\(([^)]*)\);", header)
    assert m, "lap_grad_fold is not declared in include/lap_hip.h"
    assert [a.strip() for a in m.group(1).split(",")] == ["float* acc", "const void* g", "int g_is_bf16", "long long n", "int first", "float* sumsq",
                                                         "void* stream"]
    lib = ctypes.CDLL(str(build(verbose=False)))
    assert hasattr(lib, "lap_grad_fold")
    src = (ROOT / "lap_amd" / "hip.py").read_text()
    m = re.search(r'"lap_grad_fold": \[([^\]]*)\]', src)
    assert m and [a.strip() for a in m.group(1).split(",")] == ["_vp", "_vp", "_i", "_ll", "_i", "_vp", "_vp"]
    assert re.search(r"^def grad_fold\(acc, g, first, sumsq=None\):", src, re.M)
