"""CPU side of checkpoint evaluation (lap_amd/evaluate.py, scripts/eval.py of the reference): checkpoint selection, the eval_*
config fields, the verbose row hint, restoring EMA / live parameters of checkpoints written at world size 1 and 2 (gloo), and the
command line."""
import dataclasses
import os
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from lap_amd import checkpoints as ck
from lap_amd import evaluate as E
from lap_amd.config import TrainConfig, get_config
from lap_amd.observation import CoTObservation
from lap_amd.params import ParamStore
from oracle import lap_oracle as O
from tests.common import oracle_cfg


def _cfg(**kw):
    return dataclasses.replace(get_config("debug"), **kw)


# ---------------------------------------------------------------------------------------------- select_checkpoint_steps
def test_select_all_checkpoints_is_the_default():
    assert E.select_checkpoint_steps([300, 100, 200], _cfg()) == [100, 200, 300]


def test_select_listed_steps_and_missing_step_error():
    c = _cfg(eval_all_checkpoints=False, eval_checkpoint_steps=(200, 100))
    assert E.select_checkpoint_steps([100, 200, 300], c) == [200, 100]
    with pytest.raises(ValueError, match=r"Requested checkpoint steps \[400\] not found. Available steps: \[100, 200, 300\]"):
        E.select_checkpoint_steps([100, 200, 300], dataclasses.replace(c, eval_checkpoint_steps=(100, 400)))


def test_select_single_step_and_missing_step_error():
    c = _cfg(eval_all_checkpoints=False, eval_checkpoint_step=200)
    assert E.select_checkpoint_steps([100, 200], c) == [200]
    with pytest.raises(ValueError, match=r"Requested checkpoint step 250 not found"):
        E.select_checkpoint_steps([100, 200], dataclasses.replace(c, eval_checkpoint_step=250))


def test_select_latest_when_nothing_is_named():
    assert E.select_checkpoint_steps([100, 300, 200], _cfg(eval_all_checkpoints=False)) == [300]


def test_select_start_from_step_filter():
    assert E.select_checkpoint_steps([100, 200, 300], _cfg(eval_start_from_step=200)) == [200, 300]
    c = _cfg(eval_all_checkpoints=False, eval_checkpoint_steps=(100, 300), eval_start_from_step=150)
    assert E.select_checkpoint_steps([100, 200, 300], c) == [300]
    with pytest.raises(ValueError, match="No checkpoints found >= eval_start_from_step=400"):
        E.select_checkpoint_steps([100, 200, 300], _cfg(eval_start_from_step=400))


def test_ema_rule():
    from lap_amd.config import EmaScheduleChoice

    c = _cfg(ema_schedule_choice=EmaScheduleChoice(kind="delayed", start_step=3))
    assert [E.uses_ema(s, True, c) for s in (1, 2, 3, 4)] == [False, False, True, True]
    assert not E.uses_ema(5, False, c)
    assert not E.uses_ema(5, True, dataclasses.replace(c, eval_use_ema=False))
    assert E.uses_ema(0, True, _cfg(ema_schedule_choice=EmaScheduleChoice(kind="delayed", start_step=0)))


def test_eval_fields_have_the_reference_defaults():
    f = {x.name: x.default for x in dataclasses.fields(TrainConfig)}
    assert f["eval_checkpoint_step"] is None and f["eval_checkpoint_steps"] is None and f["eval_all_checkpoints"] is True
    assert f["eval_start_from_step"] is None and f["num_eval_batches"] == 500
    assert f["eval_use_ema"] is True and f["eval_split"] == "val"


# -------------------------------------------------------------------------------------------------------- row hint
def test_metric_rows_max_counts_loss_and_class_masks_on_the_host():
    B, L = 3, 10
    la = np.zeros((B, L), bool); la[:, 4:] = True
    tl = la.copy(); tl[0, 5:8] = False          # reasoning dropout: positions 5..7 of sample 0 carry no loss
    crit = np.zeros((B, L), bool); crit[0, 5:8] = True; crit[1, 9] = True
    num = np.zeros((B, L), bool); num[2, 1:3] = True     # outside the langact span
    data = {"image": {"base_0_rgb": np.zeros((B, 4, 4, 3), np.uint8)}, "tokenized_prompt": np.zeros((B, L), np.int32),
            "tokenized_prompt_mask": np.ones((B, L), bool), "tokenized_langact_mask": la, "token_loss_mask": tl,
            "critical_token_mask": crit, "number_token_mask": num, "direction_token_mask": np.zeros((B, L), bool)}
    obs = CoTObservation.from_dict(data)
    assert obs.loss_rows_max == 6                # sample 1 / 2: positions 4..9
    assert obs.metric_rows_max == 8              # sample 2: 4..9 plus 1, 2
    del data["critical_token_mask"], data["number_token_mask"], data["direction_token_mask"]
    obs = CoTObservation.from_dict(data)
    assert obs.metric_rows_max == obs.loss_rows_max == 6


# ------------------------------------------------------------------------------------------------ restore_eval_params
def _trees(cfg):
    live = O.init_params(oracle_cfg(cfg), seed=3)
    ema = O.init_params(oracle_cfg(cfg), seed=4)
    return live, ema


def _save(ps, directory, step, has_ema):
    state = types.SimpleNamespace(model=types.SimpleNamespace(ps=ps, comm=object()), ema_decay=0.99 if has_ema else None)
    import pathlib

    mngr = ck.CheckpointManager(pathlib.Path(directory))
    mngr.directory.mkdir(parents=True, exist_ok=True)
    ck.save_state(mngr, state, None, step)


def _fill(ps, live, ema):
    """masters <- live, EMA <- ema (load_reference_tree sets both to the tree it loads)."""
    ps.load_reference_tree(ema)
    keep = {k: v.clone() for k, v in ps.master.items()}
    ps.load_reference_tree(live)
    for k in ps.ema:
        ps.ema[k].copy_(keep[k])


def _worker(rank, world, port, directory):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        cfg = get_config("debug").model
        live, ema = _trees(cfg)
        ps = ParamStore(cfg, "cpu", world_size=world, rank=rank, with_optimizer=True, with_ema=True)
        _fill(ps, live, ema)
        _save(ps, directory, 7, True)
    finally:
        dist.destroy_process_group()


def test_restore_eval_params_any_world_size(tmp_path):
    cfg = get_config("debug").model
    live, ema = _trees(cfg)
    d1, d2, d0 = tmp_path / "w1", tmp_path / "w2", tmp_path / "noema"
    ps = ParamStore(cfg, "cpu", world_size=1, rank=0, with_optimizer=True, with_ema=True)
    _fill(ps, live, ema)
    _save(ps, d1, 7, True)
    port = 29500 + (os.getpid() % 1000)
    mp.spawn(_worker, args=(2, port, str(d2)), nprocs=2, join=True)
    assert sorted(p.name for p in (d2 / "7" / "train_state").iterdir()) == ["meta.json", "rank0_of2.safetensors", "rank1_of2.safetensors"]

    ema1 = ck.restore_eval_params(d1, 7, "ema")
    live1 = ck.restore_eval_params(d1, 7, "live", cfg)
    ema2 = ck.restore_eval_params(ck.CheckpointManager(d2), 7, "ema")
    live2 = ck.restore_eval_params(d2, 7, "live", cfg)
    assert set(live1) == set(ema1) == set(live2) == set(ema2) == set(live)
    for k in live:
        assert torch.equal(live1[k], torch.as_tensor(live[k]).float()), k
        assert torch.equal(ema1[k], torch.as_tensor(ema[k]).float()), k
        assert torch.equal(live2[k], live1[k]) and torch.equal(ema2[k], ema1[k]), k
    assert any(not torch.equal(live1[k], ema1[k]) for k in live)
    with pytest.raises(ValueError, match="model_config"):
        ck.restore_eval_params(d1, 7, "live")
    with pytest.raises(FileNotFoundError):
        ck.restore_eval_params(d1, 8, "ema")

    # a run without EMA: `params/` holds the live parameters, and there is no EMA to score
    ps0 = ParamStore(cfg, "cpu", world_size=1, rank=0, with_optimizer=True, with_ema=False)
    ps0.load_reference_tree(live)
    _save(ps0, d0, 3, False)
    live0 = ck.restore_eval_params(d0, 3, "live")
    assert all(torch.equal(live0[k], live1[k]) for k in live)
    with pytest.raises(ValueError, match="no EMA"):
        ck.restore_eval_params(d0, 3, "ema")


# ----------------------------------------------------------------------------------------------------------- command line
def test_cli_parses_the_comma_list_and_own_options():
    cfg, opts = E.parse_args(["debug", "--exp-name", "run", "--batch-size", "4", "--num-eval-batches", "3",
                              "--eval-checkpoint-steps", "1000,2000", "--eval-use-ema", "false", "--verbose", "true",
                              "--checkpoint-dir", "/x/ck", "--output", "r.json"])
    assert cfg.exp_name == "run" and cfg.batch_size == 4 and cfg.num_eval_batches == 3
    assert cfg.eval_checkpoint_steps == (1000, 2000) and cfg.eval_all_checkpoints is False and cfg.eval_use_ema is False
    assert cfg.model.verbose_mode is True
    assert opts == {"checkpoint_dir": "/x/ck", "output": "r.json"}
    cfg, opts = E.parse_args(["debug", "--exp-name", "run"])
    assert cfg.eval_all_checkpoints is True and cfg.model.verbose_mode is False and opts == {"checkpoint_dir": None, "output": None}


def test_cli_rejects_unknown_and_malformed_options():
    with pytest.raises(SystemExit, match="unknown option --nope"):
        E.parse_args(["debug", "--nope", "1"])
    with pytest.raises(SystemExit, match="comma list"):
        E.parse_args(["debug", "--eval-checkpoint-steps", "10,x"])
    with pytest.raises(SystemExit, match="true / false"):
        E.parse_args(["debug", "--verbose", "maybe"])


def test_evaluator_refuses_several_processes(monkeypatch, tmp_path):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="one process"):
        E.main(_cfg(exp_name="x"), checkpoint_dir=tmp_path)
