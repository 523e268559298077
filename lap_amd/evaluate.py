"""Checkpoint evaluation: scripts/eval.py of the reference on the MI355X engine.

    python -m lap_amd.evaluate <config> --exp-name NAME [--checkpoint-dir DIR] [--batch-size N] [--num-eval-batches N]
        [--eval-checkpoint-steps 1000,2000] [--eval-use-ema false] [--verbose true] [--output results.json]

For every selected checkpoint step (`select_checkpoint_steps`, eval.py:241-283) the weights are loaded into one model created
once: the EMA parameters when the checkpoint has them, `eval_use_ema` is set and the step is at or past the EMA start step,
else the live ones (eval.py:352-364; `checkpoints.restore_eval_params`, any world size of the writing run).  Then two modes run
over each dataset:
    val_loss                 ValidationStepRunner (compute_loss(train=False, verbose_mode=config.model.verbose_mode)), the
                             scalar metrics averaged over the batches (eval.py:121-151,434-532);
    action_prediction_loss   sample_actions against the batch's actions, the per-sample MSE on the GPU (eval.py:154-188,535-636);
                             skipped for configs without action training.
Datasets: "original" (the config's data on `eval_split`) and "eval_demo_dataset" (val_fraction = 1.0, eval.py:292-306) when
`data.data_mix` is set and a loader for it is given.  Results are keyed `step_{s}/{mode}/{dataset}/eval/{mode}/{key}`.
"""
from __future__ import annotations

import dataclasses
import json
import logging
import os

import torch

from lap_amd.config import TrainConfig

EVAL_MODES = ("val_loss", "action_prediction_loss")


def select_checkpoint_steps(available, config: TrainConfig) -> list[int]:
    """eval.py:241-283: all checkpoints, the listed steps, one step, or the latest; then the `eval_start_from_step` filter."""
    available = sorted(int(s) for s in available)
    if config.eval_all_checkpoints:
        steps = list(available)
        logging.info("Evaluating all %d checkpoints: %s", len(steps), steps)
    elif config.eval_checkpoint_steps is not None:
        steps = [int(s) for s in config.eval_checkpoint_steps]
        missing = [s for s in steps if s not in available]
        if missing:
            raise ValueError(f"Requested checkpoint steps {missing} not found. Available steps: {available}")
        logging.info("Evaluating specified checkpoint steps: %s", steps)
    elif config.eval_checkpoint_step is not None:
        steps = [int(config.eval_checkpoint_step)]
        if steps[0] not in available:
            raise ValueError(f"Requested checkpoint step {steps[0]} not found. Available steps: {available}")
        logging.info("Evaluating single checkpoint step: %d", steps[0])
    else:
        latest = available[-1] if available else None
        logging.info("No checkpoint step specified, using latest: %s", latest)
        steps = [latest]
    if config.eval_start_from_step is not None:
        n = len(steps)
        steps = [s for s in steps if s is not None and s >= config.eval_start_from_step]
        if n - len(steps) > 0:
            logging.info("Skipping %d checkpoints before step %d. Remaining: %s", n - len(steps), config.eval_start_from_step, steps)
        if not steps:
            raise ValueError(f"No checkpoints found >= eval_start_from_step={config.eval_start_from_step}. Available steps: {available}")
    return steps


def uses_ema(step: int, has_ema: bool, config: TrainConfig) -> bool:
    """eval.py:352-364: the EMA parameters iff the checkpoint has them, `eval_use_ema` is set and step >= the EMA start step."""
    start = getattr(config.ema_schedule_choice, "start_step", 0) or 0
    return bool(has_ema and config.eval_use_ema and step >= start)


def _scalar_means(infos: list, mode: str) -> dict:
    """eval.py:517-532 / 622-636: the mean over batches of every scalar metric, plus the batch count."""
    out = {}
    if infos:
        for k in infos[0]:
            vals = [i[k] for i in infos if k in i and torch.is_tensor(i[k]) and i[k].numel() == 1]
            if vals:
                out[f"eval/{mode}/{k}"] = float(torch.stack([v.float().reshape(()) for v in vals]).mean())
    out[f"eval/{mode}/num_batches"] = len(infos)
    return out


def _batches(loader, num_batches):
    for i, batch in enumerate(iter(loader)):     # a fresh iterator: every checkpoint scores the same batches
        if num_batches is not None and i >= num_batches:
            break
        yield batch


def evaluate_validation_loss(config: TrainConfig, rng, state, loader, num_batches) -> dict:
    from lap_amd.train import ValidationStepRunner

    runner = ValidationStepRunner(config)
    return _scalar_means([runner(rng, state, batch) for batch in _batches(loader, num_batches)], "val_loss")


@torch.no_grad()
def action_prediction_info(model, seed, observation, actions) -> dict:
    """ActionPredictionLossEvaluator (eval.py:154-188): per-sample mean squared error of the sampled actions against the batch's."""
    from lap_amd import hip

    pred = model.sample_actions(seed, observation).to(torch.float32)
    B = pred.shape[0]
    gt = actions.to(pred.device, torch.float32).reshape(B, -1).contiguous()
    per, _ = hip.mse_fwd_bwd(pred.reshape(B, -1).contiguous(), gt, None, need_grad=False)
    return {"action_prediction_loss": per.mean(), "per_sample_action_prediction_loss": per}


def evaluate_action_prediction_loss(config: TrainConfig, rng, state, loader, num_batches) -> dict:
    seed = int(rng) * 1_000_003 + state.step          # fold_in(rng, step), as ValidationStepRunner
    infos = [action_prediction_info(state.model, seed, obs, act) for obs, act in _batches(loader, num_batches)]
    return _scalar_means(infos, "action_prediction_loss")


def load_eval_weights(model, checkpoint_manager, step: int, which: str, model_config) -> None:
    """The checkpoint's EMA or live parameters into `model` (created once): masters, bf16 mirrors and the table's residual plane are
    rewritten and the store version moves on, so cached derived weights (merged LoRA, serving packs, fp8 mirrors) rebuild."""
    from lap_amd import checkpoints as ck

    tree = ck.restore_eval_params(checkpoint_manager, step, which, model_config)
    model.ps.load_reference_tree(tree)      # masters + mirrors per unit, each write bumps ps.version


def main(config: TrainConfig, *, checkpoint_dir=None, data_loaders: dict | None = None, device: str | None = None,
         output=None, log=print) -> dict:
    """eval.py:191-433.  `data_loaders`: {"original": loader, "eval_demo_dataset": loader} (either may be missing; "original" falls
    back to the synthetic loader).  Returns {f"step_{s}/{mode}/{dataset}/eval/{mode}/{key}": float}; with `output` also as JSON."""
    import pathlib

    from lap_amd import checkpoints as ck
    from lap_amd.model import LAP
    from lap_amd.params import ParamStore
    from lap_amd.train import SyntheticDataLoader, TrainState

    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise RuntimeError("lap_amd.evaluate runs in one process on one GPU (it scores checkpoints of any world size): "
                           "start it without torch.distributed.run")
    ckdir = pathlib.Path(checkpoint_dir) if checkpoint_dir is not None else config.checkpoint_dir
    mngr = ck.CheckpointManager(ckdir, keep_period=config.keep_period)
    available = list(mngr.all_steps())
    log(f"available checkpoints: {available}")
    if not available:
        raise FileNotFoundError(f"no committed checkpoint under {ckdir}")
    steps = select_checkpoint_steps(available, config)
    num_batches = config.num_eval_batches
    data_loaders = dict(data_loaders or {})
    if device is None:
        device = "cuda"
    loaders = {"original": data_loaders.get("original")}
    if loaders["original"] is None:
        loaders["original"] = SyntheticDataLoader(config.model, config.batch_size, device, seed=config.seed + 7919,
                                                  num_batches=num_batches if num_batches is not None else 1)
    if getattr(config.data, "data_mix", None) is not None:
        if data_loaders.get("eval_demo_dataset") is not None:     # data_mix="eval_demo_dataset", val_fraction=1.0 (eval.py:292-306)
            loaders["eval_demo_dataset"] = data_loaders["eval_demo_dataset"]
        else:
            log("skipping dataset eval_demo_dataset: no loader for it (the episode store has no such dataset)")
    modes = list(EVAL_MODES)
    if not config.model.enable_action_training:
        modes.remove("action_prediction_loss")
        log("skipping mode action_prediction_loss: the config trains no action expert")

    store = ParamStore(config.model, device, with_optimizer=False, with_ema=False, with_grads=False)
    model = LAP(config.model, device=device, store=store, gemm_dtype=config.gemm_dtype)
    results = {}
    for step in steps:
        meta = json.loads((mngr.step_dir(step) / "train_state" / "meta.json").read_text())
        which = "ema" if uses_ema(step, bool(meta["has_ema"]), config) else "live"
        log(f"step {step}: evaluating the {'EMA' if which == 'ema' else 'live'} parameters")
        load_eval_weights(model, mngr, step, which, config.model)
        state = TrainState(step=int(meta["step"]), model=model, ema_decay=None)
        for mode in modes:
            for name, loader in loaders.items():
                fn = evaluate_validation_loss if mode == "val_loss" else evaluate_action_prediction_loss
                res = fn(config, config.seed, state, loader, num_batches)
                prefix = f"step_{step}/{mode}/{name}"
                results.update({f"{prefix}/{k}": v for k, v in res.items()})
                log(f"step {step} {mode} {name}: " + ", ".join(f"{k.split('/')[-1]}={v:.4f}" for k, v in res.items()))
    if output is not None:
        pathlib.Path(output).write_text(json.dumps(results, indent=1, sort_keys=True))
    return results


_OWN_OPTIONS = ("--checkpoint-dir", "--eval-checkpoint-steps", "--verbose", "--output")


def parse_args(argv=None) -> tuple[TrainConfig, dict]:
    """`<config> [--field value ...]`: the scalar TrainConfig fields through config.cli, plus --eval-checkpoint-steps (comma list),
    --verbose (the model's verbose_mode), --checkpoint-dir and --output.  Returns (config, {"checkpoint_dir", "output"})."""
    import sys

    from lap_amd.config import cli

    argv = list(sys.argv[1:] if argv is None else argv)
    rest, own = [], {}
    i = 0
    while i < len(argv):
        a = argv[i]
        if a in _OWN_OPTIONS:
            if i + 1 >= len(argv):
                raise SystemExit(f"{a} expects a value")
            own[a] = argv[i + 1]
            i += 2
        else:
            rest.append(a)
            i += 1
    config = cli(rest)
    upd = {}
    if "--eval-checkpoint-steps" in own:
        try:
            upd["eval_checkpoint_steps"] = tuple(int(s) for s in own["--eval-checkpoint-steps"].split(",") if s.strip())
        except ValueError:
            raise SystemExit(f"--eval-checkpoint-steps expects a comma list of integers, got {own['--eval-checkpoint-steps']!r}") from None
        if "--eval-all-checkpoints" not in rest:     # eval.py:244 checks eval_all_checkpoints (default True) first
            upd["eval_all_checkpoints"] = False
    if "--verbose" in own:
        v = own["--verbose"].lower()
        if v not in ("1", "0", "true", "false"):
            raise SystemExit(f"--verbose expects true / false, got {own['--verbose']!r}")
        upd["model"] = dataclasses.replace(config.model, verbose_mode=v in ("1", "true"))
    return dataclasses.replace(config, **upd), {"checkpoint_dir": own.get("--checkpoint-dir"), "output": own.get("--output")}


if __name__ == "__main__":
    logging.basicConfig(level=logging.INFO)
    cfg, opts = parse_args()
    main(cfg, **opts)
