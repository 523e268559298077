"""One validation step (compute_loss(train=False)) of `lap_bench` at B = 32 with or without verbose metrics, for a kernel-trace
comparison of the language-loss pass: the plain cross-entropy update against the fused one that also tracks the row argmax, and
the token-metrics launch.

    rocprofv3 --kernel-trace --stats -d OUT -o val -- python tools/profile_verbose_val.py --verbose 0|1 [--steps 5]

The synthetic batch carries no class masks, so `metric_rows_max = loss_rows_max` and both runs compute the same rows."""
import argparse
import dataclasses
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--verbose", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    args = ap.parse_args()
    import torch

    from lap_amd.config import get_config
    from lap_amd.model import LAP
    from lap_amd.params import ParamStore
    from lap_amd.train import SyntheticDataLoader

    cfg = get_config("lap_bench").model
    model = LAP(cfg, device="cuda", store=ParamStore(cfg, "cuda", with_optimizer=False, with_ema=False, with_grads=False))
    obs, actions = next(iter(SyntheticDataLoader(cfg, args.batch, "cuda", seed=0, num_batches=1)))
    obs = dataclasses.replace(obs, metric_rows_max=obs.loss_rows_max)
    for i in range(args.steps):
        with torch.no_grad():
            loss, m = model.compute_loss(i, obs, actions, train=False, verbose_mode=bool(args.verbose))
    torch.cuda.synchronize()
    print(f"verbose={args.verbose} loss={float(loss):.5f} token_accuracy={float(m['token_accuracy']) if 'token_accuracy' in m else None}")


if __name__ == "__main__":
    main()
