"""Gradient accumulation at the bench shapes: what a micro-step with the fold costs against the plain step (LAP-3B, `lap_bench`,
32 samples per micro-step), interleaved on one box.

    python tools/bench_accum.py [--rounds 2] [--steps 4] [--warmup 2] [--k 4]

Each measurement is a fresh child process (`--variant plain|accum`); the parent alternates plain, accum, plain, accum, ... and prints
one JSON line per child and a summary line:
  plain  the plain step: batch 32, grad_accum_steps = 1 (bench.py's workload);
  accum  batch 32 x K, grad_accum_steps = K: K forward + backward passes of 32 samples, one optimizer pass.
ms per step is wall time over the timed steps after a full device synchronize; `ms_per_micro_step` divides it by K (the optimizer
pass, once per K micro-steps, is inside).  The accum child then runs one more step with a HIP event pair around every lap_grad_fold
launch on the side stream: their summed elapsed time per micro-step is the time the folds occupy that stream beside the backward's
kernels, not their cost to the step — that is the difference of the two ms figures."""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(args):
    os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")    # as bench.py
    from bench import synthetic_batch
    from lap_amd import hip
    from lap_amd.config import get_config
    from lap_amd.train import TrainingStepRunner, init_train_state

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    K = args.k if args.variant == "accum" else 1
    tc = dataclasses.replace(get_config("lap_bench"), batch_size=args.batch * K, grad_accum_steps=K)
    state = init_train_state(tc, device=dev)
    runner = TrainingStepRunner(tc)
    micro = [synthetic_batch(tc.model, args.batch, dev, seed=i) for i in range(max(K, 2))]
    batch = lambda i: micro[i % 2] if K == 1 else micro[:K]      # noqa: E731
    for i in range(args.warmup):
        state, info = runner(0, state, batch(i), state.step)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        state, info = runner(0, state, batch(i), state.step)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    out = {"variant": args.variant, "k": K, "ms_per_step": round(dt * 1e3, 3), "ms_per_micro_step": round(dt * 1e3 / K, 3),
           "samples_per_s": round(args.batch * K / dt, 3), "max_memory_allocated_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 2),
           "loss": round(float(info["loss"]), 5)}
    if K > 1:
        rec, orig = [], hip.grad_fold

        def fold(acc, g, first, sumsq=None):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            orig(acc, g, first, sumsq)
            e.record()
            rec.append((s, e, acc.numel() * ((0 if first else 4) + 4 + g.element_size())))

        hip.grad_fold = fold
        state, info = runner(0, state, batch(0), state.step)
        torch.cuda.synchronize()
        hip.grad_fold = orig
        ms = sum(s.elapsed_time(e) for s, e, _ in rec)
        gb = sum(b for _, _, b in rec) / 1e9
        out["folds_one_step"] = {"launches": len(rec), "gb": round(gb, 2), "side_stream_ms": round(ms, 3), "side_stream_ms_per_micro_step": round(ms / K, 3),
                                 "gb_per_s_while_running": round(gb / (ms / 1e3), 1)}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=["plain", "accum"])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32, help="samples per micro-step")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child")
    args = ap.parse_args()
    if args.variant:
        return child(args)
    res = {"plain": [], "accum": []}
    for r in range(args.rounds):
        for v in ("plain", "accum"):
            cmd = [sys.executable, os.path.abspath(__file__), "--variant", v, "--steps", str(args.steps), "--warmup", str(args.warmup),
                   "--batch", str(args.batch), "--k", str(args.k)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            if p.returncode != 0:        # a failed child ends the run: nothing more is started on the device
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"child {v} (round {r}) exited with {p.returncode}")
            line = p.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            res[v].append(json.loads(line))
    print(json.dumps({"summary": {v: [x["ms_per_micro_step"] for x in xs] for v, xs in res.items()}}), flush=True)


if __name__ == "__main__":
    main()
