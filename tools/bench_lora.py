"""LoRA fine-tuning step vs the full fine-tune step of LAP-3B at the bench shapes (B = 32, `lap_bench`), interleaved on one box.

    python tools/bench_lora.py [--rounds 2] [--steps 6] [--warmup 2]

Each measurement is a fresh child process (`--variant full|lora`, one model per process, so `torch.cuda.max_memory_allocated` is that
variant's alone); the parent alternates full, lora, full, lora, ... and prints one JSON line per child and a summary line:
  full  the plain step: every parameter trainable (bench.py's workload);
  lora  `paligemma_variant="gemma_2b_lora"` with `LAPConfig.get_freeze_filter()` (VLM base weights frozen, its rank-16 adapters, SigLIP,
        the action expert and the heads trainable).
ms per step is wall time over the timed steps after a full device synchronize.  The lora child then runs one more step with a HIP event
pair around every lap_lora_* launch on the compute stream (the per-kernel figures; the timed steps ran without the wrappers)."""
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
    tc = dataclasses.replace(get_config("lap_bench"), batch_size=args.batch)
    if args.variant == "lora":
        model = dataclasses.replace(tc.model, paligemma_variant="gemma_2b_lora")
        tc = dataclasses.replace(tc, model=model, freeze_filter=model.get_freeze_filter())
    state = init_train_state(tc, device=dev)
    runner = TrainingStepRunner(tc)
    batches = [synthetic_batch(tc.model, args.batch, dev, seed=i) for i in range(2)]
    for i in range(args.warmup):
        state, info = runner(0, state, batches[i % 2], state.step)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        state, info = runner(0, state, batches[i % 2], state.step)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    out = {"variant": args.variant, "ms_per_step": round(dt * 1e3, 3), "samples_per_s": round(args.batch / dt, 3),
           "max_memory_allocated_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 2), "loss": round(float(info["loss"]), 5),
           "trainable_params": sum(state.model.ps.tensor_spec[n].numel for n in state.model.ps.names() if state.model.ps.is_trainable(n))}
    if args.variant == "lora":
        rec, main = {}, torch.cuda.current_stream().cuda_stream
        names = ("lora_down", "lora_up_add", "lora_wgrad")
        orig = {n: getattr(hip, n) for n in names}

        def wrap(n):
            def fn(*a, **kw):
                if torch.cuda.current_stream().cuda_stream != main:      # (suffix / weight-gradient streams: counted, not timed)
                    rec.setdefault(n + " (side stream, untimed)", []).append(None)
                    return orig[n](*a, **kw)
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                r = orig[n](*a, **kw)
                e.record()
                rec.setdefault(n, []).append((s, e))
                return r
            return fn
        for n in names:
            setattr(hip, n, wrap(n))
        state, info = runner(0, state, batches[0], state.step)
        torch.cuda.synchronize()
        for n in names:
            setattr(hip, n, orig[n])
        out["lora_kernels_one_step"] = {n: {"calls": len(v), "ms": round(sum(s.elapsed_time(e) for s, e in v), 3) if v[0] else None}
                                        for n, v in rec.items()}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--variant", choices=["full", "lora"])
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    args = ap.parse_args()
    if args.variant:
        return child(args)
    res = {"full": [], "lora": []}
    for r in range(args.rounds):
        for v in ("full", "lora"):
            cmd = [sys.executable, os.path.abspath(__file__), "--variant", v, "--steps", str(args.steps), "--warmup", str(args.warmup),
                   "--batch", str(args.batch)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
            if p.returncode != 0:        # a failed child ends the run: nothing more is started on the device
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"child {v} (round {r}) exited with {p.returncode}")
            line = p.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            res[v].append(json.loads(line))
    summ = {v: {"ms_per_step": [x["ms_per_step"] for x in xs], "max_memory_allocated_gb": max(x["max_memory_allocated_gb"] for x in xs),
                "trainable_params": xs[0]["trainable_params"]} for v, xs in res.items()}
    print(json.dumps({"summary": summ}), flush=True)


if __name__ == "__main__":
    main()
