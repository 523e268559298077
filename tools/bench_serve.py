"""Batch-1 action-chunk latency of LAP-3B on one MI355X (BASELINE.json config 4): prefix prefill + 10 denoise steps.
`--num-samples N[,N...]`: ms per chunk of best-of-N (`GraphedSampler(num_samples=N)`: one prefill, shared prefix cache), graph-replayed;
`--replicated` adds the way without it — the observation replicated N times, `GraphedSampler(batch_size=N)` — and `--unshared` the
`share_prefix=False` form; the variants are timed in interleaved rounds and reported as median [min, max] over the rounds."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from lap_amd.config import get_config
from lap_amd.model import LAP
from lap_amd.serve import GraphedSampler

ap = argparse.ArgumentParser()
ap.add_argument("config", nargs="?", default="lap_bench")
ap.add_argument("--num-samples", default=None, help="comma-separated candidate counts, e.g. 1,2,4,8")
ap.add_argument("--replicated", action="store_true")
ap.add_argument("--unshared", action="store_true")
ap.add_argument("--select", default=None, choices=["medoid"])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--replays", type=int, default=10)
args = ap.parse_args()
cfg = get_config(args.config).model
dev = "cuda"
model = LAP(cfg, seed=0, device=dev, with_grads=False)
g = GraphedSampler(model, 1, 10)
gen = torch.Generator(device="cpu").manual_seed(0)
for k in g.obs.images:
    g.obs.images[k].copy_(torch.rand(1, 224, 224, 3, generator=gen) * 2 - 1)
g.obs.tokenized_prompt.copy_(torch.randint(0, cfg.vocab_size, g.obs.tokenized_prompt.shape, generator=gen, dtype=torch.int32))
noise = torch.randn(1, cfg.action_horizon, cfg.action_dim, generator=gen).to(dev)
g.noise.copy_(noise)

def timeit(fn, n):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / n * 1e3

def fill(sampler):
    """The same request in every sampler (a batch repeats it); noise per row from the one generator stream."""
    for k in sampler.obs.images:
        sampler.obs.images[k].copy_(g.obs.images[k].expand_as(sampler.obs.images[k]))
    sampler.obs.tokenized_prompt.copy_(g.obs.tokenized_prompt.expand_as(sampler.obs.tokenized_prompt))
    sampler.noise.copy_(torch.randn(sampler.noise.shape, generator=torch.Generator(device="cpu").manual_seed(1)).to(dev))
    return sampler.capture()


if args.num_samples:
    out = {"metric": "ms per chunk request, LAP-3B bf16 (prefill + 10 denoise steps), hipGraph replay, median [min, max] over rounds",
           "rounds": args.rounds, "replays_per_round": args.replays, "results": {}}
    for N in [int(x) for x in args.num_samples.split(",")]:
        variants = {"shared": fill(GraphedSampler(model, 1, 10, num_samples=N, select=args.select if N > 1 else None))}
        if args.unshared and N > 1:
            variants["unshared"] = fill(GraphedSampler(model, 1, 10, num_samples=N, share_prefix=False))
        if args.replicated:
            variants["replicated"] = fill(GraphedSampler(model, N, 10))
        times = {k: [] for k in variants}
        for v in variants.values():
            timeit(v.graph.replay, 3)
        for _ in range(args.rounds):
            for k, v in variants.items():
                times[k].append(timeit(v.graph.replay, args.replays))
        out["results"][N] = {k: [round(statistics.median(t), 3), round(min(t), 3), round(max(t), 3)] for k, t in times.items()}
        del variants
    print(json.dumps(out))
    sys.exit(0)

eager = lambda: model.sample_actions(0, g.obs, num_steps=10, noise=g.noise)
for _ in range(2): eager()
t_eager = timeit(eager, 5)
ref = eager().clone()
g.capture()
t_graph = timeit(g.graph.replay, 20)
def one():
    g.graph.replay(); torch.cuda.synchronize()
t_one = timeit(one, 20)
same = torch.equal(ref, g.out)
bytes_min = 4.79e9 + 10 * 0.86e9 + 10 * 10.3e6
print(json.dumps({"metric": "batch-1 action-chunk latency LAP-3B bf16 (prefill + 10 denoise steps)", "eager_ms": round(t_eager, 3),
                  "hipgraph_ms": round(t_graph, 3), "hipgraph_one_at_a_time_ms": round(t_one, 3), "graph_equals_eager": bool(same), "hbm_floor_ms_at_6.29TBps": round(bytes_min / 6.29e12 * 1e3, 2),
                  "achieved_GBps_vs_algorithmic_bytes": round(bytes_min / (t_graph * 1e-3) / 1e9, 1),
                  "prompt_len": cfg.max_token_len, "action_horizon": cfg.action_horizon}))
