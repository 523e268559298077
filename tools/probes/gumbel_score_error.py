"""How far the device sampler's scores (logit * inv_t + Gumbel noise, lap_amd/csrc/sampling.hpp) lie from their host restatement
(lap_amd/sampling.py): the largest |device - host| over the inputs of tests/test_ar_sampling_gpu.py's Gumbel-argmax test, from
the debug build of the score (tools/probes/gumbel_scores.hip; the production kernels keep only the argmax).  That test's TIE is
four times the figure printed here.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fno-slp-vectorize -shared tools/probes/gumbel_scores.hip -o tools/probes/gumbel_scores.so
    python tools/probes/gumbel_score_error.py [--scan-seeds N]

--scan-seeds N: instead, for seeds 1 .. N, the smallest top-2 margin of the eager device-sampled scores at every step of that
test file's model cases, with the embedding table as initialised (the 12 - 14 margins that made the file scale the table down)
or with --embed-scale S.
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import pytest
import torch

from lap_amd import hip
from lap_amd import sampling as S
from tests import test_ar_sampling_gpu as T

ap = argparse.ArgumentParser()
ap.add_argument("--scan-seeds", type=int, default=0)
ap.add_argument("--embed-scale", type=float, default=1.0)
a = ap.parse_args()

if a.scan_seeds:
    from lap_amd.model import LAP
    from oracle import lap_oracle as O
    from tests.common import oracle_cfg

    with pytest.MonkeyPatch.context() as mp:
        cfg = T._gemma2b_x2_cfg(mp)
        P = O.init_params(oracle_cfg(cfg), seed=13)
        key = "PaliGemma/llm/embedder/input_embedding"
        P[key] = torch.as_tensor(P[key]).clone() * a.embed_scale
        model = LAP(cfg, params=P, device="cuda")
        obs = {case: T._to_obs(T._obs(cfg, case)) for case in ("ragged", "langact")}
        for seed in range(1, a.scan_seeds + 1):
            row = {"seed": seed}
            for case, o in obs.items():
                col = {}
                model.sample_tokens(seed, o, max_decoding_steps=T.STEPS, temperature=1.0, sampler="device", collect=col)
                row[case] = [round(float(T._margins(col[f"logit/{s}"], 1.0, seed, s).min()), 4) for s in range(T.STEPS)]
            row["first3_min"] = min(min(row[c][:3]) for c in obs)
            print(json.dumps(row), flush=True)
    sys.exit(0)

lib = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "gumbel_scores.so"))
fn = lib.probe_gumbel_scores
fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_uint, ctypes.c_uint, ctypes.c_int, ctypes.c_void_p,
               ctypes.c_void_p]
fn.restype = ctypes.c_int
worst, worst_g, big, rows = 0.0, 0.0, 0.0, 0
for B in (1, 3, 8):
    lg = T._gumbel_inputs(B)
    x = lg.cuda().contiguous()
    out = torch.empty_like(x)
    zero = torch.zeros_like(x)
    for step in range(T.GUMBEL_STEPS):
        temp = (0.5, 1.0, 2.0)[step % 3]
        lo, hi, inv_t = hip.sampling_words(T.GUMBEL_SEED, temp)
        assert fn(x.data_ptr(), B, x.shape[1], inv_t, lo, hi, step, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        dev = out.cpu().numpy()
        host = S.scores_from_logits(lg.numpy(), temp, T.GUMBEL_SEED, step)
        worst = max(worst, float(np.abs(dev.astype(np.float64) - host.astype(np.float64)).max()))
        big = max(big, float(np.abs(host).max()))
        # the noise alone (zero logits)
        assert fn(zero.data_ptr(), B, x.shape[1], inv_t, lo, hi, step, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
        g = S.gumbel_noise(T.GUMBEL_SEED, step, B, x.shape[1])
        worst_g = max(worst_g, float(np.abs(out.cpu().numpy().astype(np.float64) - g.astype(np.float64)).max()))
        rows += B
print(json.dumps({"rows": rows, "scores_per_row": T.V_FULL, "max_abs_score_error": worst, "max_abs_noise_error": worst_g,
                  "max_abs_host_score": big, "ulp_of_f32_at_16": 2.0 ** -19}))
