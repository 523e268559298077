"""The outputs of the fused decode kernels (csrc/decode.hip) pinned bit for bit (GPU).

tests/test_decode_reference_gpu.py holds the kernels to float64 within a tolerance, and tests/test_constrained_decode_gpu.py compares
the subset LM head with the full one of the same build: since both run ONE statement of the row dot product (lm_row_pair), that
comparison holds by construction.  Neither says that a logit is the bits it was before a change to that statement.  This module
does: tests/golden/decode_bits_v1.json holds, per case, the sha256 of the bytes of every output (the tokens in clear) as the
kernels wrote them at the commit the fixture names, before the LM-head bodies and the weight-stream loops were merged, and the
kernels of the tree must reproduce them.  A change that adds a rounding point, reorders a sum or moves a k to another lane fails
here; one that means to do so re-records the fixture (tests/golden/make_decode_bits_golden.py) and says so.

Inputs are drawn on the CPU from seeded generators (tests/decode_reference.py) and copied to the device, so nothing depends on the
device RNG; the fixture holds their sha256 too, and a platform whose generators do not reproduce them fails with that message.
Cases.  LM head: D 2048, V 8195 (one grid pass of the full kernel covers 1024 x 4 x 2 = 8192 rows: the grid-stride loop runs once
more with a full unit and the odd tail unit), B in {1, 5, 8} (both unroll branches, the lane-b sampler at a B that is no power of
two), planes hi + lo / hi alone / fp8, greedy and sampling at temperature 1.0 with a fixed seed and step; the debug logits, pval,
pidx and the tokens.  Projections: B in {1, 5, 8}, bf16 and fp8; qkv (q and both cache planes), gate_up, proj_residual at
K 2048 and K 16384 with kwaves 1 and 4, N = 70 (35 units: a partial last block at kwaves 1).
"""
import hashlib
import json
import pathlib

import pytest
import torch

from tests import decode_reference as C
from tests.decode_reference import DH, DHD, DNH

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = pathlib.Path(__file__).parent / "golden" / "decode_bits_v1.json"
V = 8195
BATCHES = (1, 5, 8)
TEMPERATURE, SEED, STEP = 1.0, 21, 3
RES_N = 70
PROJECTIONS = ("qkv", "gate_up", "res2048", "res16384")
WEIGHTS = ("bf16", "fp8")


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _lm_inputs(form):
    c = C.lm_case(V, form)
    return c, ("x", "gamma") + (("codes", "scales") if form == "fp8" else ("hi", "lo"))


def _proj_inputs(kind, fp8):
    c = C.decode_case(kind, fp8, RES_N if kind.startswith("res") else None)
    return c, (("a", "res") if kind.startswith("res") else ("x", "gamma")) + (("codes", "scales") if fp8 else ("w",))


def input_hashes():
    out = {}
    for form in C.LM_FORMS:
        c, names = _lm_inputs(form)
        out.update({f"lm/{form}/{n}": sha(c[n]) for n in names})
    for kind in PROJECTIONS:
        for wt in WEIGHTS:
            c, names = _proj_inputs(kind, wt == "fp8")
            out.update({f"{kind}/{wt}/{n}": sha(c[n]) for n in names})
    return out


def _state(hip, B, t, plen):
    st = hip.decode_state(B, DEV)
    st[0] = t
    st[16:16 + B] = torch.as_tensor(plen, dtype=torch.int32)[:B]
    return st


def _up(c, names):
    return {n: c[n].to(DEV).contiguous() for n in names}


def lm_results(hip, form):
    """{case: {array: sha256 | tokens}} of the full LM heads on the planes of `form`."""
    c, names = _lm_inputs(form)
    d = _up(c, names)
    hi, lo, ws = (d["codes"], None, d["scales"]) if form == "fp8" else (d["hi"], d["lo"] if form == "hilo" else None, None)
    samp = hip.decode_sampling(DEV)
    hip.decode_set_sampling(samp, SEED, TEMPERATURE)
    out = {}
    for B in BATCHES:
        x = d["x"][:B].contiguous()
        for mode in ("greedy", "sample"):
            st = _state(hip, B, STEP, [5] * 8)
            tok = torch.zeros(B, STEP + 2, dtype=torch.int32, device=DEV)
            pval, pidx = hip.decode_lm_partials(B, DEV)
            pval.fill_(float("nan")); pidx.fill_(-7)
            lg = torch.full((B, V), float("nan"), dtype=torch.float32, device=DEV)
            if mode == "sample":
                hip.decode_lm_head_sample(st, samp, x, d["gamma"], hi, lo, pval, pidx, logits=lg, wscale=ws)
            else:
                hip.decode_lm_head(st, x, d["gamma"], hi, lo, pval, pidx, logits=lg, wscale=ws)
            hip.decode_finish(st, pval, pidx, tok, eos_token=-1)
            out[f"lm/{form}/B{B}/{mode}"] = {"logits": sha(lg), "pval": sha(pval), "pidx": sha(pidx), "tokens": tok[:, STEP].tolist()}
    return out


def projection_results(hip, kind, wt):
    c, names = _proj_inputs(kind, wt == "fp8")
    d = _up(c, names)
    w, ws = (d["codes"], d["scales"]) if wt == "fp8" else (d["w"], None)
    out = {}
    for B in BATCHES:
        if kind == "qkv":
            cap, t = C.QKV_CAP, C.QKV_T
            ck = torch.zeros(B, cap, DHD, dtype=torch.bfloat16, device=DEV)
            cv, q = torch.zeros_like(ck), torch.zeros(B, DNH * DHD, dtype=torch.bfloat16, device=DEV)
            hip.decode_qkv(_state(hip, B, t, c["plen"]), d["x"][:B].contiguous(), d["gamma"], w, q, ck, cv, DNH, DHD, c["q_scale"], wscale=ws)
            out[f"qkv/{wt}/B{B}"] = {"q": sha(q), "cache_k": sha(ck), "cache_v": sha(cv)}
        elif kind == "gate_up":
            act = torch.zeros(B, DH, dtype=torch.bfloat16, device=DEV)
            hip.decode_gate_up(_state(hip, B, 1, [10] * 8), d["x"][:B].contiguous(), d["gamma"], w, act, wscale=ws)
            out[f"gate_up/{wt}/B{B}"] = {"act": sha(act)}
        else:
            for kwaves in (1, 4):
                y = torch.zeros(B, RES_N, dtype=torch.bfloat16, device=DEV)
                hip.decode_proj_residual(_state(hip, B, 1, [10] * 8), d["a"][:B].contiguous(), w, d["res"][:B].contiguous(), y, kwaves=kwaves,
                                         wscale=ws)
                out[f"{kind}/{wt}/kwaves{kwaves}/B{B}"] = {"y": sha(y)}
    return out


@pytest.fixture(scope="module")
def golden():
    g = json.loads(FIXTURE.read_text())
    got = input_hashes()
    bad = sorted(k for k in g["inputs"] if got.get(k) != g["inputs"][k])
    assert not bad and len(got) == len(g["inputs"]), (
        f"the CPU generators of torch {torch.__version__} do not reproduce the inputs the fixture was recorded on (torch {g['torch']}): {bad}")
    return g["results"]


def _compare(got, golden):
    bad = [f"{case}: {name}" for case, arrays in got.items() for name, v in arrays.items() if golden.get(case, {}).get(name) != v]
    assert not bad, f"outputs that are no longer the recorded bits (case: array): {bad}"
    assert all(set(golden[case]) == set(arrays) for case, arrays in got.items())


def test_fixture_is_complete(golden):
    cases = ([f"lm/{f}/B{B}/{m}" for f in C.LM_FORMS for B in BATCHES for m in ("greedy", "sample")]
             + [f"{k}/{w}/B{B}" for k in ("qkv", "gate_up") for w in WEIGHTS for B in BATCHES]
             + [f"{k}/{w}/kwaves{kw}/B{B}" for k in ("res2048", "res16384") for w in WEIGHTS for kw in (1, 4) for B in BATCHES])
    assert sorted(golden) == sorted(cases)


@pytest.mark.parametrize("form", C.LM_FORMS)
def test_lm_head_bits(hip, golden, form):
    _compare(lm_results(hip, form), golden)


@pytest.mark.parametrize("wt", WEIGHTS)
@pytest.mark.parametrize("kind", PROJECTIONS)
def test_projection_bits(hip, golden, kind, wt):
    _compare(projection_results(hip, kind, wt), golden)
