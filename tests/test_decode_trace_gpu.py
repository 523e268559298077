"""The launch sequence of every kind of fused decode context, pinned: `first_token` and two `step`s of a `DecodeCtx`, every library
launch with every argument, against tests/golden/decode_launch_traces.json.  The token and bit suites of the decode modes run the
workload; this one states WHAT is launched, so a dropped, reordered or re-pointed launch (a swapped buffer that happens to hold the
same values) fails here.

A launch is [entry point, argument, ...] in the order of `hip.SIGNATURES` without the stream.  A pointer inside the storage of a
tensor attribute of the context reads "<attribute>+<byte offset>", any other pointer "ext", a null pointer "null"; integers are
themselves and floats their `repr`.

The golden file is recorded with LAP_RECORD_DECODE_TRACES=1 (the test then writes its run's entry instead of comparing) on the commit
BEFORE a change that claims to keep the launches; it is never recorded from the changed tree.  The test imports only
`ar_decode.DecodeCtx`, `ar_decode.prefill`, `ar_decode.replicate_prefill` and `hip`."""
import ctypes
import json
import os

import pytest
import torch

from tests.test_beam_grammar_gpu import _hand_back_stream_scratch, ar  # noqa: F401  (the 2-layer model and the tiny-tokenizer automaton)

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "decode_launch_traces.json")
RECORD = os.environ.get("LAP_RECORD_DECODE_TRACES") == "1"
CAP = 6
REFERENCE = [5, 9, 11, 4]       # the draft of a speculating / jump-forward context, the candidate of a scoring one

# run -> (B, constructor keywords, what the test sets before the decode, whether the debug `logits=` argument is passed).
# "allowed" / "grammar" stand for the device ids / the device automaton of the fixture.
RUNS = {
    "plain_b2": (2, {}, {}, False),
    "plain_logits": (1, {}, {}, True),
    "sampling": (1, {"sampling": True}, {"sampling": (3, 0.7)}, False),
    "logprobs_greedy": (1, {"logprobs": True}, {}, False),
    "logprobs_sampling": (1, {"sampling": True, "logprobs": True}, {"sampling": (3, 0.7)}, False),
    "allowed": (1, {"allowed": True}, {}, False),
    "filter": (1, {"sampling": True, "filtering": True}, {"sampling": (3, 0.7), "filter": (5, 0.9)}, False),
    "filter_allowed": (1, {"sampling": True, "filtering": True, "allowed": True}, {"sampling": (3, 0.7), "filter": (5, 0.9)}, False),
    "filter_logits": (1, {"sampling": True, "filtering": True}, {"sampling": (3, 0.7), "filter": (5, 0.9)}, True),
    "fp8": (1, {"weights": "fp8"}, {}, False),
    "fp8_layers": (1, {"weights": "fp8_layers"}, {}, False),
    "speculate2": (1, {"speculate": 2}, {"draft": REFERENCE}, False),
    "grammar_greedy": (1, {"grammar": True}, {}, False),
    "grammar_logits": (1, {"grammar": True}, {}, True),
    "grammar_sampling_logprobs": (1, {"grammar": True, "sampling": True, "logprobs": True}, {"sampling": (3, 0.7)}, False),
    "jump2_greedy": (1, {"grammar": True, "jump_forward": 2}, {"draft": REFERENCE}, False),
    "jump2_sampling_logprobs": (1, {"grammar": True, "jump_forward": 2, "sampling": True, "logprobs": True},
                                {"sampling": (3, 0.7), "draft": REFERENCE}, False),
    "beams2": (2, {"beams": 2}, {}, False),
    "beams2_allowed": (2, {"beams": 2, "allowed": True}, {}, False),
    "beams2_grammar": (2, {"beams": 2, "grammar": True}, {}, False),
    "score1": (1, {"score": 1}, {"candidate": REFERENCE}, False),
    "score2": (1, {"score": 2}, {"candidate": REFERENCE}, False),
}


def _obs(cfg, B):
    from tests.common import make_inputs, to_observation

    obs, _, _, _ = make_inputs(cfg, B=B, seed=0, ragged=True)
    so = dict(obs)
    so.pop("tokenized_langact_mask")
    so["image_masks"] = {k: torch.ones_like(m) for k, m in so["image_masks"].items()}
    return to_observation(so | {"tokenized_langact_mask": None}, DEV)


def _name_pointer(ctx, p):
    """`p` as "<attribute>+<byte offset>" of the context's tensor attribute whose storage holds it (the first by name), else "ext"."""
    if not p:
        return "null"
    for name in sorted(vars(ctx)):
        t = getattr(ctx, name)
        if isinstance(t, torch.Tensor) and t.is_cuda:
            s = t.untyped_storage()
            if s.data_ptr() <= p < s.data_ptr() + s.nbytes():
                return f"{name}+{p - s.data_ptr()}"
    return "ext"


def _trace(hip, ctx, run):
    """The launches of `run()`: `hip.call` records and calls through while it runs."""
    launches = []
    real = hip.call

    def recording(name, *args):
        sig = hip.SIGNATURES[name]
        assert len(args) == len(sig) - 1 and sig[-1] is ctypes.c_void_p, name       # (the stream is appended by `call`)
        row = [name]
        for kind, a in zip(sig, args):
            if kind is ctypes.c_void_p:
                row.append(_name_pointer(ctx, a))
            elif isinstance(a, float):
                row.append(repr(a))
            else:
                row.append(int(a))
        launches.append(row)
        return real(name, *args)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(hip, "call", recording)
        run()
    torch.cuda.synchronize()
    return launches


def _dump(traces):
    body = ",\n".join(f" {json.dumps(k)}: [\n" + ",\n".join("  " + json.dumps(row) for row in rows) + "\n ]" for k, rows in sorted(traces.items()))
    return "{\n" + body + "\n}\n"


@pytest.mark.parametrize("name", RUNS)
def test_first_token_and_two_steps_launch_what_the_golden_says(hip, ar, name):
    from lap_amd import ar_decode

    cfg, model, a, d = ar
    B, kw, setup, debug = RUNS[name]
    kw = dict(kw)
    if kw.get("allowed"):       # sorted unique int32 ids with the EOS token, on the device
        kw["allowed"] = torch.arange(1, 100, 2, dtype=torch.int32, device=DEV)
    if kw.get("grammar"):
        kw["grammar"] = d
    with model._serving_weights():
        if kw.get("beams"):
            pre = ar_decode.replicate_prefill(ar_decode.prefill(model, _obs(cfg, 1)), B)
        else:
            pre = ar_decode.prefill(model, _obs(cfg, B))
        ctx = ar_decode.DecodeCtx(model, B, pre.Pn, CAP, **kw)
        if "sampling" in setup:
            ctx.set_sampling(*setup["sampling"])
        if "filter" in setup:
            ctx.set_filter(*setup["filter"])
        if "draft" in setup:
            ctx.set_draft(setup["draft"])
        if "candidate" in setup:
            ctx.set_candidate(setup["candidate"])
        lg = torch.empty((B, cfg.vocab_size), dtype=torch.float32, device=DEV) if debug else None

        def decode(steps):
            ctx.first_token(pre, lg)
            for _ in range(steps):
                ctx.step(lg)

        decode(1)       # untraced: what the model builds on first use (the fp8 weights) is built here
        got = _trace(hip, ctx, lambda: decode(2))
    assert got and got[0][0] == "lap_decode_init"
    traces = {}
    if os.path.exists(GOLDEN):
        with open(GOLDEN) as f:
            traces = json.load(f)
    if RECORD:
        traces[name] = got
        with open(GOLDEN, "w") as f:
            f.write(_dump(traces))
        return
    assert name in traces, f"{GOLDEN} has no entry for {name}"
    want = traces[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{name}: launch {i} is {g}, the golden says {w}"
    assert len(got) == len(want), f"{name}: {len(got)} launches, the golden says {len(want)}"
