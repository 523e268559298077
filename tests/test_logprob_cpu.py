"""Token log-probabilities and best-of-N selection: the host restatement (lap_amd/sampling.py), the argument checks of
`num_samples` and the two entry points of the built library (no GPU)."""
import pathlib
import re

import numpy as np
import pytest

from lap_amd import sampling as S

ROOT = pathlib.Path(__file__).resolve().parents[1]


def _log_softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max(axis=-1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))


def test_token_logprobs_matches_float64_log_softmax():
    rng = np.random.default_rng(0)
    lg = (rng.standard_normal((4, 301)) * 3).astype(np.float32)
    tok = rng.integers(0, 301, size=4)
    rows = np.arange(4)
    # greedy (temperature <= 0): z is the logit
    for T in (0.0, -1.0):
        got = S.token_logprobs(lg, tok, T)
        assert got.dtype == np.float64 and got.shape == (4,)
        assert np.array_equal(got, _log_softmax64(lg)[rows, tok])
    # a temperature: z is the float32 product, the rest float64
    for T in (0.7, 2.0):
        z = lg * S.inverse_temperature(T)
        assert z.dtype == np.float32
        assert np.array_equal(S.token_logprobs(lg, tok, T), _log_softmax64(z)[rows, tok])
    assert np.allclose(np.exp(np.stack([S.token_logprobs(lg, np.full(4, j), 0.7) for j in range(301)])).sum(0), 1.0, atol=1e-12)


def test_token_logprobs_allowed_set():
    rng = np.random.default_rng(1)
    lg = (rng.standard_normal((3, 64)) * 2).astype(np.float32)
    ids = np.array([5, 9, 9, 2, 40])          # order and duplicates do not matter
    tok = np.array([2, 40, 9])
    z = (lg * S.inverse_temperature(1.5))[:, [2, 5, 9, 40]]
    want = _log_softmax64(z)[np.arange(3), [0, 3, 2]]
    assert np.array_equal(S.token_logprobs(lg, tok, 1.5, allowed=ids), want)
    # an id outside the vocabulary is left out, as the kernel leaves it out
    assert np.array_equal(S.token_logprobs(lg, tok, 1.5, allowed=[5, 9, 2, 40, 64 + 5]), want)
    # a token outside the set has probability 0
    assert S.token_logprobs(lg, [3, 40, 9], 1.5, allowed=ids)[0] == -np.inf
    # one element: exactly 0
    one = S.token_logprobs(lg, [7, 7, 7], 0.7, allowed=[7])
    assert np.array_equal(one, np.zeros(3)) and not np.signbit(one).any()


def test_token_logprobs_large_logits_do_not_overflow():
    rng = np.random.default_rng(2)
    lg = (rng.standard_normal((5, 257)) * 1e3).astype(np.float32)
    tok = rng.integers(0, 257, size=5)
    with np.errstate(over="raise", invalid="raise", divide="raise"):     # (exp of a far-below-maximum z underflows to 0: fine)
        for T in (0.0, 0.7):
            got = S.token_logprobs(lg, tok, T)
            assert np.isfinite(got).all() and (got <= 0).all()
    best = lg.argmax(1)
    assert (S.token_logprobs(lg, best, 0.0) > -1e3).all()
    lg[:] = 1e3                                 # flat: log(1 / V)
    assert np.allclose(S.token_logprobs(lg, tok, 0.0), -np.log(257), rtol=0, atol=1e-12)


def test_sequence_logprob_stops_at_the_first_eos():
    eos = 1
    tok = np.array([[1, 4, 1, 6],           # EOS in the first column
                    [3, 1, 5, 1],           # in the middle (and again later)
                    [3, 4, 5, 6],           # absent
                    [3, 4, 5, 1]])          # in the last column
    lp = -np.array([[1, 2, 4, 8], [1, 2, 4, 8], [1, 2, 4, 8], [1, 2, 4, 8]], dtype=np.float32)
    got = S.sequence_logprob(tok, lp, eos)
    assert got.dtype == np.float64 and np.array_equal(got, [-1.0, -3.0, -15.0, -15.0])
    with pytest.raises(ValueError):
        S.sequence_logprob(tok, lp[:, :3], eos)


def test_select_best_rules_and_ties():
    eos = 1
    tok = np.array([[3, 4, 5, 1], [3, 1, 0, 0], [3, 4, 1, 0]])
    lp = -np.array([[1, 1, 1, 1], [2, 1.5, 9, 9], [1, 1, 1.5, 9]], dtype=np.float32)
    # sums -4, -3.5, -3.5 -> rows 1 and 2 tie: the lowest; means -1, -1.75, -1.1667 -> row 0
    assert np.array_equal(S.sequence_logprob(tok, lp, eos), [-4.0, -3.5, -3.5])
    assert S.select_best(tok, lp, eos, "sum") == 1 and S.select_best(tok, lp, eos) == 1
    assert S.select_best(tok, lp, eos, "mean") == 0
    assert S.select_best(tok[::-1], lp[::-1], eos, "sum") == 0            # the tie again, the other way round
    same = np.tile(tok[:1], (4, 1)), np.tile(lp[:1], (4, 1))
    assert S.select_best(*same, eos, "sum") == 0 and S.select_best(*same, eos, "mean") == 0
    with pytest.raises(ValueError):
        S.select_best(tok, lp, eos, "max")


def test_num_samples_argument_checks():
    from lap_amd import ar_decode

    ok = dict(decode="fused", sampler="device", temperature=1.0)
    assert ar_decode.check_num_samples(1, 1, **ok) == 1 and ar_decode.check_num_samples(8, 1, **ok) == 8
    for bad, word in (((0, 1, ok), "[1, 8]"), ((9, 1, ok), "[1, 8]"), ((2.5, 1, ok), "integer"), ((True, 1, ok), "integer"),
                      ((4, 2, ok), "batch 1"), ((4, 1, ok | {"decode": "eager"}), "decode"),
                      ((4, 1, ok | {"sampler": "host"}), "sampler"), ((4, 1, ok | {"temperature": 0.0}), "temperature")):
        with pytest.raises(ValueError, match=re.escape(word)):
            ar_decode.check_num_samples(bad[0], bad[1], **bad[2])


def test_new_entry_points_are_exported_and_declared():
    from lap_amd import hip

    header = (ROOT / "include" / "lap_hip.h").read_text()
    for name in ("lap_decode_lm_head_lp", "lap_decode_finish_lp"):
        assert getattr(hip._lib, name) is not None
        assert name in hip._fn
        assert re.search(rf"\bint {name}\(", header), name


# ---- ARPolicy behind the AR output stack (what create_trained_policy_ar builds): the new keys reach the client
class _Tok:
    """Stands in for the tokenizer of DetokenizeReasoning: the text depends on the first token, so that the test sees which
    candidate the output transforms ran on."""

    def decode(self, ids):
        return f"move forward {int(np.asarray(ids).reshape(-1)[0])} cm, open gripper"


class _Model:
    """Stands in for LAP on the host: `sample_tokens` hands back fixed candidates and records its keywords."""
    EOS_TOKEN = 1
    device = "cpu"

    def __init__(self, tokens, logp):
        import types

        self.config = types.SimpleNamespace(pi05=False)
        self.tokens, self.logp, self.calls = tokens, logp, []

    def sample_tokens(self, rng, o, **kw):
        import torch

        self.calls.append(kw)
        t, lp = torch.as_tensor(self.tokens, dtype=torch.int32), torch.as_tensor(self.logp, dtype=torch.float32)
        if kw.get("num_samples") is None:
            t, lp = t[:1], lp[:1]
        return (t, lp) if kw.get("return_logprobs") or kw.get("num_samples") is not None else t


def _served_policy(model, sample_kwargs):
    from lap_amd import policy_io as pio
    from lap_amd.serve import ARPolicy, Policy

    def to_model_inputs(req):       # the request-level input stack, reduced to what CoTObservation needs
        o = req["observation"]
        return {"image": {"base": o["image"]}, "image_mask": {"base": np.array(True)}, "state": o["state"],
                "tokenized_prompt": np.arange(4, dtype=np.int32), "tokenized_prompt_mask": np.ones(4, dtype=bool)}

    base = Policy(model, use_graph=False, transforms=[to_model_inputs],
                  output_transforms=[pio.DetokenizeReasoning(_Tok()), pio.CoTOutputs(language_action_format="verbose_with_rotation")])
    assert base._has_transforms
    return ARPolicy(base, sample_kwargs=sample_kwargs)


def test_ar_policy_result_keys_pass_the_output_transforms():
    tokens = np.array([[3, 4, 1, 0], [7, 1, 0, 0], [5, 6, 8, 1]], dtype=np.int32)
    logp = -np.array([[1, 1, 1, 9], [0.5, 0.25, 9, 9], [1, 1, 1, 1]], dtype=np.float32)      # sums -3, -0.75, -4
    req = {"observation": {"image": np.zeros((8, 8, 3), np.uint8), "state": np.zeros(7, np.float32)}, "prompt": "x"}
    kw = {"max_decoding_steps": 4, "temperature": 1.0, "sampler": "device"}
    # best-of-N: the transforms ran on the selected candidate (row 1: "move forward 7 cm"), everything else goes round them
    model = _Model(tokens, logp)
    res = _served_policy(model, kw | {"num_samples": 3, "select": "sum"}).infer(req)
    assert model.calls[0]["num_samples"] == 3 and model.calls[0]["decode"] == "fused" and "select" not in model.calls[0]
    assert res["reasoning"] == "move forward 7 cm, open gripper"
    np.testing.assert_allclose(res["actions"], [0.07, 0, 0, 0, 0, 0, 1.0])
    assert set(res) == {"actions", "reasoning", "token_logprobs", "logprob", "candidates", "policy_timing"}
    assert np.array_equal(res["candidates"]["tokens"], tokens)
    assert np.array_equal(res["candidates"]["logprob"], [-3.0, -0.75, -4.0])
    assert np.array_equal(res["token_logprobs"], logp[1:2]) and np.array_equal(res["logprob"], [-0.75])
    # the mean rule picks another row, and the transforms follow it
    res = _served_policy(_Model(tokens, logp), kw | {"num_samples": 3, "select": "mean"}).infer(req)      # means -1, -0.375, -1
    assert res["reasoning"] == "move forward 7 cm, open gripper"
    res = _served_policy(_Model(tokens[[0, 2]], logp[[0, 2]]), kw | {"num_samples": 2, "select": "mean"}).infer(req)    # a tie: the lowest row
    assert res["reasoning"] == "move forward 3 cm, open gripper" and np.array_equal(res["logprob"], [-3.0])
    # return_logprobs alone
    model = _Model(tokens, logp)
    res = _served_policy(model, kw | {"return_logprobs": True}).infer(req)
    assert set(res) == {"actions", "reasoning", "token_logprobs", "logprob", "policy_timing"}
    assert np.array_equal(res["token_logprobs"], logp[:1]) and np.array_equal(res["logprob"], [-3.0])
    # neither: the result of before
    res = _served_policy(_Model(tokens, logp), kw).infer(req)
    assert set(res) == {"actions", "reasoning", "policy_timing"}
