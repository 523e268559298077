"""Speculative decoding, host side: the draft rule and the accept rule of lap_amd/speculate.py on hand-worked cases, and every
ValueError of the surface (no GPU).  tests/test_speculate_gpu.py feeds DRAFT_CASES and ACCEPT_CASES to the kernels as well."""
import numpy as np
import pytest

from lap_amd import speculate as SP

# (name, ref, out (the first t entries are written), t, S, expected draft)
DRAFT_CASES = [
    # last = 6, prev = 5: a = 1 and a = 4 are 2-gram anchors; a = 6 matches last only and is nearer to t-1 = 6, but a 2-gram wins
    # over a 1-gram; of the two, |4 - 6| < |1 - 6|
    ("2gram_over_1gram", [5, 6, 7, 5, 6, 9, 6, 2], [0, 0, 0, 0, 0, 5, 6], 7, 4, [9, 6, 2]),
    # last = 3, no 2-gram anchor (prev = 9 never precedes a 3): 1-gram anchors a = 0, 2, 6; t-1 = 4: |2 - 4| = |6 - 4| = 2, the
    # lower index wins
    ("tie_distance_then_lower_index", [3, 1, 3, 4, 5, 8, 3, 7], [0, 0, 0, 9, 3], 5, 3, [4, 5]),
    # two 2-gram anchors at the same distance from t-1 = 3: a = 1 and a = 5 -> the lower
    ("tie_2gram_lower_index", [2, 4, 6, 0, 2, 4, 7, 7], [1, 1, 2, 4], 4, 3, [6, 0]),
    # distance decides before the index: 1-gram anchors a = 0 and a = 5, t-1 = 4 -> a = 5
    ("distance_before_index", [3, 1, 1, 1, 1, 3, 8], [0, 0, 0, 0, 3], 5, 3, [8, -1]),
    # no anchor at all: a = t-1 = 2 -> ref[3], ref[4], ref[5]
    ("positional_fallback", [10, 11, 12, 13, 14, 15], [1, 2, 3], 3, 4, [13, 14, 15]),
    # the reference runs out: a = 3 (2-gram), ref[4] is the last entry
    ("ref_runs_out", [1, 2, 3, 4, 5], [0, 0, 3, 4], 4, 4, [5, -1, -1]),
    # positional fallback beyond the reference's end
    ("fallback_past_the_end", [1, 2], [7, 7, 7, 7], 4, 3, [-1, -1]),
    ("n_zero", [], [4, 5], 2, 4, [-1, -1, -1]),
    ("n_zero_none", None, [4, 5], 2, 2, [-1]),
    # t = 1: there is no prev, so only 1-gram anchors: a = 2 and a = 0 hold 9; t-1 = 0 -> a = 0
    ("t_one", [9, 4, 9, 5], [9], 1, 4, [4, 9, 5]),
    # t = 1 and the first token is not in the reference: a = 0
    ("t_one_fallback", [8, 4, 6], [9], 1, 3, [4, 6]),
]

# (name, tok, draft, t, cap, eos, expected emitted)
ACCEPT_CASES = [
    ("all_accepted", [4, 5, 6, 7], [4, 5, 6], 3, 20, 1, [4, 5, 6, 7]),
    ("none_accepted", [4, 5, 6, 7], [9, 5, 6], 3, 20, 1, [4]),
    ("no_draft", [4, 5, 6, 7], [-1, -1, -1], 3, 20, 1, [4]),
    ("partial", [4, 5, 6, 7], [4, 5, 8], 3, 20, 1, [4, 5, 6]),
    ("right_after_wrong_is_not_taken", [4, 5, 6, 7], [4, 9, 6], 3, 20, 1, [4, 5]),
    # tok[1] is the EOS: it is emitted and nothing after it, although draft[1] matches it
    ("eos_inside", [4, 1, 6, 7], [4, 1, 6], 3, 20, 1, [4, 1]),
    ("eos_first", [1, 5, 6, 7], [1, 5, 6], 3, 20, 1, [1]),
    ("eos_last", [4, 5, 6, 1], [4, 5, 6], 3, 20, 1, [4, 5, 6, 1]),
    # t + r reaches cap: t = 18, cap = 20 -> out[18], out[19] only
    ("cap_reached", [4, 5, 6, 7], [4, 5, 6], 18, 20, 1, [4, 5]),
    ("cap_last_slot", [4, 5, 6, 7], [4, 5, 6], 19, 20, 1, [4]),
    ("cap_on_entry", [4, 5, 6, 7], [4, 5, 6], 20, 20, 1, []),
    ("two_rows", [4, 5], [4], 0, 20, 1, [4, 5]),
]


@pytest.mark.parametrize("case", DRAFT_CASES, ids=[c[0] for c in DRAFT_CASES])
def test_draft_tokens(case):
    _, ref, out, t, S, want = case
    got = SP.draft_tokens(ref, out, t, S)
    assert got.dtype == np.int32 and got.tolist() == want
    # what lies beyond the t written tokens is not read
    assert SP.draft_tokens(ref, list(out[:t]) + [123, 456], t, S).tolist() == want


@pytest.mark.parametrize("case", ACCEPT_CASES, ids=[c[0] for c in ACCEPT_CASES])
def test_accept(case):
    _, tok, draft, t, cap, eos, want = case
    got = SP.accept(tok, draft, t, cap, eos)
    assert got.dtype == np.int32 and got.tolist() == want


def test_replay_counts():
    # an answer of 8 tokens (EOS = 1 at index 7) under itself as the draft: 7 tokens after the first in ceil(7 / S) steps
    T = [3, 4, 5, 6, 7, 8, 9, 1, 0, 0]
    for S in (2, 3, 4, 8):
        steps, acc = SP.replay(T, T, S, 10, 1)
        assert steps == -(-7 // S) and acc == 7 - steps
    assert SP.replay(T, None, 4, 10, 1) == (7, 0)
    # no EOS: the budget ends the decode
    U = [3, 4, 5, 6, 7, 8, 9, 2, 6, 5]
    assert SP.replay(U, U, 4, 10, 1) == (3, 6) and SP.replay(U, None, 4, 10, 1) == (9, 0)
    # a budget of 9: 8 tokens after the first in two full steps.  With ref[3] altered the first step emits 3 tokens (draft[2] = 11
    # is not tok[2] = 6), the second falls back to a = t-1 = 3 (no 6 in the reference) and emits 4, the third emits the last
    assert SP.replay(U[:9], U[:9], 4, 9, 1) == (2, 6)
    W = list(U[:9])
    W[3] = 11
    assert SP.replay(U[:9], W, 4, 9, 1) == (3, 5)
    # a budget of one token and an EOS as the first token take no verify step
    assert SP.replay([3], [3], 4, 1, 1) == (0, 0) and SP.replay([1, 0, 0], [1], 4, 3, 1) == (0, 0)


class _Stub:
    """What `ar_decode.sample_tokens` touches before its first device call."""
    class config:
        vocab_size = 64
    EOS_TOKEN = 1

    def _serving_weights(self):
        raise AssertionError("device work before the arguments were checked")


def _obs(B=1):
    class Obs:
        class tokenized_prompt:
            shape = (B, 8)
    return Obs()


BAD = [({"speculate": 4, "decode": "eager"}, "decode"),
       ({"speculate": 4}, "decode"),                                         # (decode defaults to "eager")
       ({"speculate": 4, "decode": "fused", "temperature": 0.7, "sampler": "device"}, "temperature"),
       ({"speculate": 4, "decode": "fused", "return_logprobs": True}, "return_logprobs"),
       ({"speculate": 4, "decode": "fused", "num_samples": 2}, "num_samples"),
       ({"speculate": 4, "decode": "fused", "top_k": 5}, "top_k"),
       ({"speculate": 4, "decode": "fused", "top_p": 0.9}, "top_p"),
       ({"speculate": 4, "decode": "fused", "collect": {}}, "collect"),
       ({"speculate": 1, "decode": "fused"}, r"\[2, 8\]"),
       ({"speculate": 9, "decode": "fused"}, r"\[2, 8\]"),
       ({"speculate": 2.5, "decode": "fused"}, "integer"),
       ({"speculate": True, "decode": "fused"}, "integer"),
       ({"draft_tokens": [1, 2], "decode": "fused"}, "speculate")]


@pytest.mark.parametrize("kw, word", BAD)
def test_sample_tokens_rejects_before_device_work(kw, word):
    from lap_amd import ar_decode

    with pytest.raises(ValueError, match=word):
        ar_decode.sample_tokens(_Stub(), 0, _obs(), **kw)


def test_batch_must_be_one():
    from lap_amd import ar_decode

    with pytest.raises(ValueError, match="batch 1"):
        ar_decode.sample_tokens(_Stub(), 0, _obs(3), speculate=4, decode="fused")
    with pytest.raises(ValueError, match="batch 1"):
        SP.check_speculate(4, 2)
    assert SP.check_speculate(2, 1) == 2 and SP.check_speculate(np.int64(8), 1) == 8


def test_graphed_decoder_and_policy_reject_at_construction():
    """GraphedTokenDecoder and ARPolicy check `speculate` before they touch the model."""
    from lap_amd.serve import ARPolicy, GraphedTokenDecoder

    for kw, word in (({"batch_size": 2}, "batch 1"), ({"sampling": True}, "temperature"), ({"logprobs": True}, "return_logprobs"),
                     ({"num_samples": 2}, "speculate does not combine"),({"sampling": True, "filtering": True}, "temperature"),
                     ({"speculate": 9}, r"\[2, 8\]")):
        with pytest.raises(ValueError, match=word):
            GraphedTokenDecoder(None, **({"speculate": 4} | kw))

    class Base:
        class model:
            EOS_TOKEN = 1

            @staticmethod
            def sample_tokens(*a, **k):
                raise AssertionError("device work before the arguments were checked")

    for kw, word in (({"temperature": 0.5}, "temperature"), ({"decode": "eager"}, "decode"), ({"return_logprobs": True}, "return_logprobs"),
                     ({"speculate": 1}, r"\[2, 8\]")):
        with pytest.raises(ValueError, match=word):
            ARPolicy(Base(), sample_kwargs={"speculate": 4} | kw)
    pol = ARPolicy(Base(), sample_kwargs={"speculate": 4})
    assert pol._sample_kwargs["decode"] == "fused" and pol._prev_tokens is None


def test_signatures_default_to_no_speculation():
    import inspect

    from lap_amd import ar_decode
    from lap_amd.model import LAP
    from lap_amd.serve import GraphedTokenDecoder

    for fn in (LAP.sample_tokens, ar_decode.sample_tokens):
        p = inspect.signature(fn).parameters
        assert p["speculate"].default is None and p["draft_tokens"].default is None
    assert inspect.signature(GraphedTokenDecoder.__init__).parameters["speculate"].default is None
    assert inspect.signature(GraphedTokenDecoder.__call__).parameters["draft_tokens"].default is None
    assert inspect.signature(ar_decode.DecodeCtx.__init__).parameters["speculate"].default is None
