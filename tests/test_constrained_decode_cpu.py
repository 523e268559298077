"""Constrained-vocabulary decoding, host side: `ar_decode.check_allowed_tokens` and `policy_io.allowed_token_ids` (no GPU)."""
import numpy as np
import pytest
import torch

V, EOS = 1000, 1


def test_check_allowed_tokens_normalises():
    from lap_amd.ar_decode import check_allowed_tokens

    want = torch.tensor([1, 3, 7, 999], dtype=torch.int32)
    for ids in ([7, 3, 1, 999, 3, 7], (999, 1, 3, 7), {1, 3, 7, 999}, np.array([[7, 3], [999, 1]], dtype=np.int64),
                torch.tensor([3, 3, 999, 1, 7], dtype=torch.int16), torch.tensor([999, 7, 3, 1])):
        got = check_allowed_tokens(ids, V, EOS)
        assert got.dtype == torch.int32 and got.device.type == "cpu" and torch.equal(got, want), ids
    # the whole vocabulary, and a singleton that is the EOS token
    assert torch.equal(check_allowed_tokens(range(V), V, EOS), torch.arange(V, dtype=torch.int32))
    assert check_allowed_tokens([EOS], V, EOS).tolist() == [EOS]
    # an EOS token outside the vocabulary (a model that never stops early) asks for nothing
    assert check_allowed_tokens([5, 2], V, -1).tolist() == [2, 5]
    assert check_allowed_tokens([5, 2], V, V).tolist() == [2, 5]


@pytest.mark.parametrize("ids,match", [
    ([], "empty"),
    (torch.empty(0, dtype=torch.int64), "empty"),
    ([1, 2, V], "must lie in"),
    ([-1, 1], "must lie in"),
    ([1.0, 2.0], "integer"),
    (torch.tensor([1.0, 2.0]), "integer"),
    (np.array([1.5]), "integer"),
    (torch.tensor([True, False]), "integer"),
    ([2, 3, 4], "EOS"),
])
def test_check_allowed_tokens_rejects(ids, match):
    from lap_amd.ar_decode import check_allowed_tokens

    with pytest.raises(ValueError, match=match):
        check_allowed_tokens(ids, V, EOS)


def test_allowed_token_ids():
    from lap_amd import policy_io as pio
    from tests.common import tiny_sentencepiece_proto

    tk = pio.PaligemmaTokenizer(model_proto=tiny_sentencepiece_proto(), max_len=48)
    sp = tk._tokenizer
    texts = ["move forward 3 cm, tilt left 10 degrees, open gripper", "move right 2 cm\nand close_gripper", "move forward 3 cm"]
    extra = (5, 0, 5)
    got = pio.allowed_token_ids(tk, texts, extra_ids=extra)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.ndim == 1
    assert got.tolist() == sorted(set(got.tolist()))            # sorted, unique
    assert sp.eos_id() in got and set(extra) <= set(got.tolist())
    # every token of a language action as `tokenize` appends it (cleaned, then encoded, then EOS) is in the set
    for text in texts:
        toks, _, reason, *_ = tk.tokenize("pick up the block", text)
        assert reason.any() and set(toks[reason].tolist()) <= set(got.tolist()), text
    want = {sp.eos_id(), *extra}
    for text in texts:
        want |= set(sp.encode(text.strip().replace("_", " ").replace("\n", " ")))
    assert set(got.tolist()) == want
    assert pio.allowed_token_ids(tk, []).tolist() == [sp.eos_id()]
    # and it is what check_allowed_tokens takes as it is
    from lap_amd.ar_decode import check_allowed_tokens

    assert check_allowed_tokens(got, sp.vocab_size(), sp.eos_id()).tolist() == got.tolist()


class _StubModel:
    """What `ar_decode.sample_tokens` reads of a model before it touches the device; anything else is an error."""
    EOS_TOKEN = EOS
    device = torch.device("cpu")

    class config:
        vocab_size = V

    def __getattr__(self, name):
        raise AssertionError(f"sample_tokens reached model.{name} before it refused the set")


@pytest.mark.parametrize("bad", [[], [1, V], [1.0], [2, 3]])
def test_sample_tokens_refuses_a_bad_set_before_any_device_work(bad):
    from lap_amd import ar_decode

    with pytest.raises(ValueError, match="allowed_tokens"):
        ar_decode.sample_tokens(_StubModel(), 0, None, allowed_tokens=bad)


def test_allowed_set_is_checked_once():
    from lap_amd import ar_decode

    m = _StubModel()
    a = ar_decode.allowed_set(m, [7, 1, 7, 3])
    assert a.ids.tolist() == [1, 3, 7] and a.ids.dtype == torch.int32 and (a.vocab_size, a.eos_token) == (V, EOS)
    assert ar_decode.allowed_set(m, a) is a                 # handed back, not checked again
    m.EOS_TOKEN = 5                                         # another EOS token: checked again, and refused
    with pytest.raises(ValueError, match="EOS"):
        ar_decode.allowed_set(m, a)


def test_every_layer_takes_the_argument():
    import inspect

    from lap_amd import ar_decode
    from lap_amd.model import LAP
    from lap_amd.serve import GraphedTokenDecoder

    for fn in (LAP.sample_tokens, ar_decode.sample_tokens, GraphedTokenDecoder.__init__):
        assert inspect.signature(fn).parameters["allowed_tokens"].default is None
    assert inspect.signature(ar_decode.DecodeCtx.__init__).parameters["allowed"].default is None
