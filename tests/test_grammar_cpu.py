"""Grammar-constrained decoding, host side (no GPU): `grammar.check_automaton`, the builders on a stand-in tokenizer, the round
trip deltas -> text -> tokens -> automaton -> text -> deltas of the registered formats, `grammar.decode_reference` against
`sampling.sample_from_logits`, and every ValueError of the serving surface."""
import dataclasses

import numpy as np
import pytest

from lap_amd import grammar as G
from lap_amd import lang_actions as LA
from lap_amd import sampling as S


# ---------------------------------------------------------------------------------------------------- a stand-in tokenizer
class Pieces:
    """A word is a "▁"-prefixed head piece (the "▁" and the word's first character) and single-character pieces; ids are given in
    order of first use, from 2 (0: padding, 1: EOS)."""
    EOS = 1

    def __init__(self):
        self.ids, self.pieces = {}, {}

    def _id(self, piece):
        if piece not in self.ids:
            self.ids[piece] = 2 + len(self.ids)
            self.pieces[self.ids[piece]] = piece
        return self.ids[piece]

    def encode(self, text):
        return [self._id(p) for w in text.split() for p in ["▁" + w[0], *w[1:]]]

    def decode(self, tokens):
        return "".join(self.pieces[int(t)] for t in tokens if int(t) in self.pieces).replace("▁", " ").strip()


V = 512


def _auto(graph, tk=None):
    tk = tk or Pieces()
    return G.automaton_from_words(tk.encode, graph, tk.EOS, V), tk


# ------------------------------------------------------------------------------------------------------- check_automaton
GOOD = dict(offsets=[0, 3, 4, 5], ids=[4, 7, 9, 1, 1], next=[0, 1, 1, 2, 2], vocab_size=16, eos_token=1)

MALFORMED = [
    ("Q < 1", dict(offsets=[0], ids=[], next=[])),
    ("empty segment", dict(offsets=[0, 3, 3, 4, 5], ids=[4, 7, 9, 1, 1], next=[0, 1, 1, 3, 3])),
    (r"ids must lie in \[0, 16\)", dict(ids=[4, 7, 16, 1, 1])),
    (r"ids must lie in \[0, 16\)", dict(ids=[-1, 7, 9, 1, 1])),
    ("not strictly sorted", dict(ids=[4, 9, 7, 1, 1])),
    ("not strictly sorted", dict(ids=[4, 7, 7, 1, 1])),
    (r"next must lie in \[0, 3\)", dict(next=[0, 1, 3, 2, 2])),
    (r"next must lie in \[0, 3\)", dict(next=[0, -1, 1, 2, 2])),
    ("no EOS edge is reachable from state 0", dict(next=[0, 0, 0, 2, 2])),
    ("must lead to a sink", dict(next=[0, 1, 1, 0, 2])),
    ("offsets must rise from 0 to E", dict(offsets=[0, 3, 4, 6])),
]


def test_check_automaton_accepts_a_good_one():
    a = G.check_automaton(G.TokenAutomaton(**GOOD))
    assert a.num_states == 3 and a.num_edges == 5 and a.union().tolist() == [1, 4, 7, 9] and a.union().dtype == np.int32
    assert a.allowed(0).tolist() == [4, 7, 9] and a.step(0, 7) == 1 and a.step(0, 8) == -1 and a.step(1, 1) == 2
    assert a.accepts([4, 4, 9, 1]) and a.accepts([7, 1, 0, 0]) and a.accepts([9]) and not a.accepts([4, 4]) and not a.accepts([4, 5, 1])
    with pytest.raises(dataclasses.FrozenInstanceError):
        a.vocab_size = 3


@pytest.mark.parametrize("word, change", MALFORMED, ids=[f"{i}_{m[0][:12]}" for i, m in enumerate(MALFORMED)])
def test_check_automaton_names_the_condition(word, change):
    with pytest.raises(ValueError, match=word):
        G.check_automaton(G.TokenAutomaton(**(GOOD | change)))


# ------------------------------------------------------------------------------------------------------------ the builders
SMALL = G.WordGraph({"s": [("move", "d"), ("mow", "d"), ("open", "g"), ("close", "g")], "d": [("up", "n"), ("down", "n")],
                     "n": [("1", "u"), ("10", "u"), ("12", "u")], "u": [("cm,", "s2")], "s2": [("open", "g"), ("close", "g")],
                     "g": [("gripper", "end")]}, "s", frozenset(["end"]))


def test_words_of_one_state_merge_into_a_trie_and_a_sink_exists():
    a, tk = _auto(SMALL)
    # "move" and "mow" share the pieces "▁m", "o": one edge for "▁m" in state 0, one for "o" after it, then "v" | "w"
    m, o, v, w = (tk.ids[p] for p in ("▁m", "o", "v", "w"))
    assert a.allowed(0).tolist().count(m) == 1
    q = a.step(a.step(0, m), o)
    assert a.allowed(a.step(0, m)).tolist() == [o] and sorted(a.allowed(q).tolist()) == sorted([v, w])
    # "1" is a prefix of "10" and "12": after "▁1" the unit may follow, or a second digit
    q = 0
    for t in tk.encode("move up"):
        q = a.step(q, t)
    after_1 = a.step(q, tk.ids["▁1"])
    assert sorted(a.allowed(after_1).tolist()) == sorted(tk.ids[p] for p in ("0", "2", "▁c"))
    # the sink: the last state, EOS -> itself only; every EOS edge leads there
    sink = a.num_states - 1
    assert a.allowed(sink).tolist() == [tk.EOS] and a.step(sink, tk.EOS) == sink
    assert (a.next[a.ids == tk.EOS] == sink).all() and a.eos_token == tk.EOS and a.vocab_size == V


def test_accepts_exactly_the_sentences_of_a_small_graph():
    a, tk = _auto(SMALL)
    sents = G.sentences(SMALL)
    assert len(sents) == 2 + 2 * 2 * 3 * 2 and "mow down 12 cm, close gripper" in sents
    for s in sents:
        assert a.accepts(tk.encode(s) + [tk.EOS]) and a.accepts(tk.encode(s)), s
        assert tk.decode(tk.encode(s)) == s
    assert set(G.random_sentences(SMALL, 40, seed=3)) <= set(sents)
    rng = np.random.default_rng(0)
    long = [s for s in sents if s.startswith("move")]
    for s in long:
        words = s.split()
        shuffled = [words[i] for i in rng.permutation(len(words))]
        if " ".join(shuffled) not in sents:
            assert not a.accepts(tk.encode(" ".join(shuffled)) + [tk.EOS]), shuffled
        for cut in range(1, len(words)):            # a truncated sentence, with and without the terminator
            assert not a.accepts(tk.encode(" ".join(words[:cut])) + [tk.EOS]), words[:cut]
        toks = tk.encode(s)
        assert not a.accepts(toks[:-1]) and not a.accepts(toks[:-1] + [tk.EOS])
        doubled = words[:4] + words                 # "move up 1 cm, move up 1 cm, open gripper"
        assert not a.accepts(tk.encode(" ".join(doubled)) + [tk.EOS]), doubled
    assert not a.accepts([tk.EOS]) and not a.accepts([])


def test_builder_rejects_what_it_cannot_encode():
    tk = Pieces()
    with pytest.raises(ValueError, match="no token"):
        G.automaton_from_words(lambda w: [], SMALL, 1, V)
    with pytest.raises(ValueError, match="EOS"):
        G.automaton_from_words(lambda w: [1], SMALL, 1, V)
    with pytest.raises(ValueError, match="empty segment"):      # a dead end: "x" leads to a state that neither accepts nor goes on
        G.automaton_from_words(tk.encode, G.WordGraph({"s": [("x", "dead"), ("y", "end")]}, "s", frozenset(["end"])), 1, V)
    with pytest.raises(ValueError, match="compact"):
        LA.word_graph(LA.LanguageActionFormat(name="c", style="compact"))
    a = G.single_state_automaton([5, 9, 1, 5], 1, 16)
    assert a.num_states == 2 and a.allowed(0).tolist() == [1, 5, 9] and a.step(0, 9) == 0 and a.step(0, 1) == 1
    with pytest.raises(ValueError, match="EOS"):
        G.single_state_automaton([5, 9], 1, 16)


# ------------------------------------------------------------------------------------------------------------ round trips
VERBOSE = (LA.VERBOSE_WITH_ROTATION_FORMAT, LA.VERBOSE_EEF_WITH_ROTATION_FORMAT,
           LA.LanguageActionFormat(name="one_decimal_no_rotation", decimal_places=1))


@pytest.mark.parametrize("fmt", VERBOSE, ids=[f.name for f in VERBOSE])
def test_verbose_round_trip(fmt):
    a, tk = _auto(LA.word_graph(fmt, max_cm=12, max_degrees=60))
    rs = np.random.RandomState(5)
    deltas = [np.concatenate([rs.uniform(-0.12, 0.12, 3), rs.uniform(-1.0, 1.0, 3), rs.uniform(0, 1, 1)]) for _ in range(60)]
    deltas += [np.array([0.0] * 6 + [1.0]), np.array([0.004, 0, 0, 0.01, 0, 0, 0.2]), np.array([0.12, -0.12, 0.12, 1.0, -1.0, 1.0, 0.9]),
               np.array([0, 0, -0.05, 0, 0.5, 0, 0.0])]
    seen = set()
    for d in deltas:
        text = LA.summarize_numeric_actions(d, fmt.get_sum_decimal(), include_rotation=fmt.include_rotation)
        toks = tk.encode(text) + [tk.EOS]
        assert a.accepts(toks), text
        back = tk.decode(toks)
        assert back == text
        mv, grip = fmt.parse_language_to_deltas(back)
        nd = fmt.decimal_places
        assert np.allclose(mv[:3] * 100.0, np.round(d[:3] * 100.0, nd), atol=1e-9), (text, mv)
        if fmt.include_rotation:
            assert np.allclose(np.rad2deg(mv[3:]), [LA._nearest(abs(np.rad2deg(r)), 10) * np.sign(r) for r in d[3:6]], atol=1e-9), (text, mv)
        assert grip == (1.0 if d[6] >= 0.5 else 0.0)
        seen.add(len(text.split(",")))
    assert len(seen) >= 3 and 1 in seen         # sentences of several lengths, the gripper-only one among them
    # what the format cannot write is not accepted
    for bad in ("cm cm move 7 gripper", "move forward 3 cm, move forward 3 cm, open gripper", "move left 3 cm, move up 2 cm, open gripper",
                "move forward 13 cm, open gripper", "move forward 3 cm", "open gripper, move forward 3 cm", "move forward 0 cm, open gripper"):
        assert not a.accepts(tk.encode(bad) + [tk.EOS]), bad
    if fmt.include_rotation:
        assert not a.accepts(tk.encode("tilt left 15 degrees, open gripper") + [tk.EOS])
        assert not a.accepts(tk.encode("rotate clockwise 10 degrees, tilt left 10 degrees, open gripper") + [tk.EOS])


def test_vla0_round_trip():
    fmt = LA.VLA0ActionFormat(name="vla0_small", num_bins=20, action_horizon=2, action_dim=7)
    a, tk = _auto(LA.word_graph(fmt))
    rs = np.random.RandomState(9)
    for _ in range(30):
        acts = rs.uniform(-1.2, 1.2, (2, 7))
        text = fmt.summarize_actions(acts)
        toks = tk.encode(text) + [tk.EOS]
        assert a.accepts(toks), text
        full = fmt.parse_to_full_actions(tk.decode(toks))
        assert np.allclose(full, np.round((np.clip(acts, -1, 1) + 1) / 2 * 20) / 20 * 2 - 1)
        mv, grip = fmt.parse_language_to_deltas(tk.decode(toks))
        assert np.allclose(mv, full[0, :6]) and grip == full[0, 6]
    words = text.split()
    assert not a.accepts(tk.encode(" ".join(words[:-1])) + [tk.EOS])             # 13 integers
    assert not a.accepts(tk.encode(" ".join(words + ["3"])) + [tk.EOS])          # 15 integers
    assert not a.accepts(tk.encode(" ".join(["21"] + words[1:])) + [tk.EOS])     # beyond num_bins
    # the registered format: 70 integers in [0, 1000]
    big, tk2 = _auto(LA.word_graph(LA.VLA0_CHUNKED_FORMAT))
    text = LA.VLA0_CHUNKED_FORMAT.summarize_actions(rs.uniform(-1, 1, (10, 7)))
    assert big.accepts(tk2.encode(text) + [tk2.EOS]) and not big.accepts(tk2.encode(text + " 5") + [tk2.EOS])


def test_grammar_automaton_under_a_sentencepiece_tokenizer():
    from lap_amd import policy_io as pio
    from tests.common import tiny_sentencepiece_proto

    tk = pio.PaligemmaTokenizer(model_proto=tiny_sentencepiece_proto(), max_len=48)
    a = pio.grammar_automaton(tk, "verbose_with_rotation", max_cm=9, max_degrees=30, vocab_size=1024)
    sp = tk._tokenizer
    assert a.vocab_size == 1024 and a.eos_token == sp.eos_id()
    d = np.array([0.03, -0.02, 0.0, 0.0, 0.36, 0.0, 1.0])
    text = LA.summarize_numeric_actions(d, "0f", include_rotation=True)
    answer = tk.encode(text, add_eos=True)          # (as `tokenize` encodes a language action)
    assert answer[-1] == sp.eos_id() and a.accepts(answer) and not a.accepts(sp.encode("gripper open") + [sp.eos_id()])


# ------------------------------------------------------------------------------------------------------- decode_reference
def _five_state(Vv=64, eos=1):
    """0 -{2..20}-> 1 -{30, 31}-> 2 -{5, 40..50}-> 0 | 3; 3 -{EOS, 7}-> sink | 3; 4: the sink."""
    segs = [[(i, 1) for i in range(2, 21)], [(30, 2), (31, 2)], [(5, 0)] + [(i, 3) for i in range(40, 51)], [(eos, 4), (7, 3)], [(eos, 4)]]
    segs = [sorted(s) for s in segs]
    off = np.cumsum([0] + [len(s) for s in segs])
    return G.check_automaton(G.TokenAutomaton(off, [i for s in segs for i, _ in s], [n for s in segs for _, n in s], Vv, eos))


@pytest.mark.parametrize("T", [0.0, 0.8, 1.5])
def test_decode_reference_emits_accepted_sequences(T):
    a = _five_state()
    steps, B = 40, 6
    lg = (np.random.default_rng(3).standard_normal((steps, B, 64)) * 3).astype(np.float32)
    tok, lp, st = G.decode_reference(lg, a, T, seed=77, rows=B)
    assert tok.shape == (B, steps) and lp.shape == (B, steps) and st.shape == (B, steps + 1) and (st[:, 0] == 0).all()
    for b in range(B):
        for t in range(steps):
            assert tok[b, t] in a.allowed(st[b, t]) and st[b, t + 1] == a.step(st[b, t], tok[b, t])
            want = S.token_logprobs(lg[t, b:b + 1], tok[b:b + 1, t], T, allowed=a.allowed(st[b, t]))[0]
            assert lp[b, t] == want and lp[b, t] <= 0
        if (tok[b] == 1).any():
            assert a.accepts(tok[b])
            first = int(np.flatnonzero(tok[b] == 1)[0])
            assert (tok[b, first:] == 1).all()          # the sink keeps emitting EOS
    assert sum(bool((tok[b] == 1).any()) for b in range(B)) >= 1
    assert len({tuple(r) for r in st.tolist()}) > 1      # rows are in different states
    with pytest.raises(ValueError, match="rows"):
        G.decode_reference(lg, a, T, seed=77, rows=B + 1)
    with pytest.raises(ValueError, match="width"):
        G.decode_reference(lg[:, :, :32], a, T, seed=77)


@pytest.mark.parametrize("T", [0.0, 0.9])
def test_a_single_state_automaton_is_the_masked_sampler(T):
    A = np.array([3, 5, 8, 13, 21, 34, 55, 62])
    a = G.single_state_automaton(np.concatenate([A, [63]]), 63, 64)      # (the EOS token is given a logit that never wins)
    lg = (np.random.default_rng(4).standard_normal((12, 5, 64)) * 2).astype(np.float32)
    lg[:, :, 63] = -50.0
    lg[2, 1, 3] = lg[2, 1, 21] = 9.0            # a tie: the lowest index when greedy
    tok, lp, st = G.decode_reference(lg, a, T, seed=5)
    masked = np.full_like(lg, -np.inf)
    masked[:, :, a.allowed(0)] = lg[:, :, a.allowed(0)]
    for t in range(12):
        assert np.array_equal(tok[:, t], S.sample_from_logits(masked[t], T, 5, t))
        assert np.allclose(lp[:, t], S.token_logprobs(lg[t], tok[:, t], T, allowed=a.allowed(0)), rtol=0, atol=1e-12)
    assert (st == 0).all() and (T > 0 or tok[1, 2] == 3)


def test_few_sampled_kernel_cases_sit_on_a_near_tie():
    """The inputs of tests/test_grammar_gpu.py's sampled sweep: the share of (row, step) pairs whose two best host scores are too
    close for the host logarithm to decide stays under the cap, with the seeds of tests/grammar_cases.py."""
    from tests import grammar_cases as C

    a = C.automaton()
    assert a.num_states == 6 and [len(a.allowed(q)) for q in range(6)] == [1, 2, 63, 257, 1500, 1]
    out = total = 0
    for B in C.BS:
        for T in C.TEMPS:
            lg, tok, lp, st, clear = C.sampled_reference(a, B, T)
            out += int((~clear).sum())
            total += clear.size
            assert len(set(st[:, 0].tolist())) == min(B, 5)         # rows start in different states
    assert 0 < total and out <= C.SHARE * total, (out, total)


# --------------------------------------------------------------------------------------------------- the serving surface
class _Stub:
    """What `ar_decode.sample_tokens` touches before its first device call (tests/test_speculate_cpu.py)."""
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


def _bad():
    g = _five_state()
    broken = G.TokenAutomaton(**(GOOD | dict(vocab_size=64, next=[0, 0, 0, 2, 2])))
    return [({"grammar": g, "allowed_tokens": [1, 2, 3]}, "allowed_tokens"),
            ({"grammar": g, "top_k": 5, "temperature": 0.7, "sampler": "device"}, "top_k / top_p"),
            ({"grammar": g, "top_p": 0.9, "temperature": 0.7, "sampler": "device"}, "top_k / top_p"),
            ({"grammar": g, "speculate": 4, "decode": "fused"}, "speculate"),
            ({"grammar": g, "speculate": 4}, "grammar does not combine with speculate"),
            ({"grammar": g, "temperature": 0.7}, "sampler"),
            ({"grammar": g, "temperature": 0.7, "decode": "fused"}, "sampler"),
            ({"grammar": _five_state(Vv=128)}, "vocab_size 128"),
            ({"grammar": _five_state(eos=0)}, "EOS token 0"),
            ({"grammar": broken}, "no EOS edge is reachable"),
            ({"grammar": [1, 2, 3]}, "TokenAutomaton")]


@pytest.mark.parametrize("case", range(11))
def test_sample_tokens_rejects_before_device_work(case):
    from lap_amd import ar_decode

    kw, word = _bad()[case]
    with pytest.raises(ValueError, match=word):
        ar_decode.sample_tokens(_Stub(), 0, _obs(), **kw)


def test_graphed_decoder_and_policy_reject_at_construction():
    from lap_amd.serve import ARPolicy, GraphedTokenDecoder

    g = _five_state()
    for kw, word in (({"allowed_tokens": [1, 2]}, "allowed_tokens"), ({"sampling": True, "filtering": True}, "top_k / top_p"),
                     ({"speculate": 4}, "speculate")):
        with pytest.raises(ValueError, match=word):
            GraphedTokenDecoder(_Stub(), grammar=g, **kw)
    with pytest.raises(ValueError, match="vocab_size 128"):
        GraphedTokenDecoder(_Stub(), grammar=_five_state(Vv=128))

    class Base:
        model = _Stub()
        model.sample_tokens = None

    for kw, word in (({"allowed_tokens": [1, 2]}, "allowed_tokens"), ({"top_k": 4, "temperature": 0.5, "sampler": "device"}, "top_k / top_p"),
                     ({"temperature": 0.5}, "sampler"), ({"speculate": 4}, "speculate")):
        with pytest.raises(ValueError, match=word):
            ARPolicy(Base(), sample_kwargs={"grammar": g} | kw)


def test_signatures_default_to_no_grammar():
    import inspect

    from lap_amd import ar_decode
    from lap_amd.model import LAP
    from lap_amd.serve import GraphedTokenDecoder, create_trained_policy_ar

    for fn in (LAP.sample_tokens, ar_decode.sample_tokens, GraphedTokenDecoder.__init__, ar_decode.DecodeCtx.__init__):
        assert inspect.signature(fn).parameters["grammar"].default is None
    assert inspect.signature(create_trained_policy_ar).parameters["grammar"].default is False


def test_a_device_automaton_is_reused_only_on_the_models_own_device():
    import torch

    from lap_amd.ar_decode import _on_device

    t = torch.zeros(1)
    assert _on_device(t, "cpu") and _on_device(t, torch.device("cpu"))
    assert not _on_device(t, "cuda") and not _on_device(t, torch.device("cuda", 1))
