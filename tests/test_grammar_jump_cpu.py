"""Jump-forward grammar decoding, host side (no GPU): `speculate.grammar_drafts`, `grammar_verify` and `replay_grammar` against a
brute-force restatement, the forced-run condition under the tiny SentencePiece model, and every ValueError of the surface."""
import numpy as np
import pytest

from lap_amd import grammar as G
from lap_amd import sampling as SM
from lap_amd import speculate as SP
from tests.test_grammar_cpu import SMALL, Pieces, _five_state, _obs, _Stub

V = 64


# ------------------------------------------------------------------------------------------------- brute-force restatement
def _table(a):
    """state -> {id: next state}: the automaton without its CSR arrays."""
    return [{int(i): int(n) for i, n in zip(a.ids[a.offsets[q]:a.offsets[q + 1]], a.next[a.offsets[q]:a.offsets[q + 1]])}
            for q in range(a.num_states)]


def _brute_drafts(a, q, refdraft):
    tab, out, live = _table(a), [], True
    for want in refdraft:
        d = -1
        if live and 0 <= q < len(tab):
            edges = tab[q]
            if len(edges) == 1:
                d = next(iter(edges))
            elif int(want) in edges:
                d = int(want)
        if d < 0:
            live = False
        else:
            q = tab[q][d]
            live = d != a.eos_token
        out.append(d)
    return out


def _brute_draw(a, row, q, step, T, seed):
    """(token, log-probability, next state) of one row in state q: scores of the whole row, then the best edge by (score, -id)."""
    tab = _table(a)
    sc = SM.scores_from_logits(row[None], T, seed, step)[0]
    tok = max(tab[q], key=lambda i: (sc[i], -i))
    z = np.array([np.float32(row[i]) * SM.inverse_temperature(T) if T > 0 else row[i] for i in sorted(tab[q])], dtype=np.float64)
    zt = float(np.float32(row[tok]) * SM.inverse_temperature(T)) if T > 0 else float(row[tok])
    return tok, zt - (z.max() + np.log(np.exp(z - z.max()).sum())), tab[q][tok]


def _brute_verify(a, lg, q, drafts, t, cap, T, seed):
    toks, lps = [], []
    if t >= cap:
        return toks, lps, q
    for r in range(lg.shape[0]):
        if r and (toks[-1] == a.eos_token or drafts[r - 1] != toks[-1] or t + r >= cap):
            break
        tok, lp, q = _brute_draw(a, lg[r], q, t + r, T, seed)
        toks.append(tok)
        lps.append(lp)
    return toks, lps, q


def _chain_automaton():
    """Forced runs: 0 -{3}-> 1 -{4}-> 2 -{5}-> 3 -{6, 7, 8}-> 4 | 4 | 0; 4 -{9}-> 5 -{EOS}-> 6 (the sink)."""
    segs = [[(3, 1)], [(4, 2)], [(5, 3)], [(6, 4), (7, 4), (8, 0)], [(9, 5)], [(1, 6)], [(1, 6)]]
    off = np.cumsum([0] + [len(s) for s in segs])
    return G.check_automaton(G.TokenAutomaton(off, [i for s in segs for i, _ in s], [n for s in segs for _, n in s], V, 1))


def _small_automaton():
    tk = Pieces()
    return G.automaton_from_words(tk.encode, SMALL, tk.EOS, V), tk


AUTOMATA = {"five": _five_state, "chain": _chain_automaton, "small": lambda: _small_automaton()[0]}


@pytest.mark.parametrize("name", AUTOMATA)
def test_drafts_against_brute_force(name):
    a = AUTOMATA[name]()
    rs = np.random.RandomState(3)
    drafted = 0
    for _ in range(300):
        S = int(rs.randint(2, 9))
        q = int(rs.randint(-1, a.num_states + 1))         # (both ends lie outside the automaton)
        ref = rs.randint(-1, 52, size=S - 1)
        if 0 <= q < a.num_states and rs.rand() < 0.6:     # a reference that follows the automaton for a while
            qq = q
            for r in range(S - 1):
                seg = a.allowed(qq)
                ref[r] = seg[rs.randint(len(seg))]
                qq = a.step(qq, ref[r])
                if rs.rand() < 0.15:
                    break
        got = SP.grammar_drafts(a, q, ref)
        assert got.dtype == np.int32 and got.tolist() == _brute_drafts(a, q, ref.tolist()), (q, ref)
        drafted += int((got >= 0).sum())
        k = int((got >= 0).sum())
        assert (got[:k] >= 0).all() and (got[k:] == -1).all()          # one run, then nothing
        if a.eos_token in got.tolist():
            assert got.tolist().index(a.eos_token) == k - 1            # nothing after a drafted EOS
    assert drafted > 300
    none = SP.grammar_drafts(a, 0, [-1, -1, -1])
    if len(a.allowed(0)) > 1:
        assert none.tolist() == [-1, -1, -1]


@pytest.mark.parametrize("T", [0.0, 0.8, 1.5])
@pytest.mark.parametrize("name", ["five", "chain"])
def test_verify_against_brute_force(name, T):
    a = AUTOMATA[name]()
    rs = np.random.RandomState(5)
    lengths = set()
    for case in range(120):
        S = int(rs.randint(2, 9))
        cap = 12
        t = int(rs.randint(1, cap + 2))
        q = int(rs.randint(0, a.num_states))
        lg = (rs.standard_normal((S, V)) * 3).astype(np.float32)
        # the drafts: the tokens the rows would draw, some of them altered
        toks, qq = [], q
        for r in range(S - 1):
            tok, _, qq = _brute_draw(a, lg[r], qq, t + r, T, 40 + case)
            toks.append(tok)
        drafts = [d if rs.rand() < 0.8 else -1 for d in toks]
        want_tok, want_lp, want_q = _brute_verify(a, lg, q, drafts, t, cap, T, 40 + case)
        emitted, lp, q_after = SP.grammar_verify(lg, a, q, drafts, t, cap, T, 40 + case)
        assert emitted.dtype == np.int32 and emitted.tolist() == want_tok and q_after == want_q, (case, S, t, q)
        assert np.allclose(lp, want_lp, rtol=0, atol=1e-9)
        assert len(emitted) == (0 if t >= cap else len(SP.accept(want_tok + [-5] * (S - len(want_tok)), drafts, t, cap, a.eos_token)))
        lengths.add(len(emitted))
        # greedy, the step index plays no part: row 0 is one step of `grammar.decode_reference` from q (the sampled rows are
        # compared with it in the next test)
        if len(emitted) and T == 0.0:
            ref_tok, ref_lp, ref_st = G.decode_reference(lg[0][None, None], a, T, seed=40 + case, start=[q])
            assert ref_tok[0, 0] == emitted[0] and ref_lp[0, 0] == lp[0]
    assert lengths >= {0, 1, 2, 3}
    # a state outside the automaton: the row emits EOS with log-probability -inf and keeps its state
    for bad in (-1, a.num_states):
        e, lp, qa = SP.grammar_verify(lg, a, bad, [5] * (S - 1), 1, cap, T, 0)
        assert e.tolist() == [a.eos_token] and np.isneginf(lp).all() and qa == bad


def test_a_sampled_row_is_the_reference_at_its_step():
    """Row r of `grammar_verify` against `grammar.decode_reference`, whose step index is its loop counter: the row's logits are put
    at step t + r of a longer run whose earlier steps loop in one state."""
    a = _five_state()
    rs = np.random.RandomState(9)
    lg = (rs.standard_normal((4, V)) * 3).astype(np.float32)
    t, T, seed = 5, 0.8, 77
    # state 3 loops on token 7: a run that stays in state 3 for t + r steps (logit of 7 far above EOS), then the row under test
    emitted, lp, _ = SP.grammar_verify(lg[:1], a, 3, [], t, 20, T, seed)        # (S = 1 rows: the rule of one row)
    run = np.full((t + 1, 1, V), -50.0, dtype=np.float32)
    run[:t, 0, 7] = 50.0
    run[t, 0] = lg[0]
    tok, rlp, st = G.decode_reference(run, a, T, seed=seed, start=[3])
    assert (st[0, :t + 1] == 3).all() and tok[0, t] == emitted[0] and rlp[0, t] == lp[0]


def _answers(a, tk, n=40):
    return [tk.encode(s) + [tk.EOS] for s in G.random_sentences(SMALL, n, seed=4)]


@pytest.mark.parametrize("S", [2, 3, 4, 8])
def test_replay_properties(S):
    a, tk = _small_automaton()
    single = {q for q in range(a.num_states) if len(a.allowed(q)) == 1}
    some_forced = 0
    for ans in _answers(a, tk):
        cap = len(ans)
        vs, acc = SP.replay_grammar(ans, a, None, S, cap)
        assert vs + acc == len(ans) - 1
        # brute force, without a reference: states[i] is the state before token i; a step at t emits token t and then the
        # tokens of the k single-edge states that follow without a break, up to S tokens and up to the budget
        states = [0]
        for x in ans:
            states.append(a.step(states[-1], x))
        t, steps, accepted = 1, 0, 0
        while t < cap:
            k, q = 0, states[t]
            while k < S - 1 and q in single:
                k, q = k + 1, states[t + k + 1] if t + k + 1 < len(states) else -1
            n = min(1 + k, S, cap - t)
            steps, accepted, t = steps + 1, accepted + n - 1, t + n
        assert (vs, acc) == (steps, accepted), ans
        some_forced += acc
        # with the answer as the reference every step emits min(S, remaining) tokens
        vs2, acc2 = SP.replay_grammar(ans, a, ans, S, cap)
        assert vs2 == -(-(len(ans) - 1) // S) and vs2 + acc2 == len(ans) - 1
        # a budget below the answer's length ends the decode there
        vs3, acc3 = SP.replay_grammar(ans[:cap - 2], a, None, S, cap - 2)
        assert vs3 + acc3 == cap - 3
    assert some_forced > 0
    assert SP.replay_grammar([tk.EOS, 0, 0], a, None, S, 3) == (0, 0) and SP.replay_grammar(ans[:1], a, None, S, 1) == (0, 0)


def test_without_a_reference_every_accepted_draft_came_from_a_single_edge_state():
    a, tk = _small_automaton()
    for ans in _answers(a, tk, 20):
        q, t, cap = a.step(0, ans[0]), 1, len(ans)
        while t < cap:
            d = SP.grammar_drafts(a, q, SP.draft_tokens(None, ans, t, 4))
            e = SP.accept([ans[t + r] if t + r < cap else -2 for r in range(4)], d, t, cap, tk.EOS)
            qq = q
            for i, x in enumerate(e.tolist()):
                if i > 0:           # an accepted draft: made in the state before it, which had that one edge
                    assert d[i - 1] == e[i - 1]
                if i < len(e) - 1:
                    assert a.allowed(qq).tolist() == [x]
                qq = a.step(qq, x)
            q, t = qq, t + len(e)


# --------------------------------------------------------------------------------------------------- forced-run condition
def test_forced_runs_under_the_sentencepiece_tokenizer():
    """Passes over the weights of 200 random verbose_with_rotation sentences without a reference: 1 (the prefill's token) + the
    steps.  At S = 4 at most 0.6 of the token count (one pass per token for the plain grammar decode), and no more at a larger S."""
    from lap_amd import lang_actions as LA
    from lap_amd import policy_io as pio
    from tests.common import tiny_sentencepiece_proto

    tk = pio.PaligemmaTokenizer(model_proto=tiny_sentencepiece_proto(), max_len=48)
    a = pio.grammar_automaton(tk, "verbose_with_rotation", vocab_size=1024)
    graph = LA.word_graph(LA.VERBOSE_WITH_ROTATION_FORMAT)
    total, forced, passes = 0, 0, {2: 0, 4: 0, 8: 0}
    for s in G.random_sentences(graph, 200, seed=1):
        ans = tk.encode(s, add_eos=True)
        assert a.accepts(ans)
        total += len(ans)
        q = 0
        for x in ans:
            forced += int(len(a.allowed(q)) == 1)
            q = a.step(q, x)
        for S in passes:
            vs, acc = SP.replay_grammar(ans, a, None, S, len(ans))
            assert vs + acc == len(ans) - 1
            passes[S] += 1 + vs
    print(f"{total} tokens, {forced} from single-edge states, passes {passes}")
    assert passes[4] <= 0.6 * total
    assert passes[8] <= passes[4] <= passes[2] <= total


# -------------------------------------------------------------------------------------------------------------- surface
def _bad():
    g = _five_state()
    ok = {"grammar": g, "decode": "fused", "jump_forward": 4}
    return [({"jump_forward": 4, "decode": "fused"}, "jump_forward needs grammar"),
            (ok | {"decode": "eager"}, "jump_forward needs decode"),
            ({"grammar": g, "jump_forward": 4}, "jump_forward needs decode"),                   # (decode defaults to "eager")
            (ok | {"num_samples": 2, "temperature": 0.7, "sampler": "device"}, "jump_forward does not combine with best-of-N"),
            (ok | {"collect": {}}, "jump_forward does not hand out logits"),
            (ok | {"temperature": 0.7}, "sampler"),
            (ok | {"jump_forward": 1}, r"jump_forward must lie in \[2, 8\]"),
            (ok | {"jump_forward": 9}, r"jump_forward must lie in \[2, 8\]"),
            (ok | {"jump_forward": 2.5}, "jump_forward must be an integer"),
            (ok | {"jump_forward": True}, "jump_forward must be an integer"),
            (ok | {"top_k": 5, "temperature": 0.7, "sampler": "device"}, "top_k / top_p"),
            (ok | {"allowed_tokens": [1, 2, 3]}, "allowed_tokens"),
            # what existing tests pin stays as it was
            (ok | {"speculate": 4}, "grammar does not combine with speculate"),
            ({"draft_tokens": [1, 2], "decode": "fused"}, "draft_tokens needs speculate=S")]


@pytest.mark.parametrize("case", range(14))
def test_sample_tokens_rejects_before_device_work(case):
    from lap_amd import ar_decode

    kw, word = _bad()[case]
    with pytest.raises(ValueError, match=word):
        ar_decode.sample_tokens(_Stub(), 0, _obs(), **kw)


def test_batch_must_be_one():
    from lap_amd import ar_decode

    with pytest.raises(ValueError, match="jump_forward needs an observation of batch 1"):
        ar_decode.sample_tokens(_Stub(), 0, _obs(3), grammar=_five_state(), jump_forward=4, decode="fused")
    assert SP.check_jump_forward(2, 1, grammar=object()) == 2 and SP.check_jump_forward(np.int64(8), 1, grammar=object()) == 8


def test_decode_ctx_graphed_decoder_and_policy_reject_at_construction():
    from lap_amd.ar_decode import DecodeCtx
    from lap_amd.serve import ARPolicy, GraphedTokenDecoder

    g = _five_state()
    for kw, word in (({"jump_forward": 4}, "jump_forward needs grammar"), ({"jump_forward": 4, "grammar": g, "B": 2}, "batch 1"),
                     ({"jump_forward": 9, "grammar": g}, r"\[2, 8\]"), ({"jump_forward": "4", "grammar": g}, "integer")):
        kw = {"B": 1} | kw
        with pytest.raises(ValueError, match=word):
            DecodeCtx(_Stub(), kw.pop("B"), 8, 8, **kw)
    for kw, word in (({}, "jump_forward needs grammar"), ({"grammar": g, "batch_size": 2}, "batch 1"),
                     ({"grammar": g, "num_samples": 2, "sampling": True}, "best-of-N"), ({"grammar": g, "jump_forward": 1}, r"\[2, 8\]"),
                     ({"grammar": g, "speculate": 4}, "grammar does not combine with speculate"),
                     ({"grammar": g, "allowed_tokens": [1, 2]}, "allowed_tokens"),
                     ({"grammar": g, "sampling": True, "filtering": True}, "top_k / top_p")):
        with pytest.raises(ValueError, match=word):
            GraphedTokenDecoder(_Stub(), **({"jump_forward": 4} | kw))

    class Base:
        model = _Stub()
        model.sample_tokens = None

    for kw, word in (({}, "jump_forward needs grammar"), ({"grammar": g, "decode": "eager"}, "jump_forward needs decode"),
                     ({"grammar": g, "num_samples": 2, "temperature": 0.5, "sampler": "device"}, "best-of-N"),
                     ({"grammar": g, "collect": {}}, "collect"), ({"grammar": g, "temperature": 0.5}, "sampler"),
                     ({"grammar": g, "jump_forward": 0}, r"\[2, 8\]"), ({"grammar": g, "speculate": 4}, "speculate")):
        with pytest.raises(ValueError, match=word):
            ARPolicy(Base(), sample_kwargs={"jump_forward": 4} | kw)


def _cpu_ids(dtype="int32"):
    import torch

    return torch.tensor([1, 2, 3], dtype=getattr(torch, dtype))


# (kind the keywords would make, keywords of DecodeCtx with "B" among them, the ValueError): what the CPU suites pin of the checks
# the constructor runs (decode weights, `check_score_ctx`, `check_num_beams`, `check_speculate`, its own) in the constructor's order
CTX_BAD = [
    ("plain", {"weights": "int4"}, "decode_weights must be one of"),
    ("plain", {"allowed": _cpu_ids("int64")}, "allowed must be the int32 device ids"),
    ("sampling", {"sampling": True, "allowed": _cpu_ids()}, "allowed must be the int32 device ids"),
    ("logprob", {"logprobs": True, "weights": "fp4"}, "decode_weights must be one of"),
    ("logprob", {"logprobs": True, "sampling": True, "allowed": _cpu_ids()}, "allowed must be the int32 device ids"),
    ("filter", {"filtering": True}, "filtering needs sampling=True"),
    ("filter", {"filtering": True, "logprobs": True}, "filtering needs sampling=True"),
    ("filter", {"filtering": True, "sampling": True, "allowed": _cpu_ids()}, "allowed must be the int32 device ids"),
    ("speculate", {"speculate": 4, "B": 2}, "speculate needs an observation of batch 1"),
    ("speculate", {"speculate": 1}, r"speculate must lie in \[2, 8\]"),
    ("speculate", {"speculate": 2.5}, "speculate must be an integer"),
    ("speculate", {"speculate": 4, "sampling": True}, "speculate is greedy"),
    ("speculate", {"speculate": 4, "logprobs": True}, "speculate does not return log-probabilities"),
    ("speculate", {"speculate": 4, "filtering": True}, "filtering needs sampling=True"),
    ("speculate", {"speculate": 4, "allowed": _cpu_ids()}, "allowed must be the int32 device ids"),
    ("speculate", {"speculate": 4, "weights": "fp16"}, "decode_weights must be one of"),
    ("score", {"score": 4, "B": 2}, r"B = 1.*got B 2"),
    ("score", {"score": 9}, r"\[1, 8\].*got 9"),
    ("score", {"score": 4, "sampling": True}, "score does not combine with sampling"),
    ("score", {"score": 4, "sampling": True, "filtering": True}, "score does not combine with sampling"),
    ("score", {"score": 4, "filtering": True}, "score does not combine with filtering"),
    ("score", {"score": 4, "speculate": 4}, "score does not combine with speculate"),
    ("score", {"score": 4, "jump_forward": 4}, "score does not combine with jump_forward"),
    ("score", {"score": 4, "beams": 2}, "score does not combine with beams"),
    ("score", {"score": 4, "weights": "fp4", "sampling": True}, "decode_weights must be one of"),
    ("score", {"score": 4, "allowed": _cpu_ids()}, "allowed must be the int32 device ids"),
    ("beam", {"beams": 4, "B": 2}, "beams=4 are the rows of the batch, got B 2"),
    ("beam", {"beams": 9, "B": 9}, r"num_beams must lie in \[1, 8\]"),
    ("beam", {"beams": 2, "B": 2, "sampling": True}, "num_beams is deterministic: temperature must be 0"),
    ("beam", {"beams": 2, "B": 2, "filtering": True}, "num_beams is deterministic: top_k / top_p must be None"),
    ("beam", {"beams": 2, "B": 2, "speculate": 2}, "num_beams does not combine with speculate"),
    ("beam", {"beams": 2, "B": 2, "jump_forward": 2}, "num_beams does not combine with jump_forward"),
]


@pytest.mark.parametrize("kind, kw, word", CTX_BAD, ids=[f"{k}-{i}" for i, (k, _, _) in enumerate(CTX_BAD)])
def test_decode_ctx_of_every_kind_rejects_before_it_allocates(kind, kw, word):
    """The stub has no device and no widths: a constructor that reached its first allocation would raise AttributeError."""
    from lap_amd.ar_decode import DecodeCtx

    kw = {"B": 1} | kw
    with pytest.raises(ValueError, match=word):
        DecodeCtx(_Stub(), kw.pop("B"), 8, 8, **kw)


def test_signatures_default_to_no_jump_forward():
    import inspect

    from lap_amd import ar_decode
    from lap_amd.model import LAP
    from lap_amd.serve import GraphedTokenDecoder, create_trained_policy_ar

    for fn in (LAP.sample_tokens, ar_decode.sample_tokens, GraphedTokenDecoder.__init__, ar_decode.DecodeCtx.__init__, create_trained_policy_ar):
        assert inspect.signature(fn).parameters["jump_forward"].default is None
