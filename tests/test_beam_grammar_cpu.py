"""lap_amd/beam.py under a grammar (`grammar_beam_step`, `grammar_beam_search`): against `beam_step` on explicitly masked logits,
against the automaton's own `accepts`, against an independent enumeration of every sentence of a small automaton, and the ValueError
of `check_num_beams`; and the gap condition of every case tests/test_beam_grammar_gpu.py runs on the kernels.  No GPU."""
import itertools

import numpy as np
import pytest

from lap_amd import beam as bm
from lap_amd import grammar as G
from tests import beam_grammar_cases as C
from tests import grammar_cases as GC


@pytest.fixture(scope="module")
def auto():
    return GC.automaton()


def _want_states(a, states, fin, par, tok, sc):
    out = []
    for r in range(len(par)):
        q = int(states[par[r]])
        out.append(q if fin[par[r]] or not sc[r] > -np.inf else a.step(q, int(tok[r])))
    return out


def _same(got, want):
    for g, w in zip(got[:5], want[:5]):
        assert np.array_equal(np.asarray(g), np.asarray(w), equal_nan=True)
    assert got[5] == want[5]


@pytest.mark.parametrize("N", C.NS)
def test_step_is_beam_step_on_masked_logits(auto, N):
    """Every top-N case (all six states, finished, dead, a state of Q and of -1, an all -inf / NaN segment, NaN inside a segment)."""
    for shift in range(len(C.KINDS)):
        x, scores, fin, states, kinds = C.topn_case(auto, N, shift)
        got = bm.grammar_beam_step(x, scores, fin, states, auto, 3, 9, C.EOS)
        want = bm.beam_step(C.masked_by_hand(auto, x, states), scores, fin, 3, 9, C.EOS)
        _same(got, want)
        assert got[6].dtype == np.int32 and got[6].tolist() == _want_states(auto, states, fin, want[0], want[1], want[3])
        # the rows that may not contribute do not: no beam has such a parent (unless it is padding that names its own index)
        silent = {b for b, k in enumerate(kinds) if k in ("dead", "bad_Q", "bad_neg", "all_inf")}
        assert all(np.isneginf(want[3][r]) for r in range(N) if want[0][r] in silent)


def test_select_cases_follow_the_rule(auto):
    cases = C.select_cases(auto)
    for name, (x, scores, fin, states, t, cap) in cases.items():
        got = bm.grammar_beam_step(x, scores, fin, states, auto, t, cap, C.EOS)
        want = bm.beam_step(C.masked_by_hand(auto, x, states), scores, fin, t, cap, C.EOS)
        _same(got, want)
        assert got[6].tolist() == _want_states(auto, states, fin, want[0], want[1], want[3]), name
    par, tok, _, sc, nf, _, ns = bm.grammar_beam_step(*cases["shared"][:4], auto, 5, 9, C.EOS)
    assert par.tolist() == [1, 0, 0, 2] and nf.tolist() == [True, False, False, False]
    assert ns[0] == 5 and tok[0] == 0                                   # the finished parent: token 0, its state stays
    assert [int(ns[r]) for r in (1, 2)] == [auto.step(1, int(tok[r])) for r in (1, 2)] and ns[3] == auto.step(4, int(tok[3]))
    par, tok, _, sc, nf, _, ns = bm.grammar_beam_step(*cases["padding"][:4], auto, 0, 9, C.EOS)
    assert par.tolist() == [0, 1, 2] and tok.tolist() == [int(auto.allowed(0)[0]), 0, 0] and ns.tolist() == [1, 0, 0]
    assert np.isneginf(sc[1:]).all() and nf.tolist() == [False, True, True]
    par, tok, _, _, nf, done, ns = bm.grammar_beam_step(*cases["all_finished"][:4], auto, 4, 9, C.EOS)
    assert par.tolist() == [0, 1, 2] and not tok.any() and done and ns.tolist() == [5, 3, 5]
    par = bm.grammar_beam_step(*cases["short"][:4], auto, 2, 9, C.EOS)[0]
    assert par.tolist() != list(range(8))


def test_a_segment_outside_the_edges_offers_nothing(auto):
    broken = G.TokenAutomaton(np.array([0, 1, 9999999]), auto.ids[:3], auto.next[:3], C.V, C.EOS)      # (not checked: on purpose)
    x, _ = C.noise(2, 5)
    s, f = np.zeros(2), np.zeros(2, bool)
    par, tok, lp, sc, nf, done, ns = bm.grammar_beam_step(x, s, f, np.array([0, 1]), broken, 0, 9, C.EOS)
    assert par.tolist() == [0, 1] and np.isneginf(sc[1]) and sc[0] == 0.0 and tok[0] == broken.ids[0]


@pytest.mark.parametrize("N", [1, 3, 8])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_every_finished_beam_of_a_search_is_a_sentence(auto, N, seed):
    rng = np.random.default_rng(seed)
    cap = 12
    calls = []

    def logits_fn(prefixes):
        calls.append(prefixes.shape[1])
        return (rng.standard_normal((N, C.V)) * 3).astype(np.float32)

    tok, lp, sc, st = bm.grammar_beam_search(logits_fn, N, cap, C.EOS, auto, early_stop=False)
    assert tok.shape == (N, cap) and calls == list(range(len(calls)))
    finished = 0
    for b in range(N):
        row = tok[b].tolist()
        if np.isfinite(sc[b]) and C.EOS in row:
            finished += 1
            assert auto.accepts(tok[b]) and st[b] == auto.num_states - 1
            assert not any(row[row.index(C.EOS) + 1:])
        elif np.isfinite(sc[b]):        # cut by the budget: still a path of the automaton
            q = 0
            for t in row:
                q = auto.step(q, t)
                assert q >= 0
            assert q == st[b]
        assert not np.isfinite(sc[b]) or abs(lp[b].sum() - sc[b]) < 1e-9
    print(f"N {N} seed {seed}: {finished} finished beams")


def _small():
    """0 -{2, 3}-> 1; 1 -{4 -> 2, 5 -> 3, EOS}; 2 -{6, EOS}; 2 -6-> 3; 3 -{EOS}; sink 4.  Live prefixes per depth: 2, 4 (+2
    finished), ...: never more than 8 candidates alive or finished in all."""
    eos = 1
    segs = [([2, 3], [1, 1]), ([1, 4, 5], [4, 2, 3]), ([1, 6], [4, 3]), ([1], [4]), ([1], [4])]
    off = np.cumsum([0] + [len(i) for i, _ in segs])
    return G.check_automaton(G.TokenAutomaton(off, np.concatenate([i for i, _ in segs]), np.concatenate([n for _, n in segs]), 8, eos))


def test_eight_beams_rank_every_sentence_of_a_small_automaton():
    a = _small()
    rng = np.random.default_rng(3)
    table = {}

    def row(prefix):
        if prefix not in table:
            table[prefix] = (rng.standard_normal(8) * 2).astype(np.float32)
        return table[prefix]

    def logits_fn(prefixes):
        return np.stack([row(tuple(p.tolist())) for p in prefixes])

    # every sentence, by walking the token alphabet (independent of the beam code): score = sum of log-softmax over the state's set
    sentences = {}
    for L in range(1, 5):
        for seq in itertools.product(range(8), repeat=L):
            if seq[-1] != 1 or 1 in seq[:-1] or not a.accepts(np.array(seq)):
                continue
            q, total = 0, 0.0
            for i, t in enumerate(seq):
                z = row(tuple(seq[:i])).astype(np.float64)[a.allowed(q)]
                total += float(row(tuple(seq[:i]))[t]) - (z.max() + np.log(np.exp(z - z.max()).sum()))
                q = a.step(q, t)
            sentences[seq] = total
    assert len(sentences) == 8         # 2 first tokens x {EOS, 4 EOS, 4 6 EOS, 5 EOS}
    tok, lp, sc, st = bm.grammar_beam_search(logits_fn, 8, 4, 1, a, early_stop=False)
    ranked = sorted(sentences.items(), key=lambda kv: -kv[1])
    for r, (seq, total) in enumerate(ranked):
        assert tok[r].tolist() == list(seq) + [0] * (4 - len(seq)), (r, tok[r], seq)
        assert abs(sc[r] - total) < 1e-9
    assert (st == 4).all()


def test_check_num_beams_takes_an_automaton_and_nothing_else(auto):
    good = dict(decode="fused", temperature=0.0, sampler="host")
    assert bm.check_num_beams(4, 1, grammar=auto, **good) == 4
    dev = G.DeviceAutomaton(None, None, None, None, auto)
    assert bm.check_num_beams(4, 1, grammar=dev, **good) == 4
    with pytest.raises(ValueError, match="grammar"):
        bm.check_num_beams(4, 1, grammar=object(), **good)
    with pytest.raises(ValueError, match="jump_forward"):
        bm.check_num_beams(4, 1, grammar=auto, jump_forward=4, **good)
    for bad in ({"speculate": 4}, {"top_k": 5}, {"temperature": 0.7}, {"num_samples": 4}, {"sampler": "device"}):
        with pytest.raises(ValueError):
            bm.check_num_beams(4, 1, grammar=auto, **(good | bad))


def test_grammar_with_allowed_tokens_keeps_check_grammars_error(auto):
    from lap_amd import ar_decode

    with pytest.raises(ValueError, match="grammar does not combine with allowed_tokens"):
        ar_decode.check_grammar(auto, C.V, C.EOS, allowed_tokens=[1, 2])


@pytest.mark.parametrize("N", C.NS)
def test_kernel_cases_meet_the_gap_condition(auto, N):
    """The GPU tests assert this again before they compare selections exactly; it is checked here, on the float64 side alone, so that
    no case can be left out there."""
    for shift in range(len(C.KINDS)):
        x, scores, fin, states, _ = C.topn_case(auto, N, shift)
        tol = C.row_tol(auto, x, states)
        row_gap, _ = bm.step_gaps(C.masked_by_hand(auto, x, states), scores, fin)
        assert row_gap > 4 * tol, (N, shift, row_gap, tol)


def test_select_cases_meet_the_gap_condition(auto):
    for name, (x, scores, fin, states, t, cap) in C.select_cases(auto).items():
        s32 = np.asarray(scores, dtype=np.float32).astype(np.float64)
        tol = C.row_tol(auto, x, states) + C.EPS * C.amax(s32)
        row_gap, sel_gap = bm.step_gaps(C.masked_by_hand(auto, x, states), s32, fin)
        assert row_gap > 4 * tol and sel_gap > 4 * tol, (name, row_gap, sel_gap, tol)
