"""lap_amd/beam.py, the numpy specification of beam search over the rows of a fused decode batch: `beam_search` against brute-force
enumeration and hand-walked examples, the rules of `beam_step` one by one, and every ValueError of `check_num_beams` and of the
surfaces that call it.  No GPU."""
import itertools

import numpy as np
import pytest

from lap_amd import beam as bm

EOS = 1
V = 5


def _table(seed, scale=2.0):
    """A prefix -> f32 logits [V] table, filled on demand from one generator."""
    rng = np.random.default_rng(seed)
    tab = {}

    def row(prefix):
        k = tuple(int(x) for x in prefix)
        if k not in tab:
            tab[k] = (rng.normal(size=V) * scale).astype(np.float32)
        return tab[k]

    return row, lambda prefixes: np.stack([row(p) for p in prefixes])


def _logp(x):
    x = np.asarray(x, dtype=np.float64)
    return x - (x.max() + np.log(np.exp(x - x.max()).sum()))


def _brute(row, cap):
    """Every sequence that ends at its first EOS or at cap tokens, with its log-probability: {tokens: score}."""
    done, alive = {}, {(): 0.0}
    for _ in range(cap):
        nxt = {}
        for p, s in alive.items():
            lp = _logp(row(p))
            for tok in range(V):
                (done if tok == EOS else nxt)[p + (tok,)] = s + lp[tok]
        alive = nxt
    return done | alive


@pytest.mark.parametrize("cap", [1, 2, 3, 4])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_exhaustive_beam_is_brute_force(seed, cap):
    """N = 8 >= the sequences alive at any depth would need V^(cap-1); so V = 5 runs at the depths where 8 beams are exhaustive
    (cap <= 2), and deeper on a 2-token + EOS table (3 ids, at most 4 alive prefixes of length 2, 8 of length 3)."""
    row, fn = _table(seed)
    if cap > 2:
        row5 = row

        def row(prefix):        # ids 3 and 4 are -inf: two continuing tokens and EOS
            x = row5(prefix).copy()
            x[3:] = -np.inf
            return x

        def fn(prefixes):
            return np.stack([row(p) for p in prefixes])
    tok, lp, sc = bm.beam_search(fn, 8, cap, EOS, early_stop=False)
    want = sorted(_brute(lambda p: row(p), cap).items(), key=lambda kv: -kv[1])
    want = [(k, s) for k, s in want if s > -np.inf]
    for r in range(min(8, len(want))):
        seq, s = want[r]
        assert tuple(tok[r, :len(seq)]) == seq and not tok[r, len(seq):].any(), (r, tok[r], seq)
        assert abs(sc[r] - s) < 1e-12 and abs(lp[r].sum() - s) < 1e-12
    # early_stop on: the same rank-0 beam (nothing alive can pass a finished best beam)
    tok1, _, sc1 = bm.beam_search(fn, 8, cap, EOS, early_stop=True)
    assert tuple(tok1[0]) == tuple(tok[0]) and sc1[0] == sc[0]


def test_hand_walked_example():
    """Two steps by hand.  Step 0 rows are identical with log-probabilities log [.5, .1, .3, .06, .04]; only row 0 counts.
    N = 2: beams (0), (2).  Step 1: after (0): [.1, .6, .2, .05, .05]; after (2): [.4, .05, .5, .03, .02].
    Candidates: (0,1) .5*.6 = .30, (2,2) .3*.5 = .15, (2,0) .3*.4 = .12, (0,2) .5*.2 = .10.  N = 2 -> (0, EOS) and (2, 2);
    N = 3 adds (2, 0) at step 1, after beams (0), (2), (1 = EOS, .1) at step 0, the finished (EOS) beam carrying .1 as one candidate:
    .30, .15, .12 beat it."""
    p0 = np.log(np.array([.5, .1, .3, .06, .04])).astype(np.float32)
    after = {0: np.log(np.array([.1, .6, .2, .05, .05])).astype(np.float32), 2: np.log(np.array([.4, .05, .5, .03, .02])).astype(np.float32),
             1: np.zeros(V, np.float32)}

    def fn(prefixes):
        return np.stack([p0 if len(p) == 0 else after[int(p[-1])] for p in prefixes])

    tok, lp, sc = bm.beam_search(fn, 2, 2, EOS, early_stop=False)
    assert tok.tolist() == [[0, 1], [2, 2]]
    np.testing.assert_allclose(np.exp(sc), [.30, .15], rtol=1e-6)
    np.testing.assert_allclose(np.exp(lp), [[.5, .6], [.3, .5]], rtol=1e-6)
    tok, lp, sc = bm.beam_search(fn, 3, 2, EOS, early_stop=False)
    assert tok.tolist() == [[0, 1], [2, 2], [2, 0]]
    np.testing.assert_allclose(np.exp(sc), [.30, .15, .12], rtol=1e-6)
    # the first step alone, N = 3: the fan-out from row 0
    s0, f0 = bm.initial(3)
    par, t, l, s, f, done = bm.beam_step(fn([(), (), ()]), s0, f0, 0, 2, EOS)
    assert par.tolist() == [0, 0, 0] and t.tolist() == [0, 2, 1] and f.tolist() == [False, False, True] and not done


@pytest.mark.parametrize("seed", [0, 3])
def test_one_beam_is_greedy(seed):
    row, fn = _table(seed)
    tok, lp, sc = bm.beam_search(fn, 1, 4, EOS)
    prefix = []
    for t in range(4):
        x = row(prefix)
        g = int(np.argmax(x))
        assert tok[0, t] == g and abs(lp[0, t] - _logp(x)[g]) < 1e-12
        prefix.append(g)
        if g == EOS:
            assert not tok[0, t + 1:].any()
            break


def test_order_and_ties():
    x = np.array([[1.0, 3.0, 3.0, 0.0, 3.0]] * 2, dtype=np.float32)
    ids, lp, _ = bm.row_topn(x[0], 3)
    assert ids.tolist() == [1, 2, 4] and lp[0] == lp[1] == lp[2]            # the lower id among equal logits
    # equal scores: the lower parent, then the lower id
    par, tok, _, sc, _, _ = bm.beam_step(x, np.zeros(2), np.zeros(2, bool), 3, 9, eos=0)
    assert par.tolist() == [0, 0] and tok.tolist() == [1, 2] and sc[0] == sc[1]
    par, tok, _, _, _, _ = bm.beam_step(np.stack([x[0]] * 4), np.zeros(4), np.zeros(4, bool), 3, 9, eos=0)
    assert par.tolist() == [0, 0, 0, 1] and tok.tolist() == [1, 2, 4, 1]
    # NaN and -inf entries are no candidates and outside the sum
    y = np.array([[np.nan, 0.0, -np.inf, 0.0, np.nan]], dtype=np.float32)
    ids, lp, lse = bm.row_topn(y[0], 4)
    assert ids.tolist() == [1, 3] and abs(lse - np.log(2)) < 1e-15


def test_finished_minus_inf_and_padding():
    x = np.zeros((3, V), np.float32)
    x[0] = [0, 5, 1, 2, 3]
    # row 1 finished: exactly one candidate (token 0, logp 0, its score); row 2 at -inf: nothing, finished or not
    for fin2 in (False, True):
        par, tok, lp, sc, fin, done = bm.beam_step(x, np.array([-1.0, -1.5, -np.inf]), np.array([False, True, fin2]), 2, 9, EOS)
        assert par.tolist() == [0, 1, 0] and tok.tolist() == [1, 0, 4] and lp[1] == 0.0 and sc[1] == -1.5
        assert fin.tolist() == [True, True, False] and done       # early_stop: the rank-0 beam emitted EOS
        assert not bm.beam_step(x, np.array([-1.0, -1.5, -np.inf]), np.array([False, True, fin2]), 2, 9, EOS, early_stop=False)[5]
    assert len(bm.candidates(x, np.array([-1.0, -1.5, -np.inf]), np.array([False, True, False]), 3)) == 3 + 1
    # fewer than N candidates: a 2-id row from the initial scores at N = 3; the rest is padding
    y = np.full((3, V), -np.inf, np.float32)
    y[:, [0, 3]] = [1.0, 2.0]
    par, tok, lp, sc, fin, done = bm.beam_step(y, *bm.initial(3), 0, 9, EOS)
    assert par.tolist() == [0, 0, 2] and tok.tolist() == [3, 0, 0] and sc[2] == -np.inf and lp[2] == 0.0
    assert fin.tolist() == [False, False, True] and not done
    # a row of -inf / NaN alone contributes nothing: every beam is padding, and the search is done
    z = np.full((2, V), -np.inf, np.float32)
    z[1] = np.nan
    par, tok, _, sc, fin, done = bm.beam_step(z, np.zeros(2), np.zeros(2, bool), 0, 9, EOS)
    assert par.tolist() == [0, 1] and not tok.any() and np.isneginf(sc).all() and fin.all() and done


def test_cap_and_early_stop():
    row, fn = _table(5)
    for cap in (1, 3):
        tok, lp, sc = bm.beam_search(fn, 2, cap, eos=-1)       # nothing ends: the budget does
        assert tok.shape == (2, cap) and np.isfinite(sc).all()
    x = np.zeros((2, V), np.float32)
    assert bm.beam_step(x, np.zeros(2), np.zeros(2, bool), 2, 3, eos=-1)[5]         # t + 1 >= cap
    assert not bm.beam_step(x, np.zeros(2), np.zeros(2, bool), 1, 3, eos=-1)[5]
    # early_stop decides only when rank 0 is finished
    x[:, EOS] = 3.0
    assert bm.beam_step(x, np.zeros(2), np.zeros(2, bool), 0, 9, EOS, early_stop=True)[5]
    assert not bm.beam_step(x, np.array([0.0, -np.inf]), np.zeros(2, bool), 0, 9, EOS, early_stop=False)[5]
    tok, _, _ = bm.beam_search(lambda p: np.stack([x[0]] * 2), 2, 4, EOS, early_stop=True)
    assert tok[0].tolist() == [EOS, 0, 0, 0] and tok[1, 1:].tolist() == [0, 0, 0]
    tok, _, sc = bm.beam_search(lambda p: np.stack([x[0]] * 2), 2, 4, EOS, early_stop=False)
    assert tok[0].tolist() == [EOS, 0, 0, 0] and EOS in tok[1].tolist() and sc[0] > sc[1]


def test_step_gaps():
    x = np.array([[0.0, 4.0, 1.0, 3.0, -np.inf]] * 2, dtype=np.float32)
    row_gap, sel_gap = bm.step_gaps(x, np.array([0.0, -np.inf]), np.zeros(2, bool))
    assert abs(row_gap - 2.0) < 1e-12 and abs(sel_gap - 2.0) < 1e-12         # 3.0 against 1.0, in both
    assert bm.step_gaps(x[:, :2], np.array([0.0, -np.inf]), np.zeros(2, bool)) == (np.inf, np.inf)


GOOD = dict(decode="fused", temperature=0.0, sampler="host", num_samples=None, top_k=None, top_p=None, speculate=None, grammar=None,
            jump_forward=None, collect=None)


@pytest.mark.parametrize("n", [1, 4, 8, np.int64(3)])
def test_check_num_beams_accepts(n):
    assert bm.check_num_beams(n, 1, **GOOD) == int(n)
    assert bm.check_num_beams(n, 1, **(GOOD | {"decode": "eager"})) == int(n)


@pytest.mark.parametrize("n, batch, change, text", [
    (2.0, 1, {}, "must be an integer"), (True, 1, {}, "must be an integer"), ("2", 1, {}, "must be an integer"),
    (0, 1, {}, r"lie in \[1, 8\]"), (9, 1, {}, r"lie in \[1, 8\]"), (2, 3, {}, "batch 1"),
    (2, 1, {"decode": "graph"}, "decode="), (2, 1, {"temperature": 0.5}, "temperature must be 0"),
    (2, 1, {"sampler": "device"}, "sampler"), (2, 1, {"num_samples": 2}, "num_samples must be None"),
    (2, 1, {"top_k": 5}, "top_k / top_p"), (2, 1, {"top_p": 0.9}, "top_k / top_p"), (2, 1, {"speculate": 4}, "speculate"),
    (2, 1, {"grammar": object()}, "grammar"), (2, 1, {"jump_forward": 4}, "jump_forward"), (2, 1, {"collect": {}}, "collect"),
])
def test_check_num_beams_rejects(n, batch, change, text):
    with pytest.raises(ValueError, match=text):
        bm.check_num_beams(n, batch, **(GOOD | change))


class _Obs:
    def __init__(self, B):
        self.tokenized_prompt = np.zeros((B, 4), np.int32)


@pytest.mark.parametrize("kw, text", [
    ({"num_beams": 9}, r"lie in \[1, 8\]"), ({"num_beams": 2, "temperature": 1.0}, "temperature must be 0"),
    ({"num_beams": 2, "num_samples": 2}, "num_samples must be None"), ({"num_beams": 2, "speculate": 2}, "speculate"),
    ({"num_beams": 2, "grammar": object()}, "grammar"), ({"num_beams": 2, "jump_forward": 2}, "jump_forward"),
    ({"num_beams": 2, "top_k": 3}, "top_k / top_p"), ({"num_beams": 2, "collect": {}}, "collect"),
    ({"num_beams": 2, "sampler": "device"}, "sampler"), ({"num_beams": 2, "draft_tokens": [1]}, "draft_tokens needs speculate"),
    ({"num_beams": 2, "decode_weights": "fp8"}, "fused decode kernels only"), ({"num_beams": 2, "decode_weights": "int4"}, "decode_weights"),
    ({"num_beams": 2, "max_decoding_steps": 0}, "max_decoding_steps"),
])
def test_sample_tokens_rejects_before_any_device_work(kw, text):
    """`sample_tokens` checks a beam request before it touches the model (a bare object stands in for it)."""
    from lap_amd import ar_decode

    with pytest.raises(ValueError, match=text):
        ar_decode.sample_tokens(object(), 0, _Obs(1), **kw)
    with pytest.raises(ValueError, match="batch 1"):
        ar_decode.sample_tokens(object(), 0, _Obs(2), num_beams=2)
