"""The inputs of the grammar beam kernel tests, shared by tests/test_beam_grammar_cpu.py (which checks, without a GPU, that every
case meets the gap condition on its float64 side) and tests/test_beam_grammar_gpu.py (which runs lap_decode_beam_grammar_topn and
lap_decode_beam_grammar_select on them).  numpy only.

The automaton is tests/grammar_cases.automaton(): V = 8195 and segments of 1, 2, 63, 257 and 1500 entries beside the sink, so a
segment is shorter than N, shorter than a wave, leaves threads idle, or (1500 > 256 threads) makes the stride loop run and a
thread's list hold several entries.

Tolerance of a log-probability (`tol_lp`), from the kernel's order of operations, eps = 2^-24, for a segment of S entries:
* a thread (of 256) pushes n = ceil(S / 256) entries into its pair (m, s); a push is one expf (taken as 2 ulp), one product and one
  sum, so s gains a relative error of at most 4 eps per push;
* the pairs merge over 6 shuffle levels and 3 waves, 9 merges of two expf, two products and one sum: at most 8 eps each;
* the argument z - m of an expf is itself rounded: a relative error of up to eps |z - m| <= 2 A eps on that term, hence at most
  2 A eps on the sum (the summand 2 A below), A the largest finite |logit| of the segment;
* all terms are positive, so the relative error of the sum is at most (4 n + 72) eps (1.01 covers the second order), and that is
  the absolute error of its logarithm;
* logf (2 ulp of |log sum| <= ln S), the sum m + log (eps |lse|) and the difference logit - lse (eps |logp|), with |lse| and |logp|
  at most A + ln S each.
  tol_lp = eps (1.01 (4 n + 72) + 2 ln S + 2 (A + ln S) + 2 A).
This is `tol_lp` of tests/test_beam_gpu.py with the entries one thread handles and the segment size in place of V."""
import math

import numpy as np

from lap_amd import beam as bm
from tests import grammar_cases as GC

V, EOS = GC.V, GC.EOS
EPS = 2.0 ** -24
NS = (1, 3, 8)
# what a row of a top-N case is: in one of the six states, or one of the kinds the kernel must treat apart
KINDS = ("q0", "q1", "q2", "q3", "q4", "q5", "finished", "dead", "bad_Q", "bad_neg", "all_inf", "nan")


def tol_lp(size, A):
    n = -(-max(size, 1) // 256)
    ln = math.log(max(size, 2))
    return EPS * (1.01 * (4 * n + 72) + 2 * ln + 2 * (A + ln) + 2 * A)


def amax(x):
    f = np.asarray(x, dtype=np.float64)
    f = f[np.isfinite(f)]
    return float(np.abs(f).max()) if f.size else 0.0


def masked_by_hand(a, x, states):
    """f32 [N, V]: x with -inf outside the set of every row's state, built here from `allowed` alone (not `beam.grammar_masked`);
    a state outside [0, Q) leaves the row at -inf."""
    out = np.full(x.shape, -np.inf, dtype=np.float32)
    for b, q in enumerate(states):
        if 0 <= q < a.num_states:
            ids = a.allowed(int(q))
            out[b, ids] = x[b, ids]
    return out


def row_tol(a, x, states):
    """The largest tol_lp over the rows: each with the size of its state's segment and the largest finite |logit| inside it."""
    m = masked_by_hand(a, x, states)
    size = lambda q: len(a.allowed(int(q))) if 0 <= q < a.num_states else 1
    return max(tol_lp(size(states[b]), amax(m[b])) for b in range(x.shape[0]))


def lead(a, x, b, q, rng, n=10):
    """Row b gets min(size, n) leading entries of the segment of q, 0.5 apart from 10 down (0.03 b lower per row), at random
    entries of the segment; the rest keeps its clipped noise."""
    ids = a.allowed(q)
    pick = rng.permutation(ids)[:n]
    x[b, pick] = 10.0 - 0.5 * np.arange(pick.size) - 0.03 * b
    return pick


def noise(N, seed):
    rng = np.random.default_rng(seed)
    return np.clip(rng.normal(size=(N, V)) * 1.5, -4.0, 4.0).astype(np.float32), rng


def topn_case(a, N, shift):
    """One launch of the top-N kernel: row b is of kind KINDS[(b + shift) % 12].  Returns (x f32 [N, V], scores, finished, states,
    kinds); over shift = 0 .. 11 every row takes every kind once."""
    x, rng = noise(N, 1000 * N + shift)
    scores, fin, states = -0.25 * np.arange(N), np.zeros(N, bool), np.zeros(N, np.int32)
    kinds = [KINDS[(b + shift) % len(KINDS)] for b in range(N)]
    for b, kind in enumerate(kinds):
        q = int(kind[1]) if kind[0] == "q" else {"finished": 5, "dead": 2, "bad_Q": a.num_states, "bad_neg": -1, "all_inf": 3, "nan": 4}[kind]
        states[b] = q
        if 0 <= q < a.num_states:
            pick = lead(a, x, b, q, rng)
        if kind == "finished":
            fin[b] = True
        elif kind == "dead":
            scores[b] = -np.inf
        elif kind == "all_inf":
            ids = a.allowed(q)
            x[b, ids] = -np.inf
            x[b, ids[5]] = np.nan
        elif kind == "nan":         # the leading entry and two others of the segment are NaN: left out of the sum, no candidates
            ids = a.allowed(q)
            x[b, pick[0]] = np.nan
            x[b, ids[[3, 700]]] = np.nan
    return x, scores, fin, states, kinds


def select_cases(a):
    """{name: (x, scores, finished, states, t, cap)} for topn + select.
    shared: N = 4 at t = 5; row 0 in state 1 (2 edges), row 1 finished in the sink, row 2 in state 4 (1500 edges), row 3 dead: the
      parents are [1, 0, 0, 2], a non-identity permutation in which two beams share a parent and one parent is finished.
    padding: N = 3 from the initial scores in state 0 (one edge): one candidate, two padding beams.
    short: N = 8 at t = 2, the rows in states 1 (2 edges), 0 (1 edge), 2, 3, 4, 1, 0, 2 with spread scores: rows with fewer than N
      edges beside rows with more.
    all_finished: N = 3, every beam finished: each carries itself and its state."""
    cases = {}
    x, rng = noise(4, 41)
    st = np.array([1, 5, 4, 2], np.int32)
    for b in (0, 2, 3):
        lead(a, x, b, int(st[b]), rng)
    cases["shared"] = (x, np.array([-0.1, -0.3, -0.2, -np.inf]), np.array([False, True, False, False]), st, 5, 9)
    x, rng = noise(3, 42)
    lead(a, x, 0, 0, rng)
    s0, f0 = bm.initial(3)
    cases["padding"] = (x, s0, f0, np.zeros(3, np.int32), 0, 9)
    x, rng = noise(8, 43)
    st = np.array([1, 0, 2, 3, 4, 1, 0, 2], np.int32)
    for b in range(8):
        lead(a, x, b, int(st[b]), rng)
    cases["short"] = (x, -0.8 * np.arange(8) - 0.1, np.zeros(8, bool), st, 2, 9)
    x, rng = noise(3, 44)
    cases["all_finished"] = (x, np.array([-0.5, -0.7, -2.0]), np.ones(3, bool), np.array([5, 3, 5], np.int32), 4, 9)
    return cases
