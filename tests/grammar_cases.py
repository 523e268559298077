"""The inputs of the grammar kernel tests, shared by tests/test_grammar_cpu.py (which checks, without a GPU, that few sampled cases
sit on a near-tie) and tests/test_grammar_gpu.py (which runs lap_decode_grammar_finish on them).  numpy only."""
import numpy as np

from lap_amd import grammar as G
from lap_amd import sampling as S
from tests.topk_topp_cases import MARGIN, SCALE, SHARE  # noqa: F401  (the comparison rule of tests/test_topk_topp_gpu.py)

V = 8195
EOS = V - 1                     # the largest index: the last entry of a segment
BS = (1, 5, 8)
TEMPS = (0.7, 1.3)
SIZES = (1, 2, 63, 257, 1500)   # the segments of states 0 .. 4 (1500 > the block of 256 threads: the stride loop runs); 5: the sink
SEED = 20261020
STEPS_SAMPLED = 6               # decode steps per (B, temperature) of the sampled test


def automaton():
    """Six states.  0 -> 1; 1 -> 2 | 3; the entries of 2, 3 and 4 lead to random states 0 .. 4; 3 and 4 hold the EOS edge to the
    sink; 2 holds vocabulary index 0."""
    rng = np.random.default_rng(11)
    segs = []
    for q, n in enumerate(SIZES):
        eos = q >= 3
        ids = np.sort(rng.permutation(np.arange(1, EOS))[:n - int(eos) - int(q == 2)])
        if q == 2:
            ids = np.concatenate([[0], ids])
        nxt = rng.integers(0, 5, size=ids.shape[0])
        if q == 0:
            nxt[:] = 1
        if q == 1:
            nxt[:] = (2, 3)
        if eos:
            ids, nxt = np.concatenate([ids, [EOS]]), np.concatenate([nxt, [5]])
        segs.append((ids, nxt))
    segs.append((np.array([EOS]), np.array([5])))
    off = np.cumsum([0] + [len(i) for i, _ in segs])
    return G.check_automaton(G.TokenAutomaton(off, np.concatenate([i for i, _ in segs]), np.concatenate([n for _, n in segs]), V, EOS))


def logits(T, B, seed=0):
    """float32 [T, B, V] = SCALE * standard normal."""
    return (np.random.default_rng(7000 + 100 * T + B + seed).standard_normal((T, B, V)) * SCALE).astype(np.float32)


def start_states(B, shift=2):
    """Rows start in different states: (b + shift) % 5."""
    return (np.arange(B) + shift) % 5


def clear_rows(a, lg, q, T, step, seed=SEED):
    """bool [B]: the two best host scores of every row over its state's set lie further apart than MARGIN (the host's decision
    alone; a set of one entry is clear)."""
    masked = np.full(lg.shape, -np.inf, dtype=np.float32)
    for b in range(lg.shape[0]):
        ids = a.allowed(int(q[b]))
        masked[b, ids] = lg[b, ids]
    sc = S.scores_from_logits(masked, T, seed, step)
    top2 = np.partition(sc, -2, axis=1)[:, -2:]
    return top2[:, 1] - top2[:, 0] > MARGIN         # (inf - finite = inf: clear)


def sampled_reference(a, B, T, steps=STEPS_SAMPLED, seed=SEED):
    """`grammar.decode_reference` over `steps` steps of B rows at temperature T from `start_states`, and which (row, step) pairs
    are clear: (logits [steps, B, V], tokens [B, steps], logprobs [B, steps], states [B, steps + 1], clear [B, steps])."""
    lg = logits(steps, B, seed=int(T * 10))
    tok, lp, st = G.decode_reference(lg, a, T, seed=seed, rows=B, start=start_states(B))
    clear = np.stack([clear_rows(a, lg[t], st[:, t], T, t, seed) for t in range(steps)], 1)
    return lg, tok, lp, st, clear
