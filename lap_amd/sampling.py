"""The noise of a device-sampled LAP_AR token draw, restated on the host (numpy only; no GPU, no torch).

`LAP.sample_tokens(..., sampler="device")` draws token `t` of row `b` as the argmax over the vocabulary of

    score[j] = float32(logit[j] * inv_t) + g(seed, t, b, j)          inv_t = float32(1 / temperature)

(lowest index among ties), the Gumbel-max form of the reference's `jax.random.categorical(logits / temperature)`
(lap.py:719-724).  The noise is a pure function of (seed: uint64, step t, row b, vocabulary index j):

* Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; multipliers 0xD2511F53 /
  0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85) with key = (low, high word of the seed) and counter = (j >> 1, b, t, 0);
  index j takes output word j & 1 (words 2 and 3 are unused).
* u = ((word >> 9) + 0.5) * 2^-23: the top 23 bits, so that n + 0.5 (2 n + 1 < 2^24) and u are exact in float32 and u lies
  strictly inside (0, 1): 2^-24 <= u <= 1 - 2^-24.  (With 24 bits, n + 0.5 needs 25 significant bits once n >= 2^23; it
  rounds, and the all-ones word gives u = 1 and infinite noise.)
* g = -log(-log(u)) with the accurate float32 logarithm, so -2.81 < g < 16.64.

The kernels (csrc/sampling.hpp, used by lap_decode_lm_head_sample and lap_gumbel_argmax_rows_f32) compute the same thing; they
agree with this file up to the last bits of the two logarithms.  A served draw is reproduced offline from the raw logits with
`sample_from_logits(logits, temperature, seed, step)`.

Top-k and nucleus (top-p) filtering of such a draw (csrc/decode_filter.hip) is specified by `filter_keep` below: the token is the
argmax of the same score over the kept entries, `sample_from_logits(..., top_k=, top_p=)`.
"""
from __future__ import annotations

import numpy as np

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds.  counter: uint32 [..., 4], key: uint32 [..., 2] (broadcast against each other over the leading
    dimensions); returns uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK
    k = np.asarray(key, dtype=np.uint64) & _MASK
    if c.shape[-1] != 4 or k.shape[-1] != 2:
        raise ValueError("philox4x32_10: counter has 4 words, key has 2")
    lead = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], lead) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], lead) for i in range(2))
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(PHILOX_W0)) & _MASK
            k1 = (k1 + np.uint64(PHILOX_W1)) & _MASK
        p0, p1 = m0 * c0, m1 * c2              # 32 x 32 -> 64 bits
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _MASK, (p0 >> _S32) ^ c3 ^ k1, p0 & _MASK
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def _seed_words(seed: int):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return seed & 0xFFFFFFFF, seed >> 32


def uniform_from_word(word):
    """uint32 word -> float32 u strictly inside (0, 1), exact: ((word >> 9) + 0.5) * 2^-23."""
    n = (np.asarray(word, dtype=np.uint32) >> np.uint32(9)).astype(np.float32)
    return (n + np.float32(0.5)) * np.float32(2.0 ** -23)


def gumbel_from_word(word):
    """uint32 word -> float32 Gumbel noise -log(-log(u))."""
    u = uniform_from_word(word)
    return -np.log(-np.log(u, dtype=np.float32), dtype=np.float32)


def gumbel_noise(seed: int, step: int, rows: int, vocab_size: int) -> np.ndarray:
    """float32 [rows, vocab_size]: the noise of decode step `step` under `seed` (a 64-bit integer)."""
    lo, hi = _seed_words(seed)
    units = (vocab_size + 1) // 2
    ctr = np.zeros((rows, units, 4), dtype=np.uint32)
    ctr[..., 0] = np.arange(units, dtype=np.uint32)[None, :]
    ctr[..., 1] = np.arange(rows, dtype=np.uint32)[:, None]
    ctr[..., 2] = np.uint32(int(step) & 0xFFFFFFFF)
    words = philox4x32_10(ctr, np.array([lo, hi], dtype=np.uint32))[..., :2].reshape(rows, 2 * units)[:, :vocab_size]
    return gumbel_from_word(words)


def inverse_temperature(temperature: float) -> np.float32:
    """float32(1 / temperature); 0 (greedy) for temperature <= 0, as under the reference's `temperature > 0.0` test."""
    temperature = float(temperature)
    if temperature != temperature:
        raise ValueError("temperature is NaN")
    if temperature <= 0.0:
        return np.float32(0.0)
    with np.errstate(over="ignore"):
        inv_t = np.float32(1.0 / temperature)
    if not np.isfinite(inv_t):
        raise ValueError(f"temperature {temperature!r}: 1 / temperature is not finite in float32")
    return inv_t


def scores_from_logits(logits, temperature: float, seed: int, step: int) -> np.ndarray:
    """float32 [rows, V]: logit * inv_t + noise (two float32 roundings: the product, then the sum); the raw logits when greedy."""
    lg = np.ascontiguousarray(np.asarray(logits, dtype=np.float32))
    if lg.ndim != 2:
        raise ValueError("logits: [rows, vocab_size]")
    inv_t = inverse_temperature(temperature)
    if inv_t == 0.0:
        return lg
    return lg * inv_t + gumbel_noise(seed, step, lg.shape[0], lg.shape[1])


def sample_from_logits(logits, temperature: float, seed: int, step: int, top_k=None, top_p=None) -> np.ndarray:
    """int32 [rows]: the token every row of float32 `logits` [rows, V] draws at decode step `step` under `seed`; the argmax
    (lowest index among ties) when temperature <= 0.  top_k / top_p: the argmax runs over the entries `filter_keep` keeps; with
    both neutral (None) this is the unfiltered draw, bit for bit."""
    sc = scores_from_logits(logits, temperature, seed, step)
    k, p = check_filter(top_k, top_p)
    if (k or p < 1.0) and inverse_temperature(temperature) != 0.0:
        sc = np.where(filter_keep(logits, temperature, top_k, top_p), sc, -np.inf).astype(np.float32)
        # (a kept entry always beats -inf: its score is finite; an all -inf row keeps index 0 as before)
    return np.argmax(sc, axis=-1).astype(np.int32)


# ---- top-k and nucleus (top-p) filtering (the specification of csrc/decode_filter.hip)
def check_filter(top_k, top_p):
    """(k, p) as the kernels take them: k an int >= 0 (0: keep all), p a float32 value in (0, 1] (1: keep all); None is the
    neutral value of either.  ValueError naming the value otherwise."""
    k = 0
    if top_k is not None:
        if isinstance(top_k, bool) or not isinstance(top_k, (int, np.integer)) or int(top_k) < 0 or int(top_k) > 0x7FFFFFFF:
            raise ValueError(f"top_k must be an integer >= 0 (0 or None: no top-k filter), got {top_k!r}")
        k = int(top_k)
    p = 1.0
    if top_p is not None:
        try:
            p = float(top_p)
        except (TypeError, ValueError):
            raise ValueError(f"top_p must lie in (0, 1], got {top_p!r}") from None
        if isinstance(top_p, bool) or not 0.0 < p <= 1.0:
            raise ValueError(f"top_p must lie in (0, 1], got {top_p!r}")
        p = float(np.float32(p))        # the kernels read top_p as a float32 word
        if p <= 0.0:
            raise ValueError(f"top_p must lie in (0, 1] as a float32, got {top_p!r}")
    return k, p


def _filter_order(logits, temperature):
    """(z float64 [rows, V], order int64 [rows, V], candidates int64 [rows]): z = float32(logit * inv_t) (the raw logit when greedy),
    the columns of every row by z descending, then index ascending, and the number of entries with z > -inf (they come first)."""
    lg = np.ascontiguousarray(np.asarray(logits, dtype=np.float32))
    if lg.ndim != 2:
        raise ValueError("logits: [rows, vocab_size]")
    inv_t = inverse_temperature(temperature)
    z = (lg * inv_t if inv_t != 0.0 else lg).astype(np.float64)
    order = np.argsort(-z, axis=1, kind="stable")          # stable: equal z keep their index order
    return z, order, (z > -np.inf).sum(axis=1)


def _filter_cut(z, order, ncand, k, p):
    """Per row: (kept count, cumulative masses c [rows, V] in order relative to exp(z - max z), W [rows]) under top_k = k, top_p = p."""
    rows, V = z.shape
    zs = np.take_along_axis(z, order, axis=1)
    n_k = np.where((k == 0) | (k >= ncand), ncand, k)       # what top_k keeps
    rank = np.arange(V)[None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(rank < n_k[:, None], np.exp(zs - zs[:, :1]), 0.0)
    w = np.where(np.isfinite(w), w, 0.0)
    c = np.cumsum(w, axis=1)
    W = c[:, -1]
    if p >= 1.0:
        return n_k, c, W
    before = np.concatenate([np.zeros((rows, 1)), c[:, :-1]], axis=1)      # c_{r-1}
    keep = (rank < n_k[:, None]) & ((before < p * W[:, None]) | (rank == 0))
    return np.minimum(keep.sum(axis=1), n_k), c, W


def filter_keep(logits, temperature: float, top_k=None, top_p=None) -> np.ndarray:
    """bool [rows, V]: the entries of float32 `logits` a filtered draw chooses among.  One row at one step:

    * z[j] = float32(logit[j] * inv_t), the product the sampler forms; everything after it is float64.  The candidates are the
      entries with z > -inf (a constrained decode leaves -inf outside its set), ordered by z descending, then index ascending.
    * top_k keeps the first k of that order; None, 0 or k >= the number of candidates keeps all; ties at the cut go to the lower
      indices.
    * top_p (0 < top_p <= 1, taken as float64(float32(top_p)): the kernels read a float32 word) applies to what top_k kept:
      w = exp(z - max z), W = sum w, c_r the cumulative mass in order; rank r is kept while c_{r-1} < top_p * W; rank 0 always;
      None or 1 keeps all.
    * temperature <= 0 (greedy) ignores both: the argmax is always kept, so every candidate is reported kept."""
    k, p = check_filter(top_k, top_p)
    z, order, ncand = _filter_order(logits, temperature)
    if inverse_temperature(temperature) == 0.0:
        k, p = 0, 1.0
    n, _, _ = _filter_cut(z, order, ncand, k, p)
    keep_sorted = np.arange(z.shape[1])[None, :] < n[:, None]
    keep = np.zeros(z.shape, dtype=bool)
    np.put_along_axis(keep, order, keep_sorted, axis=1)
    return keep


# The relative mass error of the kernel's cut (csrc/decode_filter.hip), from what it computes:
#   * a mass is q = floor(expf(hi) (1 + lo) 2^40) with z - max z = hi + lo exactly (two-sum).  expf is within 1 ulp (relative
#     2^-23), the fma that applies (1 + lo) rounds once more (2^-24), exp(lo) - (1 + lo) <= lo^2 / 2 <= 2^-41 (|lo| <= ulp(hi) / 2 <=
#     2^-20 where a mass is not zero, |hi| < 32): relative error at most 1.5 * 2^-23 + 2^-40 of the entry's own mass, hence of any sum
#     of masses;
#   * the truncation to a multiple of 2^-40 loses less than 2^-40 per entry, V * 2^-40 over a row, relative to W >= 1 (the largest
#     entry has mass 1); the sums themselves are integers and exact; ceil(top_p * W) moves the threshold by less than one more unit.
# Both c_r and top_p * W carry that error (top_p <= 1), so a comparison c_r < top_p * W can come out differently from float64 only
# when |c_r - top_p W| / W <= 2 * (1.5 * 2^-23 + (V + 2) * 2^-40); for V <= 2^18 (the vocabulary has 257,152 entries):
FILTER_MARGIN = 2.0 * (1.5 * 2.0 ** -23 + (2 ** 18 + 2) * 2.0 ** -40)        # 8.35e-07


def filter_margin(logits, temperature: float, top_k=None, top_p=None) -> np.ndarray:
    """float64 [rows]: the smallest |c_r - top_p * W| / W over the comparisons next to the top_p cut: the last one that held
    (c_{n-2} < top_p W, when n >= 2 entries are kept) and the first one that failed (c_{n-1} >= top_p W, when top_p and not top_k
    or the end of the candidates ended the kept set).  inf where top_p decides nothing (None, 1, greedy).  A kernel whose masses
    are within FILTER_MARGIN of float64 keeps exactly `filter_keep`'s set in every row whose margin exceeds FILTER_MARGIN."""
    k, p = check_filter(top_k, top_p)
    z, order, ncand = _filter_order(logits, temperature)
    rows = z.shape[0]
    out = np.full(rows, np.inf)
    if p >= 1.0 or inverse_temperature(temperature) == 0.0:
        return out
    n, c, W = _filter_cut(z, order, ncand, k, p)
    n_k = np.where((k == 0) | (k >= ncand), ncand, k)
    for b in range(rows):
        if ncand[b] == 0 or not W[b] > 0.0:
            continue
        t = p * W[b]
        if n[b] >= 2:
            out[b] = min(out[b], abs(c[b, n[b] - 2] - t) / W[b])
        if n[b] < n_k[b]:
            out[b] = min(out[b], abs(c[b, n[b] - 1] - t) / W[b])
    return out


# ---- token log-probabilities and best-of-N selection (the specification of lap_decode_lm_head_lp / lap_decode_finish_lp)
def token_logprobs(logits, tokens, temperature: float, allowed=None) -> np.ndarray:
    """float64 [rows]: log softmax(z)[token] per row of float32 `logits` [rows, V], where z = float32(logit * inv_t) is the product
    the sampler forms (z = logit when temperature <= 0: a greedy decode scores its tokens at tau = 1) and everything after that
    product is float64.  allowed: the softmax runs over these vocabulary ids only (a constrained decode); a token outside the set
    has log-probability -inf.  The noise of a draw plays no part: this is the probability of the token, not of the draw."""
    lg = np.ascontiguousarray(np.asarray(logits, dtype=np.float32))
    if lg.ndim != 2:
        raise ValueError("logits: [rows, vocab_size]")
    tok = np.asarray(tokens).reshape(-1).astype(np.int64)
    if tok.shape[0] != lg.shape[0]:
        raise ValueError(f"tokens: one per row of logits, got {tok.shape[0]} for {lg.shape[0]} rows")
    inv_t = inverse_temperature(temperature)
    z = (lg * inv_t if inv_t != 0.0 else lg).astype(np.float64)
    rows = np.arange(lg.shape[0])
    z_tok = z[rows, tok]
    if allowed is not None:
        ids = np.unique(np.asarray(allowed).reshape(-1).astype(np.int64))
        ids = ids[(ids >= 0) & (ids < lg.shape[1])]
        if ids.size == 0:
            raise ValueError("allowed: no id inside the vocabulary")
        z_tok = np.where(np.isin(tok, ids), z_tok, -np.inf)
        z = z[:, ids]
    m = z.max(axis=1)
    return z_tok - (m + np.log(np.exp(z - m[:, None]).sum(axis=1)))


def _counted(tokens, eos: int) -> np.ndarray:
    """bool [rows, steps]: the positions of a row up to and including its first EOS (all of them when it has none)."""
    tok = np.asarray(tokens)
    if tok.ndim != 2:
        raise ValueError("tokens: [rows, steps]")
    after = np.cumsum(tok == eos, axis=1) - (tok == eos)        # EOS tokens strictly before a position
    return after == 0


def sequence_logprob(tokens, logprobs, eos: int) -> np.ndarray:
    """float64 [rows]: the sum of a row's token log-probabilities up to and including its first `eos` token, or over the whole
    row when it has none (a decode keeps writing a finished row until every row has finished: those tokens do not count)."""
    lp = np.asarray(logprobs, dtype=np.float64)
    keep = _counted(tokens, eos)
    if lp.shape != keep.shape:
        raise ValueError(f"logprobs {lp.shape} beside tokens {keep.shape}")
    return np.where(keep, lp, 0.0).sum(axis=1)


def select_best(tokens, logprobs, eos: int, rule: str = "sum") -> int:
    """The row a best-of-N request answers with: the largest `sequence_logprob` ("sum") or that sum divided by the number of
    tokens counted ("mean", which does not favour short answers); the lowest row among ties."""
    if rule not in ("sum", "mean"):
        raise ValueError(f"select_best: rule must be 'sum' or 'mean', got {rule!r}")
    score = sequence_logprob(tokens, logprobs, eos)
    if rule == "mean":
        score = score / _counted(tokens, eos).sum(axis=1)
    return int(np.argmax(score))
