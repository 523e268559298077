"""Top-k / top-p filtering of a device-sampled draw, without a GPU: `sampling.filter_keep` against a plain sort-based restatement,
the argument checks of `sample_tokens`, and the share of the kernel test's inputs (tests/topk_topp_cases.py) that sit on a cut."""
import numpy as np
import pytest

from lap_amd import sampling as S
from tests import topk_topp_cases as C


def _keep_by_sorting(lg, T, k, p):
    """The rules of the issue, one row at a time with python sorting: candidates z > -inf, by (-z, index); first k; then rank r
    while c_{r-1} < p W, rank 0 always."""
    inv_t = S.inverse_temperature(T)
    out = np.zeros(lg.shape, dtype=bool)
    for b, row in enumerate(lg):
        z = (row * inv_t).astype(np.float32).astype(np.float64) if inv_t != 0.0 else row.astype(np.float64)
        cand = sorted((j for j in range(len(z)) if z[j] > -np.inf), key=lambda j: (-z[j], j))
        if inv_t != 0.0:
            if k and k < len(cand):
                cand = cand[:k]
            if p is not None and p < 1.0 and cand:
                p64 = float(np.float32(p))
                w = np.exp(z[cand] - z[cand[0]])
                c = np.concatenate([[0.0], np.cumsum(w)[:-1]])
                W = np.cumsum(w)[-1]
                cand = [j for r, j in enumerate(cand) if r == 0 or c[r] < p64 * W]
        out[b, cand] = True
    return out


def _inputs(n, ties, holes):
    rng = np.random.default_rng(n + 7 * ties + 13 * holes)
    lg = (rng.standard_normal((3, n)) * 2.0).astype(np.float32)
    if ties:
        lg = (lg.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)     # bf16 values: many exact ties
    if holes:
        lg[:, rng.permutation(n)[:n // 3]] = -np.inf
        lg[2, :] = -np.inf
        lg[2, [5, n - 1]] = [0.25, 0.25]                                        # two tied candidates in a row of -inf
    return lg


@pytest.mark.parametrize("holes", [False, True])
@pytest.mark.parametrize("ties", [False, True])
def test_filter_keep_matches_the_sorting_restatement(ties, holes):
    n = 301
    lg = _inputs(n, ties, holes)
    for T in (0.7, 2.0):
        for k in (None, 0, 1, 2, 50, n - 1, n, n + 5):
            for p in (None, 1e-6, 0.5, 0.9, 1.0):
                got = S.filter_keep(lg, T, k, p)
                assert np.array_equal(got, _keep_by_sorting(lg, T, k, p)), (T, k, p)
                assert (got.sum(1) >= 1).all() and not (got & np.isneginf(lg)).any()
    if ties:        # the cut falls inside a group of equal values somewhere in the sweep: the lower indices are kept
        z = lg[0] * S.inverse_temperature(0.7)
        hit = 0
        for k in range(1, 60):
            kept = np.flatnonzero(S.filter_keep(lg[:1], 0.7, k, None)[0])
            assert len(kept) == min(k, int((z > -np.inf).sum()))
            zc = z[kept].min()
            same = np.flatnonzero(z == zc)
            if len(same) > int((z[kept] == zc).sum()):
                hit += 1
                assert np.array_equal(kept[z[kept] == zc], same[:int((z[kept] == zc).sum())])
        assert hit > 0


def test_greedy_ignores_the_filters_and_top_k_1_is_the_argmax():
    lg = _inputs(301, True, True)
    assert np.array_equal(S.filter_keep(lg, 0.0, 1, 0.1), lg > -np.inf)
    assert np.array_equal(S.sample_from_logits(lg, 0.0, 3, 1, 1, 0.1), S.sample_from_logits(lg, 0.0, 3, 1))
    z = lg * S.inverse_temperature(0.7)
    for seed in (0, 1, 2 ** 40 + 5):
        for step in (0, 7):
            assert np.array_equal(S.sample_from_logits(lg, 0.7, seed, step, top_k=1), np.argmax(z, axis=1))
            assert np.array_equal(S.sample_from_logits(lg, 0.7, seed, step, top_p=1e-6), np.argmax(z, axis=1))


def test_neutral_filters_are_the_unfiltered_draw():
    lg = _inputs(301, False, True)
    for T in (0.7, 2.0):
        plain = np.argmax(S.scores_from_logits(lg, T, 11, 4), axis=-1).astype(np.int32)
        for k, p in ((None, None), (0, None), (None, 1.0), (301, 1.0), (10 ** 6, None)):
            got = S.sample_from_logits(lg, T, 11, 4, top_k=k, top_p=p)
            assert got.dtype == np.int32 and np.array_equal(got, plain)
    # a filtered draw is the best kept score
    keep = S.filter_keep(lg, 0.7, 20, 0.8)
    tok = S.sample_from_logits(lg, 0.7, 11, 4, 20, 0.8)
    sc = S.scores_from_logits(lg, 0.7, 11, 4)
    assert keep[np.arange(3), tok].all() and np.array_equal(tok, np.where(keep, sc, -np.inf).argmax(1))


def test_filter_margin():
    lg = np.log(np.array([[0.5, 0.25, 0.125, 0.125]], dtype=np.float64)).astype(np.float32)
    assert np.isinf(S.filter_margin(lg, 1.0, 2, None)[0]) and np.isinf(S.filter_margin(lg, 0.0, None, 0.5)[0])
    # p = 0.6: ranks 0, 1 kept (c_0 = 0.5 < 0.6 <= c_1 = 0.75): the nearer comparison is 0.1 away
    assert S.filter_keep(lg, 1.0, None, 0.6)[0].tolist() == [True, True, False, False]
    assert abs(S.filter_margin(lg, 1.0, None, 0.6)[0] - 0.1) < 1e-6
    # p = 0.5 exactly: c_0 = 0.5 is not < 0.5: one entry, and the case sits on the cut
    assert S.filter_keep(lg, 1.0, None, 0.5)[0].sum() == 1 and S.filter_margin(lg, 1.0, None, 0.5)[0] <= S.FILTER_MARGIN
    # top_k = 2 first: W = 0.75, p W = 0.45: rank 0 only (0.5 >= 0.45), 0.05 / 0.75 away
    assert S.filter_keep(lg, 1.0, 2, 0.6)[0].sum() == 1 and abs(S.filter_margin(lg, 1.0, 2, 0.6)[0] - 0.05 / 0.75) < 1e-6
    assert 5e-7 < S.FILTER_MARGIN < 1e-6


class _Stub:
    """What `ar_decode.sample_tokens` touches before its first device call."""
    class config:
        vocab_size = 64
    EOS_TOKEN = 1

    def _serving_weights(self):
        raise AssertionError("device work before the arguments were checked")


class _Obs:
    class tokenized_prompt:
        shape = (1, 8)


@pytest.mark.parametrize("kw, word", [({"top_k": -1}, "-1"), ({"top_k": 2.5}, "2.5"), ({"top_k": True}, "True"), ({"top_p": 0.0}, "0.0"),
                                      ({"top_p": 1.5}, "1.5"), ({"top_p": -0.1}, "-0.1"), ({"top_p": float("nan")}, "nan"),
                                      ({"top_p": "x"}, "'x'"), ({"top_p": 1e-60}, "1e-60")])
def test_sample_tokens_rejects_bad_filter_values(kw, word):
    from lap_amd import ar_decode

    with pytest.raises(ValueError, match=word.replace(".", r"\.")):
        ar_decode.sample_tokens(_Stub(), 0, _Obs(), temperature=0.7, sampler="device", **kw)


def test_sample_tokens_filters_need_the_device_sampler():
    from lap_amd import ar_decode

    for kw in ({"top_k": 5}, {"top_p": 0.9}):
        with pytest.raises(ValueError, match="sampler"):
            ar_decode.sample_tokens(_Stub(), 0, _Obs(), temperature=0.7, sampler="host", **kw)
        with pytest.raises(ValueError, match="sampler"):
            ar_decode.sample_tokens(_Stub(), 0, _Obs(), temperature=0.7, **kw)
    assert ar_decode.check_filter(5, 0.9, sampler="device", temperature=0.7) == (5, float(np.float32(0.9)))
    assert ar_decode.check_filter(5, 0.9, sampler="host", temperature=0.0) is None        # greedy: the argmax is always kept
    assert ar_decode.check_filter(None, None, sampler="host", temperature=0.7) is None
    assert ar_decode.check_filter(0, 1.0, sampler="device", temperature=0.7) is None


def test_few_kernel_test_inputs_sit_on_a_cut():
    """The condition of tests/test_topk_topp_gpu.py's kernel sweep: at most 5 % of its (row, case) pairs have a filter margin within
    FILTER_MARGIN (there the kernel's kept set may differ from float64's)."""
    total = near = 0
    for B in C.BS:
        for V in C.VS:
            for T in C.TEMPS:
                lg = C.logits(B, V)
                for k, p in C.grid(B, V):
                    fm = S.filter_margin(lg, T, k, p)
                    total += B
                    near += int((fm <= S.FILTER_MARGIN).sum())
    assert total == sum(C.BS) * len(C.VS) * len(C.TEMPS) * 24
    assert near <= C.SHARE * total, (near, total)
