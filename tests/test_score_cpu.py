"""Teacher-forced scoring, the parts that need no GPU: `score.score_reference` against a direct float64 log-softmax, and every
ValueError of the surface (`score.check_score_args`, and the exclusions of `DecodeCtx(score=...)` through `score.check_score_ctx`,
which is what the context calls before it allocates anything)."""
import numpy as np
import pytest

from lap_amd import score as SC


def _log_softmax64(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max(axis=-1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(axis=-1, keepdims=True)))


@pytest.mark.parametrize("V", [7, 1001])
@pytest.mark.parametrize("temperature", [0.0, 0.7])
@pytest.mark.parametrize("with_set", [False, True])
def test_score_reference_is_the_float64_log_softmax(V, temperature, with_set):
    rs = np.random.RandomState(V + int(temperature * 10) + with_set)
    L = 9
    lg = (rs.randn(L, V) * 3).astype(np.float32)
    allowed = np.sort(rs.choice(V, size=max(3, V // 19), replace=False)) if with_set else None
    pool = allowed if with_set else np.arange(V)
    tgt = rs.choice(pool, size=L).astype(np.int64)
    logp, greedy = SC.score_reference(lg, tgt, temperature=temperature, allowed=allowed)
    assert logp.dtype == np.float64 and logp.shape == (L,) and greedy.dtype == np.int32 and greedy.shape == (L,)
    z = lg if temperature == 0.0 else (lg * np.float32(1.0 / temperature)).astype(np.float32)
    assert z.dtype == np.float32
    if with_set:
        full = np.full((L, V), -np.inf)
        full[:, allowed] = _log_softmax64(z[:, allowed])
        want_greedy = allowed[np.argmax(z[:, allowed], axis=1)]
    else:
        full = _log_softmax64(z)
        want_greedy = np.argmax(z, axis=1)
    np.testing.assert_allclose(logp, full[np.arange(L), tgt], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(greedy, want_greedy)
    assert np.isfinite(logp).all() and (logp <= 0).all()


def test_targets_outside_the_set_or_the_vocabulary_score_minus_inf():
    rs = np.random.RandomState(0)
    V = 7
    lg = rs.randn(4, V).astype(np.float32)
    logp, _ = SC.score_reference(lg, [V, -1, 3, 0])
    assert logp[0] == -np.inf and logp[1] == -np.inf and np.isfinite(logp[2:]).all()
    logp, greedy = SC.score_reference(lg, [2, 3, 5, V], allowed=[1, 3, 5])
    assert logp[0] == -np.inf and logp[3] == -np.inf and np.isfinite(logp[1:3]).all()
    assert set(greedy.tolist()) <= {1, 3, 5}
    with pytest.raises(ValueError, match="one per row"):
        SC.score_reference(lg, [1, 2])
    with pytest.raises(ValueError, match="no id inside the vocabulary"):
        SC.score_reference(lg, [1, 2, 3, 4], allowed=[V, -3])


def test_ties_resolve_to_the_lowest_index():
    lg = np.zeros((3, 7), dtype=np.float32)
    lg[0, [2, 5]] = 4.0
    lg[1, [6, 1, 3]] = 1.5
    _, greedy = SC.score_reference(lg, [0, 0, 0])
    np.testing.assert_array_equal(greedy, [2, 1, 0])
    _, greedy = SC.score_reference(lg, [5, 3, 6], allowed=[3, 5, 6], temperature=0.7)
    np.testing.assert_array_equal(greedy, [5, 3, 3])
    logp, _ = SC.score_reference(lg[2:], [4])
    np.testing.assert_allclose(logp, [-np.log(7.0)], rtol=0, atol=1e-15)


def test_check_score_args_accepts_one_sequence_or_many():
    import torch

    seqs, S, single = SC.check_score_args([3, 1, 2], 4, 24)
    assert single and S == 4 and len(seqs) == 1 and seqs[0].dtype == np.int32 and seqs[0].tolist() == [3, 1, 2]
    seqs, S, single = SC.check_score_args([[3], np.array([1, 2], dtype=np.int64), torch.tensor([5, 6, 7])], 1, 24)
    assert not single and S == 1 and [s.tolist() for s in seqs] == [[3], [1, 2], [5, 6, 7]]
    seqs, _, single = SC.check_score_args(torch.arange(24, dtype=torch.int32), 8, 24)
    assert single and seqs[0].shape == (24,)
    seqs, _, single = SC.check_score_args(np.arange(6).reshape(2, 3), 8, 24)
    assert not single and len(seqs) == 2


@pytest.mark.parametrize("kwargs, match", [
    (dict(tokens=[1, 2], rows=4, cap=24, batch=2), r"batch 1.*got batch 2"),
    (dict(tokens=[1, 2], rows=0, cap=24), r"\[1, 8\].*got 0"),
    (dict(tokens=[1, 2], rows=9, cap=24), r"\[1, 8\].*got 9"),
    (dict(tokens=[1, 2], rows=2.0, cap=24), r"must be an integer, got 2\.0"),
    (dict(tokens=[1, 2], rows=True, cap=24), r"must be an integer, got True"),
    (dict(tokens=[], rows=4, cap=24), r"sequence 0 is empty \(length 0\)"),
    (dict(tokens=[[1], []], rows=4, cap=24), r"sequence 1 is empty \(length 0\)"),
    (dict(tokens=[1.0, 2.0], rows=4, cap=24), r"expected integer ids, got float64"),
    (dict(tokens=[[1, 2], np.array([True, False])], rows=4, cap=24), r"sequence 1: expected integer ids, got bool"),
    (dict(tokens=list(range(25)), rows=4, cap=24), r"length 25.*<= 24"),
])
def test_check_score_args_errors(kwargs, match):
    kw = dict(kwargs)
    with pytest.raises(ValueError, match=match):
        SC.check_score_args(kw.pop("tokens"), kw.pop("rows"), kw.pop("cap"), **kw)


@pytest.mark.parametrize("kwargs, match", [
    (dict(sampling=True), "score does not combine with sampling"),
    (dict(filtering=True), "score does not combine with filtering"),
    (dict(speculate=4), "score does not combine with speculate"),
    (dict(grammar=object()), "score does not combine with grammar"),
    (dict(jump_forward=4), "score does not combine with jump_forward"),
    (dict(beams=4), "score does not combine with beams"),
])
def test_score_context_exclusions(kwargs, match):
    with pytest.raises(ValueError, match=match):
        SC.check_score_ctx(4, 1, **kwargs)


def test_score_context_rows_and_batch():
    assert SC.check_score_ctx(1, 1) == 1 and SC.check_score_ctx(8, 1) == 8
    with pytest.raises(ValueError, match=r"\[1, 8\].*got 9"):
        SC.check_score_ctx(9, 1)
    with pytest.raises(ValueError, match="B = 1.*got B 2"):
        SC.check_score_ctx(4, 2)
