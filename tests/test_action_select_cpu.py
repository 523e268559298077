"""The specification of best-of-N candidate selection (lap_amd/action_select.py; CPU): hand-computed scores, the tie rule, the
coherence weights at the ends of `executed`, and the argument errors."""
import pytest
import torch

from lap_amd import action_select as A


def test_medoid_scores_by_hand():
    # three chunks of S = 2, ad = 1: (0, 0), (1, 0), (3, 4) -> squared distances 1, 25, 20
    cand = torch.tensor([[[0.0], [0.0]], [[1.0], [0.0]], [[3.0], [4.0]]])
    s = A.medoid_scores(cand)
    assert s.dtype == torch.float64 and s.tolist() == [1.0 + 25.0, 1.0 + 20.0, 25.0 + 20.0]
    assert A.select(s) == 1
    assert A.medoid_scores(cand[:1]).tolist() == [0.0]


def test_coherence_scores_by_hand():
    cand = torch.tensor([[[1.0, 2.0], [3.0, 4.0]], [[0.0, 0.0], [1.0, 1.0]]])      # [2, 2, 2]
    known = torch.tensor([[1.0, 1.0], [1.0, 1.0]])
    w = torch.tensor([1.0, 0.5])
    s = A.coherence_scores(cand, known, w)
    assert s.tolist() == [1.0 * (0 + 1) + 0.5 * (4 + 9), 1.0 * (1 + 1) + 0.5 * 0]
    assert A.select(s) == 1
    assert torch.equal(A.coherence_scores(cand, known[None], w), s)      # known as [1, S, ad]
    assert A.coherence_scores(cand, known, torch.zeros(2)).tolist() == [0.0, 0.0]


def test_scores_are_float64_of_the_float32_inputs():
    g = torch.Generator().manual_seed(0)
    cand = torch.randn(4, 5, 3, generator=g)
    want = torch.stack([sum(((cand[n].double() - cand[m].double()) ** 2).sum() for m in range(4)) for n in range(4)])
    assert torch.allclose(A.medoid_scores(cand), want, rtol=1e-14, atol=0)


def test_ties_go_to_the_lowest_index():
    assert A.select(torch.tensor([2.0, 1.0, 1.0, 3.0])) == 1
    assert A.select(torch.tensor([0.5, 0.5])) == 0
    assert A.select(torch.tensor([7.0])) == 0
    same = torch.ones(3, 4, 2)
    assert A.select(A.medoid_scores(same)) == 0
    two = torch.stack([torch.zeros(4, 2), torch.ones(4, 2)])      # two candidates: the medoid scores always tie
    s = A.medoid_scores(two)
    assert s[0] == s[1] and A.select(s) == 0


@pytest.mark.parametrize("S", [1, 6])
def test_coherence_weights_at_the_ends_of_executed(S):
    for executed in sorted({0, 1, S - 1, S} & set(range(S + 1))):
        w = A.coherence_weights(S, executed, rho=0.5)
        assert w.dtype == torch.float32 and tuple(w.shape) == (S,)
        live = S - executed
        assert w[:live].tolist() == [0.5 ** s for s in range(live)] and w[live:].tolist() == [0.0] * executed
    assert A.coherence_weights(S, 0, rho=1.0).tolist() == [1.0] * S
    assert A.coherence_weights(S, S).tolist() == [0.0] * S      # nothing of the previous chunk is left: every candidate scores 0


def test_argument_errors():
    cand = torch.zeros(3, 4, 2)
    for bad in (torch.zeros(4, 2), torch.zeros(0, 4, 2), torch.zeros(1, 2, 3, 4)):
        with pytest.raises(ValueError, match="select"):
            A.medoid_scores(bad)
    for known, w in ((torch.zeros(3, 2), torch.zeros(4)), (torch.zeros(4, 2), torch.zeros(3)), (torch.zeros(2, 4, 2), torch.zeros(4)),
                     (torch.zeros(4, 2), torch.zeros(4, 1))):
        with pytest.raises(ValueError, match="select"):
            A.coherence_scores(cand, known, w)
    for S, ex, rho in ((4, -1, 0.5), (4, 5, 0.5), (0, 0, 0.5), (4, 1.0, 0.5), (4, True, 0.5), (4, 1, 0.0), (4, 1, 1.5)):
        with pytest.raises(ValueError, match="coherence_weights"):
            A.coherence_weights(S, ex, rho)
    for bad in (torch.zeros(2, 2), torch.zeros(0)):
        with pytest.raises(ValueError, match="select"):
            A.select(bad)


def test_check_select():
    known, w = torch.zeros(4, 2), torch.ones(4)
    assert A.check_select(None, None, 4, 2) == (None, None)
    assert A.check_select("medoid", None, 4, 2) == ("medoid", None)
    mode, (k, ww) = A.check_select("coherence", (known, w), 4, 2)
    assert mode == "coherence" and k is known and ww is w
    for sel, coh in (("best", None), ("coherence", None), ("coherence", (known,)), ("medoid", (known, w)), (None, (known, w)),
                     ("coherence", (known, w[:3])), ("coherence", (known[:3], w))):
        with pytest.raises(ValueError, match="select"):
            A.check_select(sel, coh, 4, 2)


def test_check_num_samples():
    from lap_amd.flow_sample import check_num_samples

    assert check_num_samples(None, 4, False) == 1 and check_num_samples(1, 4, False) == 1 and check_num_samples(8, 1, True) == 8
    for n, B, pi05 in ((0, 1, True), (9, 1, True), (2.0, 1, True), (True, 1, True), ("2", 1, True), (2, 2, True), (2, 1, False)):
        with pytest.raises(ValueError, match="num_samples"):
            check_num_samples(n, B, pi05)
