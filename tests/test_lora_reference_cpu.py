"""The element-wise criteria of tests/test_lora_reference_gpu.py on the CPU, no kernel involved: float32 restatements of each
kernel of csrc/lora.hip (two or three summation orders) must meet (a) the element bound and (b) the cap on the differing share on
every case, differing from the float64 reference in no larger a share than tests/lora_reference.py records; single-fault
corruptions of the restatements must fail (a) or (b) on the case named here; with every rounding switched off the references
are the plain formulas of the [UPSTREAM-RECALL] note of tests/test_lora_gpu.py, and the weight-gradient references their
gradients."""
import pytest
import torch

from tests import lora_reference as L
from tests.common import rel


@pytest.fixture(scope="module", autouse=True)
def _drop():
    yield
    L.drop_caches()


@pytest.mark.parametrize("family", list(L.CASES))
def test_float32_restatements_meet_both_criteria(family):
    fn, orders = L.F32[family]
    for spec in L.CASES[family]:
        c = L.make_case(spec)
        ref = L.REFS[family](c)
        for order in orders:
            for out, (ratio, share, cp) in L.judge(spec, fn(c, order), ref).items():
                tag = L.case_id(spec, out)
                print(f"float32 {order} {tag}: worst error / bound {ratio:.3f}" + ("" if cp is None else f", differing share {share:.2e} (cap {cp:.2e})"))
                assert ratio <= 1.0, (tag, order, ratio)
                if cp is not None:
                    assert share <= L.F32_SHARE.get(tag, 0.0), (tag, order, "share above the recorded one", share)
                    assert share <= cp < 1.0 / 64, (tag, order, share, cp)


def test_recorded_shares_name_cases_and_caps_stay_under_a_fragment_column():
    ids = {L.case_id(s, o) for cases in L.CASES.values() for s in cases for o in L.BF16_OUTPUTS}
    assert set(L.F32_SHARE) <= ids
    assert 4.0 * max(L.F32_SHARE.values()) < 1.0 / 64 and L.CAP_LIMIT < 1.0 / 64


def test_cases_cover_every_scale_and_copy_count():
    for family, cases in L.CASES.items():
        assert {c.s for c in cases} == set(L.S_VALUES), family
        assert {c.ncopy if family == "wgrad" else c.nsum for c in cases} >= {1, 8}, family
    assert [L.wgrad_split(100, m) for m in (1, 2, 3, 4)] == [(128, 1), (64, 2), (64, 2), (32, 4)]


# fault -> (family, the case that must fail (a) or (b))
CORRUPTIONS = {
    "drop_k8": ("down", L.Down(77, 72, 1, 48, s=0.75)),                              # the last 8 of K dropped
    "drop_copy": ("down", L.Down(33, 64, 1, 32, nsum=8)),                            # one of the nsum copies dropped
    "group0_cols": ("down", L.Down(45, 40, 3, 16, nsum=2, s=0.75, xg=40, px=8)),     # group 1 reads group 0's columns of X
    "t_unrounded": ("up_add", L.Up(17, 104, 5, 16, s=0.75)),                         # t not rounded before the up product
    "s_before_rounding": ("up_add", L.Up(70, 40, 3, 16, nsum=8, s=0.75, py=8, pb=8)),     # bf16(s acc) for bf16(s bf16(acc))
    "s1_shortcut": ("up_add", L.Up(17, 40, 3, 16, s=0.75)),                          # the s == 1 shortcut taken at s = 0.75
    "cd_rows": ("down", L.Down(77, 48, 1, 48)),                                      # C/D rows stored to 4 i + (lane >> 4)
    "drop_short_chunk": ("wgrad", L.Wgrad(100, 40, 1, 16, s=0.75, msplit=4)),        # the last, short M chunk (4 rows) dropped
    "copy0_only": ("wgrad", L.Wgrad(33, 40, 3, 16, ncopy=8, s=0.75, bg=40)),         # only copy 0 written
    "bs_unscaled": ("wgrad", L.Wgrad(31, 40, 1, 16, s=0.75)),                        # bs left unscaled
    "no_s": ("merge", L.Merge(1028, 3, 2, 5, nsum=8, s=0.75)),                       # merge: s omitted
    "w_after_rounding": ("merge", L.Merge(36, 8, 1, 16, s=2.0)),                     # merge: W added after the bf16 rounding
}
EXTRA = [("drop_copy", "up_add", L.Up(17, 8, 1, 16, nsum=8)), ("drop_copy", "merge", L.Merge(36, 3, 2, 5, nsum=8, s=2.0, pw=4, pa=4, pb=1, po=4)),
         ("s1_shortcut", "down", L.Down(77, 72, 1, 48, s=0.75)), ("s1_shortcut", "wgrad", L.Wgrad(31, 40, 1, 16, s=0.75))]


@pytest.mark.parametrize("fault,family,spec", [(f, fam, s) for f, (fam, s) in CORRUPTIONS.items()] + EXTRA,
                         ids=lambda v: v if isinstance(v, str) else L.case_id(v))
def test_single_fault_corruptions_fail(fault, family, spec):
    assert spec in L.CASES[family]
    fn, orders = L.F32[family]
    c = L.make_case(spec)
    ref = L.REFS[family](c)
    for order in orders:
        assert L.passes(L.judge(spec, fn(c, order), ref))
        res = L.judge(spec, fn(c, order, fault), ref)
        for out, (ratio, share, cp) in res.items():
            print(f"{fault} {order} {L.case_id(spec, out)}: worst error / bound {ratio:.2f}" + ("" if cp is None else f", differing share {share:.2e} (cap {cp:.2e})"))
        assert not L.passes(res), (fault, order, L.case_id(spec))


def test_references_reduce_to_the_plain_formulas():
    """rounded=False: down then up_add is y0 + s (x A^T) B with B summed over its copies, merge is W + s B^T A (so x Weff^T is the
    adapted projection), and the two weight-gradient references and the data-gradient form of down are the gradients of that."""
    g = L.gen("plain")
    M, K, R, Ng, nsum, s = 9, 24, 16, 8, 2, 0.75
    x, A = torch.randn(M, K, generator=g).bfloat16(), (0.05 * torch.randn(R, K, generator=g)).bfloat16()
    B, y0 = (0.05 * torch.randn(nsum * R, Ng, generator=g)).bfloat16(), torch.randn(M, Ng, generator=g).bfloat16()
    dy = torch.randn(M, Ng, generator=g).bfloat16()
    t = L.ref_down(dict(spec=L.Down(M, K, 1, R), x=x, w=A), rounded=False)
    y = L.ref_up_add(dict(spec=L.Up(M, Ng, 1, R, nsum=nsum, s=s), b=B, y0=y0), rounded=False, t=t)
    xd = x.double().requires_grad_(True)
    Ad, Bd = A.double().requires_grad_(True), B.double().requires_grad_(True)
    plain = y0.double() + s * (xd @ Ad.T) @ Bd.view(nsum, R, Ng).sum(0)
    assert rel(y, plain.detach()) < 1e-14
    (plain * dy.double()).sum().backward()
    dB = L.ref_wgrad(dict(spec=L.Wgrad(M, Ng, 1, R, ncopy=nsum, s=s), a=t, b=dy), rounded=False)
    assert rel(dB, Bd.grad) < 1e-14           # every copy of B gets the same gradient
    dt = L.ref_down(dict(spec=L.Down(M, Ng, 1, R, nsum=nsum, s=s), x=dy, w=B), rounded=False)
    dA = L.ref_wgrad(dict(spec=L.Wgrad(M, K, 1, R), a=dt, b=x), rounded=False)
    assert rel(dA, Ad.grad) < 1e-14
    dx = L.ref_up_add(dict(spec=L.Up(M, K, 1, R), b=A, y0=torch.zeros(M, K)), rounded=False, t=dt)
    assert rel(dx, xd.grad) < 1e-14
    # grouped: G = 2 groups of Ng columns, merge against the grouped down / up_add
    G = 2
    A2, B2 = 0.05 * torch.randn(G * R, K, generator=g), 0.05 * torch.randn(nsum * G * R, Ng, generator=g)
    W = 0.02 * torch.randn(G * Ng, K, generator=g)
    weff = L.ref_merge(dict(spec=L.Merge(K, Ng, G, R, nsum=nsum, s=s), w=W, a=A2, b=B2), rounded=False)
    t2 = L.ref_down(dict(spec=L.Down(M, K, 1, G * R), x=x, w=A2), rounded=False)
    y2 = L.ref_up_add(dict(spec=L.Up(M, Ng, G, R, nsum=nsum, s=s), b=B2, y0=x.double() @ W.double().T), rounded=False, t=t2)
    assert rel(x.double() @ weff.T, y2) < 1e-13
