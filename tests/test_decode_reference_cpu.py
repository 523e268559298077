"""The element-wise criteria of tests/test_decode_reference_gpu.py against corrupted references (CPU, no kernel involved), and the
float32 summation-order measurement behind its caps on the share of differing elements.

What each corruption shows about the older kernel tests' criterion (Frobenius `rel < 1e-2` against the eager kernels, B = 1 and 3):
 * one feature of act zeroed: the norm passes, the element bound rejects it.
 * one generated key dropped from the attention sum: for a key of moderate softmax weight the norm passes and the 2^-7 A_d bound
   rejects it; a key of small weight passes both (that bound is about the rounding of p, not about membership) and is caught by
   the exact-count case, where every key weighs the same.
 * rows 6 and 7 of y swapped: the norm WOULD catch this at B = 8; the old gap was that no kernel test ran B > 3.  The element
   bound rejects it too.
 * the last odd vocabulary row ignored: the old tests had no criterion that could see it (even V only, and a head that skips the
   row in its partials still writes a correct debug logit); the token check against the float64 argmax rejects it."""
import pytest
import torch

from tests import decode_reference as C
from tests.common import rel
from tests.decode_reference import DH, check_elementwise


def test_criteria_accept_the_reference_itself():
    c = C.decode_case("res2048")
    r, bound = C.ref_residual(c["a"], c["wd"], c["res"])
    assert check_elementwise(r.to(torch.bfloat16), r, bound, 0.0) == (0.0, 0.0)
    r64 = C.ref_residual(c["a"], c["wd"], c["res"], rounded=False)
    assert bool(((r - r64).abs() <= C.ulp_bf16(r)).all())              # R16 is R64 rounded once
    assert C.ulp_bf16(torch.tensor([1.0, 1.99, 2.0, 0.0078125], dtype=torch.float64)).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -14]


def test_differing_counts_behind_the_share_caps():
    """Every row of the table in the GPU module's docstring, measured again on the committed inputs."""
    for (kind, fp8, N), want in C.DIFFERING.items():
        assert C.measure_differing(kind, fp8, N) == want, (kind, fp8, N)
    c = C.decode_case("res2048")
    r, bound = C.projection_reference("res2048", c)
    for o in C.F32_ORDERS:      # a float32 restatement stays inside the element bound
        assert C.worst_ratio(C.f32_projection("res2048", c, o), r, bound) <= 1.0


def test_settled_gamma_keeps_h_off_rounding_ties():
    for kind in ("qkv", "gate_up"):
        c = C.decode_case(kind)
        assert float(C.tie_distance(C.norm_rows64(c["x"], c["gamma"])).min()) >= C.TIE_MARGIN


def test_zeroed_act_feature_fails_the_element_bound():
    c = C.decode_case("gate_up")
    r, bound = C.ref_gate_up(c["h16"], c["wd"], DH)
    bad = r.clone()
    bad[:, 4321] = 0.0
    assert rel(bad, r) < 1e-2
    with pytest.raises(AssertionError):
        check_elementwise(bad, r, bound, C.share_cap("gate_up", False), "act, one feature zeroed")


def test_swapped_rows_fail_the_element_bound():
    c = C.decode_case("res16384")
    r, bound = C.ref_residual(c["a"], c["wd"], c["res"])
    bad = r.clone()
    bad[[6, 7]] = r[[7, 6]]
    print(f"rows 6 and 7 swapped: rel {rel(bad, r):.2f} (the norm sees it at B = 8; the old kernel tests stopped at B = 3)")
    with pytest.raises(AssertionError):
        check_elementwise(bad, r, bound, C.share_cap("res16384", False), "y, rows 6 and 7 swapped")


def test_dropped_generated_key_fails_the_attention_criteria():
    Pn, cap = C.ATTN_SHAPES[0]
    t = 17
    c = C.attn_case(Pn, cap, "peaked")
    args = (c["q"], c["pk"], c["pv"], c["allowed"], c["gk"], c["gv"], t)
    r, A = C.ref_attention(*args)
    rejected, low_weight = [], []
    for j in range(t):          # sample 0 loses generated key j
        bad, _ = C.ref_attention(*args, drop=(0, j))
        if rel(bad, r) >= 1e-2:
            continue            # (the norm sees this one)
        ratio = C.worst_ratio(bad, r, 2.0 ** -7 * A)
        print(f"generated key {j} dropped: rel {rel(bad, r):.2e}, worst error / bound {ratio:.2f}")
        if ratio > 1.0:
            rejected.append(j)
            with pytest.raises(AssertionError):
                check_elementwise(bad, r, 2.0 ** -7 * A, None, f"attention, generated key {j} dropped")
        else:
            low_weight.append(j)
    assert rejected and low_weight
    # the exact-count case rejects every one of them, the low-weight keys included
    c = C.attn_case(Pn, cap, "count")
    sm, n = C.count_reference(c, t)
    n = n.view(8, 1)
    keep = C.count_separated(sm, n)
    ref = C.bf16r(sm / n)
    assert int(keep[0].sum()) > 200
    for j in rejected + low_weight:
        bad = C.bf16r((sm[0] - c["gv"][0, j].double()) / (n[0] - 1))
        assert bool(((bad - ref[0]).abs() > C.ulp_bf16(ref[0]))[keep[0]].all())


def test_ignored_last_odd_row_fails_the_token_check():
    V = 20481
    c = C.lm_case(V, "hilo")
    ref = c["ref"].clone()
    ref[0, V - 1] = ref[0].max() + 0.05         # the last row wins sample 0, by 150 logit bounds
    assert C.check_tokens(C.first_argmax(ref), ref, c["bound"]) == 0
    bad_tokens = C.first_argmax(ref[:, :V - 1])         # a head whose partials never see the last row
    with pytest.raises(AssertionError):
        C.check_tokens(bad_tokens, ref, c["bound"], "last odd row ignored")
    assert C.lm_case(V, "hilo", dup=True)["dups"][-1] == V - 1          # the GPU module's duplicated best row sits there too
