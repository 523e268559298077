"""The element-wise criteria of tests/test_attention_reference_gpu.py on the CPU, no kernel involved: float32 restatements of the
kernels' algorithm in three tile orders must meet every bound on every case; corrupted references must fail them; the exact-count
references must be exact.

Each corruption is also put to the older criterion of tests/test_kernels_gpu.py (one Frobenius ratio per tensor: < 1e-2 forward,
< 2e-2 backward) and the verdict printed next to the new one (docs/EXPERIMENTS.md holds the table)."""
import pytest
import torch

from tests import attention_reference as A
from tests.attention_reference import Spec
from tests.common import rel

OLD = {"o": 1e-2, "dq": 2e-2, "dk": 2e-2, "dv": 2e-2}        # test_kernels_gpu.py's thresholds
H8 = Spec(256, 2, 8, 1, (200, 0), (200, 0))                  # eight query heads on one key head, a ragged last tile of 8 keys
TWO = Spec(72, 2, 4, 2, (97, 50), (97, 50), "lap")


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    yield
    A.drop_caches()


def _stop_w(spec, stop):
    return A.stop_weight(sum(spec.q_len), sum(spec.k_len), spec.q_len[0], spec.k_len[0], stop)


def _verdict(what, bad, ref, bound, name):
    """Prints and returns (old norm passes, new criterion rejects) for a corrupted tensor."""
    r, ratio = rel(bad, ref), A.worst_ratio(bad, ref, bound)
    print(f"{what}: {name} rel {r:.2e} (old threshold {OLD[name]:.0e}: {'passes' if r < OLD[name] else 'fails'}), worst error / bound {ratio:.1f}")
    return r < OLD[name], ratio > 1.0


def test_float32_restatements_meet_every_bound():
    """Online softmax with bf16 P and the backward's rounding points in float32, in 64-key tiles, 32-key tiles and 64-key tiles
    with the key share split in two and combined: worst error / bound <= 1 for o, lse, dq, dk, dv on every rand case of the GPU
    module, with and without stop_q1_to_k0 where there are two segments.  The worst relative error of the float32 exponential
    seen on the way is what attention_reference.F32_EXP_ERR (and so INTR) stands on."""
    worst = {}
    for spec in A.all_random_specs():
        c = A.make_case(spec)
        sc = A.scale_of(spec)
        for stop in (False, True) if spec.q_len[1] and spec.q_len[0] else (False,):
            W = _stop_w(spec, stop)
            for order in A.F32_ORDERS:
                ref = A.reference(spec, stop, order == "split2")
                o, lse = A.f32_forward(c["q"], c["k"], c["v"], c["allowed"], sc, order)
                got = {"o": (o, ref["o16"], ref["o_bound"])}
                live = ~ref["empty"]
                assert bool((lse[ref["empty"]] == A.LSE_EMPTY).all())
                got["lse"] = (lse.double()[live], ref["lse"][live], ref["lse_bound"][live])
                dq, dk, dv = A.f32_backward(c["q"], c["k"], c["v"], c["allowed"], sc, ref["o16"], ref["lse32"], c["dO"], order, W)
                got.update(dq=(dq, ref["dq"], ref["dq_bound"]), dk=(dk, ref["dk"], ref["dk_bound"]), dv=(dv, ref["dv"], ref["dv_bound"]))
                for n, (x, r, b) in got.items():
                    ratio = A.worst_ratio(x, r, b) if x.numel() else 0.0
                    assert ratio <= 1.0, (spec, stop, order, n, ratio)
                    worst[order, n] = max(worst.get((order, n), 0.0), ratio)
        if sum(spec.q_len) > 1000:
            A._REFS.clear()
    for (order, n), r in sorted(worst.items()):
        print(f"float32 {order} {n}: worst error / bound {r:.3f}")
    print(f"float32 exp: worst relative error {A.exp_error_seen():.3e} (F32_EXP_ERR {A.F32_EXP_ERR:.3e}, INTR {A.INTR:.3e})")
    assert 0 < A.exp_error_seen() <= A.F32_EXP_ERR
    assert A.INTR <= 2.0 ** -18


def test_reference_agrees_with_autograd():
    """The float64 backward reference is the gradient of the float64 forward (torch autograd) up to its three bf16 rounding points
    (P, dS, the result; 2^-9 relative each): a check of the reference itself, so a norm is the right instrument here."""
    spec = TWO
    c = A.make_case(spec)
    q, k, v = (c[n].double().requires_grad_(True) for n in ("q", "k", "v"))
    kk, vv = A._heads(k, spec.NH), A._heads(v, spec.NH)
    s = torch.einsum("bihd,bjhd->bhij", q, kk).masked_fill(~c["allowed"][:, None], float("-inf"))
    p = torch.nan_to_num(torch.softmax(s, -1), nan=0.0)
    o = torch.einsum("bhij,bjhd->bihd", p, vv)
    (o * c["dO"].double()).sum().backward()
    ref = A.reference(spec)
    assert A.worst_ratio(o.detach(), ref["o16"], ref["o_bound"]) <= 1.0
    for n, g in (("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        print(f"{n}: reference against autograd, rel {rel(ref[n], g):.2e}")
        assert rel(ref[n], g) < 3 * 2.0 ** -9, n


def _drop_key(spec, pick):
    """Forward and backward references of `spec` with one (sample 0, query i, key j) pair taken out of `allowed`; pick(p) ->
    (i, j) from sample 0's probabilities, the largest over the heads (the mask is shared by the heads)."""
    c = A.make_case(spec)
    sc = A.scale_of(spec)
    f = A.fwd_reference(c["q"], c["k"], c["v"], c["allowed"], sc)
    i, j = pick(f["p"][0].amax(0))
    allowed = c["allowed"].clone() if c["allowed"] is not None else torch.ones(spec.B, sum(spec.q_len), sum(spec.k_len), dtype=torch.bool)
    assert bool(allowed[0, i, j])
    allowed[0, i, j] = False
    bad = A.fwd_reference(c["q"], c["k"], c["v"], allowed, sc)
    return f, bad, float(f["p"][0, :, i, j].max()), (i, j)


def test_dropped_key_of_moderate_weight_fails_the_forward_bound():
    def pick(p):
        d = (p - 0.03).abs()
        return divmod(int(d.argmin()), p.shape[1])

    f, bad, weight, ij = _drop_key(H8, pick)
    old, new = _verdict(f"key {ij[1]} (weight {weight:.3f}) dropped for query {ij[0]}", bad["o16"], f["o16"], f["o_bound"], "o")
    assert old and new


def test_strict_causal_comparison_at_a_tile_boundary_fails():
    """idx(k) < idx(q) instead of <= for the query at 160, whose own key is the first of a 32-key tile (edges mask)."""
    spec = A.edge_spec(72)
    f, bad, weight, _ = _drop_key(spec, lambda p: (160, 160))
    old, new = _verdict(f"idx(k) < idx(q) for query 160 (weight {weight:.3f})", bad["o16"], f["o16"], f["o_bound"], "o")
    assert old and new
    lse_ratio = A.worst_ratio(bad["lse"], f["lse"], f["lse_bound"].clamp(min=1e-300))
    print(f"  lse: worst error / bound {lse_ratio:.1f} (the old tests do not check lse)")
    assert lse_ratio > 1.0


def test_zeroed_ragged_rows_of_dk_fail():
    ref = A.reference(H8)
    bad = ref["dk"].clone()
    bad[:, 192:] = 0.0           # the last T % 64 = 8 keys
    old, new = _verdict("last 8 rows of dK zeroed", bad, ref["dk"], ref["dk_bound"], "dk")
    assert new
    print(f"  (old norm {'passes' if old else 'fails'} it at T = 200; 8 of 200 rows carry 4 % of the norm)")


def test_missing_head_in_one_key_tile_fails():
    """Query head 5 of 8 missing from dK / dV of keys [64, 128): one head-split partial of one 64-key tile."""
    spec = H8
    c, ref = A.make_case(spec), A.reference(spec)
    W = torch.ones(1, 8, 200, 200, dtype=torch.float64)
    W[:, 5, :, 64:128] = 0.0
    bad = A.bwd_reference(c["q"], c["k"], c["v"], c["allowed"], A.scale_of(spec), ref["o16"], ref["lse32"], c["dO"], W)
    for n in ("dk", "dv"):
        old, new = _verdict("head 5 missing from keys 64..127", bad[n], ref[n], ref[n + "_bound"], n)
        assert new


def test_ignored_stop_for_one_key_tile_fails():
    spec = TWO
    c, ref = A.make_case(spec), A.reference(spec, stop=True)
    W = _stop_w(spec, True)
    W[spec.q_len[0]:, :64] = 1.0            # the first key tile of segment 0 (image / prompt keys) takes the action queries' gradient after all
    bad = A.bwd_reference(c["q"], c["k"], c["v"], c["allowed"], A.scale_of(spec), ref["o16"], ref["lse32"], c["dO"], W)
    for n in ("dk", "dv"):
        old, new = _verdict("stop_q1_to_k0 ignored for keys 0..63", bad[n], ref[n], ref[n + "_bound"], n)
        assert new


def test_swapped_lse_rows_fail():
    spec = H8
    c, ref = A.make_case(spec), A.reference(spec)
    bad = ref["lse"].clone()
    bad[0, 0, [10, 11]] = ref["lse"][0, 0, [11, 10]]
    ratio = A.worst_ratio(bad, ref["lse"], ref["lse_bound"])
    print(f"lse of rows 10 and 11 swapped: worst error / bound {ratio:.1f} (the old tests have no lse criterion in this layout)")
    assert ratio > 1.0
    # and what a backward fed with it computes fails the dq bound
    b = A.bwd_reference(c["q"], c["k"], c["v"], c["allowed"], A.scale_of(spec), ref["o16"], bad.float(), c["dO"])
    old, new = _verdict("backward on the swapped lse", b["dq"], ref["dq"], ref["dq_bound"], "dq")
    assert new


def test_delta_of_the_neighbouring_head_fails():
    spec = H8
    c, ref = A.make_case(spec), A.reference(spec)
    delta = torch.einsum("bihd,bihd->bhi", c["dO"].double(), ref["o16"])
    delta[:, 3] = delta[:, 4]
    bad = A.bwd_reference(c["q"], c["k"], c["v"], c["allowed"], A.scale_of(spec), ref["o16"], ref["lse32"], c["dO"], delta=delta)
    for n in ("dq", "dk"):
        old, new = _verdict("delta of head 3 taken from head 4", bad[n], ref[n], ref[n + "_bound"], n)
        assert new


def test_dropped_low_weight_key_is_caught_by_the_exact_count_case():
    """A key of softmax weight ~1e-4 dropped for one query passes the old norm AND the rand-case element bound (that bound is about
    the rounding of p, not about membership).  In the exact-count case every allowed key weighs the same, and count_separated keeps
    the elements at which one key more or fewer moves bf16(mean): there it is caught."""
    def pick(p):
        d = (p.masked_fill(p <= 0, 1.0) - 1e-4).abs()
        return divmod(int(d.argmin()), p.shape[1])

    f, bad, weight, _ = _drop_key(H8, pick)
    old, new = _verdict(f"key of weight {weight:.1e} dropped", bad["o16"], f["o16"], f["o_bound"], "o")
    assert old and not new
    for spec in A.count_specs(72)[0]:
        c = A.make_case(spec)
        sm, n = A.count_forward(c)
        keep = A.count_separated(sm, n.clamp(min=1.0)) & (n > 0)
        want = A.bf16r(sm / n.clamp(min=1.0))
        b, i = 0, 3
        j = int((torch.ones(sum(spec.k_len)) if c["allowed"] is None else c["allowed"][b, i].float()).argmax())
        lost = A.bf16r((sm[b, i] - A._heads(c["v"].double(), spec.NH)[b, j]) / (n[b, i] - 1).clamp(min=1.0))
        moved = (lost != want[b, i]) & keep[b, i]
        print(f"{spec.mask}: key {j} dropped for query {i}: {int(moved.sum())} of {int(keep[b, i].sum())} kept elements differ")
        assert int(n[b, i]) > 1 and bool(moved[keep[b, i]].all()) and int(keep[b, i].sum()) > 0


def test_exact_count_references_are_exact():
    """The float64 count references against the general float64 reference (its rounding of o is the only difference), the share of
    elements count_separated keeps (at least 85 %), and the power-of-two backward case: every P a power of two, every dV a number
    bf16 holds or a float32-exact sum rounded once."""
    for HD in (16, 72, 256):
        fwd, bwd = A.count_specs(HD)
        for spec in fwd:
            c = A.make_case(spec)
            sm, n = A.count_forward(c)
            live = (n > 0).expand_as(sm)
            want = A.bf16r(sm / n.clamp(min=1.0))
            ref = A.reference(spec)
            some = live & (sm != 0)          # (a zero sum leaves ~1e-17 of float64 cancellation in the general reference)
            assert torch.equal(ref["o16"][some], want[some]) and bool((ref["o"][~some].abs() < 2.0 ** -50).all())
            keep = A.count_separated(sm, n.clamp(min=1.0)) & live
            share = float(keep[live].double().mean())
            print(f"HD {HD} {spec.mask}: count_separated keeps {share:.3f} of the elements")
            assert share >= 0.85
            lse = ref["lse"][~ref["empty"]]
            nn = n[..., 0, 0][:, None, :].expand_as(ref["lse"])[~ref["empty"]]
            assert bool(((lse - torch.log(nn)).abs() <= 2.0 ** -40).all())
        for spec in bwd:
            c = A.make_case(spec)
            want, lse32, exact = A.count_backward_dv(c)
            assert exact == (spec.mask == "pow2")
            b = A.bwd_reference(c["q"], c["k"], c["v"], c["allowed"], 1.0, torch.zeros_like(c["q"]), lse32, c["dO"])
            assert torch.equal(b["dv"], want) and bool((b["dk"] == 0).all())
            if exact:
                P = b["P"][b["P"] > 0]
                assert bool((torch.log2(A.bf16r(P)) % 1 == 0).all())
                # every partial sum is a multiple of 2^-7 (150 keys: counts up to 128) below 2^9: float32 adds them exactly
                assert float(A.bf16r(P).min()) >= 2.0 ** -7 and float(b["sens_dv"].max()) < 512.0
