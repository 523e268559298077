"""The training attention kernels (csrc/attention.hip, csrc/attention_dma.hpp) element by element against float64 (GPU).

The references, the derivation of every bound and the inputs are in tests/attention_reference.py; nothing there calls lap_amd.hip.
Each case runs hip.attention_fwd and checks o and lse, then runs hip.attention_bwd fed with the reference's own bf16(o64) and
float32(lse64), so that a backward fault cannot hide behind a forward one, and checks dq, dk, dv (the API does not expose delta).
One case per family chains the device's o / lse into the backward instead.  Every case asserts: each element within its bound;
every buffer of the case, which all live in one allocation between NaN guard rows and sentinels, bit for bit unchanged outside
the rows and columns an output owns; every output finite.

Families (hip.attention_set_variant): 0 = the generic padded-LDS kernels (HD 16 / 72 / 256), 1 = the LDS-DMA kernels (HD 72 /
256), 2 = as 1 with the backward's delta as a separate pass.  The DMA kernels run when dma_path_ok holds:
    variant != 0  and  max(ntk32, ntq32) * 144 <= 16384  and  ceil(ntk32 / nsplit) <= 64  and  ntq32 <= 64  and  scale > 0
with ntk32 / ntq32 the 32-row tiles of the key / query segments; so T = 2048 (64 tiles) is the last single-segment length they
take and T = 2080 (65) falls to the generic kernels under any variant.

Shapes are the smallest at which each mechanism exists: T around the 32- and 64-row tiles, 200 for several blocks with a ragged
last tile, the head arrangements that give the backward's head split 1, 2, 1 (three heads per key head) and 4; two segments
whose seam falls inside a joint 64-query block; the mask edges of attention_reference.infos; key splits with a masked and an
empty share; the fused q | k | v layout; 35 / 64 / 65 key tiles for bits >= 32 of the tile-decision masks."""
import pytest
import torch

from tests import attention_reference as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
FAMILIES = {16: (0,), 72: (0, 1), 256: (0, 1)}
WORST = {}          # (family, output) -> worst error / bound seen, printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def _drop_references():
    """The float64 references are computed once per shape and shared by the variants; drop them after the module."""
    yield
    for (variant, what), r in sorted(WORST.items()):        # docs/EXPERIMENTS.md quotes these
        print(f"family {variant} {what}: worst error / bound {r:.3f}")
    A.drop_caches()
    torch.cuda.empty_cache()


def _note(variant, what, ratio):
    WORST[variant, what] = max(WORST.get((variant, what), 0.0), ratio)


def _segments(arena, regions, name, spec, which):
    return [A.region_view(arena, regions[f"{name}{s}"]) if which[s] else None for s in range(2)]


def run_case(hip, spec, variant, stop=False, nsplit=1, chain=False, backward_variants=None, bwd_inputs=None):
    """Forward and backward of one case under `variant` against the float64 references; returns the device's outputs.  The
    key split is always given (the wrapper would otherwise choose one from the block count), so every launch is the one named.
    bwd_inputs = (o [B, Tq, NH, HD], lse float32 [B, NH, Tq]): what the backward is fed with instead of the forward reference's."""
    c = A.make_case(spec)
    B, NH, NKV, HD = spec.B, spec.NH, spec.NKV, spec.HD
    Tq = sum(spec.q_len)
    ref = A.reference(spec, stop, nsplit > 1)
    arena, regions = A.build_arena(c)
    dev = arena.to(DEV)
    qinfo = None if c["qinfo"] is None else c["qinfo"].to(DEV)
    kinfo = None if c["kinfo"] is None else c["kinfo"].to(DEV)
    hasq, hask = [n > 0 for n in spec.q_len], [n > 0 for n in spec.k_len]
    q, k, v = (_segments(dev, regions, n, spec, w) for n, w in (("q", hasq), ("k", hask), ("v", hask)))
    o, dO = _segments(dev, regions, "o", spec, hasq), _segments(dev, regions, "dO", spec, hasq)
    q_rs = tuple(regions[f"q{s}"].rs if hasq[s] and spec.layout == "fused" else 0 for s in range(2))
    kv_rs = tuple(regions[f"k{s}"].rs if hask[s] and spec.layout == "fused" else 0 for s in range(2))
    lse = A.lse_view(dev, regions, B, NH, Tq)
    sc = A.scale_of(spec)
    tag = f"{spec} variant {variant}"
    hip.attention_set_variant(variant)
    try:
        hip.attention_fwd(q, k, v, list(spec.q_len), list(spec.k_len), B, NH, NKV, HD, qinfo, kinfo, scale=sc, q_rs=q_rs, kv_rs=kv_rs,
                          nsplit_hint=nsplit, o_out=o, lse_out=lse)
        torch.cuda.synchronize()
        got = dev.cpu()
        assert A.untouched(arena, got, regions, ["o0", "o1", "lse"]), (tag, "forward wrote outside o / lse")
        o_dev, lse_dev = A.joint(got, regions, "o", spec), A.lse_view(got, regions, B, NH, Tq).double()
        assert bool(torch.isfinite(o_dev).all()) and bool(torch.isfinite(lse_dev).all()), (tag, "forward not finite")
        _note(variant, "o", A.check_elementwise(o_dev, ref["o16"], ref["o_bound"], None, f"{tag}: o")[0])
        assert bool((lse_dev[ref["empty"]] == A.LSE_EMPTY32).all()), (tag, "lse of a row with no allowed key")
        live = ~ref["empty"]
        if bool(live.any()):
            _note(variant, "lse", A.check_elementwise(lse_dev[live], ref["lse"][live], ref["lse_bound"][live], None, f"{tag}: lse")[0])
        if chain:       # the device's own o / lse feed the backward; its reference is recomputed from them
            W = A.stop_weight(Tq, sum(spec.k_len), spec.q_len[0], spec.k_len[0], stop)
            bref = A.bwd_reference(c["q"], c["k"], c["v"], c["allowed"], sc, o_dev, lse_dev.float(), c["dO"], W)
        else:
            o_in, lse_in = (ref["o16"], ref["lse32"]) if bwd_inputs is None else bwd_inputs
            for s in range(2):
                if hasq[s]:
                    lo = spec.q_len[0] * s
                    o[s].copy_(o_in[:, lo:lo + spec.q_len[s]].reshape(o[s].shape).to(torch.bfloat16))
            lse.copy_(lse_in)
            bref = ref
            if bwd_inputs is not None:
                W = A.stop_weight(Tq, sum(spec.k_len), spec.q_len[0], spec.k_len[0], stop)
                bref = A.bwd_reference(c["q"], c["k"], c["v"], c["allowed"], sc, o_in, lse_in, c["dO"], W)
        before = dev.cpu()
        outs = {}
        for bv in backward_variants or (variant,):
            hip.attention_set_variant(bv)
            dq, dk, dv = (_segments(dev, regions, n, spec, w) for n, w in (("dq", hasq), ("dk", hask), ("dv", hask)))
            hip.attention_bwd(q, k, v, o, dO, lse, list(spec.q_len), list(spec.k_len), B, NH, NKV, HD, qinfo, kinfo, stop_q1_to_k0=stop,
                              scale=sc, q_rs=q_rs, kv_rs=kv_rs, dq_out=dq, dk_out=dk, dv_out=dv)
            torch.cuda.synchronize()
            got = dev.cpu()
            assert A.untouched(before, got, regions, ["dq0", "dq1", "dk0", "dk1", "dv0", "dv1"]), (tag, bv, "backward wrote outside dq / dk / dv")
            for n in ("dq", "dk", "dv"):
                x = A.joint(got, regions, n, spec)
                assert bool(torch.isfinite(x).all()), (tag, bv, n, "not finite")
                _note(bv, n, A.check_elementwise(x, bref[n], bref[n + "_bound"], None, f"{tag} backward {bv}: {n}")[0])
                outs[n] = x
            for n in ("dq", "dk", "dv"):        # the sentinel again, so that the next variant has to write every element itself
                for s in range(2):
                    if f"{n}{s}" in regions:
                        A.region_view(dev, regions[f"{n}{s}"]).fill_(A.SENTINEL)
        return o_dev, lse_dev, outs
    finally:
        hip.attention_set_variant(-1)


def _bwd_variants(HD, variant):
    return (1, 2) if variant == 1 else (variant,)


def _ids(specs):
    return [f"HD{s.HD}-B{s.B}-NH{s.NH}-NKV{s.NKV}-q{s.q_len[0]}+{s.q_len[1]}-k{s.k_len[0]}+{s.k_len[1]}-{s.mask}" for s in specs]


def _with_families(specs):
    out = [(s, f) for s in specs for f in FAMILIES[s.HD]]
    return dict(argvalues=out, ids=[f"{i}-v{f}" for (s, f), i in zip(out, _ids([s for s, _ in out]))])


@pytest.mark.parametrize("spec,variant", **_with_families([s for HD in (16, 72, 256) for s in A.single_segment_specs(HD)]))
def test_single_segment_no_mask(hip, spec, variant):
    run_case(hip, spec, variant, backward_variants=_bwd_variants(spec.HD, variant))


@pytest.mark.parametrize("stop", [False, True])
@pytest.mark.parametrize("spec,variant", **_with_families([s for HD in (16, 72, 256) for s in A.two_segment_specs(HD)]))
def test_two_segments_lap_mask(hip, spec, variant, stop):
    run_case(hip, spec, variant, stop=stop, backward_variants=_bwd_variants(spec.HD, variant))


@pytest.mark.parametrize("stop", [False, True])
@pytest.mark.parametrize("spec,variant", **_with_families([A.edge_spec(HD) for HD in (16, 72, 256)]))
def test_mask_edges(hip, spec, variant, stop):
    """Causal boundary on the first key of a 32- and a 64-key tile, a whole masked tile (values ~1e3) between allowed ones, an
    all-allowed tile next to mixed ones, per-sample pads, a sample with no allowed key, index 0xFFFFFF, class bit 7."""
    _, lse, _ = run_case(hip, spec, variant, stop=stop, backward_variants=_bwd_variants(spec.HD, variant))
    assert bool((lse[2] == A.LSE_EMPTY32).all())


@pytest.mark.parametrize("spec,nsplit,variant", [(s, n, f) for HD in (16, 72, 256) for s, n in A.split_specs(HD) for f in FAMILIES[HD]],
                         ids=lambda x: str(x) if isinstance(x, int) else f"HD{x.HD}-k{x.k_len[0]}")
def test_forward_key_split(hip, spec, nsplit, variant):
    """nsplit_hint 1 / 2 / 3: a share that is masked whole, an empty share, more shares than key tiles; o and lse come from the
    combine kernel."""
    run_case(hip, spec, variant, nsplit=nsplit)


@pytest.mark.parametrize("spec,variant", **_with_families([A.fused_spec(HD) for HD in (72, 256)]))
def test_fused_qkv_layout(hip, spec, variant):
    """q | k | v are column slices of one buffer (8 NaN columns close each row); the gradients land in views of one buffer."""
    run_case(hip, spec, variant, backward_variants=_bwd_variants(spec.HD, variant))


@pytest.mark.parametrize("spec", A.MANY_TILES, ids=_ids(A.MANY_TILES))
def test_many_key_tiles(hip, spec):
    """35 / 64 / 65 tiles of 32 keys: bits >= 32 of the per-wave tile-decision masks and a second round of info staging.  2048 is
    the last length the DMA family takes; 2080 runs the generic kernels under the automatic choice."""
    T = spec.q_len[0]
    if T == 2080:
        run_case(hip, spec, -1)
    else:
        run_case(hip, spec, 1, backward_variants=(1, 2) if T == 1100 else (1,))
        if spec.mask == "run":
            run_case(hip, spec, 0)


@pytest.mark.parametrize("HD", [72, 256])
def test_variants_select_different_kernels(hip, HD):
    """Nothing reports which family a launch took, so a quiet fall-back of variant 1 to the generic kernels would pass every bound.
    The families walk the keys in tiles of 64 and of 32, so their bf16 roundings of P differ and with them some elements of o and dq:
    variants 0 and 1 must not agree bit for bit where dma_path_ok holds (T = 200), and must where it does not (T = 2080, HD 256)."""
    spec = A.Spec(HD, 3, 8, 1, (200, 0), (200, 0))
    o0, _, g0 = run_case(hip, spec, 0)
    o1, _, g1 = run_case(hip, spec, 1)
    assert not torch.equal(o0, o1) and not torch.equal(g0["dq"], g1["dq"])
    if HD == 256:
        spec = A.MANY_TILES[-1]
        o0, _, g0 = run_case(hip, spec, 0)
        o1, _, g1 = run_case(hip, spec, 1)
        assert torch.equal(o0, o1) and all(torch.equal(g0[n], g1[n]) for n in ("dq", "dk", "dv"))


@pytest.mark.parametrize("spec,variant", **_with_families([A.scale_spec(HD) for HD in (16, 72, 256)]))
def test_scale_on_unscaled_q(hip, spec, variant):
    """scale = HD^-0.5 on unscaled q (every other case but the fused layout runs the default 1.0 on pre-scaled q)."""
    run_case(hip, spec, variant, backward_variants=_bwd_variants(spec.HD, variant))


@pytest.mark.parametrize("HD,variant", [(72, 0), (72, 1), (256, 0), (256, 1)])
def test_backward_chained_to_device_forward(hip, HD, variant):
    run_case(hip, A.two_segment_specs(HD)[1], variant, stop=True, chain=True)


@pytest.mark.parametrize("HD,variant", [(HD, f) for HD in (16, 72, 256) for f in FAMILIES[HD]])
def test_exact_count_forward(hip, HD, variant):
    """q = 0, v = +-1: o is the mean of the allowed keys' signs, asserted exactly wherever one key more or fewer would show
    (count_separated; the other elements keep the general bound, which run_case asserts); lse = log(n) to 2^-22 relative.  Once in
    one launch and once through the key split's combine kernel."""
    for spec, nsplit in [(s, n) for s in A.count_specs(HD)[0] for n in (1, 2)]:
        o, lse, _ = run_case(hip, spec, variant, nsplit=nsplit)
        sm, n = A.count_forward(A.make_case(spec))
        live = (n > 0).expand_as(sm)
        want = A.bf16r(sm / n.clamp(min=1.0))
        keep = A.count_separated(sm, n.clamp(min=1.0)) & live
        assert bool((o[keep] == want[keep]).all()), (spec, "exact count")
        assert bool((o[~live] == 0).all()), (spec, "rows with no allowed key")
        nn = n[..., 0, 0][:, None, :].expand_as(lse)
        ok = nn > 0
        assert bool(((lse - torch.log(nn.clamp(min=1.0))).abs()[ok] <= 2.0 ** -22 * torch.log(nn.clamp(min=2.0))[ok]).all()), (spec, "lse")


@pytest.mark.parametrize("HD,variant", [(HD, f) for HD in (16, 72, 256) for f in FAMILIES[HD] + ((2,) if HD != 16 else ())])
def test_exact_count_backward(hip, HD, variant):
    """q = 0, dO = +-1, o passed in as zeros (delta = 0), lse = float32(log n).  Power-of-two counts: P is exact in bf16 and every
    element of dV an exactly representable sum, asserted for equality; dK is exactly 0 (q = 0).  Other counts: one bf16 spacing.
    Through run_case, so dq, dk and dv also meet their bounds from bwd_reference on these inputs, between guards and sentinels."""
    for spec in A.count_specs(HD)[1]:
        c = A.make_case(spec)
        want, lse32, exact = A.count_backward_dv(c)
        assert exact == (spec.mask == "pow2")
        _, _, g = run_case(hip, spec, min(variant, 1), bwd_inputs=(torch.zeros_like(c["q"], dtype=torch.float64), lse32), backward_variants=(variant,))
        if exact:
            assert bool((g["dv"] == want).all()), (spec, variant, "dV, exact")
        else:
            assert bool(((g["dv"] - want).abs() <= A.ulp_bf16(want)).all()), (spec, variant, "dV, one spacing")
        assert bool((g["dk"] == 0).all()), (spec, variant, "dK")
