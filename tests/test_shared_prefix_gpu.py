"""Best-of-N action chunks from one prefill (GPU): the shared-prefix few-query attention (`hip.attention_serve_shared`,
csrc/attention_serve_shared.hpp), the device-side candidate selection (`hip.action_select`) and the sampler, graph and policy
surfaces on top of them (`sample_actions(num_samples=N, select=...)`, `GraphedSampler`, `Policy`).

Kernel: bit equality with `hip.attention_fwd` on the prefix cache replicated N times is the acceptance criterion (same key runs,
same per-run arithmetic, same combine); one shape is also held to the float64 reference of the serving attention
(attention_reference.fwd_reference(split=True).o_bound, the bound tests/test_serve_reference_gpu.py applies).
Select: the f32 scores against the float64 specification to (S * ad + 2) 2^-24 relative — the worst case of an f32 sum of that
many non-negative terms; the kernel's sums are shorter (a thread's serial share plus a tree of 8) — and the index wherever the
float64 gap between the best and the runner-up exceeds twice that.
Model: the 2-layer full-width config of the inpainting tests, 3 Euler steps."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import lap_oracle as O
from lap_amd import action_select as A
from tests import serve_reference as SR
from tests.common import make_inputs, oracle_cfg, rel, to_observation
from tests.serve_reference import check_elementwise, region_view, untouched
from tests.test_model_parity_gpu import FREE_RUN_RATIO, _full_width_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 3
HD, NH, NKV = 256, 8, 1
SCALE = HD ** -0.5
PNS = (48, 200, 560)
SNS = ((10, 3), (16, 4), (50, 2), (50, 8))
_CASES = {}


# ------------------------------------------------------------------------------------------------------ the attention kernel
def attn_case(Pn, S, N):
    """Seeded inputs of N candidates (cached): q [N, S, NH, HD], fresh k / v [N, S, NKV, HD], ONE prefix k / v [Pn, NKV, HD], and
    the info words of serve_reference.attn_infos for a batch of 1 replicated N times: a hole at key 3 and a masked padding tail
    of 5 keys at the end of the prefix, whose k / v hold garbage."""
    key = (Pn, S, N)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * Pn + 10 * S + N)
        qinfo, kinfo = SR.attn_infos((1, NH, NKV, Pn, S, S), -1)
        q = torch.randn(N, S, NH, HD, generator=g) * (1.0 + torch.arange(S) % 3).view(1, S, 1, 1)
        kp, vp = torch.randn(Pn, NKV, HD, generator=g), torch.randn(Pn, NKV, HD, generator=g)
        dead = ((kinfo[0, :Pn] >> 24) == 0)[:, None, None]
        big = torch.randn(Pn, NKV, HD, generator=g) * SR.GARBAGE
        kp, vp = torch.where(dead, big, kp), torch.where(dead, -big, vp)
        kf, vf = torch.randn(N, S, NKV, HD, generator=g), torch.randn(N, S, NKV, HD, generator=g)
        bf = lambda t: t.to(torch.bfloat16)
        _CASES[key] = dict(q=bf(q), kp=bf(kp), vp=bf(vp), kf=bf(kf), vf=bf(vf), qinfo=qinfo.repeat(N, 1).contiguous(), kinfo=kinfo.repeat(N, 1).contiguous())
    return _CASES[key]


def run_shared(hip, c, Pn, S, N, o_out=None, form=None, **over):
    d = {k: v.to(DEV) for k, v in (c | over).items()}
    return hip.attention_serve_shared(d["q"].view(N * S, NH * HD), d["kf"].view(N * S, NKV * HD), d["vf"].view(N * S, NKV * HD),
                                      d["kp"].view(Pn, NKV * HD), d["vp"].view(Pn, NKV * HD), N, S, Pn, NH, NKV, HD,
                                      d["qinfo"], d["kinfo"], scale=SCALE, o_out=o_out, form=form)


def run_replicated(hip, c, Pn, S, N):
    d = {k: v.to(DEV) for k, v in c.items()}
    rep = lambda t: t.view(Pn, NKV * HD).repeat(N, 1)
    o, lse = hip.attention_fwd([None, d["q"].view(N * S, NH * HD)], [rep(d["kp"]), d["kf"].view(N * S, NKV * HD)],
                               [rep(d["vp"]), d["vf"].view(N * S, NKV * HD)], (0, S), (Pn, S), N, NH, NKV, HD,
                               qinfo=d["qinfo"], kinfo=d["kinfo"], need_lse=False, scale=SCALE)
    assert lse is None      # the serving kernel ran, not the generic one
    return o[1]


@pytest.mark.parametrize("Pn", PNS)
@pytest.mark.parametrize("S,N", SNS)
def test_shared_attention_is_bit_equal_to_the_replicated_cache(hip, Pn, S, N):
    assert hip._SERVE_ATTN and 0 < hip._fn["lap_attention_serve_splits"](Pn, S, N, NH, S) <= 16
    c = attn_case(Pn, S, N)
    want = run_replicated(hip, c, Pn, S, N)
    got = run_shared(hip, c, Pn, S, N)
    assert bool(torch.isfinite(got.float()).all())
    assert torch.equal(got, want), "resident-image form"
    assert torch.equal(run_shared(hip, c, Pn, S, N, form=1), want), "one unit per block"


def test_shared_attention_against_float64(hip):
    Pn, (S, N) = 200, (50, 2)
    c = attn_case(Pn, S, N)
    o = run_shared(hip, c, Pn, S, N).cpu().double().view(N, S, NH, HD)
    k = torch.cat([c["kp"][None].expand(N, -1, -1, -1), c["kf"]], 1)
    v = torch.cat([c["vp"][None].expand(N, -1, -1, -1), c["vf"]], 1)
    ref = SR.fwd_reference(c["q"], k, v, SR.mask_ok(c["qinfo"], c["kinfo"]), SCALE, split=True)
    assert not bool(ref["empty"].any())
    check_elementwise(o, ref["o16"], ref["o_bound"], None, f"shared attention Pn {Pn} S {S} N {N}")


def test_rows_beyond_the_candidates_stay_untouched(hip):
    Pn, (S, N) = 200, (10, 3)
    c = attn_case(Pn, S, N)
    arena, regs = SR.build_arena([("o", N * S, NH * HD, NH * HD)])
    ar = arena.to(DEV)
    got = run_shared(hip, c, Pn, S, N, o_out=region_view(ar, regs["o"]))
    torch.cuda.synchronize()
    after = ar.cpu()
    assert untouched(arena, after, regs, ("o",)), "bytes around o changed"
    assert torch.equal(region_view(after, regs["o"]), run_replicated(hip, c, Pn, S, N).cpu()) and got.data_ptr() == region_view(ar, regs["o"]).data_ptr()


def test_shared_attention_argument_errors(hip):
    Pn, (S, N) = 48, (10, 3)
    c = attn_case(Pn, S, N)
    d = {k: v.to(DEV) for k, v in c.items()}
    q, kf, vf = d["q"].view(N * S, NH * HD), d["kf"].view(N * S, HD), d["vf"].view(N * S, HD)
    kp, vp = d["kp"].view(Pn, HD), d["vp"].view(Pn, HD)
    call = lambda *a, **kw: hip.attention_serve_shared(*a, **({"qinfo": d["qinfo"], "kinfo": d["kinfo"], "scale": SCALE} | kw))
    call(q, kf, vf, kp, vp, N, S, Pn, NH, NKV, HD)
    for args, kw in (((q, kf, vf, kp, vp, 9, S, Pn, NH, NKV, HD), {}), ((q, kf, vf, kp, vp, 0, S, Pn, NH, NKV, HD), {}),
                     ((q, kf, vf, kp, vp, N, 65, Pn, NH, NKV, HD), {}), ((q, kf, vf, kp, vp, N, S, Pn, NH, NKV, 128), {}),
                     ((q[:-1], kf, vf, kp, vp, N, S, Pn, NH, NKV, HD), {}), ((q, kf, vf, kp[:-1], vp, N, S, Pn, NH, NKV, HD), {}),
                     ((q, kf, vf, kp.repeat(N, 1), vp.repeat(N, 1), N, S, Pn, NH, NKV, HD), {}),      # a replicated cache is not the shared one
                     ((q, kf, None, kp, vp, N, S, Pn, NH, NKV, HD), {}), ((q, kf, vf, kp, vp, N, S, Pn, NH, NKV, HD), {"kinfo": None}),
                     ((q, kf, vf, kp, vp, N, S, Pn, NH, NKV, HD), {"scale": 0.0}), ((q, kf, vf, kp, vp, N, S, Pn, NH, 3, HD), {})):
        with pytest.raises(ValueError, match="attention_serve_shared"):
            call(*args, **kw)
    # the C entry point itself: null pointers, N out of range, S > 64, a wrong run cap
    def raw(**over):
        a = hip.AttnFwdArgs()
        scratch = torch.empty(16 * 8 * 64 * NH * (HD + 1), dtype=torch.float32, device=DEV)
        o = torch.empty_like(q)
        f = dict(q1=q.data_ptr(), o1=o.data_ptr(), k0=kp.data_ptr(), v0=vp.data_ptr(), k1=kf.data_ptr(), v1=vf.data_ptr(), S=S, Pn=Pn, N=N,
                 ns=hip._fn["lap_attention_serve_splits"](Pn, S, N, NH, S), form=0) | over
        a.q[1], a.o[1], a.k[0], a.v[0], a.k[1], a.v[1] = f["q1"], f["o1"], f["k0"], f["v0"], f["k1"], f["v1"]
        a.q_len[1], a.k_len[0], a.k_len[1] = f["S"], f["Pn"], f["S"]
        a.scale, a.nsplit, a.scratch, a.scratch_floats = SCALE, f["ns"], scratch.data_ptr(), scratch.numel()
        a.B, a.NH, a.NKV, a.HD = f["N"], NH, NKV, HD
        import ctypes
        return hip._fn["lap_attention_serve_shared"](ctypes.byref(a), f["form"], hip._stream())
    assert raw() == 0
    for over in (dict(q1=None), dict(o1=None), dict(k0=None), dict(v1=None), dict(N=9), dict(N=0), dict(S=65), dict(Pn=0), dict(ns=1), dict(form=2)):
        assert raw(**over) == 1001, over
    torch.cuda.synchronize()


def test_a_candidates_fresh_keys_reach_that_candidate_only(hip):
    Pn, (S, N) = 200, (16, 4)
    c = attn_case(Pn, S, N)
    base = run_shared(hip, c, Pn, S, N).view(N, S, NH * HD)
    kf = c["kf"].clone()
    kf[1] = -kf[1]
    moved = run_shared(hip, c, Pn, S, N, kf=kf).view(N, S, NH * HD)
    for n in (0, 2, 3):
        assert torch.equal(moved[n], base[n]), n
    assert not torch.equal(moved[1], base[1])


# --------------------------------------------------------------------------------------------------------- candidate selection
def select_case(N, S, ad, seed=0):
    """Candidates around a known trajectory; candidate N // 2 is `known` plus small noise, the others are far: the coherence winner
    and (being the closest to the cluster centre) the medoid winner are decided by margins far above the f32 error."""
    g = torch.Generator().manual_seed(seed + 100 * N + S)
    known = torch.randn(S, ad, generator=g)
    cand = known[None] + torch.randn(N, S, ad, generator=g) * torch.linspace(1.0, 2.0, N).view(N, 1, 1)
    cand[N // 2] = known + 1e-2 * torch.randn(S, ad, generator=g)
    weights = A.coherence_weights(S, 2, 0.9)
    return cand.contiguous(), known, weights


@pytest.mark.parametrize("mode", ["medoid", "coherence"])
@pytest.mark.parametrize("N,S,ad", [(2, 10, 7), (8, 50, 32)])
def test_select_scores_index_and_best(hip, N, S, ad, mode):
    cand, known, weights = select_case(N, S, ad)
    want = A.medoid_scores(cand) if mode == "medoid" else A.coherence_scores(cand, known, weights)
    extra = () if mode == "medoid" else (known.to(DEV), weights.to(DEV))
    scores, index, best = hip.action_select(cand.to(DEV), mode, *extra)
    assert scores.dtype == torch.float32 and index.dtype == torch.int32 and tuple(best.shape) == (S, ad)
    bound = (S * ad + 2) * 2.0 ** -24
    err = ((scores.cpu().double() - want).abs() / want).max().item()
    print(f"select {mode} N {N} S {S} ad {ad}: worst relative score error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    i = int(index.item())
    assert torch.equal(best.cpu(), cand[i]), "best is a bit copy of cand[index]"
    order = torch.argsort(want)
    gap = ((want[order[1]] - want[order[0]]) / want[order[1]]).item()
    if mode == "medoid" and N == 2:      # two candidates always tie (both scores are the one distance): the lowest index, in f32 too
        assert scores[0] == scores[1] and i == 0 == A.select(scores.cpu())
    else:
        assert gap > 2 * bound, (gap, bound)
        assert i == A.select(want) == N // 2


def test_select_ties_and_argument_errors(hip):
    cand = torch.zeros(4, 6, 7)
    cand[0] += 1.0
    cand[3] -= 1.0      # candidates 1 and 2 are equal and closest to the rest: the lower index wins
    scores, index, best = hip.action_select(cand.to(DEV), "medoid")
    assert int(index.item()) == 1 == A.select(A.medoid_scores(cand)) and scores[1] == scores[2]
    c = cand.to(DEV)
    known, w = torch.zeros(6, 7, device=DEV), torch.ones(6, device=DEV)
    for args in ((c, "best"), (c, "coherence"), (c, "coherence", known), (c, "coherence", known[:5], w), (c, "coherence", known, w[:5]),
                 (c[0], "medoid"), (torch.zeros(65, 2, 2, device=DEV), "medoid"), (torch.zeros(2, 100, 50, device=DEV), "medoid"),
                 (c.transpose(1, 2), "medoid")):
        with pytest.raises(ValueError, match="action_select"):
            hip.action_select(*args)
    with pytest.raises(TypeError):
        hip.action_select(c.double(), "medoid")
    assert hip._fn["lap_action_select"](None, None, None, scores.data_ptr(), index.data_ptr(), best.data_ptr(), 4, 6, 7, 0, hip._stream()) == 1001
    assert hip._fn["lap_action_select"](c.data_ptr(), None, None, scores.data_ptr(), index.data_ptr(), best.data_ptr(), 4, 6, 7, 1, hip._stream()) == 1001
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ the sampler
class Ctx:
    """One model and one request per config, built once for the module; noise for up to 8 candidates."""

    def __init__(self, cfg, seed=5):
        from lap_amd.model import LAP

        self.cfg, self.S, self.ad = cfg, cfg.action_horizon, cfg.action_dim
        self.oc = oracle_cfg(cfg)
        self.P = O.init_params(self.oc, seed=seed)
        obs, _, self.noise1, _ = make_inputs(cfg, B=1, ragged=False)
        self.so = {k: v for k, v in obs.items() if k != "tokenized_langact_mask"}
        self.o = to_observation(self.so | {"tokenized_langact_mask": None}, DEV)
        self.model = LAP(cfg, params=self.P, device=DEV)
        g = torch.Generator().manual_seed(23)
        self.noise = torch.randn(8, self.S, self.ad, generator=g)
        self.known = torch.randn(1, self.S, self.ad, generator=g)

    def sample(self, N=None, route="skinny", **kw):
        m = self.model
        keep = m.serve_chain
        try:
            m.serve_chain = route == "chain"
            fused = {"partials": "partials", "generic": False}.get(route, True)
            if N is not None:
                kw = dict(num_samples=N, noise=self.noise[:N].to(DEV)) | kw
            return m.sample_actions(0, self.o, num_steps=STEPS, fused=fused, **kw)
        finally:
            m.serve_chain = keep


@pytest.fixture(scope="module")
def ctxs(hip):
    mp = pytest.MonkeyPatch()
    made = {}

    def get(name):
        if name not in made:
            made[name] = Ctx(_full_width_cfg(mp, **{"s50": dict(action_dim=7), "s10": dict(action_dim=7, action_horizon=10)}[name]))
        return made[name]
    yield get
    made.clear()
    mp.undo()


@pytest.mark.parametrize("name,N", [("s50", 2), ("s50", 3), ("s10", 8)])
def test_sampler_shared_equals_replicated(ctxs, name, N):
    c = ctxs(name)
    shared = c.sample(N)
    assert tuple(shared.shape) == (N, c.S, c.ad) and bool(torch.isfinite(shared).all())
    assert torch.equal(shared, c.sample(N, share_prefix=False))
    keep = c.model.serve_overlap
    try:      # step 0 beside the prefill or behind it: the same launches
        c.model.serve_overlap = not keep
        assert torch.equal(shared, c.sample(N))
    finally:
        c.model.serve_overlap = keep


@pytest.mark.parametrize("route", ["skinny", "generic"])
def test_sampler_against_the_oracle(ctxs, route):
    c = ctxs("s50")
    N = 2
    if not hasattr(c, "ref"):
        soN = {k: ({kk: vv.expand(N, *vv.shape[1:]).contiguous() for kk, vv in v.items()} if isinstance(v, dict) else v.expand(N, *v.shape[1:]).contiguous())
               for k, v in c.so.items()}
        c.ref = O.sample_actions(c.P, c.oc, soN, c.noise[:N], num_steps=STEPS)
        c.ref16 = O.sample_actions(c.P, dataclasses.replace(c.oc, emulate_bf16=True), soN, c.noise[:N], num_steps=STEPS)
    out = c.sample(N, route=route)
    err, base = rel(out, c.ref), rel(c.ref16, c.ref)
    print(f"num_samples {N} {route}: rel(out, ref) {err:.3e}, rel(ref16, ref) {base:.3e}")
    assert err < max(FREE_RUN_RATIO * base, 5e-3), (err, base)
    if route == "generic":
        assert torch.equal(out, c.sample(N, route="partials"))


def test_one_sample_is_the_plain_call_on_the_chain(ctxs):
    c = ctxs("s50")
    noise = c.noise[:1].to(DEV)
    plain = c.model.sample_actions(0, c.o, num_steps=STEPS, noise=noise)
    assert torch.equal(c.model.sample_actions(0, c.o, num_steps=STEPS, noise=noise, num_samples=1), plain)
    assert c.model._chain_ctr is not None and not c.model.serve_chain_failed()      # the one-launch chain ran


def test_candidates_are_isolated(ctxs):
    c = ctxs("s50")
    N = 3
    base = c.sample(N)
    noise = c.noise[:N].clone()
    noise[1] = -noise[1]
    moved = c.sample(N, noise=noise.to(DEV))
    assert torch.equal(moved[0], base[0]) and torch.equal(moved[2], base[2]) and not torch.equal(moved[1], base[1])


def test_inpaint_applies_to_every_candidate(ctxs):
    c = ctxs("s50")
    N = 3
    mask = torch.zeros(1, c.S, dtype=torch.uint8)
    mask[0, :c.S // 2] = 1
    fr = mask[0].bool()
    plain = c.sample(N)
    assert torch.equal(c.sample(N, inpaint=(c.known, torch.zeros_like(mask))), plain)
    for route in ("skinny", "generic"):
        out = c.sample(N, route=route, inpaint=(c.known, mask)).cpu()
        for n in range(N):
            assert torch.equal(out[n][fr], c.known[0][fr]), (route, n)
        assert not torch.equal(out[:, ~fr], c.sample(N, route=route).cpu()[:, ~fr])
    assert torch.equal(c.sample(N, inpaint=(c.known, mask)), c.sample(N, inpaint=(c.known, mask), share_prefix=False))


def test_select_in_the_sampler(ctxs):
    c = ctxs("s50")
    N = 3
    cands = c.sample(N)
    col = {}
    best = c.sample(N, select="medoid", _select_out=col)
    assert tuple(best.shape) == (1, c.S, c.ad) and torch.equal(col["candidates"], cands)
    i = int(col["index"].item())
    assert torch.equal(best[0], cands[i])
    known = cands[2].cpu() + 1e-3
    w = A.coherence_weights(c.S, 4)
    col = {}
    best = c.sample(N, select="coherence", coherence=(known, w), collect=col)      # `collect`: the slow prefill, v_t of every step too
    assert int(col["index"].item()) == 2 == A.select(A.coherence_scores(col["candidates"], known, w)) and f"v_t/{STEPS - 1}" in col
    assert torch.equal(best[0], col["candidates"][2])


def test_sampler_argument_errors(ctxs):
    c = ctxs("s50")
    n2 = c.noise[:2].to(DEV)
    w = A.coherence_weights(c.S, 0)
    for kw in (dict(num_samples=0), dict(num_samples=9), dict(num_samples=2.0), dict(num_samples=2, noise=c.noise[:3].to(DEV)),
               dict(num_samples=2, noise=n2, select="best"), dict(num_samples=2, noise=n2, select="coherence"),
               dict(num_samples=2, noise=n2, select="coherence", coherence=(c.known[0, :-1], w)),
               dict(num_samples=2, noise=n2, select="coherence", coherence=(c.known[0], w[:-1])),
               dict(num_samples=2, noise=n2, coherence=(c.known[0], w)), dict(num_samples=1, select="medoid"), dict(select="medoid"),
               dict(num_samples=2, noise=n2, inpaint=(c.known.expand(2, -1, -1), torch.zeros(2, c.S)))):
        with pytest.raises(ValueError):
            c.model.sample_actions(0, c.o, num_steps=STEPS, **kw)
    o2 = to_observation({k: ({kk: vv.expand(2, *vv.shape[1:]) for kk, vv in v.items()} if isinstance(v, dict) else v.expand(2, *v.shape[1:]))
                         for k, v in c.so.items()} | {"tokenized_langact_mask": None}, DEV)
    with pytest.raises(ValueError, match="num_samples"):
        c.model.sample_actions(0, o2, num_steps=STEPS, num_samples=2)


# ------------------------------------------------------------------------------------------------------------ graph and policy
def test_graph_replay_serves_every_known_from_one_graph(ctxs):
    from lap_amd.serve import GraphedSampler

    c = ctxs("s50")
    N = 3
    noise = c.noise[:N].to(DEV)
    cands = c.sample(N).cpu()
    sampler = GraphedSampler(c.model, 1, STEPS, inpaint=True, num_samples=N, select="coherence").capture()
    graph = sampler.graph
    picked = []
    for target, d, ex in ((0, 5, 0), (2, 0, 3)):
        # `known` near candidate `target` of the free call; d frozen rows
        known = (cands[target] + 1e-3)[None]
        mask = torch.zeros(1, c.S, dtype=torch.uint8)
        mask[0, :d] = 1
        w = A.coherence_weights(c.S, ex, 0.9)
        got = sampler(c.o, noise, (known, mask), (known[0], w)).clone()
        col = {}
        want = c.sample(N, inpaint=(known, mask), select="coherence", coherence=(known[0], w), _select_out=col)
        assert torch.equal(got, want) and torch.equal(sampler.last_candidates, col["candidates"])
        assert torch.equal(sampler.last_scores, col["scores"]) and torch.equal(sampler.last_index, col["index"])
        assert int(sampler.last_index.item()) == target == A.select(A.coherence_scores(sampler.last_candidates, known[0], w))
        assert torch.equal(got[0, :d].cpu(), known[0, :d])
        picked.append(int(sampler.last_index.item()))
        assert sampler.graph is graph
    assert picked[0] != picked[1]
    with pytest.raises(ValueError):
        sampler(c.o, noise, None, None)      # select='coherence' needs its arguments
    with pytest.raises(ValueError):
        sampler(c.o, noise, None, (c.known[0], torch.full((c.S,), float("nan"))))
    with pytest.raises(ValueError):
        sampler(c.o, noise[:2], None, (c.known[0], torch.ones(c.S)))
    plain = GraphedSampler(c.model, 1, STEPS, num_samples=N)
    assert torch.equal(plain(c.o, noise), c.sample(N)) and plain.last_candidates is plain.out and plain.last_index is None


@pytest.mark.parametrize("use_graph", [True, False])
def test_policy_serves_the_coherent_candidate(ctxs, use_graph):
    from lap_amd.chunking import shift_chunk
    from lap_amd.serve import Policy

    c = ctxs("s50")
    obs = c.so
    req = {"image": {k: v[0].numpy() for k, v in obs["images"].items()}, "image_mask": {k: np.array(True) for k in obs["images"]},
           "state": obs["state"][0].numpy(), "tokenized_prompt": obs["tokenized_prompt"][0].numpy(),
           "tokenized_prompt_mask": obs["tokenized_prompt_mask"][0].numpy()}
    N = 3
    noise = c.noise[:N].numpy()
    pol = Policy(c.model, num_steps=STEPS, use_graph=use_graph, sample_kwargs={"num_samples": N, "select": "coherence", "rho": 0.8})
    first = pol.infer(req | {"executed": 2}, noise=noise)      # no previous chunk: medoid, and said so
    sel = first["policy_timing"]["select"]
    assert sel["mode"] == "medoid" and sel["fallback"] is True and len(sel["scores"]) == N
    cands = pol.last_candidates.cpu()
    assert torch.equal(cands, c.sample(N).cpu())
    assert sel["index"] == A.select(A.medoid_scores(cands)) and np.array_equal(first["actions"], cands[sel["index"]].numpy())
    assert np.array_equal(pol._chunker.prev, first["actions"])
    second = pol.infer(req | {"executed": 2}, noise=-noise)
    sel = second["policy_timing"]["select"]
    assert sel["mode"] == "coherence" and sel["fallback"] is False
    cands = pol.last_candidates.cpu()
    known = torch.from_numpy(shift_chunk(first["actions"], 2, 0)[0])
    want = A.coherence_scores(cands, known, A.coherence_weights(c.S, 2, 0.8))
    order = torch.argsort(want)
    assert ((want[order[1]] - want[order[0]]) / want[order[1]]).item() > 2 * (c.S * c.ad + 2) * 2.0 ** -24      # decided above the f32 error
    assert sel["index"] == A.select(want) and np.array_equal(second["actions"], cands[sel["index"]].numpy())
    assert np.allclose(sel["scores"], want.numpy(), rtol=1e-4)
    assert np.array_equal(pol._chunker.prev, second["actions"])      # the chunker holds the selected chunk
    third = pol.infer(req | {"inpaint": {"executed": 4, "freeze": 3}}, noise=noise)      # composes with real-time chunking
    assert third["policy_timing"]["inpaint"] == {"applied": True, "frozen_rows": 3} and third["policy_timing"]["select"]["mode"] == "coherence"
    assert np.array_equal(third["actions"][:3], second["actions"][4:7])
    assert (len(pol._cand_samplers) > 0) == use_graph
    for bad in ({"num_samples": 3}, {"num_samples": 3, "select": "best"}, {"select": "medoid"}, {"num_samples": 9, "select": "medoid"}):
        with pytest.raises(ValueError):
            Policy(c.model, num_steps=STEPS, use_graph=False, sample_kwargs=bad)
