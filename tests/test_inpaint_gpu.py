"""Action-chunk inpainting in the flow sampler (`sample_actions(inpaint=(known, mask))`, real-time chunking; GPU).

At the LAP-3B widths with 2 layers per tower (the config of the serving parity tests: only there do the skinny projections and the
one-launch chain exist), B = 1, 3 Euler steps, action_dim 7 (the fused Euler / embed tail); one case at action_dim 32 (the plain
tail) and one at B = 2, S = 10 with a mask per sample.  Exactness is the criterion wherever the semantics state bits: an all-zero
mask is the plain call, a frozen row of the result is `known`, and the host replay of the steps from the collected velocities
(tests/inpaint_reference.py: one fused multiply-add for a free row, three f32 operations for a frozen one) is the result.
Against the oracle restatement the bound is the one of the `sample_actions` parity tests."""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import lap_oracle as O
from tests.common import debug_model_cfg, make_inputs, oracle_cfg, rel, to_observation
from tests.inpaint_reference import oracle_sample_inpaint, replay_steps
from tests.test_model_parity_gpu import FREE_RUN_RATIO, _full_width_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 3


class Ctx:
    """One model, one request and one `known` per config, built once for the module."""

    def __init__(self, cfg, B, seed=5):
        from lap_amd.model import LAP

        self.cfg, self.B, self.S, self.ad = cfg, B, cfg.action_horizon, cfg.action_dim
        self.oc = oracle_cfg(cfg)
        self.P = O.init_params(self.oc, seed=seed)
        obs, _, self.noise, _ = make_inputs(cfg, B=B, ragged=False)
        self.so = {k: v for k, v in obs.items() if k != "tokenized_langact_mask"}
        self.o = to_observation(self.so | {"tokenized_langact_mask": None}, DEV)
        self.model = LAP(cfg, params=self.P, device=DEV)
        g = torch.Generator().manual_seed(23)
        self.known = torch.randn(self.noise.shape, generator=g)
        self._oracle = {}

    def mask(self, *rows_per_sample):
        """uint8 [B, S] with the given rows of each sample frozen (an int d = the prefix of d rows)."""
        m = torch.zeros(self.B, self.S, dtype=torch.uint8)
        for b, rows in enumerate(rows_per_sample):
            m[b, list(range(rows)) if isinstance(rows, int) else list(rows)] = 1
        return m

    def sample(self, mask=None, known=None, **kw):
        if mask is not None:
            kw["inpaint"] = ((self.known if known is None else known).to(DEV), mask.to(DEV))
        return self.model.sample_actions(0, self.o, num_steps=STEPS, noise=self.noise.to(DEV), **kw)

    def route(self, name, mask=None, **kw):
        """`sample` on one denoise route: chain (fused tail where the action_dim allows), chain_plain_tail, skinny, partials, generic."""
        m = self.model
        keep = m.serve_chain, m.serve_euler_embed
        try:
            m.serve_euler_embed = name != "chain_plain_tail"
            m.serve_chain = name in ("chain", "chain_plain_tail")
            fused = {"partials": "partials", "generic": False}.get(name, True)
            return self.sample(mask, fused=fused, **kw)
        finally:
            m.serve_chain, m.serve_euler_embed = keep


ROUTES = ("chain", "chain_plain_tail", "skinny", "partials", "generic")


@pytest.fixture(scope="module")
def ctxs(hip):
    mp = pytest.MonkeyPatch()
    made = {}

    def get(name):
        if name not in made:
            kw = {"ad7": dict(action_dim=7), "ad32": dict(action_dim=32), "b2": dict(action_dim=7, action_horizon=10)}[name]
            made[name] = Ctx(_full_width_cfg(mp, **kw), B=2 if name == "b2" else 1)
        return made[name]
    yield get
    made.clear()
    mp.undo()


def test_all_zero_mask_is_the_plain_call_on_every_route(ctxs):
    c = ctxs("ad7")
    zero = c.mask()
    for r in ROUTES:
        assert torch.equal(c.route(r, zero), c.route(r)), r
    assert c.model._chain_ctr is not None and not c.model.serve_chain_failed()      # the one-launch chain ran


@pytest.mark.parametrize("which", ["d1", "dS-1", "dS", "last_row"])
def test_frozen_rows_are_known_and_the_routes_agree(ctxs, which):
    c = ctxs("ad7")
    S = c.S
    mask = c.mask({"d1": 1, "dS-1": S - 1, "dS": S, "last_row": [S - 1]}[which])
    fr = mask.bool()
    outs = {r: c.route(r, mask).cpu() for r in ROUTES}
    for r, out in outs.items():
        assert torch.equal(out[fr], c.known[fr]), r
        assert bool(torch.isfinite(out).all()), r
    assert torch.equal(outs["chain"], outs["skinny"]) and torch.equal(outs["chain"], outs["chain_plain_tail"])
    assert torch.equal(outs["generic"], outs["partials"])
    if which != "dS":
        assert not torch.equal(outs["chain"][~fr], c.route("chain").cpu()[~fr])      # the free rows saw the frozen ones


@pytest.mark.parametrize("cfg_name,route", [("ad7", "chain"), ("ad7", "skinny"), ("ad7", "generic"), ("ad32", "chain")])
def test_steps_replay_on_the_host_bit_for_bit(ctxs, cfg_name, route):
    """x replayed from the collected v_t/k: pins the free update and the interpolation of every step, and `collect` on frozen rows."""
    c = ctxs(cfg_name)
    mask = c.mask([0, 1, 2, c.S // 2, c.S - 1])
    col = {}
    out = c.route(route, mask, collect=col).cpu()
    assert sorted(col) == [f"v_t/{k}" for k in range(STEPS)]
    v_ts = [col[f"v_t/{k}"].cpu() for k in range(STEPS)]
    assert all(v.shape == out.shape and bool(torch.isfinite(v).all()) for v in v_ts)
    assert torch.equal(replay_steps(c.noise, c.known, mask, v_ts, -1.0 / STEPS), out)
    fr = mask.bool()
    assert torch.equal(c.route(route, mask).cpu()[fr], out[fr])      # (without `collect` a frozen row skips the projection)


def test_plain_tail_at_action_dim_32(ctxs):
    c = ctxs("ad32")
    zero, mask = c.mask(), c.mask(c.S // 2)
    fr = mask.bool()
    for r in ("chain", "skinny", "generic"):
        assert torch.equal(c.route(r, zero), c.route(r)), r
    outs = {r: c.route(r, mask).cpu() for r in ROUTES}
    for r, out in outs.items():
        assert torch.equal(out[fr], c.known[fr]), r
    assert torch.equal(outs["chain"], outs["skinny"]) and torch.equal(outs["generic"], outs["partials"])


def test_batch_of_two_with_a_mask_per_sample(ctxs):
    c = ctxs("b2")
    assert (c.B, c.S) == (2, 10)
    zero, mask = c.mask(), c.mask(3, [0, 9])
    fr = mask.bool()
    for r in ROUTES:
        plain = c.route(r)
        assert torch.equal(c.route(r, zero), plain), r
        col = {}
        out = c.route(r, mask, collect=col).cpu()
        assert torch.equal(out[fr], c.known[fr]), r
        assert torch.equal(replay_steps(c.noise, c.known, mask, [col[f"v_t/{k}"].cpu() for k in range(STEPS)], -1.0 / STEPS), out), r
    # sample 1's mask does not reach sample 0: with sample 1 free, sample 0 is unchanged
    assert torch.equal(c.route("skinny", c.mask(3, 0))[0], c.route("skinny", mask)[0])


@pytest.mark.parametrize("route", ["chain", "generic"])
def test_against_the_oracle_restatement(ctxs, route):
    c = ctxs("ad7")
    mask = c.mask(c.S // 2)
    if "ref" not in c._oracle:
        c._oracle["ref"] = oracle_sample_inpaint(c.P, c.oc, c.so, c.noise, c.known, mask, num_steps=STEPS)
        c._oracle["ref16"] = oracle_sample_inpaint(c.P, dataclasses.replace(c.oc, emulate_bf16=True), c.so, c.noise, c.known, mask, num_steps=STEPS)
    ref, ref16 = c._oracle["ref"], c._oracle["ref16"]
    out = c.route(route, mask)
    err, base = rel(out, ref), rel(ref16, ref)
    print(f"inpaint {route}: rel(out, ref) {err:.3e}, rel(ref16, ref) {base:.3e}")
    assert err < max(FREE_RUN_RATIO * base, 5e-3), (err, base)


def test_free_rows_depend_on_known(ctxs):
    c = ctxs("ad7")
    mask = c.mask(c.S // 2)
    fr = mask.bool()
    a, b = c.sample(mask).cpu(), c.sample(mask, known=-c.known).cpu()
    assert torch.equal(a[fr], c.known[fr]) and torch.equal(b[fr], -c.known[fr])
    assert not torch.equal(a[~fr], b[~fr]) and rel(a[~fr], b[~fr]) > 1e-3


def test_argument_errors_reach_the_caller(ctxs):
    c = ctxs("ad7")
    bad_known = c.known.clone()
    bad_known[0, 3, 2] = float("nan")
    for known, mask in ((c.known[:, :-1], c.mask()), (c.known, c.mask()[:, :-1]), (bad_known, c.mask(2)), (c.known, c.mask(2) * 3),
                        (c.known.expand(2, -1, -1), c.mask().expand(2, -1))):
        with pytest.raises(ValueError, match="inpaint"):
            c.model.sample_actions(0, c.o, num_steps=STEPS, noise=c.noise.to(DEV), inpaint=(known, mask))


def test_kernel_wrappers_check_their_arguments(hip):
    x, v = torch.zeros(6, 7, device=DEV), torch.ones(6, 7, device=DEV)
    noise, known = torch.full((6, 7), 2.0, device=DEV), torch.full((6, 7), -3.0, device=DEV)
    mask = torch.tensor([1, 0, 0, 1, 0, 0], dtype=torch.uint8, device=DEV)
    hip.euler_inpaint_f32(x, v, -0.5, noise, known, mask, (0.25, 0.75))
    want = torch.full((6, 7), -0.5)
    want[[0, 3]] = 0.25 * 2.0 + 0.75 * -3.0
    assert torch.equal(x.cpu(), want)
    hip.euler_inpaint_f32(x, v, -0.5, noise, known, mask, (0.0, 1.0))
    assert torch.equal(x.cpu()[[0, 3]], known.cpu()[[0, 3]]) and torch.equal(x.cpu()[1], torch.full((7,), -1.0))
    with pytest.raises(ValueError):
        hip.euler_inpaint_f32(x, v, -0.5, noise[:5], known, mask, (0.0, 1.0))
    with pytest.raises(ValueError):
        hip.euler_inpaint_f32(x, v, -0.5, noise, known, mask[:5], (0.0, 1.0))
    with pytest.raises(ValueError):
        hip.euler_inpaint_f32(x, v, -0.5, noise, known.t().contiguous().t(), mask, (0.0, 1.0))
    with pytest.raises(TypeError):
        hip.euler_inpaint_f32(x, v, -0.5, noise, known, mask.bool(), (0.0, 1.0))
    with pytest.raises(TypeError):
        hip.euler_inpaint_f32(x, v, -0.5, noise.double(), known, mask, (0.0, 1.0))
    with pytest.raises(hip.LapHipError):
        hip.euler_inpaint_f32(x, v, -0.5, x, known, mask, (0.0, 1.0))      # noise must not alias x_t
    with pytest.raises(hip.LapHipError):
        hip.euler_inpaint_f32(x, v, -0.5, noise, known, mask, (1.5, -0.5))


def test_graph_replay_serves_every_mask_from_one_graph(ctxs):
    from lap_amd.serve import GraphedSampler

    c = ctxs("ad7")
    sampler = GraphedSampler(c.model, 1, STEPS, inpaint=True).capture()
    graph = sampler.graph
    noise = c.noise.to(DEV)
    for mask in (c.mask(c.S // 2), c.mask(), c.mask([c.S - 1]), c.mask(c.S // 2)):
        got = sampler(c.o, noise, (c.known, mask)).clone()
        assert torch.equal(got, c.sample(mask)), mask.sum()
        assert sampler.graph is graph
    assert torch.equal(sampler(c.o, noise), c.sample())      # no inpaint argument = the all-zero mask = the plain call
    assert sampler.graph is graph
    with pytest.raises(ValueError):
        sampler(c.o, noise, (c.known, c.mask(2) * 2))
    plain = GraphedSampler(c.model, 1, STEPS)
    assert plain.inpaint is None
    with pytest.raises(ValueError):
        plain._load(c.o, noise, (c.known, c.mask(2)))


@pytest.mark.parametrize("use_graph", [True, False])
def test_policy_infer_freezes_the_head_on_its_own_last_chunk(ctxs, use_graph):
    from lap_amd.chunking import shift_chunk
    from lap_amd.serve import Policy

    c = ctxs("ad7")
    obs = c.so
    req = {"image": {k: v[0].numpy() for k, v in obs["images"].items()}, "image_mask": {k: np.array(True) for k in obs["images"]},
           "state": obs["state"][0].numpy(), "tokenized_prompt": obs["tokenized_prompt"][0].numpy(),
           "tokenized_prompt_mask": obs["tokenized_prompt_mask"][0].numpy()}
    noise = c.noise[0].numpy()
    pol = Policy(c.model, num_steps=STEPS, use_graph=use_graph)
    today = Policy(c.model, num_steps=STEPS, use_graph=use_graph).infer(req, noise=noise)
    s, d = 4, 6
    first = pol.infer(req | {"inpaint": {"executed": s, "freeze": d}}, noise=noise)      # no previous chunk: ignored, and said so
    assert first["policy_timing"]["inpaint"]["applied"] is False and "ignored" in first["policy_timing"]["inpaint"]["reason"]
    assert np.array_equal(first["actions"], today["actions"]) and "inpaint" not in today["policy_timing"]
    second = pol.infer(req | {"inpaint": {"executed": s, "freeze": d}}, noise=-noise)
    assert second["policy_timing"]["inpaint"] == {"applied": True, "frozen_rows": d}
    assert np.array_equal(second["actions"][:d], first["actions"][s:s + d])
    known, mask = shift_chunk(first["actions"], s, d)
    want = c.model.sample_actions(0, c.o, num_steps=STEPS, noise=-c.noise.to(DEV), inpaint=(known[None], mask[None]))[0].cpu().numpy()
    assert np.array_equal(second["actions"], want)
    assert (pol._inpaint_sampler is not None) == use_graph
    plain = pol.infer(req, noise=noise)      # a request without the key: today's output
    assert np.array_equal(plain["actions"], today["actions"]) and set(plain["policy_timing"]) == {"infer_ms"}
    explicit = pol.infer(req | {"inpaint": {"known": known, "mask": mask}}, noise=-noise)
    assert np.array_equal(explicit["actions"], want)
    pol.reset()
    again = pol.infer(req | {"inpaint": {"executed": s, "freeze": d}}, noise=noise)
    assert again["policy_timing"]["inpaint"]["applied"] is False and np.array_equal(again["actions"], today["actions"])
    with pytest.raises(ValueError):
        pol.infer(req | {"inpaint": {"executed": c.S, "freeze": 1}}, noise=noise)
    with pytest.raises(ValueError):
        pol.infer(req | {"inpaint": {"executed": 1}}, noise=noise)


def test_pi0_sampler_inpaints(hip):
    from lap_amd.model import LAP

    cfg = debug_model_cfg(pi05=False)
    P = O.init_params(oracle_cfg(cfg), seed=11)
    obs, _, noise, _ = make_inputs(cfg, B=2, ragged=True)
    o = to_observation({k: v for k, v in obs.items() if k != "tokenized_langact_mask"} | {"tokenized_langact_mask": None}, DEV)
    model = LAP(cfg, params=P, device=DEV)
    S = cfg.action_horizon
    known = torch.randn(noise.shape, generator=torch.Generator().manual_seed(4))
    mask = torch.zeros(2, S, dtype=torch.uint8)
    mask[0, :S // 2] = 1
    mask[1, S - 1] = 1
    sample = lambda **kw: model.sample_actions(0, o, num_steps=STEPS, noise=noise.to(DEV), **kw)
    plain = sample()
    assert torch.equal(sample(inpaint=(known, torch.zeros_like(mask))), plain)
    col = {}
    out = sample(inpaint=(known, mask), collect=col).cpu()
    fr = mask.bool()
    assert torch.equal(out[fr], known[fr]) and not torch.equal(out[~fr], plain.cpu()[~fr])
    assert torch.equal(replay_steps(noise, known, mask, [col[f"v_t/{k}"].cpu() for k in range(STEPS)], -1.0 / STEPS), out)
