"""Grammar-constrained decoding on the GPU: lap_decode_grammar_finish on stored logits against `grammar.decode_reference`, and the
model / serving surface (`grammar=`).

What is compared where.  Greedy draws, the automaton state, the EOS mask and the step bookkeeping are exact (`torch.equal`).  A
sampled draw is compared in the rows whose two best host scores over the state's set lie further apart than MARGIN (the last bits
of the two logarithms of the noise; tests/test_topk_topp_gpu.py's rule): the rows left out are the host's decision alone, they are
counted, and at most SHARE of all (row, step) pairs may be (tests/grammar_cases.py; tests/test_grammar_cpu.py holds the host
count to the same cap).  Sampled steps are teacher-forced: every launch starts from the reference's states, so a row left out at
one step is compared again at the next.  logp: within `_bound` of tests/test_logprob_gpu.py (4x the deviation from float64 of a
float32 restatement on the same logits, over the state's set) of `sampling.token_logprobs(..., allowed=allowed(q))`; as in that
file the bound is the largest over the rows of one launch, here with every row on the set of its own state."""
import numpy as np
import pytest
import torch

from lap_amd import grammar as G
from lap_amd import sampling as S
from oracle import lap_oracle as O
from tests import grammar_cases as C
from tests.common import make_inputs, oracle_cfg, to_observation
from tests.test_constrained_decode_gpu import _agrees_with_eager, _gemma2b_x2_cfg
from tests.test_logprob_gpu import _bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP = 8


@pytest.fixture(scope="module")
def auto():
    a = C.automaton()
    return a, a.to_device(DEV)


def _state(hip, B, t, done=0):
    st = hip.decode_state(B, DEV)
    st[0], st[1] = t, done
    st[16:16 + B] = 5
    return st


def _launch(hip, d, st, lg, gstate, out, T=0.0, logp=None, seed=C.SEED):
    samp = None
    if T > 0.0:
        samp = hip.decode_sampling(DEV)
        hip.decode_set_sampling(samp, seed, T)
    hip.decode_grammar_finish(st, samp, gstate, d.offsets, d.ids, d.next, lg, out, C.EOS, logp=logp)


def _dev(x, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


# --------------------------------------------------------------------------------------------------------------- kernel
@pytest.mark.parametrize("B", C.BS)
def test_greedy_steps_are_the_reference(hip, auto, B):
    a, d = auto
    steps = 6
    lg = C.logits(steps, B, seed=1)
    q0 = C.start_states(B)
    # planted ties: in the 63-entry segment (row 0 starts in state 2), and across the stride loop of the 1500-entry one
    s2 = a.allowed(2)
    lg[0, 0, s2[10]] = lg[0, 0, s2[40]] = 50.0
    if B > 2:
        s4 = a.allowed(4)                           # row 2 starts in state 4
        lg[0, 2, s4[100]] = lg[0, 2, s4[1400]] = lg[0, 2, s4[700]] = 60.0
    tok, _, st = G.decode_reference(lg, a, 0.0, seed=0, rows=B, start=q0)
    assert tok[0, 0] == s2[10] and (B <= 2 or tok[2, 0] == a.allowed(4)[100])
    state = _state(hip, B, 0)
    gstate = _dev(q0, torch.int32)
    out = torch.zeros(B, CAP, dtype=torch.int32, device=DEV)
    eos = np.zeros(B, dtype=bool)
    for t in range(steps):
        done_before = bool(eos.all())
        _launch(hip, d, state, _dev(lg[t]), gstate, out)
        if done_before:
            assert int(state[1]) == 1 and int(state[0]) == t_stop
            continue
        eos |= tok[:, t] == C.EOS
        t_stop = t + 1
        assert torch.equal(out[:, t].cpu(), torch.from_numpy(tok[:, t])), t
        assert torch.equal(gstate.cpu(), torch.from_numpy(st[:, t + 1])), t
        assert torch.equal(state[8:8 + B].cpu(), torch.from_numpy(eos.astype(np.int32))), t
        assert int(state[0]) == t + 1 and int(state[2]) == 0 and int(state[1]) == int(eos.all())
    assert float(out[:, t_stop:].abs().sum()) == 0


def test_the_sink_keeps_emitting_eos(hip, auto):
    a, d = auto
    B = 5
    lg = C.logits(2, B, seed=2)
    lg[0, :, C.EOS] = 99.0                          # rows in states 3 and 4 take their EOS edge
    lg[1, :, C.EOS] = -99.0                         # and row 2 takes none at the second step
    q0 = np.array([3, 4, 2, 3, 5])
    tok, _, st = G.decode_reference(lg, a, 0.0, seed=0, start=q0)
    assert (tok[[0, 1, 3, 4]] == C.EOS).all() and (st[[0, 1, 3, 4], 1:] == 5).all()
    state = _state(hip, B, 0)
    gstate = _dev(q0, torch.int32)
    out = torch.zeros(B, CAP, dtype=torch.int32, device=DEV)
    for t in range(2):
        _launch(hip, d, state, _dev(lg[t]), gstate, out)
    assert torch.equal(out[:, :2].cpu(), torch.from_numpy(tok)) and torch.equal(gstate.cpu(), torch.from_numpy(st[:, 2]))
    assert state[8:8 + B].tolist() == [1, 1, 0, 1, 1] and int(state[1]) == 0


def _sampled_case(hip, a, d, B, T):
    """One (B, temperature) of the sampled sweep; returns (pairs left out, pairs)."""
    lg, tok, lp, st, clear = C.sampled_reference(a, B, T)
    steps = lg.shape[0]
    out = torch.zeros(B, CAP, dtype=torch.int32, device=DEV)
    logp = torch.zeros(B, CAP, device=DEV)
    out2, logp2 = out.clone(), logp.clone()
    worst = (0.0, 0.0)
    for t in range(steps):
        x = _dev(lg[t])
        gstate = _dev(st[:, t], torch.int32)        # teacher-forced: the reference's states
        state = _state(hip, B, t)
        _launch(hip, d, state, x, gstate, out, T=T, logp=logp)
        assert int(state[0]) == t + 1 and int(state[2]) == 0
        got, nxt = out[:, t].cpu().numpy(), gstate.cpu().numpy()
        cl = clear[:, t]
        assert np.array_equal(got[cl], tok[cl, t]), (t, got, tok[:, t])
        assert np.array_equal(nxt[cl], st[cl, t + 1])
        for b in range(B):                          # every draw is an edge of the row's state, and the state follows it
            assert got[b] in a.allowed(int(st[b, t])) and nxt[b] == a.step(int(st[b, t]), int(got[b]))
        # logp: of the token the kernel drew, over the state's set, against float64 on the same logits; the bound is that of
        # this launch (its B rows, as tests/test_logprob_gpu.py pools the rows of a launch), every row on its own state's set
        sets = [a.allowed(int(st[b, t])) for b in range(B)]
        want = np.array([S.token_logprobs(lg[t, b:b + 1], got[b:b + 1], T, allowed=sets[b])[0] for b in range(B)])
        bound = max(_bound(lg[t, b:b + 1], T, ids=sets[b]) for b in range(B))
        err = np.abs(logp[:, t].cpu().numpy().astype(np.float64) - want)
        assert (err <= bound).all(), (t, err, bound)
        worst = max(worst, (float(err.max()), bound))
        # a second launch on the same inputs: identical bits
        gstate2 = _dev(st[:, t], torch.int32)
        state2 = _state(hip, B, t)
        _launch(hip, d, state2, x, gstate2, out2, T=T, logp=logp2)
        assert torch.equal(out2[:, t], out[:, t]) and torch.equal(logp2[:, t], logp[:, t]) and torch.equal(gstate2, gstate)
    print(f"B {B} T {T}: {int((~clear).sum())} of {clear.size} (row, step) pairs left out; largest |logp - float64| {worst[0]:.3e} "
          f"under a launch bound of {worst[1]:.3e}")
    return int((~clear).sum()), clear.size


def test_sampled_steps_are_the_reference(hip, auto):
    """Every (B, temperature) of the sweep, and the cap on what the sweep left out, counted over the pairs it ran."""
    a, d = auto
    out = total = 0
    for B in C.BS:
        for T in C.TEMPS:
            o, n = _sampled_case(hip, a, d, B, T)
            out, total = out + o, total + n
    print(f"{out} of {total} (row, step) pairs left out")
    assert total == sum(C.BS) * len(C.TEMPS) * C.STEPS_SAMPLED and out <= C.SHARE * total


def test_greedy_logp(hip, auto):
    a, d = auto
    B = 8
    lg = C.logits(1, B, seed=3)[0]
    q0 = np.array([0, 1, 2, 3, 4, 5, 4, 3])
    tok, lp, _ = G.decode_reference(lg[None], a, 0.0, seed=0, start=q0)
    state = _state(hip, B, 2)
    out = torch.zeros(B, CAP, dtype=torch.int32, device=DEV)
    logp = torch.zeros(B, CAP, device=DEV)
    _launch(hip, d, state, _dev(lg), _dev(q0, torch.int32), out, logp=logp)
    assert torch.equal(out[:, 2].cpu(), torch.from_numpy(tok[:, 0]))
    bound = max(_bound(lg[b:b + 1], 0.0, ids=a.allowed(int(q0[b]))) for b in range(B))
    err = np.abs(logp[:, 2].cpu().numpy().astype(np.float64) - lp[:, 0])
    print(f"greedy logp: |device - float64| up to {err.max():.3e}, bound {bound:.3e}")
    assert (err <= bound).all(), (err, bound)
    assert float(logp[0, 2]) == 0.0 and float(logp[5, 2]) == 0.0         # sets of one entry
    cols = [c for c in range(CAP) if c != 2]
    assert float(logp[:, cols].abs().sum()) == 0.0 and float(out[:, cols].abs().sum()) == 0


def test_done_and_budget_write_nothing(hip, auto):
    a, d = auto
    B = 5
    x = _dev(C.logits(1, B, seed=4)[0])
    state = _state(hip, B, 3, done=1)
    st0 = state.clone()
    out = torch.randint(0, 9, (B, CAP), dtype=torch.int32, device=DEV)
    logp = torch.full((B, CAP), -2.0, device=DEV)
    gstate = _dev(C.start_states(B), torch.int32)
    out0, g0 = out.clone(), gstate.clone()
    _launch(hip, d, state, x, gstate, out, T=0.7, logp=logp)
    torch.cuda.synchronize()
    assert torch.equal(state, st0) and torch.equal(out, out0) and bool((logp == -2.0).all()) and torch.equal(gstate, g0)
    # the budget is spent (t == cap): the flag alone
    state = _state(hip, B, CAP)
    st0 = state.clone()
    _launch(hip, d, state, x, gstate, out, T=0.7, logp=logp)
    st0[1] = 1
    assert torch.equal(state, st0) and torch.equal(out, out0) and bool((logp == -2.0).all()) and torch.equal(gstate, g0)


def test_arrivals_are_counted(hip, auto):
    a, d = auto
    B = 8
    lg = C.logits(5, B, seed=5)
    lg[:, :, C.EOS] = -99.0                         # no row ends
    state = _state(hip, B, 0)
    gstate = _dev(C.start_states(B), torch.int32)
    out = torch.zeros(B, CAP, dtype=torch.int32, device=DEV)
    for t in range(5):
        _launch(hip, d, state, _dev(lg[t]), gstate, out)
        assert int(state[0]) == t + 1 and int(state[2]) == 0 and int(state[1]) == 0
    tok, _, st = G.decode_reference(lg, a, 0.0, seed=0, start=C.start_states(B))
    assert torch.equal(out[:, :5].cpu(), torch.from_numpy(tok)) and torch.equal(gstate.cpu(), torch.from_numpy(st[:, 5]))


def test_a_state_outside_the_automaton_is_never_an_address(hip, auto):
    a, d = auto
    B = 5
    lg = C.logits(1, B, seed=6)[0]
    q0 = np.array([-1, a.num_states, 2, 3, 4])
    tok, _, st = G.decode_reference(lg[None, 2:], a, 0.0, seed=0, start=q0[2:])
    # (greedy: the reference's row index plays no part)
    state = _state(hip, B, 1)
    gstate = _dev(q0, torch.int32)
    out = torch.zeros(B, CAP, dtype=torch.int32, device=DEV)
    logp = torch.zeros(B, CAP, device=DEV)
    _launch(hip, d, state, _dev(lg), gstate, out, logp=logp)
    assert out[:2, 1].tolist() == [C.EOS, C.EOS] and gstate[:2].tolist() == [-1, a.num_states] and state[8:10].tolist() == [1, 1]
    assert bool(torch.isinf(logp[:2, 1]).all())
    assert torch.equal(out[2:, 1].cpu(), torch.from_numpy(tok[:, 0])) and torch.equal(gstate[2:].cpu(), torch.from_numpy(st[:, 1]))
    assert int(state[0]) == 2 and int(state[2]) == 0


# ---------------------------------------------------------------------------------------------------------------- model
STEPS = 13


@pytest.fixture(scope="module", autouse=True)
def _hand_back_stream_scratch(hip):
    import gc

    before = set(hip._SCRATCH)
    yield
    for k in set(hip._SCRATCH) - before:
        del hip._SCRATCH[k]
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def ar(hip):
    """The two-layer model at the Gemma-2B widths (seed 13) of tests/test_constrained_decode_gpu.py."""
    from lap_amd.model import LAP

    with pytest.MonkeyPatch.context() as mp:
        cfg = _gemma2b_x2_cfg(mp)
        model = LAP(cfg, params=O.init_params(oracle_cfg(cfg), seed=13), device=DEV)
        yield cfg, model
        model.EOS_TOKEN = 1


def _obs(cfg, B=3, seed=0):
    obs, _, _, _ = make_inputs(cfg, B=B, seed=seed, ragged=True)
    so = dict(obs)
    so.pop("tokenized_langact_mask")
    so["image_masks"] = {k: torch.ones_like(m) for k, m in so["image_masks"].items()}
    return to_observation(so | {"tokenized_langact_mask": None}, DEV)


def _chain(V, eos, L=10, n=400, seed=21):
    """States 0 .. L-2 allow disjoint random sets of n ids; an even id leads one state on, an odd id two (rows diverge); state
    L-1 allows the EOS token alone, so every row ends within L tokens; L: the sink."""
    rng = np.random.default_rng(seed)
    pool = rng.permutation(np.setdiff1d(np.arange(V), [eos]))[:n * (L - 1)].reshape(L - 1, n)
    segs = [(np.sort(s), np.minimum(q + 1 + (np.sort(s) & 1), L - 1)) for q, s in enumerate(pool)]
    segs += [(np.array([eos]), np.array([L])), (np.array([eos]), np.array([L]))]
    off = np.cumsum([0] + [len(i) for i, _ in segs])
    return G.check_automaton(G.TokenAutomaton(off, np.concatenate([i for i, _ in segs]), np.concatenate([x for _, x in segs]), V, eos))


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_a_single_state_automaton_is_the_allowed_set(ar, weights):
    cfg, model = ar
    o = _obs(cfg)
    g = torch.Generator().manual_seed(3)
    A = torch.unique(torch.randperm(cfg.vocab_size, generator=g)[:2001])
    kw = dict(max_decoding_steps=STEPS, decode="fused", decode_weights=weights)
    try:
        model.EOS_TOKEN = -1            # the greedy tokens do not depend on the EOS token; take one of A that is never drawn
        free = model.sample_tokens(0, o, allowed_tokens=A, **kw)
        eos = int(next(t for t in A.tolist() if t not in set(free.cpu().reshape(-1).tolist())))
        model.EOS_TOKEN = eos
        want = model.sample_tokens(0, o, allowed_tokens=A, **kw)
        assert torch.equal(want, free)
        got = model.sample_tokens(0, o, grammar=G.single_state_automaton(A.numpy(), eos, cfg.vocab_size), **kw)
        assert torch.equal(got, want)
    finally:
        model.EOS_TOKEN = 1


def test_a_multi_state_automaton_against_the_reference_and_the_eager_route(ar):
    cfg, model = ar
    o = _obs(cfg)
    V = cfg.vocab_size
    try:
        model.EOS_TOKEN = eos = 7
        # sets of 8 ids, seed 27: chosen (by a run of seeds 21 .. 30 at 8, 16, 40 and 400 ids) so that on the eager route the best
        # two allowed logits of every row lie more than 5e-2 apart at every step (the smallest gap is 0.0685), which is what
        # lets the two routes be compared with `torch.equal`; the test asserts that this holds
        a = _chain(V, eos, n=8, seed=27)
        col = {}
        tok = model.sample_tokens(0, o, max_decoding_steps=STEPS, decode="fused", grammar=a, collect=col)
        n = len(col)
        assert 6 <= n <= 10 and tok.shape == (3, STEPS)
        lg = np.stack([col[f"logit/{t}"].cpu().numpy() for t in range(n)])
        outside = np.setdiff1d(np.arange(V), a.union())
        assert np.isneginf(lg[:, :, outside]).all() and np.isfinite(lg[:, :, a.union()]).all()
        want, _, st = G.decode_reference(lg, a, 0.0, seed=0, rows=3)
        assert np.array_equal(tok[:, :n].cpu().numpy(), want) and float(tok[:, n:].abs().sum()) == 0
        # the grammar decides: in some state the best logit of the union is not an edge of that state
        free = lg.argmax(-1).T                      # [3, n]
        illegal = [(b, t) for b in range(3) for t in range(n) if free[b, t] not in a.allowed(int(st[b, t]))]
        assert illegal and all(want[b, t] != free[b, t] for b, t in illegal)
        for b in range(3):
            assert a.accepts(tok[b].cpu().numpy()), b
        assert len({tuple(r) for r in st.tolist()}) > 1                  # rows in different states
        assert torch.equal(model.sample_tokens(0, o, max_decoding_steps=STEPS, decode="fused", grammar=a), tok)
        cole = {}
        eager = model.sample_tokens(0, o, max_decoding_steps=STEPS, grammar=a, collect=cole)
        ok, clear = _agrees_with_eager(tok, eager, cole)
        print(f"eager {eager.tolist()} fused {tok.tolist()}, {clear} of {n} steps with every margin above 5e-2")
        assert len(cole) == n and clear == n        # every step of every row was compared
        assert ok and torch.equal(eager, tok)
        for b in range(3):
            assert a.accepts(eager[b].cpu().numpy()), b
        # log-probabilities: over the state's set, on either route
        tok2, lp = model.sample_tokens(0, o, max_decoding_steps=STEPS, decode="fused", grammar=a, return_logprobs=True)
        assert torch.equal(tok2, tok)
        _, ref_lp, _ = G.decode_reference(lg, a, 0.0, seed=0)
        # (one bound over the steps and rows of the decode, as the model-level check of tests/test_logprob_gpu.py takes it)
        assert np.abs(lp[:, :n].cpu().numpy() - ref_lp).max() <= max(_bound(lg[t, b:b + 1], 0.0, ids=a.allowed(int(st[b, t])))
                                                                   for b in range(3) for t in range(n))
    finally:
        model.EOS_TOKEN = 1


def test_best_of_n_rows_diverge_and_the_policy_answers_with_the_best(ar):
    from lap_amd.serve import ARPolicy, Policy

    cfg, model = ar
    try:
        model.EOS_TOKEN = eos = 7
        a = _chain(cfg.vocab_size, eos)
        o1 = _obs(cfg, B=1, seed=1)
        kw = dict(max_decoding_steps=STEPS, decode="fused", sampler="device", temperature=0.8, num_samples=4, grammar=a)
        tok, lp = model.sample_tokens(3, o1, **kw)
        assert tok.shape == (4, STEPS) and lp.shape == (4, STEPS)
        rows = tok.cpu().numpy()
        for b in range(4):
            assert a.accepts(rows[b]), rows[b]
        assert len({tuple(r) for r in rows.tolist()}) >= 2
        tok2, lp2 = model.sample_tokens(3, o1, **kw)
        assert torch.equal(tok, tok2) and torch.equal(lp, lp2)
        obs, _, _, _ = make_inputs(cfg, B=1, seed=2, ragged=True)
        req = {"image": {k: v[0].numpy() for k, v in obs["images"].items()}, "image_mask": {k: np.array(True) for k in obs["images"]},
               "state": obs["state"][0].numpy(), "tokenized_prompt": obs["tokenized_prompt"][0].numpy(),
               "tokenized_prompt_mask": obs["tokenized_prompt_mask"][0].numpy()}
        skw = {k: v for k, v in kw.items() if k != "decode"}
        for use_graph in (False, True):
            pol = ARPolicy(Policy(model, use_graph=False), sample_kwargs=skw, use_graph=use_graph)
            assert (pol._decoder is not None) == use_graph
            res = pol.infer(req)
            cand = res["candidates"]["tokens"]
            t_ref, lp_ref = (x.cpu().numpy() for x in model.sample_tokens(1, pol._base._to_observation(req)[0], **kw))     # call counter 1
            assert np.array_equal(cand, t_ref)
            best = S.select_best(t_ref, lp_ref, eos)
            assert np.array_equal(res["tokens"], cand[best:best + 1]) and a.accepts(res["tokens"][0])
            assert all(a.accepts(r) for r in cand)
    finally:
        model.EOS_TOKEN = 1


def test_one_capture_serves_every_request(ar):
    """Two different observations through one GraphedTokenDecoder: each request's tokens are the un-graphed fused decode's, which
    fails if gstate is not put back to the start state inside the captured prefill."""
    from lap_amd.serve import GraphedTokenDecoder

    cfg, model = ar
    try:
        model.EOS_TOKEN = eos = 7
        a = _chain(cfg.vocab_size, eos)
        dec = GraphedTokenDecoder(model, 3, STEPS, grammar=a)
        for seed in (0, 5, 0):
            o = _obs(cfg, seed=seed)
            want = model.sample_tokens(0, o, max_decoding_steps=STEPS, decode="fused", grammar=a)
            got = dec(o)
            assert torch.equal(got, want), seed
            assert all(a.accepts(r) for r in got.cpu().numpy())
        assert int(dec.ctx.gstate.min()) == a.num_states - 1             # every row ended in the sink, and the next request started anew
        sdec = GraphedTokenDecoder(model, 3, STEPS, sampling=True, logprobs=True, weights="fp8", grammar=a)
        for seed in (4, 9):
            o = _obs(cfg, seed=seed)
            want = model.sample_tokens(seed, o, max_decoding_steps=STEPS, decode="fused", sampler="device", temperature=0.8,
                                       decode_weights="fp8", return_logprobs=True, grammar=a)
            got = sdec(o, temperature=0.8, seed=seed)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    finally:
        model.EOS_TOKEN = 1
