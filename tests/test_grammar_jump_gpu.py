"""Jump-forward grammar decoding on the GPU: lap_decode_grammar_draft and lap_decode_grammar_spec_finish against
`speculate.grammar_drafts` / `grammar_verify`, and the model / serving surface (`jump_forward=S`).

What is compared where.  Drafts, tokens, the automaton state, the state words and the counters are exact.  A log-probability of the
multi-row finish is compared bit for bit with lap_decode_grammar_finish launched on the same logits row and automaton state at
step t + r (the two kernels call one row body), and a jump-forward decode of the model with the plain grammar decode by
`torch.equal`, log-probabilities included, greedy and sampled.  The kernel cases are drawn so that the host reference decides
every draw by more than MARGIN (the last bits of the two logarithms of the noise; tests/grammar_cases.py's rule): a logits row
whose two best host scores over its state's set lie closer is drawn again, which is the host's decision alone."""
import numpy as np
import pytest
import torch

from lap_amd import sampling as SM
from lap_amd import speculate as SP
from tests.common import make_inputs, to_observation
from tests.grammar_cases import MARGIN
from tests.test_grammar_cpu import _five_state
from tests.test_grammar_jump_cpu import _chain_automaton
from tests.test_speculate_gpu import CHAIN, _chain_params, _gemma2b_x2_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
V, CAP, EOS, SEED = 64, 12, 1, 20261020


@pytest.fixture(scope="module")
def autos():
    return [(a, a.to_device(DEV)) for a in (_five_state(), _chain_automaton())]


def _state(hip, t, done=0):
    st = hip.decode_state(1, DEV)
    st[0], st[1], st[16] = t, done, 5
    st[24], st[25] = 3, 7
    return st


def _i32(x):
    return torch.tensor(np.asarray(x, dtype=np.int32).reshape(-1), dtype=torch.int32, device=DEV)


def _walk(a, rs, q, n):
    """n tokens along random edges of the automaton from state q (it stops in the sink)."""
    out = []
    for _ in range(n):
        seg = a.allowed(q)
        out.append(int(seg[rs.randint(len(seg))]))
        q = a.step(q, out[-1])
    return out


# --------------------------------------------------------------------------------------------------------- draft kernel
def draft_cases(hosts, S):
    """The 50 cases of the draft-kernel test at S rows, from the host alone: [(automaton index, t, written tokens, reference, q)]."""
    rs = np.random.RandomState(100 + S)
    cases = []
    for case in range(50):
        a = hosts[case % 2]
        t = int(rs.randint(1, CAP + 1))
        seq = _walk(a, rs, 0, CAP)                      # what was written, and a reference that resembles it
        ref = list(seq)
        if rs.rand() < 0.5:
            ref[int(rs.randint(CAP))] = int(rs.randint(V))
        ref = [None, ref, ref[:int(rs.randint(1, CAP))]][int(rs.randint(3))]
        q = 0
        for x in seq[:t]:
            q = a.step(q, x)
        if case % 10 == 9:                              # a state outside the automaton is never an address
            q = [-1, a.num_states, 1 << 30, -(1 << 31)][(case // 10) % 4]
        cases.append((case % 2, t, seq[:t], ref, q))
    return cases


@pytest.mark.parametrize("S", [2, 4, 8])
def test_draft_kernel_matches_the_numpy_rule(hip, autos, S):
    refbuf = hip.decode_spec_ref(CAP, DEV)
    drafted = from_ref = outside = 0
    for case, (a_i, t, written, ref, q) in enumerate(draft_cases([a for a, _ in autos], S)):
        a, d = autos[a_i]
        outside += int(not 0 <= q < a.num_states)
        out = torch.full((1, CAP), 5, dtype=torch.int32, device=DEV)
        out[0, :t] = _i32(written)
        hip.decode_set_spec_ref(refbuf, ref)
        draft = torch.full((S - 1,), -7, dtype=torch.int32, device=DEV)
        gstate = _i32([q])
        st = _state(hip, t)
        st0 = st.clone()
        hip.decode_spec_draft(st, refbuf, out, draft)
        raw = draft.tolist()
        assert raw == SP.draft_tokens(ref, out[0].tolist(), t, S).tolist()
        hip.decode_grammar_draft(st, gstate, d.offsets, d.ids, d.next, draft, out, V, EOS)
        want = SP.grammar_drafts(a, q, raw)
        assert draft.tolist() == want.tolist(), (case, q, t, raw)
        assert gstate.tolist() == [q] and torch.equal(st, st0)
        drafted += int((want >= 0).sum())
        if 0 <= q < a.num_states:
            qq = q
            for x in want.tolist():
                if x < 0:
                    break
                from_ref += int(len(a.allowed(qq)) > 1)
                qq = a.step(qq, x)
        else:
            assert (want == -1).all()
    assert drafted >= 25 and from_ref >= 3 and outside == 5
    # done is set: the drafts stay what they were
    a, d = autos[1]
    draft = torch.full((S - 1,), -7, dtype=torch.int32, device=DEV)
    hip.decode_grammar_draft(_state(hip, 2, done=1), _i32([0]), d.offsets, d.ids, d.next, draft, torch.zeros(1, CAP, dtype=torch.int32, device=DEV), V, EOS)
    assert draft.tolist() == [-7] * (S - 1)
    # a forced run of the chain automaton, without a reference: 3 -> 4 -> 5, then the state with a choice ends the run
    hip.decode_grammar_draft(_state(hip, 2), _i32([0]), d.offsets, d.ids, d.next, draft, torch.zeros(1, CAP, dtype=torch.int32, device=DEV), V, EOS)
    assert draft.tolist() == ([3, 4, 5] + [-1] * 4)[:S - 1]


# -------------------------------------------------------------------------------------------------------- finish kernel
def _clear(a, row, q, T, step):
    seg = a.allowed(q)
    if len(seg) == 1 or T <= 0.0:
        return True
    masked = np.full((1, V), -np.inf, dtype=np.float32)
    masked[0, seg] = row[seg]
    top2 = np.partition(SM.scores_from_logits(masked, T, SEED, step)[0], -2)[-2:]
    return bool(top2[1] - top2[0] > MARGIN)


def _rows(a, rs, q, t, S, T):
    """S rows of logits and the tokens / states of the rows when every draft is right (the run ends with an EOS); each row is
    drawn again until the host decides its draw by more than MARGIN."""
    lg = np.zeros((S, V), dtype=np.float32)
    toks, states = [], [q]
    for r in range(S):
        if toks and toks[-1] == EOS:
            lg[r] = (rs.standard_normal(V) * 3).astype(np.float32)
            continue
        for _ in range(100):
            lg[r] = (rs.standard_normal(V) * 3).astype(np.float32)
            if _clear(a, lg[r], states[-1], T, t + r):
                break
        else:
            raise AssertionError("no clear row in 100 draws")
        e, _, qn = SP.grammar_verify(lg[r:r + 1], a, states[-1], [], t + r, 1 << 20, T, SEED)
        toks.append(int(e[0]))
        states.append(qn)
    return lg, toks, states


def _lp_tol(row, seg, T, want):
    """The forward error of z_tok - (M + logf(s)) in float32 over a set of n entries, on the float32 products z both sides share:
    s is a sum of n terms exp(z - M) <= 1, each expf within 2 ulp (2^-22 relative) and each addition within 2^-24 relative, so
    log s is off by at most (n + 4) 2^-24, plus logf's own 2^-23 |log s| with |log s| <= log n; M + logf(s) rounds once (2^-24 of
    at most |M| + log n) and the final difference once (2^-24 |result|).  Summed and rounded up to units of 2^-23:
    2^-23 (|M| + 2 log n + |result| + n + 4)."""
    z = np.abs(row[seg].astype(np.float64) * (float(SM.inverse_temperature(T)) if T > 0.0 else 1.0))
    n = len(seg)
    return 2.0 ** -23 * (float(z.max()) + 2.0 * np.log(n) + abs(float(want)) + n + 4)


def _finish(hip, d, st, lg, gstate, draft, out, logp, T):
    samp = None
    if T > 0.0:
        samp = hip.decode_sampling(DEV)
        hip.decode_set_sampling(samp, SEED, T)
    hip.decode_grammar_spec_finish(st, samp, gstate, d.offsets, d.ids, d.next, lg, draft, out, EOS, logp=logp)
    return samp


def finish_cases(hosts, T):
    """The cases of the finish-kernel test at temperature T and what they cover, from the host specification alone:
    ([(automaton index, S, q, t, logits, draft, states of the rows, emitted, logp, q_after)], coverage)."""
    rs = np.random.RandomState(int(T * 10) + 1)
    seen = {"wrong0": 0, "middle": 0, "nowhere": 0, "eos_inside": 0, "cap": 0, "sizes": set()}
    cases, built = [], []
    for i in range(36):
        a_i = i % 2
        a = hosts[a_i]
        S = (2, 4, 8)[i % 3]
        q = int(rs.randint(a.num_states - 1))
        t = int(rs.randint(1, CAP))
        kind = ("nowhere", "wrong0", "middle")[(i // 6) % 3]
        cases.append((a_i, S, q, t, kind))
    cases += [(1, 4, 3, 2, "nowhere"), (1, 8, 4, 5, "nowhere"), (1, 4, 4, 1, "nowhere"),      # chain: 9, EOS inside the run
              (0, 4, 0, CAP - 2, "nowhere"), (1, 8, 0, CAP - 3, "nowhere"), (0, 2, 2, CAP - 1, "nowhere")]      # t + r reaches cap
    for a_i, S, q, t, kind in cases:
        a = hosts[a_i]
        lg, toks, states = _rows(a, rs, q, t, S, T)
        draft = (toks + [-1] * S)[:S - 1]
        if kind == "wrong0":
            draft[0] = (draft[0] + 1) % V if draft[0] >= 0 else 3
        if kind == "middle" and S > 2:
            draft[(S - 1) // 2] = -1
        want, want_lp, q_after = SP.grammar_verify(lg, a, q, draft, t, CAP, T, SEED)
        n = len(want)
        assert want.tolist() == toks[:n]
        built.append((a_i, S, q, t, lg, draft, states, want, want_lp, q_after))
        # what the case covers
        stopped_by_draft = n < S and n < len(toks) and want[n - 1] != EOS and t + n < CAP
        seen["wrong0"] += int(kind == "wrong0" and n == 1 and stopped_by_draft)
        seen["middle"] += int(kind == "middle" and S > 2 and n == (S - 1) // 2 + 1 and stopped_by_draft)
        seen["nowhere"] += int(kind == "nowhere" and n == S)
        seen["eos_inside"] += int(n >= 2 and want[-1] == EOS and n < S)
        seen["cap"] += int(n >= 2 and t + n == CAP and want[-1] != EOS and n < S)
        seen["sizes"].add(n)
    return built, seen


@pytest.mark.parametrize("T", [0.0, 0.8, 1.5])
def test_finish_kernel_matches_the_numpy_rule(hip, autos, T):
    built, seen = finish_cases([a for a, _ in autos], T)
    assert min(seen[k] for k in ("wrong0", "middle", "nowhere", "eos_inside", "cap")) >= 1, seen
    assert seen["sizes"] >= {1, 2, 3, 4}, seen
    for a_i, S, q, t, lg, draft, states, want, want_lp, q_after in built:
        a, d = autos[a_i]
        n = len(want)
        st = _state(hip, t)
        out0 = torch.randint(10, 20, (1, CAP), dtype=torch.int32, device=DEV)
        out, logp = out0.clone(), torch.full((1, CAP), -2.0, device=DEV)
        gstate = _i32([q])
        x = torch.from_numpy(lg).to(DEV)
        _finish(hip, d, st, x, gstate, _i32(draft), out, logp, T)
        exp = out0.clone()
        exp[0, t:t + n] = _i32(want)
        assert torch.equal(out, exp), (a_i, S, q, t, out.tolist(), want.tolist())
        assert gstate.tolist() == [q_after]
        s = st.tolist()
        saw_eos = int(EOS in want.tolist())
        assert s[0] == t + n and s[8] == saw_eos and s[1] == int(t + n >= CAP or saw_eos), (s[:9], t, n)
        assert (s[24], s[25]) == (4, 7 + n - 1) and s[16] == 5 and s[2] == 0
        # log-probabilities: bit for bit the single-row kernel's on the same row and state at step t + r, and close to float64
        got_lp = logp[0].cpu().numpy()
        assert (got_lp[:t] == -2.0).all() and (got_lp[t + n:] == -2.0).all()
        for r in range(n):
            st1 = hip.decode_state(1, DEV)
            st1[0] = t + r
            out1, lp1, g1 = torch.zeros(1, CAP, dtype=torch.int32, device=DEV), torch.zeros(1, CAP, device=DEV), _i32([states[r]])
            samp = None
            if T > 0.0:
                samp = hip.decode_sampling(DEV)
                hip.decode_set_sampling(samp, SEED, T)
            hip.decode_grammar_finish(st1, samp, g1, d.offsets, d.ids, d.next, x[r:r + 1].contiguous(), out1, EOS, logp=lp1)
            assert int(out1[0, t + r]) == int(want[r]) and g1.tolist() == [states[r + 1]]
            assert torch.equal(lp1[0, t + r].view(torch.int32), logp[0, t + r].view(torch.int32)), (r, float(lp1[0, t + r]), got_lp[t + r])
        # and it is the specification's float64 value to float32 rounding (the single-row kernel's own accuracy is the business of
        # tests/test_grammar_gpu.py): `_lp_tol` below
        for r in range(n):
            tol = _lp_tol(lg[r], a.allowed(states[r]), T, want_lp[r])
            assert abs(float(got_lp[t + r]) - want_lp[r]) <= tol, (r, got_lp[t + r], want_lp[r], tol)


def test_finish_kernel_budget_done_and_a_bad_state(hip, autos):
    a, d = autos[0]
    S, T = 4, 0.8
    x = torch.from_numpy((np.random.RandomState(2).standard_normal((S, V)) * 3).astype(np.float32)).to(DEV)
    draft = _i32([30, 5, 2])
    out0 = torch.randint(10, 20, (1, CAP), dtype=torch.int32, device=DEV)
    # done is set: nothing is written
    for t, done in ((3, 1), (CAP, 1)):
        st = _state(hip, t, done=done)
        st0, out, logp, gstate = st.clone(), out0.clone(), torch.full((1, CAP), -2.0, device=DEV), _i32([1])
        _finish(hip, d, st, x, gstate, draft, out, logp, T)
        torch.cuda.synchronize()
        assert torch.equal(st, st0) and torch.equal(out, out0) and bool((logp == -2.0).all()) and gstate.tolist() == [1]
    # t >= cap on entry: the flag alone
    st = _state(hip, CAP)
    st0, out, logp, gstate = st.clone(), out0.clone(), torch.full((1, CAP), -2.0, device=DEV), _i32([1])
    _finish(hip, d, st, x, gstate, draft, out, logp, T)
    st0[1] = 1
    assert torch.equal(st, st0) and torch.equal(out, out0) and bool((logp == -2.0).all()) and gstate.tolist() == [1]
    assert len(SP.grammar_verify(x.cpu().numpy(), a, 1, draft.tolist(), CAP, CAP, T, SEED)[0]) == 0
    # a state outside the automaton: the row emits EOS with log-probability -inf and the state is kept
    for bad in (-1, a.num_states, 1 << 30):
        st = _state(hip, 4)
        out, logp, gstate = out0.clone(), torch.full((1, CAP), -2.0, device=DEV), _i32([bad])
        _finish(hip, d, st, x, gstate, draft, out, logp, T)
        want, want_lp, q_after = SP.grammar_verify(x.cpu().numpy(), a, bad, draft.tolist(), 4, CAP, T, SEED)
        assert want.tolist() == [EOS] and q_after == bad and np.isneginf(want_lp).all()
        exp = out0.clone()
        exp[0, 4] = EOS
        assert torch.equal(out, exp) and gstate.tolist() == [bad] and bool(torch.isneginf(logp[0, 4])) and float(logp[0, 5]) == -2.0
        s = st.tolist()
        assert (s[0], s[1], s[8], s[24], s[25]) == (5, 1, 1, 4, 7)


# ---------------------------------------------------------------------------------------------------------------- model
BUDGETS = (13, 5)
MODEL_EOS = 7


@pytest.fixture(scope="module", autouse=True)
def _hand_back_stream_scratch(hip):
    import gc

    before = set(hip._SCRATCH)
    yield
    for k in set(hip._SCRATCH) - before:
        del hip._SCRATCH[k]
    gc.collect()
    torch.cuda.empty_cache()


def _model_automaton(vocab):
    """Over the chain ids of tests/test_speculate_gpu.py, whose answer is c_1, c_2, ..: token k is drawn in state k.  States 1, 4,
    7 and 8 offer the successor among other ids (two of them chain ids), every other state has the successor as its single edge;
    state 10 allows the EOS token alone, so an answer of the larger budget ends in an EOS that a forced run carries."""
    from lap_amd import grammar as G

    segs = []
    for k in range(10):
        ids = {CHAIN[k + 1]}
        if k in (1, 4, 7, 8):
            ids |= {CHAIN[k + 4], CHAIN[(k + 8) % 20], 100 + k, 9000 + k}
        segs.append((sorted(ids), k + 1))
    segs += [([MODEL_EOS], 11), ([MODEL_EOS], 11)]
    off = np.cumsum([0] + [len(i) for i, _ in segs])
    return G.check_automaton(G.TokenAutomaton(off, [i for s, _ in segs for i in s], [n for s, n in segs for _ in s], vocab, MODEL_EOS))


@pytest.fixture(scope="module")
def ar(hip):
    """(cfg, model, observation of batch 1, automaton) on the 2-layer chain model of tests/test_speculate_gpu.py."""
    from lap_amd.model import LAP

    with pytest.MonkeyPatch.context() as mp:
        cfg = _gemma2b_x2_cfg(mp)
        model = LAP(cfg, params=_chain_params(cfg), device=DEV)
        model.EOS_TOKEN = MODEL_EOS
        obs, _, _, _ = make_inputs(cfg, B=1, ragged=True)
        so = dict(obs)
        so.pop("tokenized_langact_mask")
        so["image_masks"] = {k: torch.ones_like(m) for k, m in so["image_masks"].items()}
        last = int(torch.nonzero(so["tokenized_prompt_mask"][0]).max())
        so["tokenized_prompt"] = so["tokenized_prompt"].clone()
        so["tokenized_prompt"][0, last] = CHAIN[0]
        o = to_observation(so | {"tokenized_langact_mask": None}, DEV)
        yield cfg, model, o, _model_automaton(cfg.vocab_size)
        model.EOS_TOKEN = 1


def _answer(row):
    """A row of tokens up to and including its EOS."""
    row = list(row)
    return row[:row.index(MODEL_EOS) + 1] if MODEL_EOS in row else row


def _refs(ans):
    mid = len(ans) // 2
    altered = list(ans)
    altered[mid] = (ans[mid] + 1) % 16384
    return {"answer": list(ans), "none": None, "altered": altered, "short": list(ans[:mid])}


_PLAIN = {}


def _plain(model, o, a, steps, T, weights="bf16"):
    """The grammar decode without jump_forward (tokens, logprobs), computed once per configuration."""
    key = (steps, T, weights)
    if key not in _PLAIN:
        _PLAIN[key] = model.sample_tokens(5, o, max_decoding_steps=steps, decode="fused", grammar=a, return_logprobs=True,
                                          temperature=T, sampler="device", decode_weights=weights)
    return _PLAIN[key]


def _check_all_refs(model, o, a, steps, S, T, weights="bf16"):
    tok, lp = _plain(model, o, a, steps, T, weights)
    row = tok[0].tolist()
    ans = _answer(row)
    q = 0
    for x in ans:                       # the answer is a path of the automaton, to its EOS or to the budget
        q = a.step(q, x)
        assert q >= 0
    assert (ans[-1] == MODEL_EOS and a.accepts(row)) or len(ans) == steps
    kw = dict(max_decoding_steps=steps, decode="fused", grammar=a, jump_forward=S, temperature=T, sampler="device", decode_weights=weights)
    forced = 0
    for name, ref in _refs(ans).items():
        got, glp = model.sample_tokens(5, o, draft_tokens=ref, return_logprobs=True, **kw)
        assert torch.equal(got, tok), (name, got.tolist(), row)
        assert torch.equal(glp.view(torch.int32), lp.view(torch.int32)), (name, (glp - lp).abs().max())
        vs, acc = model.last_spec_stats
        assert (vs, acc) == SP.replay_grammar(row, a, ref, S, steps), name
        assert vs + acc == len(ans) - 1
        if name == "answer":
            assert vs == -(-(len(ans) - 1) // S)
        if name == "none":
            forced = acc
    assert forced > 0                   # the single-edge states alone save passes
    only = model.sample_tokens(5, o, draft_tokens=ans, **kw)     # without log-probabilities: the tokens alone
    assert torch.equal(only, tok)
    return row


@pytest.mark.parametrize("T", [0.0, 0.7])
@pytest.mark.parametrize("S", [2, 4, 8])
@pytest.mark.parametrize("steps", BUDGETS)
def test_jump_forward_returns_the_grammar_decodes_tokens_and_logprobs(ar, steps, S, T):
    _, model, o, a = ar
    row = _check_all_refs(model, o, a, steps, S, T)
    if steps == 13 and T == 0.0:        # the fixture's premise: the answer walks up the chain and ends in the forced EOS
        assert row[:11] == CHAIN[1:11] + [MODEL_EOS] and row[11:] == [0, 0]


def test_jump_forward_on_fp8_weights(ar):
    _, model, o, a = ar
    _check_all_refs(model, o, a, 13, 4, 0.7, weights="fp8")


def test_one_capture_serves_greedy_and_sampled_requests_and_any_reference(ar):
    from lap_amd.serve import GraphedTokenDecoder

    cfg, model, o, a = ar
    steps = 13
    dec = GraphedTokenDecoder(model, 1, steps, prompt_len=cfg.max_token_len, steps_per_replay=3, grammar=a, jump_forward=4,
                              sampling=True, logprobs=True)
    prev = None
    for T, seed, ref_name in ((0.0, 0, "none"), (0.0, 0, "answer"), (0.7, 5, "answer"), (0.7, 5, "altered"), (0.7, 9, "prev"), (0.0, 0, "short")):
        kw = dict(max_decoding_steps=steps, decode="fused", grammar=a, return_logprobs=True, temperature=T, sampler="device")
        tok, lp = model.sample_tokens(seed, o, **kw)
        ref = prev if ref_name == "prev" else _refs(_answer(tok[0].tolist()))[ref_name]
        want = model.sample_tokens(seed, o, jump_forward=4, draft_tokens=ref, **kw)
        stats = model.last_spec_stats
        got = dec(o, temperature=T, seed=seed, draft_tokens=ref)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)), (T, seed, ref_name)
        assert torch.equal(got[0], tok) and torch.equal(got[1].view(torch.int32), lp.view(torch.int32))
        assert dec.last_stats == stats == SP.replay_grammar(tok[0].tolist(), a, ref, 4, steps)
        prev = _answer(tok[0].tolist())
    with pytest.raises(ValueError, match="speculate"):
        GraphedTokenDecoder(model, 1, steps, grammar=a)(o, draft_tokens=[1, 2])


@pytest.mark.parametrize("use_graph", [False, True])
def test_ar_policy_drafts_from_the_previous_answer(ar, use_graph):
    from lap_amd.serve import ARPolicy, Policy

    cfg, model, _, a = ar
    obs, _, _, _ = make_inputs(cfg, B=1, seed=2, ragged=True)
    prompt = obs["tokenized_prompt"][0].numpy().copy()
    prompt[int(np.flatnonzero(obs["tokenized_prompt_mask"][0].numpy()).max())] = CHAIN[0]
    req = {"image": {k: v[0].numpy() for k, v in obs["images"].items()}, "image_mask": {k: np.array(True) for k in obs["images"]},
           "state": obs["state"][0].numpy(), "tokenized_prompt": prompt, "tokenized_prompt_mask": obs["tokenized_prompt_mask"][0].numpy()}
    steps = 13
    base = {"grammar": a, "decode": "fused", "max_decoding_steps": steps, "return_logprobs": True}
    want = ARPolicy(Policy(model, use_graph=False), sample_kwargs=base, use_graph=use_graph).infer(req)
    assert "spec_steps" not in want["policy_timing"]
    pol = ARPolicy(Policy(model, use_graph=False), sample_kwargs=base | {"jump_forward": 4}, use_graph=use_graph)
    assert (pol._decoder is not None) == use_graph
    first, second = pol.infer(req), pol.infer(req)
    ans = _answer(want["tokens"][0].tolist())
    for res in (first, second):
        assert np.array_equal(res["tokens"], want["tokens"])
        assert np.array_equal(res["token_logprobs"].view(np.int32), want["token_logprobs"].view(np.int32))
    t1, t2 = first["policy_timing"], second["policy_timing"]
    assert (t1["spec_steps"], t1["spec_accepted"]) == SP.replay_grammar(want["tokens"][0], a, None, 4, steps)
    assert (t2["spec_steps"], t2["spec_accepted"]) == SP.replay_grammar(want["tokens"][0], a, ans, 4, steps)
    assert 0 < t1["spec_accepted"] < t2["spec_accepted"] and t2["spec_steps"] == -(-(len(ans) - 1) // 4)
    assert pol._prev_tokens.tolist() == ans
