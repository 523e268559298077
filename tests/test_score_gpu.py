"""Teacher-forced scoring (csrc/decode_score.hip, the TARGET LM heads of csrc/decode.hip) and its surface (GPU).

Kernels: a row of the S-row score head holds the single-row LOGP head's bits, the target word is the stored logit of the target,
the finish writes exactly the rows it owns, and the log-probabilities agree with `score.score_reference` on the head's own stored
f32 logits within the bound tests/test_logprob_gpu.py applies to the same quantity (`_bound`: 4x the deviation of a float32
restatement of the reduction from float64).  End to end: scoring the answer of a greedy `return_logprobs=True` decode reproduces
its log-probabilities bit for bit, whatever the number of rows per step.
"""
import numpy as np
import pytest
import torch

from lap_amd import sampling, score as SC
from oracle import lap_oracle as O
from tests.common import make_inputs, oracle_cfg, tiny_sentencepiece_proto, to_observation
from tests.test_logprob_gpu import ORDER_MARGIN, _bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, NH, HD = 2048, 8, 256
V, S4, CAP, PN = 1001, 4, 24, 40
T07 = 0.7


def _state(hip, t, plen=33, done=0):
    st = hip.decode_state(1, DEV)
    st[0], st[1], st[16] = t, done, plen
    return st


def _bf(*shape, scale=1.0, g=None):
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(torch.bfloat16)


def _cand(hip, ids):
    buf = hip.decode_spec_ref(CAP, DEV)
    hip.decode_set_spec_ref(buf, ids)
    return buf


@pytest.fixture(scope="module")
def heads(hip):
    """Seeded random weights, once: the table in the forms the heads stream, the final norm's gamma, S rows of input, a 52-id set."""
    g = torch.Generator(device=DEV).manual_seed(1701)
    table = torch.randn(V, D, generator=g, device=DEV) * 0.03
    hi, lo = hip.split_f32_hilo(table)
    codes, scales = hip.quantize_fp8_rows(table)
    gamma = torch.randn(D, generator=g, device=DEV) * 0.1
    x = _bf(S4, D, g=g)
    ids = torch.sort(torch.randperm(V, generator=torch.Generator().manual_seed(3))[:52]).values.to(torch.int32)
    ids[-1] = V - 1             # the odd vocabulary's last row is in the set
    return {"bf16": (hi, lo, {}), "fp8": (codes, None, {"wscale": scales}), "gamma": gamma, "x": x, "ids": ids.to(DEV)}


def _samp(hip, temperature):
    if not temperature:
        return None
    w = hip.decode_sampling(DEV)
    hip.decode_set_sampling(w, 0, temperature)
    return w


def _score_head(hip, heads, form, cand, t, temperature=0.0, subset=False, rows=S4):
    hi, lo, kw = heads[form]
    kw = dict(kw, ids=heads["ids"]) if subset else dict(kw)
    pval, pidx = hip.decode_lm_partials(rows, DEV)
    pval.fill_(7.0); pidx.fill_(-7)
    plp = hip.decode_lm_logp_partials(rows, DEV).fill_(float("nan"))
    lg = torch.full((rows, V), float("-inf"), device=DEV)
    hip.decode_lm_head_score(_state(hip, t), _samp(hip, temperature), cand, heads["x"][:rows].contiguous(), heads["gamma"], hi, lo,
                             pval, pidx, plp, logits=lg, **kw)
    return pval, pidx, plp, lg


# ------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("temperature", [0.0, T07])
@pytest.mark.parametrize("form, subset", [("bf16", False), ("fp8", False), ("bf16", True)])
def test_head_rows_are_the_single_row_heads_bits(hip, heads, form, subset, temperature):
    """Row r of the S = 4 score head against lap_decode_lm_head_lp at B = 1 on row r's input: pval / pidx are the greedy head's
    (samp = None) at either temperature, and the (m, s) words are those of the LOGP head at the same temperature (at temperature 0
    that is the greedy one).  The target word is the stored f32 logit of the target (times inv_t in float32 at 0.7), present in
    exactly one block; a row whose target lies outside the set, outside [0, V) or past the length has none."""
    t = 5
    allowed = heads["ids"].tolist()
    inside = allowed[7] if subset else 123
    ids = list(range(100, 100 + CAP))
    ids[t], ids[t + 1], ids[t + 2] = inside, (allowed[3] + 1 if subset else V), V - 1
    assert not subset or ids[t + 1] not in allowed
    L = t + 3                                   # row 3's target index t + 3 is the length: no target
    cand = _cand(hip, ids[:L])
    pval, pidx, plp, lg = _score_head(hip, heads, form, cand, t, temperature, subset)
    hi, lo, kw = heads[form]
    kw = dict(kw, ids=heads["ids"]) if subset else dict(kw)
    nb = plp.shape[0]
    pv, pi = pval.view(nb, S4), pidx.view(nb, S4)
    inv_t = np.float32(sampling.inverse_temperature(temperature))
    for r in range(S4):
        xr = heads["x"][r:r + 1].contiguous()
        for samp, words in ((None, "partials"), (_samp(hip, temperature), "lse")):
            p1v, p1i = hip.decode_lm_partials(1, DEV)
            plp1 = hip.decode_lm_logp_partials(1, DEV)
            lg1 = torch.full((1, V), float("-inf"), device=DEV)
            hip.decode_lm_head_lp(_state(hip, t), samp, xr, heads["gamma"], hi, lo, p1v, p1i, plp1, logits=lg1, **kw)
            if words == "partials":
                assert torch.equal(pv[:, r], p1v) and torch.equal(pi[:, r], p1i), r
                assert torch.equal(lg[r], lg1[0]), r
            else:
                assert torch.equal(plp[:, r, :2], plp1[:, 0, :2]), r
        zw = plp[:, r, 2].cpu().numpy()
        assert not np.isnan(zw).any()
        tgt = ids[t + r] if t + r < L else None
        has = tgt is not None and 0 <= tgt < V and (not subset or tgt in allowed)
        assert int(np.isfinite(zw).sum()) == (1 if has else 0), (r, tgt)
        assert np.isneginf(zw[~np.isfinite(zw)]).all()
        if has:
            logit = np.float32(lg[r, tgt].item())
            want = logit if inv_t == 0 else np.float32(logit * inv_t)
            assert zw[np.isfinite(zw)][0] == want, (r, zw[np.isfinite(zw)][0], want)
    assert [r for r in range(S4) if np.isfinite(plp[:, r, 2].cpu().numpy()).any()] == [0, 2]


@pytest.mark.parametrize("left", [1, 3, 4, 9])
def test_finish_writes_its_rows_and_moves_the_state(hip, heads, left):
    """length - t = `left`, S = 4: n = min(4, left) rows of logp / greedy are written at [t, t + n), nothing else; t += n, done =
    (t >= length), steps += 1, extra tokens += n - 1.  The candidate holds the id V (row 0's target) and, where a second row is
    scored, the id -1: both score -inf.  The others agree with float64 on the head's stored logits."""
    L = 14
    t = L - left
    rs = np.random.RandomState(left)
    ids = rs.randint(0, V, size=L).tolist()
    ids[t] = V
    if left >= 2:
        ids[t + 1] = -1
    cand = _cand(hip, ids)
    pval, pidx, plp, lg = _score_head(hip, heads, "bf16", cand, t)
    st = _state(hip, t)
    st[24], st[25] = 3, 7
    logp = torch.full((CAP,), -2.0, device=DEV)
    greedy = torch.full((CAP,), -5, dtype=torch.int32, device=DEV)
    hip.decode_score_finish(st, pval, pidx, plp, cand, logp, greedy, S4)
    torch.cuda.synchronize()
    n = min(S4, left)
    s = st.tolist()
    assert s[0] == t + n and s[1] == int(t + n >= L) and (s[24], s[25]) == (4, 7 + n - 1) and s[16] == 33 and s[8] == 0
    others = [i for i in range(CAP) if not t <= i < t + n]
    assert bool((logp[others] == -2.0).all()) and bool((greedy[others] == -5).all())
    lgn = lg.cpu().numpy()
    want_lp, want_gr = SC.score_reference(lgn[:n], ids[t:t + n])
    got = logp[t:t + n].cpu().numpy().astype(np.float64)
    assert greedy[t:t + n].tolist() == want_gr.tolist()
    assert np.isneginf(got[0]) and np.isneginf(want_lp[0])
    if n >= 2:
        assert np.isneginf(got[1]) and np.isneginf(want_lp[1])
    fin = np.isfinite(want_lp)
    assert fin.sum() == max(0, n - 2) and (np.isfinite(got) == fin).all()
    bound = _bound(lgn[:n], 0.0)
    err = np.abs(got[fin] - want_lp[fin])
    print(f"left {left}: |device - float64| {err.max() if err.size else 0.0:.3e}, bound {bound:.3e} (= {ORDER_MARGIN} x float32 restatement)")
    assert (err <= bound).all()
    # t >= length on entry: done, nothing else
    st2 = _state(hip, L)
    before = (logp.clone(), greedy.clone())
    hip.decode_score_finish(st2, pval, pidx, plp, cand, logp, greedy, S4)
    assert st2.tolist()[:2] == [L, 1] and torch.equal(logp, before[0]) and torch.equal(greedy, before[1])


@pytest.mark.parametrize("form, subset, temperature", [("bf16", False, 0.0), ("bf16", False, T07), ("fp8", False, 0.0), ("bf16", True, T07)])
def test_logp_against_float64_on_the_heads_own_logits(hip, heads, form, subset, temperature):
    t = 3
    rs = np.random.RandomState(17)
    allowed = heads["ids"].cpu().numpy() if subset else None
    ids = rs.choice(allowed if subset else np.arange(V), size=CAP).tolist()
    cand = _cand(hip, ids)
    pval, pidx, plp, lg = _score_head(hip, heads, form, cand, t, temperature, subset)
    logp = torch.zeros(CAP, device=DEV)
    greedy = torch.zeros(CAP, dtype=torch.int32, device=DEV)
    hip.decode_score_finish(_state(hip, t), pval, pidx, plp, cand, logp, greedy, S4)
    lgn = lg.cpu().numpy()
    want_lp, want_gr = SC.score_reference(lgn, ids[t:t + S4], temperature=temperature, allowed=allowed)
    got = logp[t:t + S4].cpu().numpy().astype(np.float64)
    bound = _bound(lgn, temperature, allowed)
    err = np.abs(got - want_lp)
    print(f"{form} subset {subset} T {temperature}: logp {got.tolist()}, |device - float64| {err.max():.3e}, bound {bound:.3e}")
    assert np.isfinite(got).all() and (got <= 0).all() and (err <= bound).all()
    assert greedy[t:t + S4].tolist() == want_gr.tolist()


def test_done_state_writes_nothing(hip, heads):
    g = torch.Generator(device=DEV).manual_seed(13)
    st = _state(hip, 3, 20, done=1)
    st[24], st[25] = 5, 6
    st0 = st.clone()
    cand = _cand(hip, list(range(10, 20)))
    x = _bf(S4, D, g=g)
    x0 = x.clone()
    table = torch.randn(64, D, generator=g, device=DEV)
    hip.decode_score_embed(st, table, 0, 64, cand, x, 45.25)
    hi, lo, _ = heads["bf16"]
    pval, pidx = hip.decode_lm_partials(S4, DEV)
    pval.fill_(3.0); pidx.fill_(11)
    plp = hip.decode_lm_logp_partials(S4, DEV).fill_(9.0)
    lg = torch.full((S4, V), 5.0, device=DEV)
    logp = torch.full((CAP,), -2.0, device=DEV)
    greedy = torch.full((CAP,), -5, dtype=torch.int32, device=DEV)
    for kw in ({}, {"ids": heads["ids"]}):
        hip.decode_lm_head_score(st, _samp(hip, T07), cand, x, heads["gamma"], hi, lo, pval, pidx, plp, logits=lg, **kw)
    codes, _, kw8 = heads["fp8"]
    hip.decode_lm_head_score(st, None, cand, x, heads["gamma"], codes, None, pval, pidx, plp, logits=lg, **kw8)
    hip.decode_score_finish(st, pval, pidx, plp, cand, logp, greedy, S4)
    torch.cuda.synchronize()
    assert torch.equal(st, st0) and torch.equal(x, x0)
    assert bool((pval == 3.0).all()) and bool((pidx == 11).all()) and bool((plp == 9.0).all()) and bool((lg == 5.0).all())
    assert bool((logp == -2.0).all()) and bool((greedy == -5).all())


def test_embed_rows_follow_the_candidate(hip):
    """Row r is lap_decode_embed's row for ids[t-1+r]; a row at or past the length, and an id outside the table, are zero."""
    g = torch.Generator(device=DEV).manual_seed(5)
    table = torch.randn(64, D, generator=g, device=DEV)
    ids = [3, 70, 9, 12, 5]
    cand = _cand(hip, ids)
    t = 2                                       # rows feed ids[1] = 70 (outside the table), ids[2], ids[3], ids[4]; at t = 4: two past the end
    for t, fed in ((2, [70, 9, 12, 5]), (4, [12, 5, None, None])):
        x = _bf(S4, D, g=g)
        hip.decode_score_embed(_state(hip, t), table, 0, 64, cand, x, 45.25)
        for r, tok in enumerate(fed):
            if tok is None or tok >= 64:
                assert float(x[r].float().abs().sum()) == 0.0, (t, r)
                continue
            out = torch.zeros(1, CAP, dtype=torch.int32, device=DEV)
            out[0, 0] = tok
            x1 = torch.zeros(1, D, dtype=torch.bfloat16, device=DEV)
            hip.decode_embed(_state(hip, 1), table, 0, 64, out, x1, 45.25)
            assert torch.equal(x[r], x1[0]) and float(x1.float().abs().sum()) > 0, (t, r)


# ---------------------------------------------------------------------------------------------------------------- model
def _gemma2b_x2_cfg(mp, **kw):
    """tests/test_speculate_gpu.py::_gemma2b_x2_cfg: LAP-3B widths with 2 layers per tower and a 16k vocabulary."""
    from lap_amd import config as C
    from lap_amd.config import LAPConfig

    mp.setitem(C._GEMMA, "gemma_2b_x2", C.GemmaConfig(2048, 2, 16384, 8, 1, 256))
    mp.setitem(C._GEMMA, "gemma_300m_x2", C.GemmaConfig(1024, 2, 4096, 8, 1, 256))
    mp.setitem(C._SIGLIP, "So400m/14_x2", C.SiglipConfig(1152, 2, 4304, 16))
    mp.setitem(O.GEMMA, "gemma_2b_x2", O.GemmaCfg(2048, 2, 16384, 8, 1, 256))
    mp.setitem(O.GEMMA, "gemma_300m_x2", O.GemmaCfg(1024, 2, 4096, 8, 1, 256))
    mp.setitem(O.SIGLIP, "So400m/14_x2", O.SiglipCfg(1152, 2, 4304, 16))
    base = dict(paligemma_variant="gemma_2b_x2", action_expert_variant="gemma_300m_x2", siglip_variant="So400m/14_x2",
                image_size=224, vocab_size=16384, action_dim=32, action_horizon=50, max_token_len=48,
                language_loss_weight=0.4, enable_image_augmentation=False, enable_action_training=True)
    return LAPConfig(**(base | kw))


ANSWER = "move left 5 cm and up 3"      # its tokens under the tiny tokenizer are all different (the chain below needs that)
OTHER = "pick up the block"
C0 = 16000                              # the prompt's last token, the start of the chain


def _tokenizer():
    from lap_amd import policy_io as pio

    return pio.PaligemmaTokenizer(model_proto=tiny_sentencepiece_proto(), max_len=48)


def _chain_params(cfg, chain):
    """tests/test_speculate_gpu.py::_chain_params: the embedding rows of `chain` are built so that the greedy successor of
    chain[i] is chain[i + 1] (randomly initialised weights would repeat one token)."""
    P = O.init_params(oracle_cfg(cfg), seed=13)
    E = torch.as_tensor(P["PaliGemma/llm/embedder/input_embedding"]).clone()
    gamma = torch.as_tensor(P["PaliGemma/llm/final_norm/scale"]).clone()
    s, A = 4.0, 1.0
    for i, tok in enumerate(chain):
        b = 0.5 + 0.15 * i
        row = torch.zeros(E.shape[1])
        row[2 * i], row[2 * i + 1], row[2 * i + 2] = s * A, s * (A * A + b * b) ** 0.5, s * b
        E[tok] = row
        gamma[2 * i + 1] = -2.0
    gamma[[2 * i for i in range(len(chain) + 1)]] = 0.0
    P["PaliGemma/llm/embedder/input_embedding"] = E
    P["PaliGemma/llm/final_norm/scale"] = gamma
    return P


@pytest.fixture(scope="module")
def ar(hip):
    """(cfg, model, observation of batch 1, the greedy answer's ids, the same observation as a policy request).  The prompt ends in C0 and the chain is C0 -> the tokens of
    ANSWER -> EOS, so the greedy answer is ANSWER's tokens and the EOS (the fixture's own premise, asserted here)."""
    from lap_amd.model import LAP

    ids = list(_tokenizer().encode(ANSWER))
    with pytest.MonkeyPatch.context() as mp:
        cfg = _gemma2b_x2_cfg(mp)
        eos = LAP.EOS_TOKEN
        chain = [C0] + ids + [eos]
        assert len(set(chain)) == len(chain) and len(ids) >= 8
        model = LAP(cfg, params=_chain_params(cfg, chain), device=DEV)
        obs, _, _, _ = make_inputs(cfg, B=1, ragged=True)
        so = dict(obs)
        so.pop("tokenized_langact_mask")
        so["image_masks"] = {k: torch.ones_like(m) for k, m in so["image_masks"].items()}
        last = int(torch.nonzero(so["tokenized_prompt_mask"][0]).max())
        so["tokenized_prompt"] = so["tokenized_prompt"].clone()
        so["tokenized_prompt"][0, last] = C0
        o = to_observation(so | {"tokenized_langact_mask": None}, DEV)
        T = model.sample_tokens(0, o, max_decoding_steps=13, decode="fused")[0].tolist()
        assert T[:len(ids) + 1] == ids + [eos], (T, ids)
        req = {"image": {k: v[0].numpy() for k, v in so["images"].items()}, "image_mask": {k: np.array(True) for k in so["images"]},
               "state": so["state"][0].numpy(), "tokenized_prompt": so["tokenized_prompt"][0].numpy(),
               "tokenized_prompt_mask": so["tokenized_prompt_mask"][0].numpy()}
        yield cfg, model, o, ids + [eos], req


def _allowed52(answer):
    rs = np.random.RandomState(2)
    rest = [int(i) for i in rs.choice(15000, size=52 - len(answer), replace=False) + 200]
    return sorted(set(answer) | set(rest))


@pytest.mark.parametrize("weights, constrained", [("bf16", False), ("fp8", False), ("bf16", True)])
def test_scoring_a_greedy_answer_reproduces_its_logprobs(ar, weights, constrained):
    """Decode with return_logprobs=True, then score the answer (up to and including its EOS) with S = 1, 2, 4, 8 rows per step:
    `logp` is the decoder's, bit for bit, and `greedy` is the answer itself."""
    _, model, o, answer, _ = ar
    allowed = _allowed52(answer) if constrained else None
    assert allowed is None or len(allowed) == 52
    tok, lp = model.sample_tokens(0, o, max_decoding_steps=13, decode="fused", return_logprobs=True, decode_weights=weights,
                                  allowed_tokens=allowed)
    row = tok[0].tolist()
    n = row.index(model.EOS_TOKEN) + 1 if model.EOS_TOKEN in row else len(row)
    assert n >= 9 and float(lp[0, :n].abs().sum()) > 0
    for S in (1, 2, 4, 8):
        res = model.score_tokens(o, row[:n], rows=S, decode_weights=weights, allowed_tokens=allowed, max_decoding_steps=13)
        assert len(res.logp) == 1 and res.logp[0].dtype == torch.float32 and res.greedy[0].dtype == torch.int32
        assert torch.equal(res.logp[0], lp[0, :n]), (S, res.logp[0], lp[0, :n])
        assert res.greedy[0].tolist() == row[:n], S
        assert torch.equal(res.total, res.logp[0].sum().view(1))


def test_any_candidate_any_rows(ar):
    """A candidate of length 13 that is no greedy answer (random ids, one of them the id 0 that this model never picks, a stretch of
    the chain in the middle): the S = 1, 2, 4, 8 vectors are equal (a row does not depend on the rows beside it), and they agree
    with `score_reference` on the f32 logits of an eagerly launched teacher-forced pass (one position per step, the head's stored
    logits collected after every launch) within test_logprob_gpu's bound."""
    from lap_amd import ar_decode

    cfg, model, o, answer, _ = ar
    rs = np.random.RandomState(31)
    cand = rs.randint(2, cfg.vocab_size, size=13).tolist()
    cand[2] = 0
    cand[5:9] = answer[1:5]
    assert cand[:len(answer)] != answer[:13]
    res = {S: model.score_tokens(o, cand, rows=S, max_decoding_steps=13) for S in (1, 2, 4, 8)}
    for S in (2, 4, 8):
        assert torch.equal(res[S].logp[0], res[1].logp[0]) and torch.equal(res[S].greedy[0], res[1].greedy[0]), S
    with model._serving_weights():
        pre = ar_decode.prefill(model, o)
        ctx = ar_decode.DecodeCtx(model, 1, pre.Pn, 13, score=1)
        ctx.set_candidate(cand)
        lg = torch.empty((1, cfg.vocab_size), dtype=torch.float32, device=DEV)
        rows = []
        ctx.first_token(pre, lg)
        rows.append(lg[0].clone())
        for _ in range(12):
            ctx.step(lg)
            rows.append(lg[0].clone())
        assert ctx.state[:2].tolist() == [13, 1] and ctx.stats() == (13, 0)
    lgn = torch.stack(rows).cpu().numpy()
    want_lp, want_gr = SC.score_reference(lgn, cand)
    got = res[4].logp[0].cpu().numpy().astype(np.float64)
    bound = _bound(lgn, 0.0)
    err = np.abs(got - want_lp)
    print(f"candidate logp {got.tolist()}, |device - float64| {err.max():.3e}, bound {bound:.3e}")
    assert np.isfinite(got).all() and (err <= bound).all()
    assert res[4].greedy[0].tolist() == want_gr.tolist()


def test_many_candidates_share_one_prefill(ar, monkeypatch):
    from lap_amd import ar_decode

    cfg, model, o, answer, _ = ar
    rs = np.random.RandomState(41)
    cands = [[answer[0]], answer[:3] + rs.randint(2, 9000, size=2).tolist(), rs.randint(2, cfg.vocab_size, size=CAP).tolist()]
    assert [len(c) for c in cands] == [1, 5, CAP]
    calls = []
    real = ar_decode.prefill
    monkeypatch.setattr(ar_decode, "prefill", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    res = model.score_tokens(o, cands, rows=4, max_decoding_steps=CAP)
    assert len(calls) == 1 and res.total.shape == (3,) and [t.numel() for t in res.logp] == [1, 5, CAP]
    for i, c in enumerate(cands):
        one = model.score_tokens(o, c, rows=4, max_decoding_steps=CAP)
        assert torch.equal(one.logp[0], res.logp[i]) and torch.equal(one.greedy[0], res.greedy[i]), i
        assert torch.equal(one.total[0], res.total[i])
    assert len(calls) == 4
    with pytest.raises(ValueError, match="length 25"):
        model.score_tokens(o, list(range(25)), max_decoding_steps=CAP)
    assert len(calls) == 4                      # (checked before any device work)


def test_ar_policy_score(ar):
    """Two answer strings, one of which the policy itself generates greedily: that one has token accuracy 1 and wins under "mean"."""
    from lap_amd.serve import ARPolicy, Policy

    _, model, o, answer, req = ar
    tok = _tokenizer()
    pol = ARPolicy(Policy(model, use_graph=False), sample_kwargs={"max_decoding_steps": 13}, tokenizer=tok)
    own = pol.infer(req)
    row = np.asarray(own["tokens"])[0].tolist()
    assert row[:len(answer)] == answer and tok.decode(answer[:-1]) == ANSWER      # the policy's own greedy answer is ANSWER
    r = pol.score(req, [OTHER, ANSWER], select="mean")
    assert r["tokens"][1].tolist() == answer and r["tokens"][0].tolist() == list(tok.encode(OTHER)) + [model.EOS_TOKEN]
    assert r["token_accuracy"][1] == 1.0 and r["token_accuracy"][0] < 1.0
    assert r["best"] == 1 and r["logp_mean"][1] > r["logp_mean"][0] and "infer_ms" in r["policy_timing"]
    np.testing.assert_allclose(r["logp_sum"][1], r["token_logprobs"][1].astype(np.float64).sum(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(r["logp_mean"], r["logp_sum"] / np.array([len(t) for t in r["tokens"]]), rtol=0, atol=1e-12)
    ids = pol.score(req, [r["tokens"][0], answer], select="sum")               # id sequences are taken as they are
    np.testing.assert_array_equal(ids["logp_sum"], r["logp_sum"])
    with pytest.raises(ValueError, match="select must be 'sum' or 'mean', got 'max'"):
        pol.score(req, [ANSWER], select="max")
