"""Exact speculative decoding (csrc/decode_spec.hip, the *_spec_* instances of csrc/decode.hip) and its surface (GPU).

Every comparison here is exact.  The verify step's rows run the arithmetic of the single-row kernels (the accumulation of a row
does not depend on the batch width), so the QKV and attention variants are compared bit for bit with the plain kernels at
state[0] = t + r, the draft and accept kernels with lap_amd/speculate.py, and a speculating decode with the plain fused decode by
torch.equal, whatever the draft.
"""
import numpy as np
import pytest
import torch

from lap_amd import speculate as SP
from oracle import lap_oracle as O
from tests.common import make_inputs, oracle_cfg, to_observation
from tests.test_speculate_cpu import ACCEPT_CASES, DRAFT_CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
D, NH, HD, H = 2048, 8, 256, 16384
PN, CAP = 40, 24                # Pn is no multiple of the 16-key chunk; cap = 24 leaves a half-filled last chunk


def _state(hip, t, plen, done=0):
    st = hip.decode_state(1, DEV)
    st[0], st[1], st[16] = t, done, plen
    return st


def _bf(*shape, scale=1.0, g=None):
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(torch.bfloat16)


# ------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("t", [15, 23, 24])
def test_qkv_rows_are_the_plain_kernels_bits(hip, t, fp8):
    """Row r of the S = 4 variant against lap_decode_qkv at state[0] = t + r with row r's input: q row r and cache row t-1+r.  At
    t = 23 and 24 rows run past cap = 24: the plain kernel writes nothing at t + r > cap, and the variant must leave the same
    bytes (q row included) as they were."""
    S, plen = 4, 33
    g = torch.Generator(device=DEV).manual_seed(11)
    x = _bf(S, D, g=g)
    gamma = torch.randn(D, generator=g, device=DEV) * 0.1
    w = _bf((NH + 2) * HD, D, scale=0.02, g=g)
    kw = {}
    if fp8:
        w, scales = hip.quantize_fp8_rows(w)
        kw = {"wscale": scales}
    ck0, cv0, q0 = _bf(1, CAP, HD, g=g), _bf(1, CAP, HD, g=g), _bf(S, NH * HD, g=g)
    ck, cv, q = ck0.clone(), cv0.clone(), q0.clone()
    hip.decode_spec_qkv(_state(hip, t, plen), x, gamma, w, q, ck, cv, NH, HD, HD ** -0.5, **kw)
    ckp, cvp, qp = ck0.clone(), cv0.clone(), q0.clone()
    for r in range(S):
        qr = q0[r:r + 1].clone()
        hip.decode_qkv(_state(hip, t + r, plen), x[r:r + 1].contiguous(), gamma, w, qr, ckp, cvp, NH, HD, HD ** -0.5, **kw)
        qp[r] = qr[0]
    written = [r for r in range(S) if t - 1 + r < CAP]
    assert written == list(range(S))[:CAP - t + 1]
    for r in written:       # (the plain kernel did write: the comparison below is not of two untouched buffers)
        assert not torch.equal(ckp[0, t - 1 + r], ck0[0, t - 1 + r]) and not torch.equal(qp[r], q0[r])
    assert torch.equal(q, qp) and torch.equal(ck, ckp) and torch.equal(cv, cvp)
    for r in range(S):
        if r not in written:
            assert torch.equal(q[r], q0[r])
    rows = [t - 1 + r for r in written]
    others = [r for r in range(CAP) if r not in rows]
    assert torch.equal(ck[:, others], ck0[:, others]) and torch.equal(cv[:, others], cv0[:, others])


@pytest.mark.parametrize("t", [15, 23, 24])
def test_attention_rows_are_the_plain_kernels_bits(hip, t):
    """Row r's partials (o and lse of every chunk) and output against lap_decode_attention at state[0] = t + r, B = 1.  t = 15:
    rows 0, 1 end in the first generated chunk, rows 2, 3 reach into the second."""
    S = 4
    g = torch.Generator(device=DEV).manual_seed(12)
    q = _bf(S, NH * HD, scale=HD ** -0.5, g=g)
    pk, pv = _bf(PN, HD, g=g), _bf(PN, HD, g=g)
    gk, gv = _bf(1, CAP, HD, g=g), _bf(1, CAP, HD, g=g)
    ok = torch.rand(1, PN, generator=g, device=DEV) < 0.8
    ok[:, :3] = False
    kinfo = (ok.to(torch.int32) << 24).contiguous()
    nchunk = (PN + 15) // 16 + (CAP + 15) // 16
    o = torch.zeros(S, NH * HD, dtype=torch.bfloat16, device=DEV)
    scr = hip.decode_attn_scratch(S, PN, CAP, DEV).zero_()
    hip.decode_spec_attention(_state(hip, t, PN), q, pk, pv, kinfo, PN, gk, gv, o, scr, NH, 1, HD)
    no = nchunk * NH * HD
    op, lp = scr[:S * no].view(S, no), scr[S * no:S * no + S * nchunk * NH].view(S, nchunk * NH)
    for r in range(S):
        o1 = torch.zeros(1, NH * HD, dtype=torch.bfloat16, device=DEV)
        s1 = hip.decode_attn_scratch(1, PN, CAP, DEV).zero_()
        hip.decode_attention(_state(hip, t + r, PN), q[r:r + 1].contiguous(), pk, pv, kinfo, PN, gk, gv, o1, s1, NH, 1, HD)
        assert torch.equal(op[r], s1[:no]), r
        assert torch.equal(lp[r], s1[no:no + nchunk * NH]), r
        assert torch.equal(o[r], o1[0]), r
    assert float(o.float().abs().sum()) > 0
    if t == 15:         # the rows differ in their key counts: row 2 sees key 16, row 1 does not
        assert not torch.equal(lp[1].view(nchunk, NH)[-1], lp[2].view(nchunk, NH)[-1])


def test_done_state_writes_nothing(hip):
    S = 4
    g = torch.Generator(device=DEV).manual_seed(13)
    st = _state(hip, 3, 20, done=1)
    st[24], st[25] = 5, 6
    st0 = st.clone()
    out = torch.randint(0, 9, (1, CAP), dtype=torch.int32, device=DEV)
    bufs = dict(x=_bf(S, D, g=g), q=_bf(S, NH * HD, g=g), o=_bf(S, NH * HD, g=g), ck=_bf(1, CAP, HD, g=g), cv=_bf(1, CAP, HD, g=g),
                out=out, draft=torch.full((S - 1,), 77, dtype=torch.int32, device=DEV))
    before = {k: v.clone() for k, v in bufs.items()}
    ref = hip.decode_spec_ref(CAP, DEV)
    hip.decode_set_spec_ref(ref, out[0].tolist())
    gamma = torch.ones(D, device=DEV)
    table = torch.randn(64, D, generator=g, device=DEV)
    hip.decode_spec_draft(st, ref, bufs["out"], bufs["draft"])
    hip.decode_spec_embed(st, table, 0, 64, bufs["out"], bufs["draft"], bufs["x"], 45.25)
    hip.decode_spec_qkv(st, bufs["x"], gamma, _bf((NH + 2) * HD, D, g=g), bufs["q"], bufs["ck"], bufs["cv"], NH, HD, HD ** -0.5)
    hip.decode_spec_attention(st, bufs["q"], _bf(PN, HD, g=g), _bf(PN, HD, g=g), torch.full((1, PN), 1 << 24, dtype=torch.int32, device=DEV),
                              PN, bufs["ck"], bufs["cv"], bufs["o"], hip.decode_attn_scratch(S, PN, CAP, DEV), NH, 1, HD)
    pval, pidx = hip.decode_lm_partials(S, DEV)
    pval.fill_(1.0)
    pidx.fill_(3)
    hip.decode_spec_accept(st, pval, pidx, bufs["draft"], bufs["out"], eos_token=1)
    torch.cuda.synchronize()
    assert torch.equal(st, st0)
    for k, v in bufs.items():
        assert torch.equal(v, before[k]), k


def _random_cases(seed, n=50, vocab=8):
    rs = np.random.RandomState(seed)
    for _ in range(n):
        S = int(rs.randint(2, 9))
        t = int(rs.randint(1, CAP + 1))
        yield rs, S, t, rs.randint(0, vocab, size=int(rs.randint(0, CAP + 1))).tolist(), rs.randint(0, vocab, size=CAP).tolist()


def test_draft_kernel_matches_the_numpy_rule(hip):
    cases = [(ref, out, t, S) for _, ref, out, t, S, _ in DRAFT_CASES]
    cases += [(ref, out, t, S) for _, S, t, ref, out in _random_cases(5)]
    refbuf = hip.decode_spec_ref(CAP, DEV)
    hits = 0
    for ref, out, t, S in cases:
        o = torch.zeros(1, CAP, dtype=torch.int32, device=DEV)
        o[0, :t] = torch.tensor(list(out[:t]), dtype=torch.int32)
        o[0, t:] = 5                    # (a vocabulary id: what lies beyond t must not be read as a token)
        hip.decode_set_spec_ref(refbuf, ref)
        draft = torch.full((S - 1,), -7, dtype=torch.int32, device=DEV)
        hip.decode_spec_draft(_state(hip, t, 9), refbuf, o, draft)
        want = SP.draft_tokens(ref, o[0].tolist(), t, S)
        assert draft.tolist() == want.tolist(), (ref, out, t, S)
        hits += int(want[0] >= 0)
    assert hits > len(cases) // 2       # the cases do draft
    for _, ref, out, t, S, want in DRAFT_CASES:     # (the hand-worked expectations themselves, through the kernel)
        o = torch.zeros(1, CAP, dtype=torch.int32, device=DEV)
        o[0, :t] = torch.tensor(list(out[:t]), dtype=torch.int32)
        hip.decode_set_spec_ref(refbuf, ref)
        draft = torch.full((S - 1,), -7, dtype=torch.int32, device=DEV)
        hip.decode_spec_draft(_state(hip, t, 9), refbuf, o, draft)
        assert draft.tolist() == want
    # a reference longer than the capacity is truncated to it
    hip.decode_set_spec_ref(refbuf, list(range(100, 100 + 2 * CAP)))
    assert refbuf[:3].tolist() == [CAP, 100, 101] and int(refbuf[CAP]) == 100 + CAP - 1


def _partials(hip, rs, toks, S):
    """pval / pidx [blocks][S] whose argmax of row r is toks[r]: the best value sits in one block with index toks[r] and, a tie
    across blocks, in another block with a higher index; every other block holds a lower value or the neutral partial."""
    nb = hip._fn["lap_decode_lm_blocks"]()
    pval = np.full((nb, S), -np.inf, np.float32)
    pidx = np.full((nb, S), 0x7fffffff, np.int32)
    for r in range(S):
        blocks = rs.choice(nb, size=6, replace=False)
        pval[blocks[2:], r] = rs.uniform(-3.0, 4.0, size=4).astype(np.float32)
        pidx[blocks[2:], r] = rs.randint(0, 1 << 18, size=4)
        hi, lo = (blocks[0], blocks[1]) if rs.rand() < 0.5 else (blocks[1], blocks[0])      # the tie's winner in the later or the earlier block
        pval[hi, r], pidx[hi, r] = 5.0, toks[r]
        pval[lo, r], pidx[lo, r] = 5.0, toks[r] + 1 + int(rs.randint(0, 1000))
    return torch.from_numpy(pval).to(DEV).reshape(-1), torch.from_numpy(pidx).to(DEV).reshape(-1)


def test_accept_kernel_matches_the_numpy_rule(hip):
    rs = np.random.RandomState(7)
    cases = [(tok, draft, t, cap, eos) for _, tok, draft, t, cap, eos, _ in ACCEPT_CASES]
    for r2, S, t, _, _ in _random_cases(9):
        tok = r2.randint(0, 8, size=S)
        draft = np.where(r2.rand(S - 1) < 0.7, tok[:-1], r2.randint(0, 8, size=S - 1))       # mostly right drafts
        cases.append((tok.tolist(), draft.tolist(), min(t, CAP), CAP, 1))
    ns = []
    for tok, draft, t, cap, eos in cases:
        S = len(tok)
        pval, pidx = _partials(hip, rs, tok, S)
        st = _state(hip, t, 9)
        st[24], st[25] = 3, 7
        out0 = torch.randint(10, 20, (1, cap), dtype=torch.int32, device=DEV)
        out = out0.clone()
        hip.decode_spec_accept(st, pval, pidx, torch.tensor(draft, dtype=torch.int32, device=DEV), out, eos)
        e = SP.accept(tok, draft, t, cap, eos)
        n = len(e)
        ns.append(n)
        want = out0.clone()
        if n:
            want[0, t:t + n] = torch.from_numpy(e).to(DEV)
        assert torch.equal(out, want), (tok, draft, t, cap)
        s = st.tolist()
        if n == 0:      # t >= cap on entry: done, nothing else
            assert s[0] == t and s[1] == 1 and s[8] == 0 and (s[24], s[25]) == (3, 7)
            continue
        saw_eos = int(eos in e.tolist())
        assert s[0] == t + n and s[8] == saw_eos and s[1] == int(t + n >= cap or saw_eos), (tok, draft, t, cap, s[:9])
        assert (s[24], s[25]) == (4, 7 + n - 1) and s[16] == 9
    assert len(set(ns)) >= 5        # every acceptance length up to a few rows occurs


# ---------------------------------------------------------------------------------------------------------------- model
def _gemma2b_x2_cfg(mp, **kw):
    """tests/test_ar_decode_gpu.py::_gemma2b_x2_cfg: LAP-3B widths with 2 layers per tower and a 16k vocabulary."""
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


BUDGETS = (13, 5)
CHAIN = [16000 + 3 * i for i in range(20)]      # token ids of the chain below


def _chain_params(cfg):
    """Randomly initialised weights echo the last token (the LM head is tied to the embedding table, and the residual stream of
    two layers stays close to the embedded token), so their greedy answer is one repeated token, on which every draft is right.
    The drafts here need an answer that varies, so the table gets a chain of rows c_0 -> c_1 -> ..: with the final norm's
    multiplier 1 + gamma = -1 on the dims m_i the logit of row j after token c_i is close to the indefinite form B(c_i, c_j) =
    sum_d (1 + gamma_d) c_i[d] c_j[d], and with
        c_i = s (A e[p_i] + sqrt(A^2 + b_i^2) e[m_i] + b_i e[p_{i+1}]),  p_i = 2 i, m_i = 2 i + 1,
    B(c_i, c_i) = 0, B(c_i, c_{i+1}) = s^2 A b_i, B(c_i, c_{i-1}) = s^2 A b_{i-1} and 0 for every other pair; b_i grows with i,
    so the successor wins.  s = 4 lifts the rows over the layers' contribution to the residual stream."""
    P = O.init_params(oracle_cfg(cfg), seed=13)
    E = torch.as_tensor(P["PaliGemma/llm/embedder/input_embedding"]).clone()
    gamma = torch.as_tensor(P["PaliGemma/llm/final_norm/scale"]).clone()
    s, A = 4.0, 1.0
    for i, tok in enumerate(CHAIN):
        b = 0.5 + 0.15 * i
        row = torch.zeros(E.shape[1])
        row[2 * i], row[2 * i + 1], row[2 * i + 2] = s * A, s * (A * A + b * b) ** 0.5, s * b
        E[tok] = row
        gamma[2 * i + 1] = -2.0
    gamma[[2 * i for i in range(len(CHAIN) + 1)]] = 0.0
    P["PaliGemma/llm/embedder/input_embedding"] = E
    P["PaliGemma/llm/final_norm/scale"] = gamma
    return P


@pytest.fixture(scope="module")
def ar(hip):
    """(cfg, model, observation of batch 1, {budget: the plain fused decode's tokens}); no row stops early (EOS_TOKEN = -1).  The
    prompt ends in c_0 of the chain, so the answer walks up the chain: its tokens are all different."""
    from lap_amd.model import LAP

    with pytest.MonkeyPatch.context() as mp:
        cfg = _gemma2b_x2_cfg(mp)
        model = LAP(cfg, params=_chain_params(cfg), device=DEV)
        model.EOS_TOKEN = -1
        obs, _, _, _ = make_inputs(cfg, B=1, ragged=True)
        so = dict(obs)
        so.pop("tokenized_langact_mask")
        so["image_masks"] = {k: torch.ones_like(m) for k, m in so["image_masks"].items()}
        last = int(torch.nonzero(so["tokenized_prompt_mask"][0]).max())
        so["tokenized_prompt"] = so["tokenized_prompt"].clone()
        so["tokenized_prompt"][0, last] = CHAIN[0]
        o = to_observation(so | {"tokenized_langact_mask": None}, DEV)
        T = {n: model.sample_tokens(0, o, max_decoding_steps=n, decode="fused") for n in BUDGETS}
        assert len(set(T[13][0].tolist())) >= 8, T[13][0].tolist()      # (the fixture's own premise: the answer varies)
        yield cfg, model, o, T
        model.EOS_TOKEN = 1


def _drafts(T):
    """name -> reference sequence, from the answer T (a list)."""
    mid = len(T) // 2
    altered = list(T)
    altered[mid] = (T[mid] + 1) % 16384
    return {"answer": list(T), "none": None, "altered": altered, "shifted": [(T[0] + 7) % 16384] + list(T), "short": list(T[:mid])}


@pytest.mark.parametrize("S", [2, 4, 8])
@pytest.mark.parametrize("steps", BUDGETS)
def test_speculating_decode_returns_the_plain_tokens(ar, steps, S):
    _, model, o, Ts = ar
    T = Ts[steps]
    row = T[0].tolist()
    assert len(set(row)) > 2        # the answer is no single repeated token
    for name, ref in _drafts(row).items():
        got = model.sample_tokens(0, o, max_decoding_steps=steps, decode="fused", speculate=S, draft_tokens=ref)
        assert torch.equal(got, T), (name, got.tolist(), row)
        vs, acc = model.last_spec_stats
        assert (vs, acc) == SP.replay(row, ref, S, steps, model.EOS_TOKEN), name
        if name == "answer":        # full acceptance: len - 1 tokens after the first, S per step
            assert vs == -(-(steps - 1) // S) and acc == steps - 1 - vs
        if name == "none":          # one token per step, the price of a wrong guess
            assert vs == steps - 1 and acc == 0
        if name == "shifted":       # the n-gram anchor recovers the shift: as many steps as under the answer itself, or one more
            assert vs <= -(-(steps - 1) // S) + 1
        assert vs + acc == steps - 1


def test_eos_inside_an_accepted_block(ar):
    _, model, o, Ts = ar
    steps, S = 13, 4
    row = Ts[steps][0].tolist()
    # a token whose first occurrence is row 1 or 2 of a verify step under full acceptance (the steps emit out[1 .. 4], out[5 .. 8], ..)
    k = next(k for k in range(2, steps - 1) if row.index(row[k]) == k and (k - 1) % S in (1, 2))
    model.EOS_TOKEN = row[k]
    try:
        ref = model.sample_tokens(0, o, max_decoding_steps=steps, decode="fused")
        got = model.sample_tokens(0, o, max_decoding_steps=steps, decode="fused", speculate=S, draft_tokens=row)
        stats = model.last_spec_stats
    finally:
        model.EOS_TOKEN = -1
    assert ref[0, :k + 1].tolist() == row[:k + 1] and int(ref[0, k + 1:].abs().sum()) == 0
    assert torch.equal(got, ref)
    assert stats == SP.replay(ref[0].tolist(), row, S, steps, row[k]) == (-(-k // S), k - -(-k // S))


@pytest.mark.parametrize("kw", [{"decode_weights": "fp8"}, {"allowed_tokens": sorted(set(range(0, 16384, 37)) | set(CHAIN))}], ids=["fp8", "allowed"])
def test_compositions(ar, kw):
    _, model, o, _ = ar
    steps, S = 13, 4
    T = model.sample_tokens(0, o, max_decoding_steps=steps, decode="fused", **kw)
    row = T[0].tolist()
    if "allowed_tokens" in kw:
        assert set(row) <= set(kw["allowed_tokens"])
    for ref in (row, None):
        got = model.sample_tokens(0, o, max_decoding_steps=steps, decode="fused", speculate=S, draft_tokens=ref, **kw)
        assert torch.equal(got, T)
        assert model.last_spec_stats == SP.replay(row, ref, S, steps, model.EOS_TOKEN)


def test_graphed_decoder(ar):
    from lap_amd.serve import GraphedTokenDecoder

    cfg, model, o, Ts = ar
    steps = 13          # 12 steps after the first token: no multiple of steps_per_replay = 8
    dec = GraphedTokenDecoder(model, 1, steps, prompt_len=cfg.max_token_len, steps_per_replay=8, speculate=4)
    first = dec(o)
    assert torch.equal(first, Ts[steps]) and dec.last_stats == (steps - 1, 0)
    assert torch.equal(first, model.sample_tokens(0, o, max_decoding_steps=steps, decode="fused", speculate=4))
    second = dec(o, draft_tokens=first[0].tolist())
    assert torch.equal(second, first)
    assert dec.last_stats == (3, 9) == SP.replay(first[0].tolist(), first[0].tolist(), 4, steps, model.EOS_TOKEN)
    third = dec(o)      # no draft again: the reference of the call before is gone
    assert torch.equal(third, first) and dec.last_stats == (steps - 1, 0)
    with pytest.raises(ValueError, match="speculate"):
        GraphedTokenDecoder(model, 1, steps)(o, draft_tokens=[1, 2])


@pytest.mark.parametrize("use_graph", [False, True])
def test_ar_policy_drafts_from_the_previous_answer(ar, use_graph):
    from lap_amd.serve import ARPolicy, Policy

    cfg, model, _, _ = ar
    obs, _, _, _ = make_inputs(cfg, B=1, seed=2, ragged=True)
    prompt = obs["tokenized_prompt"][0].numpy().copy()
    prompt[int(np.flatnonzero(obs["tokenized_prompt_mask"][0].numpy()).max())] = CHAIN[0]      # (the answer walks up the chain)
    req = {"image": {k: v[0].numpy() for k, v in obs["images"].items()}, "image_mask": {k: np.array(True) for k in obs["images"]},
           "state": obs["state"][0].numpy(), "tokenized_prompt": prompt, "tokenized_prompt_mask": obs["tokenized_prompt_mask"][0].numpy()}
    steps = 13
    plain = ARPolicy(Policy(model, use_graph=False), sample_kwargs={"decode": "fused", "max_decoding_steps": steps}, use_graph=use_graph)
    want = plain.infer(req)
    assert "spec_steps" not in want["policy_timing"]
    pol = ARPolicy(Policy(model, use_graph=False), sample_kwargs={"speculate": 4, "decode": "fused", "max_decoding_steps": steps},
                   use_graph=use_graph)
    assert (pol._decoder is not None) == use_graph
    a, b = pol.infer(req), pol.infer(req)
    assert len(set(want["tokens"][0].tolist())) >= 8
    assert np.array_equal(a["tokens"], want["tokens"]) and np.array_equal(b["tokens"], want["tokens"])
    assert a["policy_timing"]["spec_steps"] == steps - 1 and a["policy_timing"]["spec_accepted"] == 0       # the first request drafts nothing
    assert b["policy_timing"]["spec_accepted"] > 0
    assert b["policy_timing"]["spec_steps"] + b["policy_timing"]["spec_accepted"] == steps - 1
