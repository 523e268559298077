"""Top-k / top-p filtering of a device-sampled draw on the GPU: lap_filter_gumbel_argmax_rows_f32 and lap_decode_filter_finish
against `sampling.filter_keep` / `sample_from_logits(..., top_k, top_p)`, and the model / serving surface.

What is compared where.  The kernel's counts are integers and exact, so a top_k cut is compared in every row.  Its masses are within
`sampling.FILTER_MARGIN` (relative) of float64's, so a top_p cut (`kept`, `cut`) is compared in the rows whose `filter_margin`
exceeds that; a token also needs the host's best two kept scores further apart than MARGIN (the last bits of the two logarithms of
the noise).  The rows left out are counted, and at most SHARE of all (row, case) pairs may be (tests/topk_topp_cases.py; the filter
part of that is a CPU test).  logp: within 4x the deviation from float64 of a float32 restatement of z - (M + log S) on the same
logits (the `_bound` rule of tests/test_logprob_gpu.py, recomputed here)."""
import functools

import numpy as np
import pytest
import torch

from lap_amd import sampling as S
from oracle import lap_oracle as O
from tests import topk_topp_cases as C
from tests.common import make_inputs, oracle_cfg, to_observation

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = 2048
ORDER_MARGIN = 4.0
TALLY = {}                      # (B, V, T) -> (rows left out, rows) of the host-step sweep


def _run(hip, lg, T, k, p, seed=C.SEED, step=C.STEP):
    x = torch.from_numpy(lg).to(DEV)
    B = lg.shape[0]
    kept = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    cut = torch.full((B,), float("nan"), device=DEV)
    tok = hip.filter_gumbel_argmax_rows(x, T, seed, step, k, p, kept=kept, cut=cut)
    return tok.cpu().numpy(), kept.cpu().numpy(), cut.cpu().numpy()


def _check(hip, lg, T, k, p, what, count_exact=False):
    """One case against the host; returns the number of rows left out of a comparison."""
    tok, kept, cut = _run(hip, lg, T, k, p)
    h = C.host(lg, T, k, p)
    fc = np.ones_like(h["filter_clear"]) if count_exact else h["filter_clear"]
    assert np.array_equal(kept[fc], h["kept"][fc]), (what, k, p, kept, h["kept"])
    assert np.array_equal(cut[fc], h["cut"][fc]), (what, k, p, cut, h["cut"])
    cl = h["clear"]
    assert np.array_equal(tok[cl], h["token"][cl]), (what, k, p, tok, h["token"])
    assert ((tok >= 0) & (tok < lg.shape[1])).all()
    return int((~cl).sum())


@pytest.mark.parametrize("T", C.TEMPS)
@pytest.mark.parametrize("V", C.VS)
@pytest.mark.parametrize("B", C.BS)
def test_host_step_kernel_sweep(hip, B, V, T):
    lg = C.logits(B, V)
    out = sum(_check(hip, lg, T, k, p, f"B {B} V {V} T {T}") for k, p in C.grid(B, V))
    TALLY[(B, V, T)] = (out, B * len(C.grid(B, V)))
    print(f"B {B} V {V} T {T}: {out} of {TALLY[(B, V, T)][1]} (row, case) pairs left out")


def test_host_step_kernel_sweep_leaves_few_rows_out():
    """The cap over the whole sweep.  Which rows are left out is the host's decision alone, so a case that did not run is counted
    from the host."""
    out = total = 0
    for B in C.BS:
        for V in C.VS:
            for T in C.TEMPS:
                if (B, V, T) not in TALLY:
                    lg = C.logits(B, V)
                    TALLY[(B, V, T)] = (sum(int((~C.host(lg, T, k, p)["clear"]).sum()) for k, p in C.grid(B, V)), B * len(C.grid(B, V)))
                out += TALLY[(B, V, T)][0]
                total += TALLY[(B, V, T)][1]
    print(f"{out} of {total} (row, case) pairs left out")
    assert out <= C.SHARE * total


@pytest.mark.parametrize("V", C.VS)
def test_ties_at_the_top_k_cut(hip, V):
    """bf16-rounded logits: many exactly equal entries, the top_k count is exact in every row and the lower indices are kept."""
    B = 3
    lg = C.logits(B, V, ties=True)
    assert len(np.unique(lg[0])) < V // 2
    for T in C.TEMPS:
        for k in C.ks(V) + (7, 300, 1000):
            _check(hip, lg, T, k, None, f"ties V {V} T {T}", count_exact=True)
            _check(hip, lg, T, k, 0.9, f"ties V {V} T {T}")
    # every entry equal: top_k = 5 keeps the indices 0 .. 4, whatever the noise
    flat = np.zeros((B, V), dtype=np.float32)
    flat[:, 1::2] = -0.0
    for step in range(12):
        tok, kept, cut = _run(hip, flat, 1.0, 5, None, step=step)
        assert (kept == 5).all() and (cut == 0).all() and (tok < 5).all()
        assert np.array_equal(tok, S.sample_from_logits(flat, 1.0, C.SEED, step, 5, None))


def test_the_real_vocabulary(hip):
    lg = C.logits(1, 257152)
    left = 0
    for T, k, p in ((0.7, 40, 0.9), (0.7, None, 0.9), (0.7, None, 0.5), (2.0, 1000, 0.99), (2.0, 257151, None), (0.7, 1, None)):
        h = C.host(lg, T, k, p)
        left += _check(hip, lg, T, k, p, f"V 257152 T {T}")
        assert h["filter_clear"].all(), (T, k, p)
    assert left <= 1


@pytest.mark.parametrize("n", [37, 700])
def test_minus_inf_outside_an_allowed_set(hip, n):
    B, V = 3, 4097
    ids = np.sort(np.random.default_rng(n).permutation(V)[:n])
    lg = np.full((B, V), -np.inf, dtype=np.float32)
    lg[:, ids] = C.logits(B, V)[:, ids]
    left = 0
    for T in C.TEMPS:
        for k in C.ks(n):
            for p in C.PS:
                left += _check(hip, lg, T, k, p, f"{n} ids T {T}")
    tok, kept, _ = _run(hip, lg, 0.7, None, None)
    assert (kept == n).all() and np.isin(tok, ids).all()
    assert left <= C.SHARE * B * 2 * 24 + 1


def test_neutral_and_greedy_are_the_unfiltered_kernels(hip):
    lg = C.logits(8, 16384)
    x = torch.from_numpy(lg).to(DEV)
    for T in (0.7, 2.0):
        plain = hip.gumbel_argmax_rows(x, T, C.SEED, 5)
        for k, p in ((None, None), (0, 1.0), (16384, None), (10 ** 6, 1.0)):
            assert torch.equal(hip.filter_gumbel_argmax_rows(x, T, C.SEED, 5, k, p), plain)
    assert torch.equal(hip.filter_gumbel_argmax_rows(x, 0.0, C.SEED, 5, 3, 0.2), hip.argmax_rows(x))
    with pytest.raises(ValueError, match="top_p"):
        hip.filter_gumbel_argmax_rows(x, 1.0, 1, 0, None, 0.0)


# ------------------------------------------------------------------------------------------------------ the fused entry
def _state(hip, B, t, plen, done=0):
    st = hip.decode_state(B, DEV)
    st[0], st[1] = t, done
    st[16:16 + B] = torch.as_tensor(plen, dtype=torch.int32)
    return st


@functools.lru_cache(maxsize=None)
def _table(V):
    from lap_amd import hip

    g = torch.Generator(device=DEV).manual_seed(700 + V)
    table = torch.randn(V, D, generator=g, device=DEV) * 0.03
    hi, lo = hip.split_f32_hilo(table)
    gamma = torch.randn(D, generator=g, device=DEV) * 0.1
    return hi, lo, gamma


def _x(B, V):
    g = torch.Generator(device=DEV).manual_seed(900 + 10 * B + V % 7)
    return torch.randn(B, D, generator=g, device=DEV).to(torch.bfloat16)


def _f32_deviation(z):
    """float64 [rows]: the largest |float32 restatement - float64| of z - (M + log S) over every entry, in two summation orders."""
    z64 = z.astype(np.float64)
    m = z64.max(1, keepdims=True)
    ref = z64 - (m + np.log(np.exp(z64 - m).sum(1, keepdims=True)))
    M = z.max(1)
    e = np.exp(z - M[:, None], dtype=np.float32)
    seq = np.zeros(z.shape[0], np.float32)
    for j in range(z.shape[1]):
        seq = seq + e[:, j]
    devs = []
    for Ssum in (seq, e.sum(1, dtype=np.float32)):
        lse = M + np.log(Ssum, dtype=np.float32)
        devs.append(np.abs((z - lse[:, None]).astype(np.float32).astype(np.float64) - ref).max(1))
    return np.max(devs, 0)


@pytest.mark.parametrize("T", [0.0, 0.7, 2.0])
@pytest.mark.parametrize("V", [4097, 16384])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_fused_entry_with_neutral_words_is_the_sampling_head_and_finish(hip, B, V, T):
    hi, lo, gamma = _table(V)
    x = _x(B, V)
    samp = hip.decode_sampling(DEV)
    hip.decode_set_sampling(samp, 0xC0FFEE1234, T)
    cap, t = 6, 2
    eos = -1
    for _ in range(2):          # the second round: the EOS token is row 0's token
        st_o, st_n = _state(hip, B, t, [5] * B), _state(hip, B, t, [5] * B)
        out_o = torch.zeros(B, cap, dtype=torch.int32, device=DEV)
        out_n = out_o.clone()
        pval, pidx = hip.decode_lm_partials(B, DEV)
        hip.decode_lm_head_sample(st_o, samp, x, gamma, hi, lo, pval, pidx)
        hip.decode_finish(st_o, pval, pidx, out_o, eos_token=eos)
        lg = torch.full((B, V), float("nan"), device=DEV)
        logp = torch.zeros(B, cap, device=DEV)
        hip.decode_lm_head(st_n, x, gamma, hi, lo, pval, pidx, logits=lg)
        hip.decode_filter_finish(st_n, samp, hip.decode_filter(DEV), lg, out_n, eos, logp=logp)
        assert torch.equal(out_o, out_n) and torch.equal(st_o, st_n)
        assert int(st_n[0]) == t + 1 and int(st_n[2]) == 0
        eos = int(out_o[0, t])
    assert int(st_n[8]) == 1 and int(st_n[1]) == (1 if B == 1 else int(bool((out_n[:, t] == eos).all())))
    # logp: the log-softmax over all candidates at tau = inv_t, on the logits the launch read
    lgn = lg.cpu().numpy()
    tok = out_n[:, t].cpu().numpy()
    want = S.token_logprobs(lgn, tok, T)
    inv_t = float(S.inverse_temperature(T))
    z = (lgn * np.float32(inv_t)).astype(np.float32) if inv_t else lgn
    bound = ORDER_MARGIN * float(_f32_deviation(z).max())
    err = np.abs(logp[:, t].cpu().numpy().astype(np.float64) - want)
    print(f"B {B} V {V} T {T}: |logp - float64| {err.max():.3e}, bound {bound:.3e}")
    assert (err <= bound).all(), (err, bound)
    cols = [c for c in range(cap) if c != t]
    assert float(logp[:, cols].abs().sum()) == 0.0


def test_fused_entry_filters_like_the_host_step_entry(hip):
    """The same body: the fused entry with words (k, p) at step state[0] draws the host-step entry's tokens, keeps logp over all
    candidates, and reads new words from the same buffer."""
    B, V, T, cap = 3, 16384, 0.7, 8
    lg = C.logits(B, V)
    x = torch.from_numpy(lg).to(DEV)
    samp = hip.decode_sampling(DEV)
    hip.decode_set_sampling(samp, C.SEED, T)
    filt = hip.decode_filter(DEV)
    for t, (k, p) in enumerate(((50, 0.9), (None, 0.5), (2, None), (None, None))):
        hip.decode_set_filter(filt, k, p)
        st = _state(hip, B, t, [5] * B)
        out = torch.zeros(B, cap, dtype=torch.int32, device=DEV)
        logp = torch.zeros(B, cap, device=DEV)
        kept = torch.zeros(B, dtype=torch.int32, device=DEV)
        cut = torch.zeros(B, device=DEV)
        hip.decode_filter_finish(st, samp, filt, x, out, -1, logp=logp, kept=kept, cut=cut)
        k2, c2 = torch.zeros_like(kept), torch.zeros_like(cut)
        tok = hip.filter_gumbel_argmax_rows(x, T, C.SEED, t, k, p, kept=k2, cut=c2)
        assert torch.equal(out[:, t], tok) and torch.equal(kept, k2) and torch.equal(cut, c2)
        want = S.token_logprobs(lg, tok.cpu().numpy(), T)
        assert np.abs(logp[:, t].cpu().numpy() - want).max() <= ORDER_MARGIN * float(_f32_deviation((lg * S.inverse_temperature(T)).astype(np.float32)).max())
        assert int(st[0]) == t + 1 and int(st[1]) == 0


def test_fused_entry_writes_nothing_when_done(hip):
    B, V = 3, 4097
    x = torch.from_numpy(C.logits(B, V)).to(DEV)
    samp = hip.decode_sampling(DEV)
    hip.decode_set_sampling(samp, 5, 1.0)
    filt = hip.decode_filter(DEV)
    hip.decode_set_filter(filt, 40, 0.9)
    st = _state(hip, B, 3, [20] * B, done=1)
    st0 = st.clone()
    out = torch.randint(0, 9, (B, 16), dtype=torch.int32, device=DEV)
    out0 = out.clone()
    logp = torch.full((B, 16), -2.0, device=DEV)
    kept = torch.full((B,), -3, dtype=torch.int32, device=DEV)
    cut = torch.full((B,), 7.0, device=DEV)
    hip.decode_filter_finish(st, samp, filt, x, out, 1, logp=logp, kept=kept, cut=cut)
    torch.cuda.synchronize()
    assert torch.equal(st, st0) and torch.equal(out, out0) and bool((logp == -2.0).all()) and bool((kept == -3).all()) and bool((cut == 7.0).all())
    # the budget is spent (t == cap): the flag alone
    st = _state(hip, B, 16, [20] * B)
    hip.decode_filter_finish(st, samp, filt, x, out, 1, logp=logp)
    assert int(st[1]) == 1 and int(st[0]) == 16 and torch.equal(out, out0)


# ---------------------------------------------------------------------------------------------------------------- model
def _gemma2b_x2_cfg(mp, **kw):
    """LAP-3B widths with 2 layers per tower and a 16k vocabulary (tests/test_logprob_gpu.py's configuration)."""
    from lap_amd import config as Cfg
    from lap_amd.config import LAPConfig

    mp.setitem(Cfg._GEMMA, "gemma_2b_x2", Cfg.GemmaConfig(2048, 2, 16384, 8, 1, 256))
    mp.setitem(Cfg._GEMMA, "gemma_300m_x2", Cfg.GemmaConfig(1024, 2, 4096, 8, 1, 256))
    mp.setitem(Cfg._SIGLIP, "So400m/14_x2", Cfg.SiglipConfig(1152, 2, 4304, 16))
    mp.setitem(O.GEMMA, "gemma_2b_x2", O.GemmaCfg(2048, 2, 16384, 8, 1, 256))
    mp.setitem(O.GEMMA, "gemma_300m_x2", O.GemmaCfg(1024, 2, 4096, 8, 1, 256))
    mp.setitem(O.SIGLIP, "So400m/14_x2", O.SiglipCfg(1152, 2, 4304, 16))
    base = dict(paligemma_variant="gemma_2b_x2", action_expert_variant="gemma_300m_x2", siglip_variant="So400m/14_x2",
                image_size=224, vocab_size=16384, action_dim=32, action_horizon=50, max_token_len=48,
                language_loss_weight=0.4, enable_image_augmentation=False, enable_action_training=True)
    return LAPConfig(**(base | kw))


EMBED_SCALE = 0.05              # tests/test_logprob_gpu.py: nearly flat logits, so that draws spread
STEPS = 6
K, P, T_MODEL = 40, 0.9, 1.0


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
    from lap_amd.model import LAP

    with pytest.MonkeyPatch.context() as mp:
        cfg = _gemma2b_x2_cfg(mp)
        Pm = O.init_params(oracle_cfg(cfg), seed=13)
        key = "PaliGemma/llm/embedder/input_embedding"
        Pm[key] = torch.as_tensor(Pm[key]).clone() * EMBED_SCALE
        model = LAP(cfg, params=Pm, device=DEV)
        model.EOS_TOKEN = -1    # no row stops early
        yield cfg, model
        model.EOS_TOKEN = 1


def _obs(cfg, B=3, seed=0):
    obs, _, _, _ = make_inputs(cfg, B=B, seed=seed, ragged=True)
    so = dict(obs)
    so.pop("tokenized_langact_mask")
    so["image_masks"] = {k: torch.ones_like(m) for k, m in so["image_masks"].items()}
    return to_observation(so | {"tokenized_langact_mask": None}, DEV)


def _host_tokens(col, T, seed, k, p, steps):
    """(tokens [rows, steps], clear [rows, steps], stable [rows, steps]) of the host on collected logits: clear as in the kernel
    tests; stable: the draw is the same with the cut a few ranks to either side (another route's logits differ in their last bits,
    which can move an entry across the cut)."""
    tok, clear, stable = [], [], []
    for s in range(steps):
        lg = col[f"logit/{s}"].float().cpu().numpy()
        h = C.host(lg, T, k, p, seed=seed, step=s)
        tok.append(h["token"]); clear.append(h["clear"])
        near = [S.sample_from_logits(lg, T, seed, s, max(1, k + dk), min(1.0, p + dp)) for dk, dp in ((-3, -0.03), (3, 0.03))]
        stable.append(h["clear"] & (near[0] == h["token"]) & (near[1] == h["token"]))
    return np.stack(tok, 1), np.stack(clear, 1), np.stack(stable, 1)


def test_top_k_1_is_the_greedy_decode(ar):
    cfg, model = ar
    o = _obs(cfg)
    greedy = model.sample_tokens(0, o, max_decoding_steps=STEPS, decode="fused")
    got = model.sample_tokens(9, o, max_decoding_steps=STEPS, decode="fused", sampler="device", temperature=1.0, top_k=1)
    assert torch.equal(got, greedy)


def test_routes_agree_under_filters(ar):
    from lap_amd.serve import GraphedTokenDecoder

    cfg, model = ar
    o = _obs(cfg)
    seed = 5
    base = dict(max_decoding_steps=STEPS, temperature=T_MODEL, sampler="device", top_k=K, top_p=P)
    cole, colf = {}, {}
    tok_e = model.sample_tokens(seed, o, collect=cole, **base)
    tok_f = model.sample_tokens(seed, o, decode="fused", collect=colf, **base)
    tok_n = model.sample_tokens(seed, o, decode="fused", **base)
    assert torch.equal(tok_f, tok_n)
    assert torch.equal(tok_n, model.sample_tokens(seed, o, decode="fused", **base))         # a repeated request
    assert not torch.equal(tok_n, model.sample_tokens(seed, o, decode="fused", **(base | {"top_k": None, "top_p": None})))
    dec = GraphedTokenDecoder(model, 3, STEPS, sampling=True, filtering=True)
    tok_g = dec(o, temperature=T_MODEL, seed=seed, top_k=K, top_p=P)
    assert torch.equal(tok_g, tok_n)
    graphs, ctx = (dec.g_prefill, dec.g_step), dec.ctx
    # the same capture: another (k, p), a neutral call (the filtering=False decoder's tokens), and the first pair again
    other = dec(o, temperature=T_MODEL, seed=seed, top_k=3, top_p=0.5)
    assert torch.equal(other, model.sample_tokens(seed, o, decode="fused", **(base | {"top_k": 3, "top_p": 0.5})))
    plain = GraphedTokenDecoder(model, 3, STEPS, sampling=True)(o, temperature=T_MODEL, seed=seed)
    assert torch.equal(dec(o, temperature=T_MODEL, seed=seed), plain)
    assert torch.equal(dec(o, temperature=T_MODEL, seed=seed, top_k=K, top_p=P), tok_g)
    assert (dec.g_prefill, dec.g_step) == graphs and dec.ctx is ctx
    with pytest.raises(ValueError, match="filtering"):
        GraphedTokenDecoder(model, 3, STEPS, sampling=True)(o, temperature=T_MODEL, seed=seed, top_k=K)
    with pytest.raises(ValueError, match="sampling"):
        GraphedTokenDecoder(model, 3, STEPS, filtering=True)
    # each route against the host on its own logits
    compared = 0
    for name, tok, col in (("eager", tok_e, cole), ("fused", tok_f, colf)):
        want, clear, _ = _host_tokens(col, T_MODEL, seed, K, P, STEPS)
        got = tok.cpu().numpy()
        assert np.array_equal(got[clear], want[clear]), name
        compared += int(clear.sum())
    assert compared >= 0.75 * 2 * 3 * STEPS
    # eager against fused over the prefix where the eager draw is clear and does not hang on the exact place of the cut
    _, _, stable = _host_tokens(cole, T_MODEL, seed, K, P, STEPS)
    prefix = np.cumprod(stable, axis=1).astype(bool)
    assert np.array_equal(tok_e.cpu().numpy()[prefix], tok_f.cpu().numpy()[prefix])
    assert prefix.sum() >= 3
    # every drawn token is inside the kept set of its own logits
    for s in range(STEPS):
        keep = S.filter_keep(colf[f"logit/{s}"].cpu().numpy(), T_MODEL, K, P)
        fm = S.filter_margin(colf[f"logit/{s}"].cpu().numpy(), T_MODEL, K, P) > S.FILTER_MARGIN
        assert keep[np.arange(3), tok_f[:, s].cpu().numpy()][fm].all()


def test_filters_compose_with_best_of_n_fp8_and_an_allowed_set(ar):
    from lap_amd.serve import GraphedTokenDecoder

    cfg, model = ar
    o1 = _obs(cfg, B=1, seed=1)
    N = 4
    kw = dict(max_decoding_steps=STEPS, temperature=T_MODEL, sampler="device", decode="fused", num_samples=N, decode_weights="fp8",
              top_k=K, top_p=P)
    col = {}
    tok, lp = model.sample_tokens(3, o1, collect=col, **kw)
    assert tok.shape == (N, STEPS) and lp.shape == (N, STEPS) and bool((lp < 0).all())
    tok2, lp2 = model.sample_tokens(3, o1, **kw)
    assert torch.equal(tok, tok2) and torch.equal(lp, lp2)
    want, clear, _ = _host_tokens(col, T_MODEL, 3, K, P, STEPS)
    assert np.array_equal(tok.cpu().numpy()[clear], want[clear])
    # the log-probability is the model's: over all candidates, not over the kept set
    lg = np.concatenate([col[f"logit/{s}"].cpu().numpy() for s in range(STEPS)], 0)
    ref = S.token_logprobs(lg, tok.cpu().numpy().T.reshape(-1), T_MODEL)
    bound = ORDER_MARGIN * float(_f32_deviation(lg).max())
    assert np.abs(lp.cpu().numpy().T.reshape(-1) - ref).max() <= bound
    dec = GraphedTokenDecoder(model, 1, STEPS, sampling=True, num_samples=N, weights="fp8", filtering=True)
    tg, lg_ = dec(o1, temperature=T_MODEL, seed=3, top_k=K, top_p=P)
    assert torch.equal(tg, tok) and torch.equal(lg_, lp)
    # an allowed set: the candidates are the set, the kept entries lie inside it
    g = torch.Generator().manual_seed(3)
    allowed = torch.unique(torch.randperm(cfg.vocab_size, generator=g)[:2001])
    cola = {}
    ta = model.sample_tokens(4, _obs(cfg), max_decoding_steps=STEPS, temperature=T_MODEL, sampler="device", decode="fused",
                             allowed_tokens=allowed, top_k=K, top_p=P, collect=cola)
    assert np.isin(ta.cpu().numpy(), allowed.numpy()).all()
    want, clear, _ = _host_tokens(cola, T_MODEL, 4, K, P, STEPS)
    assert np.array_equal(ta.cpu().numpy()[clear], want[clear]) and clear.mean() >= 0.5
    te = model.sample_tokens(4, _obs(cfg), max_decoding_steps=2, temperature=T_MODEL, sampler="device", allowed_tokens=allowed,
                             top_k=K, top_p=P)
    assert np.isin(te.cpu().numpy(), allowed.numpy()).all()


@pytest.mark.parametrize("use_graph", [False, True])
def test_ar_policy_with_filters(ar, use_graph):
    from lap_amd.serve import ARPolicy, Policy

    cfg, model = ar
    obs, _, _, _ = make_inputs(cfg, B=1, seed=2, ragged=True)
    req = {"image": {k: v[0].numpy() for k, v in obs["images"].items()}, "image_mask": {k: np.array(True) for k in obs["images"]},
           "state": obs["state"][0].numpy(), "tokenized_prompt": obs["tokenized_prompt"][0].numpy(),
           "tokenized_prompt_mask": obs["tokenized_prompt_mask"][0].numpy()}
    kw = {"top_k": 40, "top_p": 0.9, "temperature": 0.7, "sampler": "device", "max_decoding_steps": STEPS}
    pol = ARPolicy(Policy(model, use_graph=False), sample_kwargs=kw, use_graph=use_graph)
    assert (pol._decoder is not None) == use_graph and (not use_graph or pol._decoder.filtering)
    res = pol.infer(req)
    o = pol._base._to_observation(req)[0]
    want = model.sample_tokens(1, o, decode="fused", **kw)      # call counter 1
    assert res["tokens"].shape == (1, STEPS)
    if use_graph:
        assert np.array_equal(res["tokens"], want.cpu().numpy())
    with pytest.raises(ValueError, match="sampler"):
        ARPolicy(Policy(model, use_graph=False), sample_kwargs={"top_k": 40, "temperature": 0.7})
    with pytest.raises(ValueError, match="top_p"):
        ARPolicy(Policy(model, use_graph=False), sample_kwargs={"top_p": 2.0, "temperature": 0.7, "sampler": "device"})
