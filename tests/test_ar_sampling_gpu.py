"""Temperature sampling inside the fused, graph-replayed LAP_AR decoder (GPU): the sampling LM head, the one-pass Gumbel argmax
and their model / serving surface against the host restatement of the noise (lap_amd/sampling.py).

The draw rule.  A device draw is accepted when it is the argmax of the host-restated scores, or when the host score of the index
it chose lies within TIE of the host's best score.  TIE covers the last bits of the two accurate logarithms of the noise
(-log(-log(u)), |g| < 16.7, scores up to ~25 in magnitude) and nothing else: the Philox words and u are exact on both sides and
the product logit * inv_t and the sum are rounded separately on both sides.  The largest |device score - host score| over
`_gumbel_inputs` (the inputs of test_gumbel_argmax_rows_matches_host: 432 rows of 257,152 scores up to 25.96 in magnitude),
measured on an MI355X with the debug build of the score (tools/probes/gumbel_scores.hip, tools/probes/gumbel_score_error.py), is
OBSERVED_SCORE_ERROR = 3.814697265625e-06 (two ulp of a float32 in [16, 32); the noise alone: 1.9073486328125e-06); TIE is four
times that, 1.52587890625e-05.  At most 1 draw in 1,000 may use the allowance (ALLOWANCE_CAP), so that it cannot hide a wrong generator: a wrong
noise stream disagrees on nearly every draw.
"""
import numpy as np
import pytest
import torch

from lap_amd import sampling as S
from oracle import lap_oracle as O
from tests.common import make_inputs, oracle_cfg, to_observation

pytestmark = pytest.mark.gpu
DEV = "cuda"
OBSERVED_SCORE_ERROR = 3.814697265625e-06       # tools/probes/gumbel_score_error.py on an MI355X
TIE = 4 * OBSERVED_SCORE_ERROR
ALLOWANCE_CAP = 1e-3
MARGIN = 5e-2                   # tests/test_ar_decode_gpu.py's MARGIN, here on scores
CHI2_999_DF7 = 24.32            # 99.9 % quantile of chi-square with 7 degrees of freedom

D, NH, HD, H = 2048, 8, 256, 16384
V_FULL = 257152


def _state(hip, B, t, plen, done=0):
    st = hip.decode_state(B, DEV)
    st[0], st[1] = t, done
    st[16:16 + B] = torch.as_tensor(plen, dtype=torch.int32)
    return st


def _bf(*shape, scale=1.0, g=None):
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(torch.bfloat16)


class _Rule:
    """Counts the draws checked and those that needed the TIE allowance."""

    def __init__(self):
        self.draws = self.allowed = 0

    def check(self, tokens, logits, temperature, seed, step, what="", scores=None):
        sc = _scores(logits, temperature, seed, step) if scores is None else scores
        tok = np.asarray(tokens.detach().cpu().numpy() if isinstance(tokens, torch.Tensor) else tokens).reshape(-1)
        assert tok.shape[0] == sc.shape[0]
        for b in range(sc.shape[0]):
            self.draws += 1
            best = int(np.argmax(sc[b]))
            if int(tok[b]) == best:
                continue
            assert 0 <= int(tok[b]) < sc.shape[1], (what, step, b, int(tok[b]))
            gap = float(sc[b, best] - sc[b, int(tok[b])])
            assert gap <= TIE, (what, step, b, int(tok[b]), best, gap)
            self.allowed += 1

    def within_cap(self):
        return self.allowed <= ALLOWANCE_CAP * self.draws


def _scores(logits, temperature, seed, step):
    return S.scores_from_logits(logits.detach().float().cpu().numpy(), temperature, seed, step)


def _margins(logits, temperature, seed, step, scores=None):
    """top-2 margin of the host-restated scores, per row."""
    sc = _scores(logits, temperature, seed, step) if scores is None else scores
    top2 = np.partition(sc, -2, axis=1)[:, -2:]
    return top2[:, 1] - top2[:, 0]


@pytest.fixture(scope="module", autouse=True)
def _hand_back_stream_scratch(hip):
    """Every captured decoder warms up on a fresh side stream, and lap_amd.hip keeps a 640 MB split-K scratch per stream for the
    life of the process.  Hand back the ones this module caused, so that the tests after it find the device memory as they would
    without this file."""
    import gc

    before = set(hip._SCRATCH)
    yield
    for k in set(hip._SCRATCH) - before:
        del hip._SCRATCH[k]
    gc.collect()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------- kernels
GUMBEL_SEED = 0x123456789ABCDEF
GUMBEL_STEPS = 36


def _gumbel_inputs(B):
    """The logits of the Gumbel-argmax test (and of the score-error probe): N(0, 2^2), so that scores reach ~25."""
    g = torch.Generator(device="cpu").manual_seed(40 + B)
    return torch.randn(B, V_FULL, generator=g) * 2.0


@pytest.mark.parametrize("B", [1, 3, 8])
def test_gumbel_argmax_rows_matches_host(hip, B):
    lg = _gumbel_inputs(B)
    x = lg.to(DEV)
    rule = _Rule()
    close = 0
    for step in range(GUMBEL_STEPS):
        T = (0.5, 1.0, 2.0)[step % 3]
        tok = hip.gumbel_argmax_rows(x, T, GUMBEL_SEED, step)
        sc = _scores(lg, T, GUMBEL_SEED, step)
        rule.check(tok, lg, T, GUMBEL_SEED, step, "gumbel_argmax_rows", scores=sc)
        # on the CPU: a perturbation of the host scores by TIE (either way) flips the argmax only where the top-2 margin is
        # within 2 TIE; correct noise must keep such draws within the cap too
        close += int((_margins(lg, T, GUMBEL_SEED, step, scores=sc) <= 2 * TIE).sum())
    print(f"B {B}: {rule.draws} draws, {rule.allowed} used the allowance, {close} with a top-2 margin within 2 TIE")
    assert rule.within_cap() and close <= ALLOWANCE_CAP * rule.draws
    # greedy: inv_t = 0 is lap_argmax_rows_f32; a strided view; ties take the lowest index
    assert torch.equal(hip.gumbel_argmax_rows(x, 0.0, GUMBEL_SEED, 3), hip.argmax_rows(x))
    assert torch.equal(hip.gumbel_argmax_rows(x, -1.0, GUMBEL_SEED, 3), hip.argmax_rows(x))
    view = x[:, :1001]
    tok = hip.gumbel_argmax_rows(view, 1.0, 7, 2)
    _Rule().check(tok, lg[:, :1001], 1.0, 7, 2, "odd width, strided")
    with pytest.raises(ValueError):
        hip.gumbel_argmax_rows(x, 1e-45, 7, 2)


def _lm_inputs(hip, B, V, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    table = torch.randn(V, D, generator=g, device=DEV) * 0.03
    hi, lo = hip.split_f32_hilo(table)
    gamma = torch.randn(D, generator=g, device=DEV) * 0.1
    return hi, lo, gamma, _bf(B, D, g=g)


@pytest.mark.parametrize("B", [1, 3, 8])
def test_sampling_lm_head(hip, B):
    V, cap = V_FULL, 8
    hi, lo, gamma, x = _lm_inputs(hip, B, V, 50 + B)
    seed = 0xDEADBEEF12345
    samp = hip.decode_sampling(DEV)
    assert samp.dtype == torch.int32 and samp.numel() == 4 and int(samp.abs().sum()) == 0
    pval, pidx = hip.decode_lm_partials(B, DEV)
    pval_s, pidx_s = hip.decode_lm_partials(B, DEV)
    lg, lg_s = torch.empty(B, V, device=DEV), torch.empty(B, V, device=DEV)
    # greedy reference
    st = _state(hip, B, 2, [5] * B)
    out = torch.zeros(B, cap, dtype=torch.int32, device=DEV)
    hip.decode_lm_head(st, x, gamma, hi, lo, pval, pidx, logits=lg)
    hip.decode_finish(st, pval, pidx, out, eos_token=-1)
    # inv_t == 0 (the zeroed buffer, then temperature 0 and a negative temperature with a seed): the greedy partials bit for bit
    for temp, sd in ((None, 0), (0.0, seed), (-3.0, seed)):
        if temp is not None:
            hip.decode_set_sampling(samp, sd, temp)
            words = samp.cpu().numpy().view(np.uint32)
            assert (int(words[0]), int(words[1]), int(words[2]), int(words[3])) == (sd & 0xFFFFFFFF, sd >> 32, 0, 0)
        pval_s.fill_(7.0); pidx_s.fill_(-7)
        st_s = _state(hip, B, 2, [5] * B)
        out_s = torch.zeros(B, cap, dtype=torch.int32, device=DEV)
        hip.decode_lm_head_sample(st_s, samp, x, gamma, hi, lo, pval_s, pidx_s, logits=lg_s)
        hip.decode_finish(st_s, pval_s, pidx_s, out_s, eos_token=-1)
        assert torch.equal(lg_s, lg) and torch.equal(pval_s, pval) and torch.equal(pidx_s, pidx) and torch.equal(out_s, out)
        assert torch.equal(st_s, st)
    # T = 1: the raw logits stay raw, the token is the host's draw for the step in state[0]; two states that differ in t only
    rule = _Rule()
    hip.decode_set_sampling(samp, seed, 1.0)
    assert int(samp[2]) == 0x3F800000
    toks = {}
    for t in (2, 5):
        st_s = _state(hip, B, t, [5] * B)
        out_s = torch.zeros(B, cap, dtype=torch.int32, device=DEV)
        lg_s.zero_()
        hip.decode_lm_head_sample(st_s, samp, x, gamma, hi, lo, pval_s, pidx_s, logits=lg_s)
        hip.decode_finish(st_s, pval_s, pidx_s, out_s, eos_token=-1)
        assert torch.equal(lg_s, lg)
        assert int(st_s[0]) == t + 1 and int(st_s[1]) == 0
        cols = [c for c in range(cap) if c != t]
        assert int(out_s[:, cols].abs().sum()) == 0
        rule.check(out_s[:, t], lg, 1.0, seed, t, f"lm head t={t}")
        toks[t] = out_s[:, t].clone()
        # without the debug output: the same partials
        pv2, pi2 = hip.decode_lm_partials(B, DEV)
        hip.decode_lm_head_sample(_state(hip, B, t, [5] * B), samp, x, gamma, hi, lo, pv2, pi2)
        assert torch.equal(pv2, pval_s) and torch.equal(pi2, pidx_s)
    assert not torch.equal(toks[2], toks[5])                # (every row repeating its draw at another step: not by chance)
    assert not torch.equal(toks[2], out[:, 2])              # the noise decides, not the greedy maximum (flat random logits)
    # T = 0.5 with another seed
    hip.decode_set_sampling(samp, 99, 0.5)
    st_s = _state(hip, B, 0, [5] * B)
    out_s = torch.zeros(B, cap, dtype=torch.int32, device=DEV)
    hip.decode_lm_head_sample(st_s, samp, x, gamma, hi, lo, pval_s, pidx_s)
    hip.decode_finish(st_s, pval_s, pidx_s, out_s, eos_token=-1)
    rule.check(out_s[:, 0], lg, 0.5, 99, 0, "lm head T=0.5")
    assert rule.within_cap()
    print(f"B {B}: {rule.draws} draws, {rule.allowed} used the allowance")
    # a temperature whose inverse is not finite is rejected on the host; the buffer keeps its words
    before = samp.clone()
    with pytest.raises(ValueError):
        hip.decode_set_sampling(samp, 1, 1e-45)
    assert torch.equal(samp, before)


def test_sampling_lm_head_odd_vocabulary(hip):
    """V odd: the last unit has one row; hi-only planes (lo = None)."""
    B, V = 3, 4097
    hi, lo, gamma, x = _lm_inputs(hip, B, V, 61)
    samp = hip.decode_sampling(DEV)
    hip.decode_set_sampling(samp, 5, 1.0)
    pval, pidx = hip.decode_lm_partials(B, DEV)
    rule = _Rule()
    for planes in ((hi, lo), (hi, None)):
        lg = torch.empty(B, V, device=DEV)
        st = _state(hip, B, 1, [5] * B)
        out = torch.zeros(B, 4, dtype=torch.int32, device=DEV)
        hip.decode_lm_head_sample(st, samp, x, gamma, *planes, pval, pidx, logits=lg)
        hip.decode_finish(st, pval, pidx, out, eos_token=-1)
        rule.check(out[:, 1], lg, 1.0, 5, 1, "odd V")
    assert rule.allowed == 0


@pytest.mark.parametrize("B", [1, 3])
def test_done_state_writes_nothing_under_sampling(hip, B):
    hi, lo, gamma, x = _lm_inputs(hip, B, 4096, 62)
    samp = hip.decode_sampling(DEV)
    hip.decode_set_sampling(samp, 5, 1.0)
    samp0 = samp.clone()
    st = _state(hip, B, 3, [20] * B, done=1)
    st0 = st.clone()
    pval, pidx = hip.decode_lm_partials(B, DEV)
    pval.fill_(3.0); pidx.fill_(11)
    lg = torch.full((B, 4096), 5.0, device=DEV)
    out = torch.randint(0, 9, (B, 16), dtype=torch.int32, device=DEV)
    out0 = out.clone()
    hip.decode_lm_head_sample(st, samp, x, gamma, hi, lo, pval, pidx, logits=lg)
    hip.decode_finish(st, pval, pidx, out, eos_token=1)
    torch.cuda.synchronize()
    assert torch.equal(st, st0) and torch.equal(samp, samp0) and torch.equal(out, out0)
    assert bool((pval == 3.0).all()) and bool((pidx == 11).all()) and bool((lg == 5.0).all())


def test_device_draws_follow_the_softmax(hip):
    """4,000 steps of one seed through the sampling LM head + finish on a table whose first 8 rows give chosen logits and whose
    other 257,144 rows sit 40 below them: chi-square against softmax(raw logits) below the 99.9 % quantile (7 degrees)."""
    V, n = V_FULL, 4000
    want = torch.tensor([1.2, -0.3, 0.0, 2.1, 0.7, -1.5, 1.9, 0.4])
    # x = a e_0 with gamma = 0: h = RMSNorm(x) = sqrt(D) e_0 = 45.25 e_0 in bf16, so logit[v] = 45.25 (hi + lo)[v][0]
    table = torch.zeros(V, D, device=DEV)
    table[:, 0] = (want.min() - 40.0) / 45.25
    table[:8, 0] = want.to(DEV) / 45.25
    hi, lo = hip.split_f32_hilo(table)
    del table
    gamma = torch.zeros(D, device=DEV)
    x = torch.zeros(1, D, dtype=torch.bfloat16, device=DEV)
    x[0, 0] = 3.0
    samp = hip.decode_sampling(DEV)
    hip.decode_set_sampling(samp, 20240917, 1.0)
    pval, pidx = hip.decode_lm_partials(1, DEV)
    st = _state(hip, 1, 0, [5])
    out = torch.zeros(1, n, dtype=torch.int32, device=DEV)
    lg = torch.empty(1, V, device=DEV)
    hip.decode_lm_head_sample(st, samp, x, gamma, hi, lo, pval, pidx, logits=lg)       # step 0, with the raw logits
    hip.decode_finish(st, pval, pidx, out, eos_token=-1)
    for _ in range(n - 1):       # the step comes from state[0], which lap_decode_finish advances
        hip.decode_lm_head_sample(st, samp, x, gamma, hi, lo, pval, pidx)
        hip.decode_finish(st, pval, pidx, out, eos_token=-1)
    assert int(st[0]) == n and int(st[1]) == 1
    raw = lg[0].double().cpu()
    assert float((raw[:8] - want.double()).abs().max()) < 1e-3 and float(raw[8:].max()) < float(want.min()) - 39.9
    tok = out[0].cpu().numpy()
    assert tok.max() < 8
    p = torch.softmax(raw, 0)[:8].numpy()
    counts = np.bincount(tok, minlength=8).astype(np.float64)
    chi2 = float(((counts - n * p) ** 2 / (n * p)).sum())
    print(f"device draws: counts {counts.tolist()}, expected {(n * p).round(1).tolist()}, chi-square {chi2:.2f}")
    assert chi2 < CHI2_999_DF7
    # and every one of the first 64 draws is the host's
    rule = _Rule()
    for s in range(64):
        rule.check(out[:, s], lg, 1.0, 20240917, s, "distribution")
    assert rule.allowed == 0


# ---------------------------------------------------------------------------------------------------------------- model
def _gemma2b_x2_cfg(mp, **kw):
    """LAP-3B widths with 2 layers per tower and a 16k vocabulary (tests/test_ar_decode_gpu.py's configuration)."""
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


def _obs(cfg, case, B=3):
    obs, _, _, _ = make_inputs(cfg, B=B, ragged=True)
    so = dict(obs)
    if case != "langact":
        so.pop("tokenized_langact_mask")
    so["image_masks"] = {k: torch.ones_like(m) for k, m in so["image_masks"].items()}
    return so


def _to_obs(so):
    return to_observation(so if "tokenized_langact_mask" in so else so | {"tokenized_langact_mask": None}, DEV)


EMBED_SCALE = 0.05


@pytest.fixture(scope="module")
def ar(hip):
    """(cfg, model): one model for the module: the random parameters of tests/test_ar_decode_gpu.py (seed 13) with the embedding
    table scaled by EMBED_SCALE.  With the table as initialised the tied LM head echoes the last input token with a top-2 logit
    margin of 12 - 14 (measured: tools/probes/gumbel_score_error.py --scan-seeds), so that a T = 1 draw is the greedy token
    whatever the noise and every comparison below would pass without a sampler.  The final RMSNorm fixes the length of h, so the
    logits h . e_v scale with the table: at 0.05 the margin is ~0.6 against Gumbel noise of spread ~1.3 and the draws spread
    over the vocabulary (test_host_sampler_is_untouched_and_greedy_is_greedy asserts that they leave the greedy token)."""
    from lap_amd.model import LAP

    with pytest.MonkeyPatch.context() as mp:
        cfg = _gemma2b_x2_cfg(mp)
        P = O.init_params(oracle_cfg(cfg), seed=13)
        key = "PaliGemma/llm/embedder/input_embedding"
        P[key] = torch.as_tensor(P[key]).clone() * EMBED_SCALE
        model = LAP(cfg, params=P, device=DEV)
        yield cfg, model
        model.EOS_TOKEN = 1


def _agrees_with_eager_scores(out, ref, col, temperature, seed):
    """tokens equal step by step while the top-2 margins of the eager SCORES (raw logit * inv_t + host-restated noise) exceed
    MARGIN; from the first step where one does not, the contexts may diverge.  Returns (agrees, steps whose margins all
    exceeded MARGIN before that)."""
    clear = 0
    for s in range(ref.shape[1]):
        if not torch.equal(out[:, :s], ref[:, :s]):
            return False, clear
        lg = col.get(f"logit/{s}")
        if lg is None:
            break
        if bool((_margins(lg, temperature, seed, s) <= MARGIN).any()):
            return True, clear
        clear += 1
    return torch.equal(out, ref), clear


# The seed of the eager / fused / graphed comparison.  On nearly flat logits the top-2 margin of a draw's scores is close to an
# Exp(1) variable, so about 1 draw in 20 falls below MARGIN; with 3 rows the first 3 steps are 9 draws, and roughly 4 seeds in 10
# have one such draw among them.  The comparison uses the smallest seed of SEED_CANDIDATES whose eager scores keep every margin of
# the first 3 steps above MARGIN (a fixed choice: the margins are a function of the committed inputs), and fails if there is
# none, so it cannot pass vacuously.
SEED_CANDIDATES = tuple(range(1, 17))
STEPS = 5


def _clear_steps(col, temperature, seed):
    n = 0
    while f"logit/{n}" in col and not bool((_margins(col[f"logit/{n}"], temperature, seed, n) <= MARGIN).any()):
        n += 1
    return n


def _pick_seed(model, o, temperature):
    for seed in SEED_CANDIDATES:
        col = {}
        eager = model.sample_tokens(seed, o, max_decoding_steps=STEPS, temperature=temperature, sampler="device", collect=col)
        if _clear_steps(col, temperature, seed) >= 3:
            return seed, eager, col
    pytest.fail(f"no seed of {SEED_CANDIDATES} keeps the margins of the first 3 steps above {MARGIN}")


@pytest.mark.parametrize("case", ["ragged", "langact"])
def test_eager_fused_graphed_sampling_agree(ar, case):
    from lap_amd.serve import GraphedTokenDecoder

    cfg, model = ar
    o = _to_obs(_obs(cfg, case))
    T = 1.0
    seed, eager, cole = _pick_seed(model, o, T)
    colf = {}
    fused = model.sample_tokens(seed, o, max_decoding_steps=STEPS, temperature=T, sampler="device", decode="fused", collect=colf)
    fused_nc = model.sample_tokens(seed, o, max_decoding_steps=STEPS, temperature=T, sampler="device", decode="fused")
    assert eager.shape == (3, STEPS) and eager.dtype == torch.int32 and fused.shape == (3, STEPS) and fused.dtype == torch.int32
    assert torch.equal(fused, fused_nc)
    dec = GraphedTokenDecoder(model, 3, STEPS, prompt_len=cfg.max_token_len, sampling=True)
    got = dec(o, temperature=T, seed=seed)
    assert torch.equal(got, fused_nc)           # same kernels, same order: the replay is the fused path bit for bit
    ok, clear = _agrees_with_eager_scores(fused, eager, cole, T, seed)
    print(f"{case}: seed {seed}, eager {eager.tolist()} fused {fused.tolist()}, {clear} steps with every margin above {MARGIN}")
    assert clear >= 3 and clear == min(_clear_steps(cole, T, seed), STEPS), clear
    assert ok
    # every token is the host's draw from the raw logits its own path collected: a served draw is reproducible offline
    rule = _Rule()
    for name, toks, col in (("eager", eager, cole), ("fused", fused, colf)):
        assert len(col) == STEPS
        for s in range(STEPS):
            rule.check(toks[:, s], col[f"logit/{s}"], T, seed, s, name)
    assert rule.allowed == 0, rule.allowed      # (30 draws: the cap leaves no room)
    # the collected logits are raw: those of the greedy decode of the same context at step 0
    colg = {}
    model.sample_tokens(0, o, max_decoding_steps=1, collect=colg)
    assert torch.equal(colg["logit/0"], cole["logit/0"])


def test_seeds_and_repeats(ar):
    cfg, model = ar
    o = _to_obs(_obs(cfg, "ragged"))
    for decode in ("eager", "fused"):
        kw = dict(max_decoding_steps=STEPS, temperature=1.0, sampler="device", decode=decode)
        a = model.sample_tokens(11, o, **kw)
        assert torch.equal(a, model.sample_tokens(11, o, **kw))
        assert not torch.equal(a, model.sample_tokens(12, o, **kw))
        assert not torch.equal(a, model.sample_tokens(11 + (1 << 32), o, **kw))       # the high seed word counts
        assert not torch.equal(a, model.sample_tokens(11, o, **(kw | {"temperature": 0.0})))


def test_one_capture_serves_greedy_and_sampled(ar):
    from lap_amd.serve import GraphedTokenDecoder

    cfg, model = ar
    o = _to_obs(_obs(cfg, "ragged"))
    greedy = GraphedTokenDecoder(model, 3, STEPS)(o)
    with pytest.raises(ValueError):
        GraphedTokenDecoder(model, 3, STEPS)(o, temperature=1.0)
    dec = GraphedTokenDecoder(model, 3, STEPS, sampling=True).capture()
    graphs = (dec.g_prefill, dec.g_step)
    ctx = dec.ctx
    c1 = dec(o)
    c2 = dec(o, temperature=1.0, seed=5)
    c3 = dec(o, temperature=0.0, seed=5)
    c4 = dec(o, temperature=1.0, seed=5)
    assert torch.equal(c1, greedy) and torch.equal(c3, greedy)
    assert torch.equal(c2, c4) and not torch.equal(c2, greedy)
    assert torch.equal(c2, model.sample_tokens(5, o, max_decoding_steps=STEPS, temperature=1.0, sampler="device", decode="fused"))
    assert dec.g_prefill is graphs[0] and dec.g_step is graphs[1] and dec.ctx is ctx


def test_host_sampler_is_untouched_and_greedy_is_greedy(ar):
    cfg, model = ar
    o = _to_obs(_obs(cfg, "ragged"))
    kw = dict(max_decoding_steps=STEPS)
    host = model.sample_tokens(3, o, temperature=1.0, **kw)
    assert torch.equal(host, model.sample_tokens(3, o, temperature=1.0, sampler="host", **kw))
    assert torch.equal(host, model.sample_tokens(3, o, temperature=1.0, sampler="host", decode="fused", **kw))   # (the eager loop)
    assert not torch.equal(host, model.sample_tokens(3, o, temperature=1.0, sampler="device", **kw))
    greedy_fused = model.sample_tokens(0, o, decode="fused", **kw)
    assert torch.equal(greedy_fused, model.sample_tokens(9, o, temperature=0.0, sampler="device", decode="fused", **kw))
    assert torch.equal(greedy_fused, model.sample_tokens(9, o, temperature=-1.0, sampler="device", decode="fused", **kw))
    greedy = model.sample_tokens(0, o, **kw)
    assert torch.equal(greedy, model.sample_tokens(9, o, temperature=0.0, sampler="device", **kw))
    with pytest.raises(ValueError):
        model.sample_tokens(0, o, sampler="gpu", **kw)
    with pytest.raises(ValueError):
        model.sample_tokens(0, o, temperature=1e-45, sampler="device", **kw)


def test_eos_under_sampling(ar):
    from lap_amd.serve import GraphedTokenDecoder

    cfg, model = ar
    so = _obs(cfg, "ragged")
    o1 = _to_obs({k: ({kk: vv[:1] for kk, vv in v.items()} if isinstance(v, dict) else v[:1]) for k, v in so.items()})
    kw = dict(max_decoding_steps=STEPS, temperature=1.0, sampler="device")
    try:
        for decode in ("eager", "fused"):
            model.EOS_TOKEN = -1
            free = model.sample_tokens(21, o1, decode=decode, **kw)
            assert int(free[0, 1]) != int(free[0, 0]) and int(free[0, 2:].abs().sum()) != 0
            model.EOS_TOKEN = int(free[0, 1])           # the token drawn at step 1
            got = model.sample_tokens(21, o1, decode=decode, **kw)
            assert torch.equal(got[0, :2], free[0, :2]) and int(got[0, 2:].abs().sum()) == 0, decode
        dec = GraphedTokenDecoder(model, 1, STEPS, sampling=True)
        got = dec(o1, temperature=1.0, seed=21)
        assert torch.equal(got[0, :2], free[0, :2]) and int(got[0, 2:].abs().sum()) == 0
        assert int(dec.ctx.state[0]) == 2 and int(dec.ctx.state[1]) == 1 and int(dec.ctx.state[8]) == 1
    finally:
        model.EOS_TOKEN = 1


def test_ar_policy_serves_sampled_requests_from_the_graphs(ar, monkeypatch):
    from lap_amd.serve import ARPolicy, Policy

    cfg, model = ar
    reqs = []
    for seed in (1, 2):
        obs, _, _, _ = make_inputs(cfg, B=1, seed=seed, ragged=True)
        reqs.append({"image": {k: v[0].numpy() for k, v in obs["images"].items()},
                     "image_mask": {k: np.array(True) for k in obs["images"]},
                     "state": obs["state"][0].numpy(), "tokenized_prompt": obs["tokenized_prompt"][0].numpy(),
                     "tokenized_prompt_mask": obs["tokenized_prompt_mask"][0].numpy()})
    kw = {"max_decoding_steps": STEPS, "temperature": 1.0, "sampler": "device"}
    # the eager route of the same requests (call counter 1, 2 as the seed)
    want = [model.sample_tokens(i + 1, ARPolicy(Policy(model, use_graph=False))._base._to_observation(r)[0], **kw).cpu().numpy()
            for i, r in enumerate(reqs)]
    real = model.sample_tokens
    pols = [ARPolicy(Policy(model, use_graph=False), sample_kwargs=kw, use_graph=True) for _ in range(2)]
    assert all(p._decoder is not None and p._decoder.sampling for p in pols)

    def boom(*a, **k):
        raise AssertionError("sample_tokens called: the graphs were not replayed")

    monkeypatch.setattr(model, "sample_tokens", boom)
    got = [[p.infer(r)["tokens"] for r in reqs] for p in pols]
    monkeypatch.setattr(model, "sample_tokens", real)
    for i in range(2):
        assert np.array_equal(got[0][i], got[1][i])
        assert got[0][i].shape == (1, STEPS)
    assert not np.array_equal(got[0][0], got[0][1])
    # the graphed route draws what the fused route draws with the call counter as the seed; the eager route agrees wherever
    # the margins allow (checked on the first token, whose context is the prompt alone)
    for i, r in enumerate(reqs):
        o = pols[0]._base._to_observation(r)[0]
        assert np.array_equal(got[0][i], model.sample_tokens(i + 1, o, decode="fused", **kw).cpu().numpy())
        col = {}
        model.sample_tokens(i + 1, o, collect=col, **(kw | {"max_decoding_steps": 1}))
        if float(_margins(col["logit/0"], 1.0, i + 1, 0)[0]) > MARGIN:
            assert int(got[0][i][0, 0]) == int(want[i][0, 0])
    # without sampler="device": today's route (sample_tokens with the torch-generator stream), the decoder stays greedy-only
    calls = []

    def spy(*a, **k):
        calls.append(k)
        return real(*a, **k)

    pol = ARPolicy(Policy(model, use_graph=False), sample_kwargs={"max_decoding_steps": STEPS, "temperature": 1.0}, use_graph=True)
    assert pol._decoder is not None and not pol._decoder.sampling
    monkeypatch.setattr(model, "sample_tokens", spy)
    tok = pol.infer(reqs[0])["tokens"]
    monkeypatch.setattr(model, "sample_tokens", real)
    assert len(calls) == 1 and "sampler" not in calls[0]
    assert np.array_equal(tok, model.sample_tokens(1, pols[0]._base._to_observation(reqs[0])[0], max_decoding_steps=STEPS, temperature=1.0).cpu().numpy())
    with pytest.raises(ValueError):
        ARPolicy(Policy(model, use_graph=False), sample_kwargs={"sampler": "gpu"})
