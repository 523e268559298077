"""Token log-probabilities and best-of-N decoding in the fused LAP_AR decoder (GPU): lap_decode_lm_head_lp / lap_decode_finish_lp
against the float64 restatement `sampling.token_logprobs`, and their model / serving surface.

Reference and bound.  The reference is `token_logprobs` evaluated on the raw f32 logits that the SAME launch wrote (its debug
output), so the error of the dot products, which tests/test_decode_kernels_f64_gpu.py bounds, cancels: what is left is the float32
arithmetic of z = logit * inv_t -> (M, S) -> z_tok - (M + log S).  `_f32_deviation` restates that arithmetic in float32 numpy in
three summation orders (sequential running pair, pairwise sum, the kernel's unit / wave / block order) on the very logits of the
case, takes the largest |float32 - float64| over every row, every vocabulary entry of the set and the three orders, and the device
is allowed 4x that (the margin of tests/decode_reference.py for order-dependent float32 sums).  Nothing is hard-coded; the values
measured on an MI355X are in docs/EXPERIMENTS.md (section "Token log-probabilities and best-of-N").
Across routes (eager / fused see different logits) the bound is the bf16 logit criterion of test_sample_tokens_matches_oracle, a
relative Frobenius error of 1e-2, taken as the per-entry perturbation d = 1e-2 |z row|_2 and propagated through the log-softmax:
a perturbation of at most d in every logit moves logp by at most 2 d.  That is a worst case: at V = 16384 it comes to one to
several nats, so the eager-against-fused comparison of logp asserts little beyond the equality of the tokens; the accuracy check of
every route is the one against float64 on its own logits (`_own_logit_check`).
"""
import functools

import numpy as np
import pytest
import torch

from lap_amd import sampling as S
from oracle import lap_oracle as O
from tests.common import make_inputs, oracle_cfg, to_observation

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 5e-2                   # tests/test_ar_sampling_gpu.py's MARGIN on scores (cross-route token agreement)
ORDER_MARGIN = 4.0              # allowed multiple of the float32 restatement's own deviation (tests/decode_reference.py)
TIE = 4 * 3.814697265625e-06    # tests/test_ar_sampling_gpu.py's allowance on a device draw's host-restated score
ROUTE_REL = 1e-2                # test_sample_tokens_matches_oracle's bf16 logit criterion
D = 2048
LM_BLOCKS = 1024


# --------------------------------------------------------------------------------------- helpers of test_ar_sampling_gpu.py
def _state(hip, B, t, plen, done=0):
    st = hip.decode_state(B, DEV)
    st[0], st[1] = t, done
    st[16:16 + B] = torch.as_tensor(plen, dtype=torch.int32)
    return st


def _bf(*shape, scale=1.0, g=None):
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(torch.bfloat16)


@pytest.fixture(scope="module", autouse=True)
def _hand_back_stream_scratch(hip):
    """Captured decoders warm up on fresh side streams, each of which gets a split-K scratch for the life of the process: hand
    back the ones this module caused (as tests/test_ar_sampling_gpu.py does)."""
    import gc

    before = set(hip._SCRATCH)
    yield
    for k in set(hip._SCRATCH) - before:
        del hip._SCRATCH[k]
    gc.collect()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _tables(V):
    """One table per V, in the three forms the LM heads stream: (hi, lo, None), (hi, None, None), (codes, None, scales)."""
    from lap_amd import hip

    g = torch.Generator(device=DEV).manual_seed(700 + V)
    table = torch.randn(V, D, generator=g, device=DEV) * 0.03
    hi, lo = hip.split_f32_hilo(table)
    codes, scales = hip.quantize_fp8_rows(table)
    gamma = torch.randn(D, generator=g, device=DEV) * 0.1
    return {"hilo": (hi, lo, None), "hi": (hi, None, None), "fp8": (codes, None, scales)}, gamma


def _x(B, V):
    return _bf(B, D, g=torch.Generator(device=DEV).manual_seed(900 + 10 * B + V % 7))


# ------------------------------------------------------------------------------------------- the float32 restatement
def _push(z, m, s):
    """lse_push of csrc/decode.hip in float32 numpy, elementwise over arrays."""
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.where(np.isneginf(m) | np.isneginf(z), np.float32(0), np.exp(-np.abs(z - m), dtype=np.float32))
    up = z > m
    s = np.where(up, s * e + np.float32(1), s + e).astype(np.float32)
    return np.where(up, z, m).astype(np.float32), s


def _merge(m2, s2, m, s):
    M = np.maximum(m, m2)
    with np.errstate(invalid="ignore"):
        a = np.where(np.isneginf(m), np.float32(0), s * np.exp(m - M, dtype=np.float32))
        b = np.where(np.isneginf(m2), np.float32(0), s2 * np.exp(m2 - M, dtype=np.float32))
    return M, (a + b).astype(np.float32)


def _lse_orders(z, subset):
    """z: float32 [B, n] (the set's entries in id order).  (M + log S) in float32, three orders: [3][B]."""
    B, n = z.shape
    out = []
    # sequential running pair
    m = np.full(B, -np.inf, np.float32)
    s = np.zeros(B, np.float32)
    for j in range(n):
        m, s = _push(z[:, j], m, s)
    out.append(m + np.log(s, dtype=np.float32))
    # maximum first, then numpy's pairwise float32 sum
    M = z.max(1)
    out.append(M + np.log(np.exp(z - M[:, None], dtype=np.float32).sum(1, dtype=np.float32), dtype=np.float32))
    # the kernel: unit u = entries 2u, 2u + 1; full: u = 4 block + wave (+ 4096 k); subset: u = block + 1024 wave (+ 4096 k);
    # a wave pushes its units' entries in order, a block merges its waves in order, the finish adds s_k exp(m_k - M) in block order
    units = (n + 1) // 2
    rounds = (units + 4 * LM_BLOCKS - 1) // (4 * LM_BLOCKS)
    zp = np.full((B, 2 * rounds * 4 * LM_BLOCKS), -np.inf, np.float32)
    zp[:, :n] = z
    zu = zp.reshape(B, rounds, 4 * LM_BLOCKS, 2)
    zu = zu.reshape(B, rounds, 4, LM_BLOCKS, 2).transpose(0, 3, 2, 1, 4) if subset else zu.reshape(B, rounds, LM_BLOCKS, 4, 2).transpose(0, 2, 3, 1, 4)
    zu = zu.reshape(B, LM_BLOCKS, 4, 2 * rounds)           # [B, block, wave, the wave's entries in order]
    m = np.full((B, LM_BLOCKS, 4), -np.inf, np.float32)
    s = np.zeros((B, LM_BLOCKS, 4), np.float32)
    for j in range(2 * rounds):
        m, s = _push(zu[..., j], m, s)
    bm, bs = m[..., 0], s[..., 0]
    for w in range(1, 4):
        bm, bs = _merge(m[..., w], s[..., w], bm, bs)
    M = bm.max(1)
    with np.errstate(invalid="ignore"):
        term = np.where(np.isneginf(bm), np.float32(0), bs * np.exp(bm - M[:, None], dtype=np.float32)).astype(np.float32)
    Ssum = np.zeros(B, np.float32)
    for k in range(LM_BLOCKS):
        Ssum = Ssum + term[:, k]
    out.append(M + np.log(Ssum, dtype=np.float32))
    return out


def _f32_deviation(logits, inv_t, ids=None):
    """float64 [rows]: the largest |float32 restatement - float64| of logp over every entry of the set and the three orders."""
    lg = np.asarray(logits, dtype=np.float32)
    if ids is not None:
        lg = lg[:, np.asarray(ids)]
    z = (lg * np.float32(inv_t)).astype(np.float32) if inv_t != 0.0 else lg
    z64 = z.astype(np.float64)
    m = z64.max(1, keepdims=True)
    ref = z64 - (m + np.log(np.exp(z64 - m).sum(1, keepdims=True)))
    return np.max([np.abs((z - lse[:, None]).astype(np.float32).astype(np.float64) - ref).max(1) for lse in _lse_orders(z, ids is not None)], 0)


def _bound(logits, temperature, ids=None):
    """What the device may differ by from float64 on these logits: 4x the largest deviation of the restatement over the case."""
    return ORDER_MARGIN * float(_f32_deviation(logits, float(S.inverse_temperature(temperature)), ids).max())


# ------------------------------------------------------------------------------------------------------------- kernels
def _run_heads(hip, B, V, form, temperature, *, ids=None, gamma=None, t=2, seed=0xC0FFEE1234, cap=6):
    """The existing head + finish and the _lp pair on the same inputs.  Returns a dict of everything they wrote."""
    (hi, lo, ws), g0 = _tables(V)[0][form], _tables(V)[1]
    gamma = g0 if gamma is None else gamma
    x = _x(B, V)
    kw = {}
    if ws is not None:
        kw["wscale"] = ws
    if ids is not None:
        kw["ids"] = ids
    samp = None
    if temperature is not None:
        samp = hip.decode_sampling(DEV)
        hip.decode_set_sampling(samp, seed, temperature)
    r = {}
    for name in ("old", "new"):
        st = _state(hip, B, t, [5] * B)
        out = torch.zeros(B, cap, dtype=torch.int32, device=DEV)
        pval, pidx = hip.decode_lm_partials(B, DEV)
        pval.fill_(7.0); pidx.fill_(-7)
        lg = torch.full((B, V), float("-inf"), device=DEV)
        if name == "old":
            if samp is None:
                hip.decode_lm_head(st, x, gamma, hi, lo, pval, pidx, logits=lg, **kw)
            else:
                hip.decode_lm_head_sample(st, samp, x, gamma, hi, lo, pval, pidx, logits=lg, **kw)
            hip.decode_finish(st, pval, pidx, out, eos_token=-1)
        else:
            plp = hip.decode_lm_logp_partials(B, DEV)
            plp.fill_(float("nan"))
            logp = torch.zeros(B, cap, device=DEV)
            hip.decode_lm_head_lp(st, samp, x, gamma, hi, lo, pval, pidx, plp, logits=lg, **kw)
            hip.decode_finish_lp(st, pval, pidx, plp, out, logp, eos_token=-1)
            r["plp"], r["logp"] = plp, logp
        r[name] = (pval, pidx, lg, out, st)
    return r


def _check_bits(r):
    for a, b in zip(r["old"], r["new"]):
        assert torch.equal(a, b)


def _check_logp(r, temperature, t=2, ids=None, what=""):
    lg = r["new"][2].cpu().numpy()
    tok = r["new"][3][:, t].cpu().numpy()
    T = 0.0 if temperature is None else temperature
    want = S.token_logprobs(lg, tok, T, allowed=ids)
    got = r["logp"][:, t].cpu().numpy().astype(np.float64)
    bound = _bound(lg, T, ids)
    err = np.abs(got - want)
    print(f"{what}: logp {got.tolist()}, |device - float64| {err.max():.3e}, float32 restatement {bound / ORDER_MARGIN:.3e}, "
          f"bound {bound:.3e}")
    assert np.isfinite(got).all() and (got <= 0).all()
    assert (err <= bound).all(), (what, err, bound)
    cols = [c for c in range(r["logp"].shape[1]) if c != t]
    assert float(r["logp"][:, cols].abs().sum()) == 0.0      # only column t is written
    return err, bound


@pytest.mark.parametrize("temperature", [None, 0.7, 2.0])
@pytest.mark.parametrize("form", ["hilo", "hi", "fp8"])
@pytest.mark.parametrize("V", [4097, 16384])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_lm_head_lp_bits_and_logp(hip, B, V, form, temperature):
    r = _run_heads(hip, B, V, form, temperature)
    _check_bits(r)
    assert bool(torch.isfinite(r["new"][2]).all())
    _check_logp(r, temperature, what=f"B {B} V {V} {form} T {temperature}")
    plp = r["plp"].cpu().numpy()
    assert not np.isnan(plp).any()
    has = np.isfinite(plp[..., 0])              # (V = 4097 leaves the blocks past its 2049 units without a row: neutral partials)
    assert (plp[..., 1][has] >= 1.0).all() and (plp[..., 1][~has] == 0.0).all() and np.isneginf(plp[..., 0][~has]).all()


@pytest.mark.parametrize("temperature", [None, 0.7])
@pytest.mark.parametrize("form", ["hilo", "fp8"])
@pytest.mark.parametrize("n", [1, 37, 700])
def test_subset_lp(hip, n, form, temperature):
    B, V = 3, 4097
    g = torch.Generator().manual_seed(n)
    ids = torch.sort(torch.randperm(V, generator=g)[:n]).values.to(torch.int32)
    if n > 1:
        ids[-1] = V - 1                         # the odd vocabulary's last row is in the set
    r = _run_heads(hip, B, V, form, temperature, ids=ids.to(DEV))
    _check_bits(r)
    _check_logp(r, temperature, ids=ids.numpy(), what=f"subset n {n} {form} T {temperature}")
    plp = r["plp"].cpu().numpy()
    used = min((n + 1) // 2, LM_BLOCKS)
    assert np.isneginf(plp[used:, :, 0]).all() and (plp[used:, :, 1] == 0).all()      # the neutral partials
    assert np.isfinite(plp[:used, :, 0]).all()
    if n == 1:
        lp = r["logp"][:, 2].cpu().numpy()
        assert (lp == 0.0).all() and bool((r["new"][3][:, 2] == int(ids[0])).all())


@pytest.mark.parametrize("n", [37, 700])
def test_subset_lp_leaves_out_an_id_outside_the_vocabulary(hip, n):
    B, V, T = 3, 4097, 0.7
    g = torch.Generator().manual_seed(50 + n)
    ids = torch.sort(torch.randperm(V, generator=g)[:n]).values.to(torch.int32)
    # the best row of the whole set is replaced by V + 5 (kept in place: the kernel never orders the ids)
    whole = _run_heads(hip, B, V, "hilo", T, ids=ids.to(DEV))
    gone = int(np.flatnonzero(ids.numpy() == int(whole["new"][3][0, 2]))[0])
    broken = ids.clone()
    broken[gone] = V + 5
    r = _run_heads(hip, B, V, "hilo", T, ids=broken.to(DEV))
    _check_bits(r)
    rest = np.delete(ids.numpy(), gone)
    assert int(r["new"][3][0, 2]) != int(ids[gone])
    _check_logp(r, T, ids=rest, what=f"n {n} with ids[{gone}] = V + 5")
    # and it differs from the whole set's by that row's mass
    assert float((r["logp"][:, 2] - whole["logp"][:, 2]).abs().max()) > 0


def test_large_logits_stay_finite(hip):
    """Final-norm gamma scaled so that |logit| reaches ~100 at inv_t ~ 1.43: no overflow, logp finite, <= 0, within the bound."""
    B, V, T = 3, 16384, 0.7
    gamma = (1.0 + _tables(V)[1]) * 18.0 - 1.0
    for form in ("hilo", "fp8"):
        r = _run_heads(hip, B, V, form, T, gamma=gamma)
        _check_bits(r)
        peak = float(r["new"][2].abs().max())
        assert 80.0 < peak < 400.0, peak
        _check_logp(r, T, what=f"|logit| up to {peak:.1f}, {form}")
        assert bool(torch.isfinite(r["plp"]).all())


@pytest.mark.parametrize("ids_n", [None, 37])
def test_done_state_writes_nothing(hip, ids_n):
    B, V = 3, 4097
    (hi, lo, _), gamma = _tables(V)[0]["hilo"], _tables(V)[1]
    ids = None if ids_n is None else torch.arange(0, 2 * ids_n, 2, dtype=torch.int32, device=DEV)
    samp = hip.decode_sampling(DEV)
    hip.decode_set_sampling(samp, 5, 1.0)
    st = _state(hip, B, 3, [20] * B, done=1)
    st0 = st.clone()
    pval, pidx = hip.decode_lm_partials(B, DEV)
    pval.fill_(3.0); pidx.fill_(11)
    plp = hip.decode_lm_logp_partials(B, DEV)
    plp.fill_(9.0)
    logp = torch.full((B, 16), -2.0, device=DEV)
    lg = torch.full((B, V), 5.0, device=DEV)
    out = torch.randint(0, 9, (B, 16), dtype=torch.int32, device=DEV)
    out0 = out.clone()
    hip.decode_lm_head_lp(st, samp, _x(B, V), gamma, hi, lo, pval, pidx, plp, logits=lg, ids=ids)
    hip.decode_finish_lp(st, pval, pidx, plp, out, logp, eos_token=1)
    torch.cuda.synchronize()
    assert torch.equal(st, st0) and torch.equal(out, out0)
    assert bool((pval == 3.0).all()) and bool((pidx == 11).all()) and bool((lg == 5.0).all())
    assert bool((plp == 9.0).all()) and bool((logp == -2.0).all())


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


EMBED_SCALE = 0.05              # tests/test_ar_sampling_gpu.py: the tied LM head's margins shrink to the spread of the noise
STEPS = 6
SEED_CANDIDATES = tuple(range(1, 17))
SHARE = 0.75                    # of the compared (row, step) entries, the least that must survive the margin filter


def _model(scale):
    from lap_amd.model import LAP

    with pytest.MonkeyPatch.context() as mp:
        cfg = _gemma2b_x2_cfg(mp)
        P = O.init_params(oracle_cfg(cfg), seed=13)
        key = "PaliGemma/llm/embedder/input_embedding"
        P[key] = torch.as_tensor(P[key]).clone() * scale
        model = LAP(cfg, params=P, device=DEV)
        model.EOS_TOKEN = -1    # no row stops early: every step of the budget is compared
        yield cfg, model
        model.EOS_TOKEN = 1


@pytest.fixture(scope="module")
def ar(hip):
    """(cfg, model) with the embedding table scaled by EMBED_SCALE: nearly flat logits, so that draws spread (sampled cases)."""
    yield from _model(EMBED_SCALE)


@pytest.fixture(scope="module")
def ar_sharp(hip):
    """(cfg, model) with the table as initialised: the tied LM head echoes the last token with a top-2 logit margin of 12 - 14
    (tests/test_ar_sampling_gpu.py), which a greedy comparison across routes needs: on the flat model the greedy margins of the
    first token are 0.005 - 0.02 (measured), below MARGIN in every row."""
    yield from _model(1.0)


def _obs(cfg, B=3):
    obs, _, _, _ = make_inputs(cfg, B=B, ragged=True)
    so = dict(obs)
    so.pop("tokenized_langact_mask")
    so["image_masks"] = {k: torch.ones_like(m) for k, m in so["image_masks"].items()}
    return to_observation(so | {"tokenized_langact_mask": None}, DEV)


def _margins(logits, temperature, seed, step):
    sc = S.scores_from_logits(logits.detach().float().cpu().numpy(), temperature, seed, step)
    top2 = np.partition(sc, -2, axis=1)[:, -2:]
    return top2[:, 1] - top2[:, 0]


def _clear_prefix(col, temperature, seed, steps):
    """bool [rows, steps]: the steps of a row before the first one whose top-2 score margin does not exceed MARGIN (until then
    another route has the same context in that row)."""
    ok = np.stack([_margins(col[f"logit/{s}"], temperature, seed, s) > MARGIN for s in range(steps)], 1)
    return np.cumprod(ok, axis=1).astype(bool)


def _own_logit_check(name, tok, lp, col, temperature, allowed):
    steps = tok.shape[1]
    ids = None if allowed is None else np.asarray(allowed)
    lg = np.concatenate([col[f"logit/{s}"].cpu().numpy() for s in range(steps)], 0)           # [steps * rows, V]: one pass
    toks = tok.cpu().numpy().T.reshape(-1)
    want = S.token_logprobs(lg, toks, temperature, allowed=ids)
    bound = _bound(lg, temperature, ids)
    err = np.abs(lp.cpu().numpy().T.reshape(-1).astype(np.float64) - want)
    print(f"{name}: |logp - float64 on its own logits| up to {err.max():.3e}, bound {bound:.3e}")
    assert (err <= bound).all(), (name, err, bound)


def _allowed_ids(cfg):
    g = torch.Generator().manual_seed(3)
    ids = torch.randperm(cfg.vocab_size, generator=g)[:2001]
    return torch.unique(ids)


@pytest.mark.parametrize("constrained", [False, True])
@pytest.mark.parametrize("temperature", [0.0, 1.0])
def test_routes_return_logprobs(request, temperature, constrained):
    from lap_amd.serve import GraphedTokenDecoder

    cfg, model = request.getfixturevalue("ar" if temperature > 0.0 else "ar_sharp")
    o = _obs(cfg)
    allowed = _allowed_ids(cfg) if constrained else None
    if constrained and temperature <= 0.0:
        # greedy: the set also holds the tokens of the unconstrained greedy decode, so that the constrained decode keeps their clear
        # margins (among 2001 random ids alone the best two lie closer than MARGIN); the softmax still runs over the set only
        free = model.sample_tokens(0, o, max_decoding_steps=STEPS)
        allowed = torch.unique(torch.cat([allowed, free.reshape(-1).cpu().long()]))
    akw = {"allowed_tokens": allowed} if constrained else {}
    base = dict(max_decoding_steps=STEPS, temperature=temperature, sampler="device", **akw)
    # a seed for which the eager route alone keeps the share of clear (row, step) entries
    for seed in SEED_CANDIDATES:
        cole = {}
        tok_e, lp_e = model.sample_tokens(seed, o, return_logprobs=True, collect=cole, **base)
        clear = _clear_prefix(cole, temperature, seed, STEPS)
        if clear.mean() >= SHARE:
            break
    else:
        pytest.fail(f"no seed of {SEED_CANDIDATES} keeps {SHARE} of the steps clear of the margin {MARGIN}")
    assert clear.mean() >= SHARE
    assert lp_e.shape == (3, STEPS) and lp_e.dtype == torch.float32
    assert torch.equal(tok_e, model.sample_tokens(seed, o, **base))
    colf = {}
    tok_f, lp_f = model.sample_tokens(seed, o, decode="fused", return_logprobs=True, collect=colf, **base)
    tok_n, lp_n = model.sample_tokens(seed, o, decode="fused", return_logprobs=True, **base)
    assert torch.equal(tok_f, tok_n) and torch.equal(lp_f, lp_n)
    assert torch.equal(tok_n, model.sample_tokens(seed, o, decode="fused", **base))
    dec = GraphedTokenDecoder(model, 3, STEPS, sampling=True, logprobs=True, **akw)
    tok_g, lp_g = dec(o, temperature=temperature, seed=seed)
    assert torch.equal(tok_g, tok_n) and torch.equal(lp_g, lp_n)          # the replay is the fused route bit for bit
    assert torch.equal(tok_g, GraphedTokenDecoder(model, 3, STEPS, sampling=True, **akw)(o, temperature=temperature, seed=seed))
    assert dec.ctx.logp.data_ptr() != lp_g.data_ptr()
    # each route against the float64 restatement on its own logits
    ids = None if allowed is None else allowed.numpy()
    _own_logit_check("eager", tok_e, lp_e, cole, temperature, ids)
    _own_logit_check("fused", tok_f, lp_f, colf, temperature, ids)
    assert bool((lp_f <= 0).all())
    # eager against fused where the margins keep the contexts together: 2 d, d = ROUTE_REL |z row|_2
    inv_t = float(S.inverse_temperature(temperature)) or 1.0
    compared = 0
    for s in range(STEPS):
        lg = cole[f"logit/{s}"].double().cpu().numpy()
        z = np.where(np.isneginf(lg), 0.0, lg) * inv_t
        d = ROUTE_REL * np.sqrt((z * z).sum(1))
        for b in np.flatnonzero(clear[:, s]):
            assert int(tok_f[b, s]) == int(tok_e[b, s]), (b, s)
            assert abs(float(lp_f[b, s]) - float(lp_e[b, s])) <= 2 * d[b], (b, s, float(lp_f[b, s]), float(lp_e[b, s]), d[b])
            compared += 1
    assert compared >= SHARE * 3 * STEPS
    print(f"T {temperature} constrained {constrained}: seed {seed}, {compared} of {3 * STEPS} (row, step) entries compared")


@pytest.mark.parametrize("temperature", [0.0, 1.0])
@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_fused_and_graphed_logprobs_on_the_flat_model(ar, weights, temperature):
    """Fused and graphed on the nearly flat model (log-probabilities around -log V, greedy ones included), bf16 and fp8 weights."""
    from lap_amd.serve import GraphedTokenDecoder

    cfg, model = ar
    o = _obs(cfg)
    base = dict(max_decoding_steps=STEPS, temperature=temperature, sampler="device", decode="fused", decode_weights=weights)
    col = {}
    tok_f, lp_f = model.sample_tokens(4, o, return_logprobs=True, collect=col, **base)
    tok_n, lp_n = model.sample_tokens(4, o, return_logprobs=True, **base)
    assert torch.equal(tok_f, tok_n) and torch.equal(lp_f, lp_n) and torch.equal(tok_n, model.sample_tokens(4, o, **base))
    tok_g, lp_g = GraphedTokenDecoder(model, 3, STEPS, sampling=True, weights=weights, logprobs=True)(o, temperature=temperature, seed=4)
    assert torch.equal(tok_g, tok_n) and torch.equal(lp_g, lp_n)
    _own_logit_check(f"fused {weights}", tok_f, lp_f, col, temperature, None)
    assert bool((lp_f < -1.0).all())


def _first_row(cfg):
    obs, _, _, _ = make_inputs(cfg, B=1, seed=1, ragged=True)
    so = dict(obs)
    so.pop("tokenized_langact_mask")
    so["image_masks"] = {k: torch.ones_like(m) for k, m in so["image_masks"].items()}
    return to_observation(so | {"tokenized_langact_mask": None}, DEV)


def test_best_of_n(ar):
    from lap_amd.serve import GraphedTokenDecoder

    cfg, model = ar
    o1 = _first_row(cfg)
    N, T = 4, 1.5
    kw = dict(max_decoding_steps=STEPS, temperature=T, sampler="device", decode="fused", num_samples=N)
    # the smallest seed whose first draws are clear of ties in every row (the choice is a function of the committed inputs)
    for seed in SEED_CANDIDATES:
        col = {}
        tok, lp = model.sample_tokens(seed, o1, collect=col, **kw)
        if bool((_margins(col["logit/0"], T, seed, 0) > MARGIN).all()):
            break
    else:
        pytest.fail("no seed with clear first draws")
    assert tok.shape == (N, STEPS) and tok.dtype == torch.int32 and lp.shape == (N, STEPS) and lp.dtype == torch.float32
    assert len({tuple(r) for r in tok.tolist()}) > 1                      # the rows are not one draw repeated
    # the prefix was prefilled once and copied: every row starts from the same logits
    lg0 = col["logit/0"]
    assert all(torch.equal(lg0[0], lg0[b]) for b in range(1, N))
    # ... which are the batch-1 decode's
    c1 = {}
    model.sample_tokens(seed, o1, max_decoding_steps=1, temperature=T, sampler="device", decode="fused", collect=c1)
    assert torch.equal(c1["logit/0"][0], lg0[0])
    # row b draws with Philox row b from its own logits, and its log-probabilities are the restatement's on those logits
    for s in range(STEPS):      # (the host's argmax, or within tests/test_ar_sampling_gpu.py's TIE of it: the last bits of the logarithms)
        sc = S.scores_from_logits(col[f"logit/{s}"].cpu().numpy(), T, seed, s)
        mine = sc[np.arange(N), tok[:, s].cpu().numpy()]
        assert (sc.max(1) - mine <= TIE).all(), s
    _own_logit_check("best-of-4", tok, lp, col, T, None)
    tok_n, lp_n = model.sample_tokens(seed, o1, **kw)
    assert torch.equal(tok_n, tok) and torch.equal(lp_n, lp)
    # one capture serves two seeds; the same seed twice gives the same bits
    dec = GraphedTokenDecoder(model, 1, STEPS, sampling=True, num_samples=N).capture()
    graphs, ctx = (dec.g_prefill, dec.g_step), dec.ctx
    a = dec(o1, temperature=T, seed=seed)
    b = dec(o1, temperature=T, seed=seed + 100)
    c = dec(o1, temperature=T, seed=seed)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    assert not torch.equal(a[0], b[0])
    assert torch.equal(a[0], tok) and torch.equal(a[1], lp)
    assert (dec.g_prefill, dec.g_step) == graphs and dec.ctx is ctx and ctx.B == N
    with pytest.raises(ValueError, match="temperature"):
        dec(o1, temperature=0.0)
    # the conditions, each named by its ValueError
    good = dict(max_decoding_steps=STEPS, temperature=T, sampler="device", decode="fused")
    for bad, word in (({"num_samples": 9}, "[1, 8]"), ({"num_samples": 0}, "[1, 8]"), ({"decode": "eager"}, "decode"),
                      ({"sampler": "host"}, "sampler"), ({"temperature": 0.0}, "temperature")):
        with pytest.raises(ValueError, match=word.replace("[", r"\[")):
            model.sample_tokens(1, o1, **({"num_samples": N} | good | bad))
    with pytest.raises(ValueError, match="batch 1"):
        model.sample_tokens(1, _obs(cfg), num_samples=N, **good)
    with pytest.raises(ValueError):
        GraphedTokenDecoder(model, 1, STEPS, num_samples=N)
    with pytest.raises(ValueError, match="batch 1"):
        GraphedTokenDecoder(model, 3, STEPS, sampling=True, num_samples=N)


@pytest.mark.parametrize("use_graph", [False, True])
def test_ar_policy_best_of_n(ar, use_graph):
    from lap_amd.serve import ARPolicy, Policy

    cfg, model = ar
    obs, _, _, _ = make_inputs(cfg, B=1, seed=2, ragged=True)
    req = {"image": {k: v[0].numpy() for k, v in obs["images"].items()}, "image_mask": {k: np.array(True) for k in obs["images"]},
           "state": obs["state"][0].numpy(), "tokenized_prompt": obs["tokenized_prompt"][0].numpy(),
           "tokenized_prompt_mask": obs["tokenized_prompt_mask"][0].numpy()}
    N = 4
    kw = {"max_decoding_steps": STEPS, "temperature": 1.5, "sampler": "device"}
    for select in ("sum", "mean"):
        pol = ARPolicy(Policy(model, use_graph=False), sample_kwargs=kw | {"num_samples": N, "select": select}, use_graph=use_graph)
        assert (pol._decoder is not None) == use_graph
        res = pol.infer(req)
        cand = res["candidates"]
        assert cand["tokens"].shape == (N, STEPS) and cand["logprob"].shape == (N,)
        o = pol._base._to_observation(req)[0]
        tok, lp = (t.cpu().numpy() for t in model.sample_tokens(1, o, decode="fused", num_samples=N, **kw))     # call counter 1
        assert np.array_equal(cand["tokens"], tok)
        assert np.array_equal(cand["logprob"], S.sequence_logprob(tok, lp, model.EOS_TOKEN))
        best = S.select_best(tok, lp, model.EOS_TOKEN, select)
        assert res["tokens"].shape == (1, STEPS) and np.array_equal(res["tokens"][0], tok[best])
        assert np.array_equal(res["token_logprobs"][0], lp[best])
        assert res["logprob"].shape == (1,) and float(res["logprob"][0]) == float(S.sequence_logprob(tok, lp, model.EOS_TOKEN)[best])
    # return_logprobs alone: one decode, its log-probabilities and their sum
    pol = ARPolicy(Policy(model, use_graph=False), sample_kwargs=kw | {"return_logprobs": True}, use_graph=use_graph)
    res = pol.infer(req)
    assert "candidates" not in res and res["tokens"].shape == (1, STEPS) and res["token_logprobs"].shape == (1, STEPS)
    assert float(res["logprob"][0]) == float(S.sequence_logprob(res["tokens"], res["token_logprobs"], model.EOS_TOKEN)[0])
    with pytest.raises(ValueError, match="select"):
        ARPolicy(Policy(model, use_graph=False), sample_kwargs=kw | {"num_samples": N, "select": "max"})
    with pytest.raises(ValueError, match="temperature"):
        ARPolicy(Policy(model, use_graph=False), sample_kwargs={"num_samples": N, "sampler": "device"})
