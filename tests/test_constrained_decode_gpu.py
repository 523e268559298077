"""Constrained-vocabulary decoding of the fused LAP_AR decoder (GPU): the subset LM heads of csrc/decode.hip
(lap_decode_lm_head_subset*) and `allowed_tokens=` of `LAP.sample_tokens`, `GraphedTokenDecoder` and `ARPolicy`.

Bounds.  The subset kernel runs the full kernel's dot product of a vocabulary row (same k-to-lane map, same order of additions,
same wave_sum), so every comparison of logits, partials and greedy tokens with the unconstrained kernels is torch.equal: no
tolerance, no margin rule.  A sampled draw on a proper subset is checked against the host restatement of the noise
(lap_amd.sampling.scores_from_logits on the logits masked to -inf outside the set) under the draw rule of
tests/test_ar_sampling_gpu.py: the pick is the host argmax or lies within TIE = 4 x 3.814697265625e-06 of it (the score error
measured there), at most 1 draw in 1,000 may use the allowance, and the draws whose host top-2 margin is within 2 TIE are counted
on the CPU and held to the same cap.  Eager against fused tokens: the MARGIN = 5e-2 rule of tests/test_ar_decode_gpu.py, on the
masked eager logits.
"""
import numpy as np
import pytest
import torch

from lap_amd import sampling as S
from oracle import lap_oracle as O
from tests.common import make_inputs, oracle_cfg, to_observation

pytestmark = pytest.mark.gpu
DEV = "cuda"
TIE = 4 * 3.814697265625e-06        # tests/test_ar_sampling_gpu.py: four times the measured score error
ALLOWANCE_CAP = 1e-3
MARGIN = 5e-2                       # tests/test_ar_decode_gpu.py
D = 2048
V_ODD, V_LOOP, V_FULL = 4097, 16385, 257152
CAP, T0 = 8, 2                      # token columns of `out`; the step the kernel tests decode at
NEG_INF = float("-inf")


@pytest.fixture(scope="module", autouse=True)
def _hand_back_stream_scratch(hip):
    """Captured decoders warm up on fresh side streams and lap_amd.hip keeps a split-K scratch per stream: hand them back."""
    import gc

    before = set(hip._SCRATCH)
    yield
    for k in set(hip._SCRATCH) - before:
        del hip._SCRATCH[k]
    gc.collect()
    torch.cuda.empty_cache()


def _state(hip, B, t, plen, done=0):
    st = hip.decode_state(B, DEV)
    st[0], st[1] = t, done
    st[16:16 + B] = torch.as_tensor(plen, dtype=torch.int32)
    return st


def _ids(v):
    return torch.as_tensor(sorted(set(int(i) for i in v)), dtype=torch.int32, device=DEV)


def _random_ids(V, n, seed, must=()):
    g = torch.Generator(device="cpu").manual_seed(seed)
    pick = set(int(i) for i in must)
    for i in torch.randperm(V, generator=g).tolist():
        if len(pick) >= n:
            break
        pick.add(i)
    return _ids(pick)


class _Inputs:
    """Table planes, gamma, x of one (B, V) and, computed once, what the unconstrained kernels give on them."""

    def __init__(self, hip, B, V, seed, tie_rows=None):
        g = torch.Generator(device=DEV).manual_seed(seed)
        table = torch.randn(V, D, generator=g, device=DEV) * 0.03
        if tie_rows is not None:        # two equal rows: equal logits, bit for bit
            table[tie_rows[1]] = table[tie_rows[0]]
        self.hi, self.lo = hip.split_f32_hilo(table)
        self.table = table
        self.gamma = torch.randn(D, generator=g, device=DEV) * 0.1
        self.x = (torch.randn(B, D, generator=g, device=DEV)).to(torch.bfloat16)
        self.B, self.V = B, V
        self._f8 = None
        self._full = {}

    def planes(self, hip, f8):
        if not f8:
            return self.hi, self.lo, {}
        if self._f8 is None:
            self._f8 = hip.quantize_fp8_rows(self.table)
        return self._f8[0], None, {"wscale": self._f8[1]}

    def full(self, hip, f8=False):
        """(logits, greedy token) of the unconstrained kernel."""
        if f8 not in self._full:
            r = _run(hip, self, f8=f8)
            self._full[f8] = (r["lg"], r["tok"])
        return self._full[f8]


def _run(hip, inp, ids=None, samp=None, f8=False, t=T0, want_logits=True):
    """One LM head + finish at step t: the debug logits (pre-filled with -inf), the token, the partials, the state, out."""
    B, V = inp.B, inp.V
    hi, lo, kw = inp.planes(hip, f8)
    if ids is not None:
        kw = dict(kw, ids=ids)
    st = _state(hip, B, t, [5] * B)
    out = torch.zeros(B, CAP, dtype=torch.int32, device=DEV)
    pval, pidx = hip.decode_lm_partials(B, DEV)
    pval.fill_(7.0); pidx.fill_(-7)
    lg = torch.full((B, V), NEG_INF, device=DEV) if want_logits else None
    if samp is None:
        hip.decode_lm_head(st, inp.x, inp.gamma, hi, lo, pval, pidx, logits=lg, **kw)
    else:
        hip.decode_lm_head_sample(st, samp, inp.x, inp.gamma, hi, lo, pval, pidx, logits=lg, **kw)
    pv, pi = pval.clone(), pidx.clone()
    hip.decode_finish(st, pval, pidx, out, eos_token=-1)
    return dict(lg=lg, tok=out[:, t].clone(), pval=pv, pidx=pi, st=st, out=out)


def _masked(lg, ids):
    m = torch.full_like(lg, NEG_INF)
    m[:, ids.long()] = lg[:, ids.long()]
    return m


def _first_argmax(lg):
    """argmax per row, the lowest index among ties (numpy's rule), as int32 on the device."""
    return torch.from_numpy(np.argmax(lg.detach().cpu().numpy(), axis=1).astype(np.int32)).to(DEV)


def _check_logits_and_greedy(hip, inp, ids, f8=False):
    """Criteria 1 and 2: logits equal to the full kernel's at the allowed indices and -inf elsewhere; the token is the masked
    argmax with the lowest index among ties; state and out advance as with the full kernel."""
    full_lg, _ = inp.full(hip, f8)
    want = _masked(full_lg, ids)
    r = _run(hip, inp, ids=ids, f8=f8)
    assert torch.equal(r["lg"], want)
    assert torch.equal(r["tok"], _first_argmax(want))
    ref = _run(hip, inp, f8=f8, want_logits=False)
    assert torch.equal(r["st"], ref["st"]) and int(r["st"][0]) == T0 + 1 and int(r["st"][1]) == 0
    cols = [c for c in range(CAP) if c != T0]
    assert int(r["out"][:, cols].abs().sum()) == 0
    # partials carry vocabulary ids of the set (or the neutral pair), and there are as many as ever
    pi = r["pidx"].cpu()
    assert pi.numel() == ref["pidx"].numel()
    assert bool((torch.isin(pi, ids.cpu()) | (pi == 0x7fffffff)).all())
    # without the debug output: the same partials
    r2 = _run(hip, inp, ids=ids, f8=f8, want_logits=False)
    assert torch.equal(r2["pval"], r["pval"]) and torch.equal(r2["pidx"], r["pidx"])
    return r


_CACHE = {}


def _inputs(hip, B, V):
    key = (B, V)
    if key not in _CACHE:
        _CACHE[key] = _Inputs(hip, B, V, 700 + B + V % 1000, tie_rows=(7, 4000) if V == V_ODD else None)
    return _CACHE[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_inputs():
    yield
    _CACHE.clear()


# ------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("B", [1, 3, 8])
def test_subset_logits_are_the_full_kernels_and_greedy_is_exact(hip, B):
    V = V_ODD
    inp = _inputs(hip, B, V)
    sets = [_ids([0, V - 1]), _ids([1234]), _random_ids(V, 301, 11), _ids([7, 4000])]
    for ids in sets:
        r = _check_logits_and_greedy(hip, inp, ids)
        assert bool(torch.isin(r["tok"].cpu(), ids.cpu()).all())
    # rows 7 and 4000 of the table are equal: a tie, and the lowest index wins
    assert bool((r["lg"][:, 7] == r["lg"][:, 4000]).all()) and r["tok"].tolist() == [7] * B
    # fp8: the one e4m3 plane with its row scales
    _check_logits_and_greedy(hip, inp, sets[2], f8=True)


@pytest.mark.parametrize("f8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_the_full_set_is_the_identity(hip, B, f8):
    V = V_ODD
    inp = _inputs(hip, B, V)
    every = torch.arange(V, dtype=torch.int32, device=DEV)
    full_lg, full_tok = inp.full(hip, f8)
    r = _run(hip, inp, ids=every, f8=f8)
    assert torch.equal(r["lg"], full_lg) and torch.equal(r["tok"], full_tok)
    samp = hip.decode_sampling(DEV)
    for temp, seed in ((1.0, 0xDEADBEEF12345), (0.5, 99)):
        hip.decode_set_sampling(samp, seed, temp)
        want = _run(hip, inp, samp=samp, f8=f8)
        got = _run(hip, inp, ids=every, samp=samp, f8=f8)
        assert torch.equal(got["tok"], want["tok"]) and torch.equal(got["lg"], full_lg)
    # inv_t = 0 on the sampling instance: the greedy subset partials bit for bit
    for ids in (every, _random_ids(V, 301, 11)):
        greedy = _run(hip, inp, ids=ids, f8=f8)
        for temp, seed in ((None, 0), (0.0, 5), (-2.0, 5)):
            if temp is None:
                samp.zero_()
            else:
                hip.decode_set_sampling(samp, seed, temp)
            got = _run(hip, inp, ids=ids, samp=samp, f8=f8)
            assert torch.equal(got["pval"], greedy["pval"]) and torch.equal(got["pidx"], greedy["pidx"])
            assert torch.equal(got["lg"], greedy["lg"]) and torch.equal(got["tok"], greedy["tok"])


def test_the_grid_stride_loop_runs(hip):
    """10,001 ids are 5,001 units: more than four waves times the grid of lap_decode_lm_blocks() = 1024 blocks."""
    B, V = 3, V_LOOP
    assert (10001 + 1) // 2 > 4 * hip._fn["lap_decode_lm_blocks"]()
    inp = _inputs(hip, B, V)
    _check_logits_and_greedy(hip, inp, _random_ids(V, 10001, 12, must=(0, V - 1)))


@pytest.mark.parametrize("B", [1, 3, 8])
def test_sampling_on_a_proper_subset(hip, B):
    V = V_ODD
    inp = _inputs(hip, B, V)
    full_lg, _ = inp.full(hip)
    pairs = _ids([2 * m + e for m in (0, 17, 600, 2047) for e in (0, 1)] + [V - 1])       # 2m, 2m + 1 share a Philox block
    apart = _ids(list(range(0, V, 14)) + [3, 4001])                                        # every j >> 1 differs
    assert len(set((apart.cpu() >> 1).tolist())) == apart.numel()
    sets = [("pairs", pairs), ("apart", apart), ("random", _random_ids(V, 301, 13))]
    samp = hip.decode_sampling(DEV)
    draws = allowed = close = 0
    toks = {2: [], 5: []}
    for temp, seed in ((1.0, 0x5EED0001), (0.5, 1234567890123)):
        hip.decode_set_sampling(samp, seed, temp)
        for name, ids in sets:
            masked = _masked(full_lg, ids).cpu().numpy()
            for t in (2, 5):
                r = _run(hip, inp, ids=ids, samp=samp, t=t)
                assert torch.equal(r["lg"], _masked(full_lg, ids))         # the debug logits stay raw
                with np.errstate(invalid="ignore"):
                    sc = S.scores_from_logits(masked, temp, seed, t)
                tok = r["tok"].cpu().numpy()
                top2 = np.partition(sc, -2, axis=1)[:, -2:]
                close += int(((top2[:, 1] - top2[:, 0]) <= 2 * TIE).sum())
                for b in range(B):
                    draws += 1
                    assert int(tok[b]) in set(ids.tolist()), (name, temp, t, b, int(tok[b]))
                    best = int(np.argmax(sc[b]))
                    if int(tok[b]) != best:
                        gap = float(sc[b, best] - sc[b, int(tok[b])])
                        assert gap <= TIE, (name, temp, t, b, int(tok[b]), best, gap)
                        allowed += 1
                toks[t] += tok.tolist()
    print(f"B {B}: {draws} draws, {allowed} used the allowance, {close} with a host top-2 margin within 2 TIE")
    assert close <= ALLOWANCE_CAP * draws
    assert allowed <= ALLOWANCE_CAP * draws
    assert toks[2] != toks[5]           # the step is part of the counter


def test_full_vocabulary(hip):
    B, V = 1, V_FULL
    inp = _Inputs(hip, B, V, 77)
    inp.table = None                    # (bf16 planes only: 2.1 GB handed back)
    ids = _random_ids(V, 204, 14, must=(0, 1, V - 2, V - 1))
    assert ids.numel() == 204
    _check_logits_and_greedy(hip, inp, ids)


@pytest.mark.parametrize("f8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampling"])
def test_done_state_writes_nothing(hip, sample, f8):
    B, V = 3, V_ODD
    inp = _inputs(hip, B, V)
    hi, lo, kw = inp.planes(hip, f8)
    ids = _random_ids(V, 301, 11)
    samp = hip.decode_sampling(DEV)
    hip.decode_set_sampling(samp, 5, 1.0)
    samp0 = samp.clone()
    st = _state(hip, B, 3, [20] * B, done=1)
    st0 = st.clone()
    pval, pidx = hip.decode_lm_partials(B, DEV)
    pval.fill_(3.0); pidx.fill_(11)
    lg = torch.full((B, V), 5.0, device=DEV)
    out = torch.randint(0, 9, (B, 16), dtype=torch.int32, device=DEV)
    out0 = out.clone()
    if sample:
        hip.decode_lm_head_sample(st, samp, inp.x, inp.gamma, hi, lo, pval, pidx, logits=lg, ids=ids, **kw)
    else:
        hip.decode_lm_head(st, inp.x, inp.gamma, hi, lo, pval, pidx, logits=lg, ids=ids, **kw)
    hip.decode_finish(st, pval, pidx, out, eos_token=1)
    torch.cuda.synchronize()
    assert torch.equal(st, st0) and torch.equal(samp, samp0) and torch.equal(out, out0)
    assert bool((pval == 3.0).all()) and bool((pidx == 11).all()) and bool((lg == 5.0).all())


def test_bad_arguments_are_rejected(hip):
    B, V = 1, V_ODD
    inp = _inputs(hip, B, V)
    st = _state(hip, B, 1, [4])
    pval, pidx = hip.decode_lm_partials(B, DEV)
    samp = hip.decode_sampling(DEV)
    good = _ids([1, 2, 3])
    codes, _, kw8 = inp.planes(hip, True)
    heads = (lambda **k: hip.decode_lm_head(st, inp.x, inp.gamma, inp.hi, inp.lo, pval, pidx, **k),
             lambda **k: hip.decode_lm_head_sample(st, samp, inp.x, inp.gamma, inp.hi, inp.lo, pval, pidx, **k),
             lambda **k: hip.decode_lm_head(st, inp.x, inp.gamma, codes, None, pval, pidx, **kw8, **k),
             lambda **k: hip.decode_lm_head_sample(st, samp, inp.x, inp.gamma, codes, None, pval, pidx, **kw8, **k))
    for head in heads:
        with pytest.raises(ValueError):
            head(ids=torch.empty(0, dtype=torch.int32, device=DEV))                 # n = 0
        with pytest.raises(ValueError):
            head(ids=torch.zeros(V + 1, dtype=torch.int32, device=DEV))             # n > V
        with pytest.raises(TypeError):
            head(ids=good.long())                                                   # not int32
        with pytest.raises(TypeError):
            head(ids=good.cpu())                                                    # not on the device
    with pytest.raises(TypeError):
        hip.decode_lm_head(st, inp.x, inp.gamma, codes, None, pval, pidx, ids=good)              # fp8 codes without scales
    with pytest.raises(TypeError):
        hip.decode_lm_head_sample(st, samp, inp.x, inp.gamma, codes, None, pval, pidx, ids=good)
    # the C ABI itself: a null ids, n < 1 and n > V are LAP_ERR_ARG
    p = lambda t: None if t is None else t.data_ptr()
    for ids_p, n in ((None, 3), (p(good), 0), (p(good), -1), (p(good), V + 1)):
        with pytest.raises(hip.LapHipError):
            hip.call("lap_decode_lm_head_subset", p(st), p(inp.x), p(inp.gamma), p(inp.hi), p(inp.lo), ids_p, n, B, D, V, 1e-6, None,
                     p(pval), p(pidx))
        with pytest.raises(hip.LapHipError):
            hip.call("lap_decode_lm_head_subset_sample_fp8", p(st), p(samp), p(inp.x), p(inp.gamma), p(codes), p(kw8["wscale"]), ids_p,
                     n, B, D, V, 1e-6, None, p(pval), p(pidx))
    torch.cuda.synchronize()


@pytest.mark.parametrize("f8", [False, True], ids=["bf16", "fp8"])
def test_an_id_outside_the_vocabulary_is_never_an_address(hip, f8):
    """The entry points document that an id outside [0, V) is left out, not dereferenced (`check_allowed_tokens` refuses such a
    set long before; this is the kernel's own guard).  Units here: (bad, 3) -> row 3 alone, (10, bad) -> row 10 alone,
    (21, 22), (bad, bad) -> skipped, (bad) -> skipped."""
    B, V = 3, V_ODD
    inp = _inputs(hip, B, V)
    full_lg, _ = inp.full(hip, f8)
    ids = torch.tensor([-5, 3, 10, V, 21, 22, V + 7, 0x7fffffff, -(1 << 31)], dtype=torch.int32, device=DEV)
    want = _masked(full_lg, _ids([3, 10, 21, 22]))
    r = _run(hip, inp, ids=ids, f8=f8)
    assert torch.equal(r["lg"], want) and torch.equal(r["tok"], _first_argmax(want))
    samp = hip.decode_sampling(DEV)
    hip.decode_set_sampling(samp, 77, 1.0)
    r = _run(hip, inp, ids=ids, samp=samp, f8=f8)
    assert torch.equal(r["lg"], want)
    with np.errstate(invalid="ignore"):
        sc = S.scores_from_logits(want.cpu().numpy(), 1.0, 77, T0)
    tok = r["tok"].cpu().tolist()
    for b in range(B):          # the draw rule of test_sampling_on_a_proper_subset
        assert tok[b] in (3, 10, 21, 22) and float(sc[b].max() - sc[b, tok[b]]) <= TIE, (b, tok[b])


# ---------------------------------------------------------------------------------------------------------------- model
STEPS = 5


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


def _obs(cfg, B=3):
    obs, _, _, _ = make_inputs(cfg, B=B, ragged=True)
    so = dict(obs)
    so.pop("tokenized_langact_mask")
    so["image_masks"] = {k: torch.ones_like(m) for k, m in so["image_masks"].items()}
    return so


def _to_obs(so):
    return to_observation(so | {"tokenized_langact_mask": None}, DEV)


@pytest.fixture(scope="module")
def ar(hip):
    """(cfg, model, S, o): the two-layer model at the Gemma-2B widths (seed 13), a fixed random set of 300 ids plus EOS, and the
    ragged B = 3 observation."""
    from lap_amd.model import LAP

    with pytest.MonkeyPatch.context() as mp:
        cfg = _gemma2b_x2_cfg(mp)
        model = LAP(cfg, params=O.init_params(oracle_cfg(cfg), seed=13), device=DEV)
        allowed = _random_ids(cfg.vocab_size, 301, 15, must=(model.EOS_TOKEN,)).cpu()
        yield cfg, model, allowed, _to_obs(_obs(cfg))
        model.EOS_TOKEN = 1


def _outside(allowed, V):
    m = torch.ones(V, dtype=torch.bool)
    m[allowed.long()] = False
    return m


def test_fused_route_decodes_inside_the_set(ar):
    cfg, model, allowed, o = ar
    col = {}
    out = model.sample_tokens(0, o, max_decoding_steps=STEPS, decode="fused", allowed_tokens=allowed, collect=col)
    assert out.shape == (3, STEPS) and out.dtype == torch.int32 and len(col) == STEPS
    assert bool(torch.isin(out.cpu(), allowed).all())
    outside = _outside(allowed, cfg.vocab_size)
    for t in range(STEPS):
        lg = col[f"logit/{t}"].cpu()
        assert lg.shape == (3, cfg.vocab_size)
        assert bool((lg[:, outside] == NEG_INF).all()) and bool(torch.isfinite(lg[:, ~outside]).all())
        assert torch.equal(out[:, t].cpu(), _first_argmax(lg).cpu()), t
    # the set decides: the unconstrained decode leaves it; without `collect` the same tokens; order and duplicates do not matter
    free = model.sample_tokens(0, o, max_decoding_steps=STEPS, decode="fused")
    assert not bool(torch.isin(free.cpu(), allowed).all())
    assert torch.equal(model.sample_tokens(0, o, max_decoding_steps=STEPS, decode="fused", allowed_tokens=allowed), out)
    shuffled = torch.cat([allowed.flip(0), allowed[:7]]).tolist()
    assert torch.equal(model.sample_tokens(0, o, max_decoding_steps=STEPS, decode="fused", allowed_tokens=shuffled), out)
    with pytest.raises(ValueError):
        model.sample_tokens(0, o, max_decoding_steps=STEPS, decode="fused", allowed_tokens=[5, cfg.vocab_size])
    with pytest.raises(ValueError):
        model.sample_tokens(0, o, max_decoding_steps=STEPS, allowed_tokens=[t for t in allowed.tolist() if t != model.EOS_TOKEN])


def _agrees_with_eager(out, ref, col):
    """tokens equal step by step while the (masked) eager top-2 margins exceed MARGIN; from the first step where one does not,
    the contexts may diverge.  Returns (agrees, steps whose margins all exceeded MARGIN before that)."""
    clear = 0
    for s in range(ref.shape[1]):
        if not torch.equal(out[:, :s], ref[:, :s]):
            return False, clear
        lg = col.get(f"logit/{s}")
        if lg is None:
            break
        top2 = lg.topk(2, dim=1).values
        if bool(((top2[:, 0] - top2[:, 1]) <= MARGIN).any()):
            return True, clear
        clear += 1
    return torch.equal(out, ref), clear


def test_eager_and_fused_agree(ar):
    cfg, model, allowed, o = ar
    cole = {}
    eager = model.sample_tokens(0, o, max_decoding_steps=STEPS, allowed_tokens=allowed, collect=cole)
    fused = model.sample_tokens(0, o, max_decoding_steps=STEPS, decode="fused", allowed_tokens=allowed)
    assert bool(torch.isin(eager.cpu(), allowed).all())
    outside = _outside(allowed, cfg.vocab_size)
    for t in range(STEPS):
        assert bool((cole[f"logit/{t}"].cpu()[:, outside] == NEG_INF).all())
    ok, clear = _agrees_with_eager(fused, eager, cole)
    print(f"eager {eager.tolist()} fused {fused.tolist()}, {clear} steps with every margin above {MARGIN}")
    assert ok
    # the eager route under both samplers stays inside the set, and the device sampler's draws are the host restatement's on
    # the masked logits it collected
    cold = {}
    drawn = model.sample_tokens(4, o, max_decoding_steps=STEPS, temperature=0.7, sampler="device", allowed_tokens=allowed, collect=cold)
    hosted = model.sample_tokens(4, o, max_decoding_steps=STEPS, temperature=0.7, allowed_tokens=allowed)
    assert bool(torch.isin(drawn.cpu(), allowed).all()) and bool(torch.isin(hosted.cpu(), allowed).all())
    assert bool((cold["logit/0"].cpu()[:, outside] == NEG_INF).all())


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_graphs_replay_the_constrained_decode(ar, weights):
    from lap_amd.serve import GraphedTokenDecoder

    cfg, model, allowed, o = ar
    kw = dict(max_decoding_steps=STEPS, decode="fused", decode_weights=weights)
    fused = model.sample_tokens(0, o, allowed_tokens=allowed, **kw)
    drawn = model.sample_tokens(9, o, temperature=0.7, sampler="device", allowed_tokens=allowed, **kw)
    free = model.sample_tokens(0, o, **kw)
    assert bool(torch.isin(drawn.cpu(), allowed).all()) and not torch.equal(free, fused)
    dec = GraphedTokenDecoder(model, 3, STEPS, prompt_len=cfg.max_token_len, weights=weights, allowed_tokens=allowed)
    assert torch.equal(dec(o), fused)
    sdec = GraphedTokenDecoder(model, 3, STEPS, sampling=True, weights=weights, allowed_tokens=allowed.tolist())
    assert torch.equal(sdec(o), fused)
    assert torch.equal(sdec(o, temperature=0.7, seed=9), drawn)
    assert torch.equal(sdec(o), fused)
    # a decoder built without a set returns what it returned before
    assert torch.equal(GraphedTokenDecoder(model, 3, STEPS, weights=weights)(o), free)
    with pytest.raises(ValueError):
        GraphedTokenDecoder(model, 3, STEPS, allowed_tokens=[])


def test_ar_policy_hands_the_set_to_both_routes(ar, monkeypatch):
    from lap_amd.serve import ARPolicy, Policy

    cfg, model, allowed, _ = ar
    so1 = _obs(cfg, B=1)
    direct = model.sample_tokens(0, _to_obs(so1), max_decoding_steps=STEPS, decode="fused", allowed_tokens=allowed).cpu().numpy()
    req = {"image": {k: v[0].numpy() for k, v in so1["images"].items()},
           "image_mask": {k: v[0].numpy() for k, v in so1["image_masks"].items()},
           "state": so1["state"][0].numpy(), "tokenized_prompt": so1["tokenized_prompt"][0].numpy(),
           "tokenized_prompt_mask": so1["tokenized_prompt_mask"][0].numpy()}
    kw = {"max_decoding_steps": STEPS, "allowed_tokens": allowed.tolist()}
    pol = ARPolicy(Policy(model, use_graph=False), sample_kwargs=kw, use_graph=True)
    assert pol._decoder is not None and torch.equal(pol._decoder.allowed.cpu(), allowed)
    real = model.sample_tokens

    def boom(*a, **k):
        raise AssertionError("sample_tokens called: the graphs were not replayed")

    monkeypatch.setattr(model, "sample_tokens", boom)
    got = pol.infer(req)["tokens"]
    monkeypatch.setattr(model, "sample_tokens", real)
    assert np.array_equal(got, direct) and bool(np.isin(got, allowed.numpy()).all())
    # the sample_tokens route of the same policy surface (fused kernels: the same bits)
    plain = ARPolicy(Policy(model, use_graph=False), sample_kwargs=kw | {"decode": "fused"})
    assert plain._decoder is None and np.array_equal(plain.infer(req)["tokens"], direct)


def test_eos_inside_the_set_stops_the_decode(ar):
    from lap_amd.serve import GraphedTokenDecoder

    cfg, model, allowed, _ = ar
    o1 = _to_obs(_obs(cfg, B=1))
    try:
        free = model.sample_tokens(0, o1, max_decoding_steps=STEPS, decode="fused", allowed_tokens=allowed)
        first = int(free[0, 0])
        assert first in allowed.tolist() and int(free[0, 1:].abs().sum()) != 0
        model.EOS_TOKEN = first         # the constrained first token
        for decode in ("eager", "fused"):
            got = model.sample_tokens(0, o1, max_decoding_steps=STEPS, decode=decode, allowed_tokens=allowed)
            assert int(got[0, 0]) == first and int(got[0, 1:].abs().sum()) == 0, decode
        dec = GraphedTokenDecoder(model, 1, STEPS, allowed_tokens=allowed)
        got = dec(o1)
        assert int(got[0, 0]) == first and int(got[0, 1:].abs().sum()) == 0
        assert int(dec.ctx.state[0]) == 1 and int(dec.ctx.state[1]) == 1 and int(dec.ctx.state[8]) == 1
    finally:
        model.EOS_TOKEN = 1
