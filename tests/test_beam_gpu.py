"""csrc/decode_beam.hip against lap_amd/beam.py (float64), kernel by kernel and inside the fused decode of the 2-layer
Gemma-2B-width model.

Tolerance of a log-probability (`tol_lp`), from the kernel's order of operations, eps = 2^-24:
* a thread (of 1024) pushes n = ceil(V / 1024) entries into its pair (m, s); a push is one expf (taken as 2 ulp; the device library documents
  1), one product and one sum, so s gains a relative error of at most 4 eps per push;
* the pairs merge over 6 shuffle levels and 15 waves, 21 merges of two expf, two products and one sum: at most 8 eps each;
* the argument z - m of an expf is itself rounded: a relative error of up to eps |z - m| <= 2 A eps on that term, hence at most
  2 A eps on S (the summand 2 A below);
* all terms are positive, so the relative error of S is at most (4 n + 168) eps (1.01 covers the second order), and that is the
  absolute error of log S;
* logf (2 ulp of |log S| <= ln V), the sum m + log S (eps |lse|) and the difference logit - lse (eps |logp|), with |lse| and
  |logp| at most A + ln V each, A the largest finite |logit| of the row.
  tol_lp = eps (1.01 (4 n + 168) + 2 ln V + 2 (A + ln V) + 2 A).
A score is the f32 sum of a beam's log-probabilities, one rounded sum per step: after k steps it is within
k (tol_lp + eps max|score|) of the float64 one (`tol_score`).
Selections are compared exactly, so every case asserts the gap condition on its float64 side first: the N-th and (N+1)-th
log-probability of every contributing row, and the N-th and (N+1)-th candidate score, lie more than 4 tolerances apart
(`beam.step_gaps`); the inputs are built so that it holds (the leading logits are set 0.5 apart above clipped noise)."""
import math

import numpy as np
import pytest
import torch

from lap_amd import beam as bm

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24
EOS = 1


def tol_lp(V, A):
    n = -(-V // 1024)
    return EPS * (1.01 * (4 * n + 168) + 2 * math.log(max(V, 2)) + 2 * (A + math.log(max(V, 2))) + 2 * A)


def tol_score(V, A, steps, smax):
    return steps * (tol_lp(V, A) + EPS * smax)


def _amax(lg):
    f = np.asarray(lg, dtype=np.float64)
    f = f[np.isfinite(f)]
    return float(np.abs(f).max()) if f.size else 0.0


def _logits(N, V, seed):
    """f32 [N, V]: noise clipped to [-4, 4] with min(V, 10) leading entries per row 0.5 apart from 10 down, at random ids."""
    rng = np.random.default_rng(seed)
    x = np.clip(rng.normal(size=(N, V)) * 1.5, -4.0, 4.0).astype(np.float32)
    for b in range(N):
        ids = rng.permutation(V)[:10]
        x[b, ids] = 10.0 - 0.5 * np.arange(ids.size) - 0.03 * b
    return x


def _beam_words(hip, N, scores, finished, early_stop=True):
    w = hip.decode_beam_init_words(N, early_stop, "cpu")
    w[0:N] = torch.from_numpy(np.asarray(scores, dtype=np.float32).view(np.int32).copy())
    w[8:8 + N] = torch.as_tensor(np.asarray(finished, dtype=np.int32))
    return w.to(DEV)


def _state(hip, t, done=0):
    st = hip.decode_state(1, DEV)
    st[0], st[1] = t, done
    return st


def _assert_gaps(logits, scores, finished, tol):
    row_gap, sel_gap = bm.step_gaps(logits, scores, finished)
    assert row_gap > 4 * tol and sel_gap > 4 * tol, (row_gap, sel_gap, tol)


# ------------------------------------------------------------------------------------------------------------------ topn
KINDS = ("plain", "six", "empty", "finished", "dead")


@pytest.mark.parametrize("N", [1, 2, 3, 8])
@pytest.mark.parametrize("V", [1, 7, 1003, 257152])
def test_topn_matches_the_specification(hip, V, N):
    base = _logits(N, V, seed=V + N)
    dev_logits = torch.empty((N, V), dtype=torch.float32, device=DEV)
    worst = 0.0
    for shift in range(len(KINDS)):         # every row takes every kind once
        x = base.copy()
        scores, fin = np.zeros(N), np.zeros(N, bool)
        kinds = [KINDS[(b + shift) % len(KINDS)] for b in range(N)]
        for b, kind in enumerate(kinds):
            scores[b] = -0.25 * b
            if kind == "six":
                keep = np.argsort(-x[b], kind="stable")[:6]
                row = np.full(V, -np.inf, np.float32)
                row[keep] = x[b, keep]
                x[b] = row
            elif kind == "empty":
                x[b] = -np.inf
                if V > 1:
                    x[b, V // 2] = np.nan
            elif kind == "finished":
                fin[b] = True
            elif kind == "dead":
                scores[b] = -np.inf
        tol = tol_lp(V, _amax(x))
        assert bm.step_gaps(x, scores, fin)[0] > 4 * tol
        dev_logits.copy_(torch.from_numpy(x))
        cl = torch.full((N, N), 7.0, dtype=torch.float32, device=DEV)
        ci = torch.full((N, N), 7, dtype=torch.int32, device=DEV)
        hip.decode_beam_topn(_state(hip, 3), _beam_words(hip, N, scores, fin), dev_logits, cl, ci, cap=9)
        cl, ci = cl.cpu().numpy(), ci.cpu().numpy()
        for b, kind in enumerate(kinds):
            if kind == "dead":
                want_i, want_l = [], []
            elif kind == "finished":
                want_i, want_l = [0], [0.0]
            else:
                ids, lp, _ = bm.row_topn(x[b], N)
                want_i, want_l = ids.tolist(), lp.tolist()
            k = len(want_i)
            assert ci[b, :k].tolist() == want_i and (ci[b, k:] == -1).all(), (kind, b, ci[b], want_i)
            assert np.isneginf(cl[b, k:]).all()
            if k:
                err = np.abs(cl[b, :k].astype(np.float64) - np.asarray(want_l))
                worst = max(worst, float(err.max()))
                assert (err <= tol).all(), (kind, b, err, tol)
    print(f"V {V} N {N}: |logp - float64| up to {worst:.3e}, tolerance {tol_lp(V, _amax(base)):.3e}")


def test_topn_writes_nothing_when_done_or_past_the_budget(hip):
    x = torch.from_numpy(_logits(2, 7, 0)).to(DEV)
    for st in (_state(hip, 3, done=1), _state(hip, 9), _state(hip, -1)):
        cl = torch.full((2, 2), 7.0, dtype=torch.float32, device=DEV)
        ci = torch.full((2, 2), 7, dtype=torch.int32, device=DEV)
        hip.decode_beam_topn(st, _beam_words(hip, 2, [0, 0], [0, 0]), x, cl, ci, cap=9)
        assert bool((cl == 7.0).all()) and bool((ci == 7).all())


# ---------------------------------------------------------------------------------------------------------------- select
def _step(hip, x, scores, fin, t, cap, early_stop=True, eos=EOS, done=0):
    """topn + select on the device from sentinel-filled histories; everything the step may touch, before and after."""
    N, V = x.shape
    rng = np.random.default_rng(t + 17 * N)
    out0 = rng.integers(2, 1000, size=(N, cap)).astype(np.int32)
    lp0 = -rng.random((N, cap)).astype(np.float32)
    if cap > 1:
        lp0[:, cap - 1] = np.nan            # a sentinel that no copy may move
    st = _state(hip, t, done)
    bw = _beam_words(hip, N, scores, fin, early_stop)
    out, logp = torch.from_numpy(out0).to(DEV), torch.from_numpy(lp0).to(DEV)
    cl = torch.zeros((N, N), dtype=torch.float32, device=DEV)
    ci = torch.full((N, N), -1, dtype=torch.int32, device=DEV)
    before = (st.clone(), bw.clone())
    lg = torch.from_numpy(x).to(DEV)
    hip.decode_beam_topn(st, bw, lg, cl, ci, cap)
    hip.decode_beam_select(st, bw, cl, ci, out, logp, V, eos)
    torch.cuda.synchronize()
    return dict(st=st.cpu().numpy(), bw=bw.cpu().numpy(), out=out.cpu().numpy(), logp=logp.cpu().numpy(), out0=out0, lp0=lp0,
                st0=before[0].cpu().numpy(), bw0=before[1].cpu().numpy())


def _check_step(r, x, scores, fin, t, cap, early_stop=True, eos=EOS, prior_steps=1):
    N, V = x.shape
    scores32 = np.asarray(scores, dtype=np.float32).astype(np.float64)
    tol = tol_lp(V, _amax(x))
    _assert_gaps(x, scores32, fin, max(tol, tol_score(V, _amax(x), 1, _amax(scores32))))
    par, tok, lp, sc, nf, done = bm.beam_step(x, scores32, fin, t, cap, eos, early_stop)
    bw, st = r["bw"], r["st"]
    assert bw[16:16 + N].tolist() == par.tolist() and r["out"][:, t].tolist() == tok.tolist()
    assert bw[8:8 + N].tolist() == nf.astype(int).tolist() == st[8:8 + N].tolist()
    assert st[0] == t + 1 and st[1] == int(done)
    got_sc = bw[:N].copy().view(np.float32).astype(np.float64)
    live = np.isfinite(sc)
    assert np.isneginf(got_sc[~live]).all()
    assert (np.abs(got_sc[live] - sc[live]) <= tol + EPS * _amax(sc[live])).all(), (got_sc, sc)
    assert (np.abs(r["logp"][:, t].astype(np.float64) - lp) <= tol).all()
    # the histories below t follow the parents; everything beyond column t is untouched, NaN sentinels included
    assert np.array_equal(r["out"][:, :t], r["out0"][par][:, :t]) and np.array_equal(r["out"][:, t + 1:], r["out0"][:, t + 1:])
    assert np.array_equal(r["logp"][:, :t].view(np.int32), r["lp0"][par][:, :t].view(np.int32))
    assert np.array_equal(r["logp"][:, t + 1:].view(np.int32), r["lp0"][:, t + 1:].view(np.int32))
    assert bw[25] == r["bw0"][25] + int(par.tolist() != list(range(N)))
    return par, tok, nf, done


@pytest.mark.parametrize("N", [1, 2, 3, 8])
@pytest.mark.parametrize("t, cap", [(0, 9), (5, 9), (8, 9), (299, 300)])
def test_select_from_the_initial_scores_and_mid_decode(hip, N, t, cap):
    x = _logits(N, 1003, seed=N)
    s0, f0 = bm.initial(N)
    par, tok, nf, done = _check_step(_step(hip, x, s0, f0, t, cap), x, s0, f0, t, cap)
    assert par.tolist() == [0] * N and done == (t + 1 >= cap)
    # mid decode: spread scores, one finished beam, one beam at -inf (where N allows)
    scores = -0.8 * np.arange(N) - 0.1
    fin = np.zeros(N, bool)
    if N >= 2:
        fin[1] = True
    if N >= 3:
        scores[2] = -np.inf
    _check_step(_step(hip, x, scores, fin, t, cap), x, scores, fin, t, cap)


@pytest.mark.parametrize("early_stop", [True, False])
def test_select_early_stop_finished_and_padding(hip, early_stop):
    # row 0's best token is EOS: rank 0 finishes; early_stop decides done
    x = _logits(3, 7, seed=2)
    x[:, EOS] = 14.0
    scores, fin = np.array([-0.1, -9.0, -9.5]), np.zeros(3, bool)      # ranks 1 and 2 continue row 0 with other tokens
    par, tok, nf, done = _check_step(_step(hip, x, scores, fin, 2, 9, early_stop), x, scores, fin, 2, 9, early_stop)
    assert tok[0] == EOS and nf[0] and done == early_stop
    # fewer than N candidates: 2-id rows from the initial scores at N = 3 leave one padding beam
    y = np.full((3, 7), -np.inf, np.float32)
    y[:, [0, 3]] = [1.0, 2.0]
    s0, f0 = bm.initial(3)
    par, tok, nf, done = _check_step(_step(hip, y, s0, f0, 0, 9, early_stop), y, s0, f0, 0, 9, early_stop)
    assert par.tolist() == [0, 0, 2] and tok.tolist() == [3, 0, 0] and nf.tolist() == [False, False, True]
    # nothing anywhere: all padding, done
    z = np.full((2, 7), -np.inf, np.float32)
    z[1] = np.nan
    par, tok, nf, done = _check_step(_step(hip, z, np.zeros(2), np.zeros(2, bool), 1, 9, early_stop), z, np.zeros(2), np.zeros(2, bool), 1, 9,
                                     early_stop)
    assert nf.all() and done
    # every beam finished: each carries itself, done
    f = np.ones(3, bool)
    par, tok, nf, done = _check_step(_step(hip, x, scores, f, 4, 9, early_stop), x, scores, f, 4, 9, early_stop)
    assert par.tolist() == [0, 1, 2] and not tok.any() and done


def test_select_ties_inside_the_kept_set(hip):
    """Three equal logits at the top of the better row: the lower ids first; the cut (against the other row, 1 below) is clear."""
    x = np.array([[1.0, 3.0, 3.0, 0.0, 3.0]], dtype=np.float32)
    r = _step(hip, np.stack([x[0]] * 3), np.array([0.0, -1.0, -2.0]), np.zeros(3, bool), 1, 9, eos=0)
    par, tok, _, _ = _check_step(r, np.stack([x[0]] * 3), np.array([0.0, -1.0, -2.0]), np.zeros(3, bool), 1, 9, eos=0)
    assert par.tolist() == [0, 0, 0] and tok.tolist() == [1, 2, 4]


@pytest.mark.parametrize("t, done", [(9, 0), (12, 0), (3, 1)])
def test_select_past_the_budget_or_done_writes_nothing_else(hip, t, done):
    x = _logits(3, 7, seed=1)
    r = _step(hip, x, np.zeros(3), np.zeros(3, bool), t, 9, done=done)
    want = r["st0"].copy()
    want[1] = 1
    assert np.array_equal(r["st"], want) and np.array_equal(r["bw"], r["bw0"]) and np.array_equal(r["out"], r["out0"])
    assert np.array_equal(r["logp"].view(np.int32), r["lp0"].view(np.int32))


# --------------------------------------------------------------------------------------------------------------- reorder
def _perms(N):
    p = {"identity": list(range(N)), "swap": [1, 0] + list(range(2, N)), "all_from_one": [N - 1] * N}
    if N >= 3:
        p["cycle3"] = [1, 2, 0] + list(range(3, N))
    return list(p.items())


@pytest.mark.parametrize("N, name, parent", [(N, n, p) for N in (2, 3, 8) for n, p in _perms(N)])
@pytest.mark.parametrize("t", [0, 1, 5, 13])
def test_reorder_is_index_select_below_t(hip, t, N, name, parent):
    depth, cap, HD = 2, 13, 256
    g = torch.Generator(device=DEV).manual_seed(t + N)
    gen0 = torch.randn((depth, 2, N, cap, HD), generator=g, device=DEV).to(torch.bfloat16)
    gen0[..., cap - 1, 0] = float("nan")
    bw = _beam_words(hip, N, np.zeros(N), np.zeros(N, bool))
    bw[16:16 + N] = torch.as_tensor(parent, dtype=torch.int32)
    gen = gen0.clone()
    hip.decode_beam_reorder(_state(hip, t), bw, gen)
    want = gen0.clone()
    want[:, :, :, :t] = gen0.index_select(2, torch.as_tensor(parent, device=DEV))[:, :, :, :t]
    assert torch.equal(gen.view(torch.int16), want.view(torch.int16))
    # done, or a parent outside [0, N): untouched
    for st, par in ((_state(hip, 5, done=1), parent), (_state(hip, 5), [N] + parent[1:]), (_state(hip, 5), [-1] + parent[1:])):
        bw[16:16 + N] = torch.as_tensor(par, dtype=torch.int32)
        gen = gen0.clone()
        hip.decode_beam_reorder(st, bw, gen)
        assert torch.equal(gen.view(torch.int16), gen0.view(torch.int16))


# ----------------------------------------------------------------------------------------------------------------- model
@pytest.fixture(scope="module")
def ar(hip):
    """(cfg, model): LAP-3B widths with 2 layers per tower and a 16k vocabulary (the configuration of tests/test_ar_decode_gpu.py),
    as initialised; EOS -1, so no row stops before its budget."""
    from lap_amd import config as C
    from lap_amd.config import LAPConfig
    from lap_amd.model import LAP
    from oracle import lap_oracle as O
    from tests.common import oracle_cfg

    with pytest.MonkeyPatch.context() as mp:
        mp.setitem(C._GEMMA, "gemma_2b_x2", C.GemmaConfig(2048, 2, 16384, 8, 1, 256))
        mp.setitem(C._GEMMA, "gemma_300m_x2", C.GemmaConfig(1024, 2, 4096, 8, 1, 256))
        mp.setitem(C._SIGLIP, "So400m/14_x2", C.SiglipConfig(1152, 2, 4304, 16))
        mp.setitem(O.GEMMA, "gemma_2b_x2", O.GemmaCfg(2048, 2, 16384, 8, 1, 256))
        mp.setitem(O.GEMMA, "gemma_300m_x2", O.GemmaCfg(1024, 2, 4096, 8, 1, 256))
        mp.setitem(O.SIGLIP, "So400m/14_x2", O.SiglipCfg(1152, 2, 4304, 16))
        cfg = LAPConfig(paligemma_variant="gemma_2b_x2", action_expert_variant="gemma_300m_x2", siglip_variant="So400m/14_x2",
                        image_size=224, vocab_size=16384, action_dim=32, action_horizon=50, max_token_len=48,
                        language_loss_weight=0.4, enable_image_augmentation=False, enable_action_training=True)
        model = LAP(cfg, params=O.init_params(oracle_cfg(cfg), seed=13), device=DEV)
        model.EOS_TOKEN = -1
        yield cfg, model


def _obs1(cfg, seed=0):
    from tests.common import make_inputs, to_observation

    obs, _, _, _ = make_inputs(cfg, B=1, seed=seed, ragged=True)
    so = dict(obs)
    so.pop("tokenized_langact_mask")
    so["image_masks"] = {k: torch.ones_like(m) for k, m in so["image_masks"].items()}
    return to_observation(so | {"tokenized_langact_mask": None}, DEV)


# The observation of every (N, budget, variant) case: a seed of tests/common.py `make_inputs` at which every step of the decode
# meets the gap condition.  The condition is asserted, not searched: if a change moves the logits, the case fails and says so.
OBS_SEED = {(2, 13, "bf16"): 9, (4, 13, "bf16"): 9, (8, 13, "bf16"): 3, (2, 5, "bf16"): 9, (4, 5, "bf16"): 0, (8, 5, "bf16"): 0,
            (2, 13, "fp8"): 9, (4, 13, "fp8"): 5, (8, 13, "fp8"): 8, (2, 5, "fp8"): 9, (4, 5, "fp8"): 5, (8, 5, "fp8"): 3,
            (2, 13, "allowed"): 4, (4, 13, "allowed"): 2, (8, 13, "allowed"): 5, (2, 5, "allowed"): 4, (4, 5, "allowed"): 2,
            (8, 5, "allowed"): 1}


def _allowed50(cfg):
    g = torch.Generator().manual_seed(5)
    return torch.unique(torch.randperm(cfg.vocab_size, generator=g)[:50])


@pytest.mark.parametrize("decode", ["fused", "eager"])
def test_one_beam_is_the_greedy_decode(ar, decode):
    cfg, model = ar
    o = _obs1(cfg)
    want = model.sample_tokens(0, o, max_decoding_steps=6, decode=decode)
    got, lp = model.sample_tokens(0, o, max_decoding_steps=6, decode=decode, num_beams=1, return_logprobs=True)
    assert torch.equal(got, want) and lp.shape == (1, 6) and bool((lp <= 0).all())


@pytest.mark.parametrize("variant", ["bf16", "fp8", "allowed"])
@pytest.mark.parametrize("budget", [13, 5])
@pytest.mark.parametrize("N", [2, 4, 8])
def test_fused_decode_follows_the_specification_step_by_step(ar, N, budget, variant):
    """The fused beam decode, one step at a time: every step's stored logits go through `beam.beam_step` in float64 (under the gap
    condition), and parents, tokens, scores, finished flags, histories and the reordered K / V cache must be what it says; the
    result equals `sample_tokens(num_beams=N)` and `beam_decode_fused`.  Every step starts from the device's own f32 scores, so
    a step's tolerance is tol_lp plus the one rounded sum."""
    cfg, model = ar
    _follow(model, cfg, _obs1(cfg, OBS_SEED[(N, budget, variant)]), N, budget, variant)


def _follow(model, cfg, o, N, budget, variant, probe=False):
    """probe (choosing OBS_SEED): no assertion is made; the smallest of (gap / (4 tol)) over the steps is returned."""
    from lap_amd import ar_decode

    V = cfg.vocab_size
    allowed = ar_decode.allowed_set(model, _allowed50(cfg)).ids if variant == "allowed" else None
    weights = "fp8" if variant == "fp8" else "bf16"
    with model._serving_weights():
        pre = ar_decode.replicate_prefill(ar_decode.prefill(model, o), N)
        ctx = ar_decode.DecodeCtx(model, N, pre.Pn, budget, weights=weights, allowed=allowed, beams=N)
        scores, fin = bm.initial(N)
        tokens, logp = np.zeros((N, budget), np.int32), np.zeros((N, budget))
        smax, room = 0.0, np.inf
        for t in range(budget):
            gen0 = ctx.gen.clone()
            ctx.first_token(pre) if t == 0 else ctx.step()
            lg = ctx.logits.cpu().numpy()
            s32 = ctx_scores if t else scores
            tol = tol_lp(V, _amax(lg)) + EPS * max(smax, _amax(s32))
            row_gap, sel_gap = bm.step_gaps(lg, s32, fin)
            room = min(room, min(row_gap, sel_gap) / (4 * tol))
            assert probe or (row_gap > 4 * tol and sel_gap > 4 * tol), (t, row_gap, sel_gap, tol)
            par, tok, lp, new_scores, fin, done = bm.beam_step(lg, s32, fin, t, budget, model.EOS_TOKEN)
            st, bw = ctx.state.cpu().numpy(), ctx.beam.cpu().numpy()
            if probe and not (bw[16:16 + N].tolist() == par.tolist()):
                return 0.0
            assert bw[16:16 + N].tolist() == par.tolist() and st[0] == t + 1 and st[1] == int(done)
            tokens, logp = tokens[par], logp[par]
            tokens[:, t], logp[:, t] = tok, lp
            assert np.array_equal(ctx.out.cpu().numpy()[:, :t + 1], tokens[:, :t + 1])
            assert (np.abs(ctx.logp.cpu().numpy()[:, :t + 1] - logp[:, :t + 1]) <= tol).all()
            ctx_scores = bw[:N].copy().view(np.float32).astype(np.float64)      # the next step adds to the device's own f32 sums
            assert (np.abs(ctx_scores - new_scores) <= tol + EPS * _amax(new_scores)).all()
            smax = max(smax, _amax(new_scores))
            if t:       # this step began by moving the K / V rows to the parents the step before chose; it then wrote row t - 1
                want = gen0.clone()
                want[:, :, :, :t] = gen0.index_select(2, torch.as_tensor(prev_par, device=DEV))[:, :, :, :t]
                assert torch.equal(ctx.gen[:, :, :, :t - 1].view(torch.int16), want[:, :, :, :t - 1].view(torch.int16))
                assert torch.equal(ctx.gen[:, :, :, t:].view(torch.int16), gen0[:, :, :, t:].view(torch.int16))
            prev_par = par.tolist()
        res = ctx.beam_result()
        tok_f, lp_f, sc_f = ar_decode.beam_decode_fused(model, o, N, max_decoding_steps=budget, weights=weights, allowed=allowed)
    assert torch.equal(res[0], tok_f) and torch.equal(res[1], lp_f) and torch.equal(res[2], sc_f)
    kw = {"allowed_tokens": _allowed50(cfg)} if variant == "allowed" else {}
    one, lp1 = model.sample_tokens(0, o, max_decoding_steps=budget, decode="fused", decode_weights=weights, num_beams=N,
                                   return_logprobs=True, **kw)
    assert torch.equal(one, tok_f[:1]) and torch.equal(lp1, lp_f[:1])
    assert bool((sc_f[:-1] >= sc_f[1:]).all())          # rank order
    return room


ROUTE_REL = 1e-2        # tests/test_logprob_gpu.py: the routes' logit rows differ by at most this share of the row's norm


def _teacher_forced_logits(model, o, prefix, outside):
    """float64 [V]: the eager logits after `prefix`, from a batch-1 forward of its own (prefill, then one generic step per token
    with its own positions): nothing of the beam code is in it."""
    from lap_amd import ar_decode

    pre = ar_decode.prefill(model, o)
    logits = ar_decode._lm_logits(model, pre.x_last)
    gen = [(None, None)] * model.v.depth
    for s, tok in enumerate(prefix):
        token = torch.tensor([tok], dtype=torch.int32, device=DEV)
        pos = (pre.plen + s).to(torch.int32).view(1, 1).contiguous()
        logits = ar_decode._vlm_decode_step(model, token, pos, s, pre.cache, gen, pre.qinfo_d, pre.kinfo_prefix, 1, pre.Pn)
    return logits[0].masked_fill(outside, float("-inf")).double().cpu().numpy()


# the cases whose pinned observation keeps every step of the eager side above MARGIN (asserted): there fused and eager must agree
# in tokens and rank order over the whole decode
WHOLE_DECODE_CLEAR = {(2, 13, "allowed"), (2, 5, "allowed"), (4, 5, "allowed")}
MARGIN = 5e-2           # tests/test_logprob_gpu.py: the score margin above which the routes are held to the same choice


def _teacher_forced_logp(model, pre, row, outside):
    """(logp float64 [len(row)], d float64 [len(row)]): the eager log-probability of every token of `row` given the tokens before
    it, from ONE batch-1 chain of its own over the batch-1 prefill `pre` (nothing of the beam code is in it), and the route
    tolerance d = ROUTE_REL |z|_2 of the logits row each came from."""
    from lap_amd import ar_decode

    logits = ar_decode._lm_logits(model, pre.x_last)
    gen = [(None, None)] * model.v.depth
    lps, ds = [], []
    for s, tok in enumerate(row):
        z = logits[0].double()
        if outside is not None:
            z = z.masked_fill(outside, float("-inf"))
        z = z.cpu().numpy()
        fin = z[np.isfinite(z)]
        ds.append(ROUTE_REL * float(np.sqrt((fin * fin).sum())))
        lps.append(float(z[tok] - (fin.max() + np.log(np.exp(fin - fin.max()).sum()))))
        if s + 1 < len(row):
            token = torch.tensor([int(tok)], dtype=torch.int32, device=DEV)
            pos = (pre.plen + s).to(torch.int32).view(1, 1).contiguous()
            logits = ar_decode._vlm_decode_step(model, token, pos, s, pre.cache, gen, pre.qinfo_d, pre.kinfo_prefix, 1, pre.Pn)
    return np.asarray(lps), np.asarray(ds)


@pytest.mark.parametrize("variant", ["bf16", "allowed"])
@pytest.mark.parametrize("budget", [13, 5])
@pytest.mark.parametrize("N", [2, 4, 8])
def test_both_routes_against_teacher_forced_eager_forwards(ar, N, budget, variant):
    """Every beam of the fused route and of the eager route, scored again token by token with a teacher-forced batch-1 eager
    forward of its own: this ties `out`, `logp`, the scores and the reordered K / V of a whole decode to a second
    implementation, whatever was selected, so it needs no gap condition.  The routes' logit rows differ by at most
    d = ROUTE_REL |z|_2 (tests/test_logprob_gpu.py), so a log-probability by at most 2 d and a score by the sum of those, plus
    the f32 sum's own tol_score.  (The eager route has no fp8 weights, so fp8 is not a case here.)
    Then the routes against each other, tokens and rank order, step by step over the clear prefix: the steps before the first
    one at which a gap of the eager side (`beam.step_gaps`) does not exceed MARGIN, the repository's cross-route gate.  The length
    of that prefix is printed and not bounded below: on this model only the leading logit of a row is clear."""
    from lap_amd import ar_decode

    cfg, model = ar
    o = _obs1(cfg, OBS_SEED[(N, budget, variant)])
    V = cfg.vocab_size
    allowed, outside = None, None
    if variant == "allowed":
        allowed = ar_decode.allowed_set(model, _allowed50(cfg)).ids
        outside = torch.ones((V,), dtype=torch.bool, device=DEV)
        outside[allowed.long()] = False
    eager_steps = []

    def record(t, logits, scores, finished, res):
        prev = eager_steps[-1][1] if eager_steps else np.zeros((N, budget), np.int32)
        hist = prev[res[0]].copy()
        hist[:, t] = res[1]
        eager_steps.append((min(bm.step_gaps(logits, scores, finished)), hist))

    with model._serving_weights():
        pre1 = ar_decode.prefill(model, o)
        tok_e, lp_e, sc_e = ar_decode.beam_decode_eager(model, o, N, max_decoding_steps=budget, allowed=allowed, on_step=record)
        pre = ar_decode.replicate_prefill(pre1, N)
        ctx = ar_decode.DecodeCtx(model, N, pre.Pn, budget, allowed=allowed, beams=N)
        fused_steps = []
        for t in range(budget):
            ctx.first_token(pre) if t == 0 else ctx.step()
            fused_steps.append(ctx.out.cpu().numpy().copy())
        tok_f, lp_f, sc_f = ctx.beam_result()
        worst = 0.0
        for name, tok, lp, sc in (("fused", tok_f, lp_f, sc_f), ("eager", tok_e, lp_e, sc_e)):
            tok, lp, sc = tok.cpu().numpy(), lp.cpu().numpy().astype(np.float64), sc.cpu().numpy().astype(np.float64)
            assert tok.shape == (N, budget) and np.isfinite(sc).all() and len({tuple(r) for r in tok.tolist()}) == N
            for b in range(N):
                want, d = _teacher_forced_logp(model, pre1, tok[b], outside)
                err = np.abs(lp[b] - want)
                worst = max(worst, float((err / (2 * d)).max()))
                assert (err <= 2 * d).all(), (name, b, err, d)
                assert abs(sc[b] - want.sum()) <= 2 * d.sum() + tol_score(V, 0.0, budget, abs(want.sum())) + EPS * 64 * budget, (name, b)
    assert len(eager_steps) == budget
    clear = 0
    for t in range(budget):
        if not eager_steps[t][0] > MARGIN:
            break
        assert np.array_equal(fused_steps[t][:, :t + 1], eager_steps[t][1][:, :t + 1]), t
        clear += 1
    if (N, budget, variant) in WHOLE_DECODE_CLEAR:      # at these seeds every step is clear: the whole decodes are equal
        assert clear == budget and np.array_equal(tok_f.cpu().numpy(), tok_e.cpu().numpy())
    print(f"N {N} budget {budget} {variant}: largest |logp - teacher-forced| / (2 d) {worst:.3f}; clear prefix {clear} of {budget} steps")


def test_exhaustive_beam_finds_the_most_probable_sequence(ar):
    """allowed = {a, b, EOS}, cap 3, N = 8: at most 3, then 7 candidates exist before the last step, so nothing is cut until then
    and the rank-0 beam must be the most probable of the 15 sequences.  The 15 are enumerated here and scored in float64 with
    teacher-forced eager logits from separate batch-1 forwards.  a is the model's greedy first token (the tied head echoes, so
    the distributions are peaked and the best sequence leads clearly), b another id.
    Route tolerance of a sequence score: the routes' logit rows differ by at most d = ROUTE_REL |z|_2 (over the three finite
    entries), a log-probability by at most 2 d, a score of three tokens by 6 d.  The best sequence must lead the second by more
    than four times that (asserted); then both routes' rank-0 beams must be it, and every beam of either route must carry the
    enumerated score of its own sequence within 6 d."""
    from lap_amd import ar_decode

    cfg, model = ar
    o = _obs1(cfg)
    a = int(model.sample_tokens(0, o, max_decoding_steps=1)[0, 0])
    b = 4321 if a != 4321 else 4322
    assert a not in (0, 1)
    model.EOS_TOKEN = 1
    try:
        allowed = ar_decode.allowed_set(model, torch.tensor([1, a, b])).ids
        outside = torch.ones((cfg.vocab_size,), dtype=torch.bool, device=DEV)
        outside[allowed.long()] = False
        total, dmax = {}, 0.0
        with model._serving_weights():
            alive = {(): 0.0}
            for _ in range(3):
                nxt = {}
                for prefix, sc in alive.items():
                    z = _teacher_forced_logits(model, o, prefix, outside)
                    fin = z[np.isfinite(z)]
                    dmax = max(dmax, ROUTE_REL * float(np.sqrt((fin * fin).sum())))
                    lse = fin.max() + np.log(np.exp(fin - fin.max()).sum())
                    for tok in (1, a, b):
                        (total if tok == 1 else nxt)[prefix + (tok,)] = sc + float(z[tok] - lse)
                alive = nxt
            total |= alive
            tok_e, lp_e, sc_e = ar_decode.beam_decode_eager(model, o, 8, max_decoding_steps=3, early_stop=False, allowed=allowed)
            tok_f, lp_f, sc_f = ar_decode.beam_decode_fused(model, o, 8, max_decoding_steps=3, early_stop=False, allowed=allowed)
        assert len(total) == 15          # 7 that end in EOS within three tokens, 8 of three tokens without it
        ranked = sorted(total.items(), key=lambda kv: -kv[1])
        tol = 6 * dmax
        print(f"best two sequences {ranked[0]}, {ranked[1]}; route tolerance of a score {tol:.3e}")
        assert ranked[0][1] - ranked[1][1] > 4 * tol, (ranked[:2], tol)
        best = list(ranked[0][0]) + [0] * (3 - len(ranked[0][0]))
        for name, tok, lp, sc in (("eager", tok_e, lp_e, sc_e), ("fused", tok_f, lp_f, sc_f)):
            tok, lp, sc = tok.cpu().numpy(), lp.cpu().numpy().astype(np.float64), sc.cpu().numpy().astype(np.float64)
            assert tok[0].tolist() == best, (name, tok[0], best)
            for r in range(8):                  # every beam is one of the 15, with its enumerated score
                seq = tuple(tok[r].tolist())
                seq = seq[:seq.index(1) + 1] if 1 in seq else seq
                assert seq in total and abs(sc[r] - total[seq]) <= tol and abs(lp[r].sum() - total[seq]) <= tol, (name, r, seq)
            assert len({tuple(r) for r in tok.tolist()}) == 8 and (sc[:-1] >= sc[1:]).all()
    finally:
        model.EOS_TOKEN = -1


def test_one_capture_serves_two_observations(ar):
    from lap_amd.serve import GraphedTokenDecoder
    from tests.common import make_inputs, to_observation

    cfg, model = ar
    dec = GraphedTokenDecoder(model, 1, 6, num_beams=4, logprobs=True).capture()
    graphs, ctx = (dec.g_prefill, dec.g_step), dec.ctx
    answers = []
    for seed in (1, 2):
        obs, _, _, _ = make_inputs(cfg, B=1, seed=seed, ragged=True)
        so = dict(obs)
        so.pop("tokenized_langact_mask")
        so["image_masks"] = {k: torch.ones_like(m) for k, m in so["image_masks"].items()}
        o = to_observation(so | {"tokenized_langact_mask": None}, DEV)
        tok, lp = dec(o)
        want_t, want_l = model.sample_tokens(0, o, max_decoding_steps=6, decode="fused", num_beams=4, return_logprobs=True)
        assert torch.equal(tok, want_t) and torch.equal(lp, want_l)
        beams = dec.last_beams
        assert beams[0].shape == (4, 6) and beams[2].shape == (4,) and torch.equal(beams[0][:1], tok)
        answers.append(beams[0].cpu().numpy())
    assert (dec.g_prefill, dec.g_step) == graphs and dec.ctx is ctx and ctx.B == 4
    assert not np.array_equal(answers[0], answers[1])
    with pytest.raises(ValueError, match="temperature must be 0"):
        GraphedTokenDecoder(model, 1, 6, sampling=True, num_beams=4)
    with pytest.raises(ValueError, match="batch 1"):
        GraphedTokenDecoder(model, 3, 6, num_beams=4)


@pytest.mark.parametrize("use_graph", [False, True])
def test_ar_policy_answers_with_the_selected_beam(ar, use_graph):
    from lap_amd import ar_decode, sampling
    from lap_amd.serve import ARPolicy, Policy
    from tests.common import make_inputs

    cfg, model = ar
    obs, _, _, _ = make_inputs(cfg, B=1, seed=2, ragged=True)
    req = {"image": {k: v[0].numpy() for k, v in obs["images"].items()}, "image_mask": {k: np.array(True) for k in obs["images"]},
           "state": obs["state"][0].numpy(), "tokenized_prompt": obs["tokenized_prompt"][0].numpy(),
           "tokenized_prompt_mask": obs["tokenized_prompt_mask"][0].numpy()}
    for select in ("sum", "mean"):
        pol = ARPolicy(Policy(model, use_graph=False), sample_kwargs={"num_beams": 4, "select": select, "max_decoding_steps": 6},
                       use_graph=use_graph)
        assert (pol._decoder is not None) == use_graph
        res = pol.infer(req)
        o = pol._base._to_observation(req)[0]
        with model._serving_weights():
            tok, lp, _ = (t.cpu().numpy() for t in ar_decode.beam_decode_fused(model, o, 4, max_decoding_steps=6,
                                                                               early_stop=select != "mean"))
        cand = res["candidates"]
        assert cand["tokens"].shape == (4, 6) and np.array_equal(cand["tokens"], tok)
        assert np.array_equal(cand["logprob"], sampling.sequence_logprob(tok, lp, model.EOS_TOKEN))
        best = sampling.select_best(tok, lp, model.EOS_TOKEN, select)
        assert res["tokens"].shape == (1, 6) and np.array_equal(res["tokens"][0], tok[best])
        assert np.array_equal(res["token_logprobs"][0], lp[best])
    with pytest.raises(ValueError, match="temperature must be 0"):
        ARPolicy(Policy(model, use_graph=False), sample_kwargs={"num_beams": 4, "temperature": 1.0})
