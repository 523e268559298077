"""Grammar-constrained beam search on the device: lap_decode_beam_grammar_topn and lap_decode_beam_grammar_select against
lap_amd/beam.py `grammar_beam_step` (float64) on the cases of tests/beam_grammar_cases.py, and inside the fused decode of the 2-layer
Gemma-2B-width model under the verbose-with-rotation automaton of the test suite's tiny tokenizer.

Tolerance of a log-probability: `beam_grammar_cases.tol_lp` (derived there from the kernel's order of operations: n = the entries
one of the 256 threads handles, 9 merges, the segment size in place of V).  A score is the f32 sum of a beam's log-probabilities,
one rounded sum per step.  Selections are compared exactly, so every case asserts the gap condition on its float64 side first
(`beam.step_gaps` on the masked rows, more than 4 tolerances); tests/test_beam_grammar_cpu.py checks without a GPU that the kernel
cases meet it, so none is skipped here."""
import numpy as np
import pytest
import torch

from lap_amd import beam as bm
from tests import beam_grammar_cases as C
from tests import grammar_cases as GC

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = C.EPS


@pytest.fixture(scope="module")
def auto():
    a = GC.automaton()
    return a, a.to_device(DEV)


def _beam_words(hip, N, scores, finished, early_stop=True):
    w = hip.decode_beam_init_words(N, early_stop, "cpu")
    w[0:N] = torch.from_numpy(np.asarray(scores, dtype=np.float32).view(np.int32).copy())
    w[8:8 + N] = torch.as_tensor(np.asarray(finished, dtype=np.int32))
    return w.to(DEV)


def _state(hip, t, done=0):
    st = hip.decode_state(1, DEV)
    st[0], st[1] = t, done
    return st


def _cands(N):
    return (torch.full((N, N), 7.0, dtype=torch.float32, device=DEV), torch.full((N, N), 7, dtype=torch.int32, device=DEV),
            torch.full((N, N), 7, dtype=torch.int32, device=DEV))


# ------------------------------------------------------------------------------------------------------------------ topn
@pytest.mark.parametrize("N", C.NS)
def test_topn_matches_the_specification(hip, auto, N):
    """Rows over all six states and the kinds finished, dead, state Q, state -1, all -inf segment and NaN inside a segment, every
    row taking every kind once.  cand_id and cand_next exactly (missing: -1), cand_logp within `tol_lp` of the row's segment."""
    a, d = auto
    worst, worst_tol = 0.0, 0.0
    for shift in range(len(C.KINDS)):
        x, scores, fin, states, kinds = C.topn_case(a, N, shift)
        masked = C.masked_by_hand(a, x, states)
        assert bm.step_gaps(masked, scores, fin)[0] > 4 * C.row_tol(a, x, states)
        cl, ci, cn = _cands(N)
        gq = torch.from_numpy(states).to(DEV)
        hip.decode_beam_grammar_topn(_state(hip, 3), _beam_words(hip, N, scores, fin), gq, d.offsets, d.ids, d.next,
                                     torch.from_numpy(x).to(DEV), cl, ci, cn, cap=9)
        assert torch.equal(gq.cpu(), torch.from_numpy(states))
        cl, ci, cn = cl.cpu().numpy(), ci.cpu().numpy(), cn.cpu().numpy()
        for b, kind in enumerate(kinds):
            q = int(states[b])
            if kind in ("dead", "bad_Q", "bad_neg", "all_inf"):
                want_i, want_l, want_n = [], [], []
            elif kind == "finished":
                want_i, want_l, want_n = [0], [0.0], [q]
            else:
                ids, lp, _ = bm.row_topn(masked[b], N)
                want_i, want_l, want_n = ids.tolist(), lp.tolist(), [a.step(q, int(i)) for i in ids]
                assert len(want_i) == min(N, len(a.allowed(q)) - (3 if kind == "nan" else 0))
            k = len(want_i)
            assert ci[b, :k].tolist() == want_i and (ci[b, k:] == -1).all(), (kind, b, ci[b], want_i)
            assert cn[b, :k].tolist() == want_n and (cn[b, k:] == -1).all(), (kind, b, cn[b], want_n)
            assert np.isneginf(cl[b, k:]).all()
            if k:
                tol = C.tol_lp(len(a.allowed(q)), C.amax(masked[b]))
                err = np.abs(cl[b, :k].astype(np.float64) - np.asarray(want_l))
                if float(err.max()) >= worst:
                    worst, worst_tol = float(err.max()), tol
                assert (err <= tol).all(), (kind, b, err, tol)
    print(f"N {N}: |logp - float64| up to {worst:.3e} (tolerance of that row {worst_tol:.3e})")


def test_topn_reads_nothing_outside_the_segment(hip, auto):
    """NaN everywhere outside the state's set: the candidates are those of the clean row, bit for bit."""
    a, d = auto
    x, scores, fin, states, _ = C.topn_case(a, 3, 2)        # states 2, 3, 4
    res = []
    for poison in (False, True):
        y = x.copy()
        if poison:
            for b in range(3):
                out = np.ones(C.V, bool)
                out[a.allowed(int(states[b]))] = False
                y[b, out] = np.nan
        cl, ci, cn = _cands(3)
        hip.decode_beam_grammar_topn(_state(hip, 0), _beam_words(hip, 3, scores, fin), torch.from_numpy(states).to(DEV), d.offsets, d.ids,
                                     d.next, torch.from_numpy(y).to(DEV), cl, ci, cn, cap=9)
        res.append((cl.cpu(), ci.cpu(), cn.cpu()))
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32)) and torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][2], res[1][2]) and bool((res[0][1] >= 0).all())


def test_topn_never_uses_a_bad_segment_or_id_as_an_address(hip, auto):
    """offsets that leave [0, E] and an id outside [0, V) (automata `to_device` would reject): such a row writes no candidates."""
    a, d = auto
    x, _ = C.noise(3, 9)
    off = a.offsets.copy()
    off[2] = a.num_edges + 1000000                      # the segment of state 1 ends past E; state 2 then starts past E
    ids = a.ids.copy()
    ids[a.offsets[3] + 4] = C.V + 12345                 # one id of state 3 outside the vocabulary
    put = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(DEV)
    cl, ci, cn = _cands(3)
    hip.decode_beam_grammar_topn(_state(hip, 0), _beam_words(hip, 3, np.zeros(3), np.zeros(3, bool)), put([1, 2, 3]), put(off), put(ids),
                                 d.next, torch.from_numpy(x).to(DEV), cl, ci, cn, cap=9)
    assert bool((ci == -1).all()) and bool((cn == -1).all()) and bool(torch.isinf(cl).all())


def test_topn_writes_nothing_when_done_or_past_the_budget(hip, auto):
    a, d = auto
    x, scores, fin, states, _ = C.topn_case(a, 3, 0)
    for st in (_state(hip, 3, done=1), _state(hip, 9), _state(hip, -1)):
        cl, ci, cn = _cands(3)
        hip.decode_beam_grammar_topn(st, _beam_words(hip, 3, scores, fin), torch.from_numpy(states).to(DEV), d.offsets, d.ids, d.next,
                                     torch.from_numpy(x).to(DEV), cl, ci, cn, cap=9)
        assert bool((cl == 7.0).all()) and bool((ci == 7).all()) and bool((cn == 7).all())


# ---------------------------------------------------------------------------------------------------------------- select
def _step(hip, d, x, scores, fin, states, t, cap, early_stop=True, eos=C.EOS, done=0):
    """topn + select on the device from sentinel-filled histories; everything the step may touch, before and after."""
    N = x.shape[0]
    rng = np.random.default_rng(t + 17 * N)
    out0 = rng.integers(2, 1000, size=(N, cap)).astype(np.int32)
    lp0 = -rng.random((N, cap)).astype(np.float32)
    lp0[:, cap - 1] = np.nan                # a sentinel that no copy may move
    st, bw = _state(hip, t, done), _beam_words(hip, N, scores, fin, early_stop)
    gq = torch.from_numpy(np.asarray(states, dtype=np.int32)).to(DEV)
    out, logp = torch.from_numpy(out0).to(DEV), torch.from_numpy(lp0).to(DEV)
    cl, ci, cn = _cands(N)
    before = (st.clone(), bw.clone())
    hip.decode_beam_grammar_topn(st, bw, gq, d.offsets, d.ids, d.next, torch.from_numpy(x).to(DEV), cl, ci, cn, cap)
    hip.decode_beam_grammar_select(st, bw, gq, cl, ci, cn, out, logp, x.shape[1], eos)
    torch.cuda.synchronize()
    return dict(st=st.cpu().numpy(), bw=bw.cpu().numpy(), out=out.cpu().numpy(), logp=logp.cpu().numpy(), out0=out0, lp0=lp0,
                st0=before[0].cpu().numpy(), bw0=before[1].cpu().numpy(), gq=gq.cpu().numpy())


@pytest.mark.parametrize("name", ["shared", "padding", "short", "all_finished"])
@pytest.mark.parametrize("early_stop", [True, False])
def test_select_moves_the_states_along_the_parents(hip, auto, name, early_stop):
    """Parents, tokens, finished flags, scores, histories and state words as lap_decode_beam_select's tests hold them, and gstate =
    new_states: a non-identity permutation in which two beams share a parent and one parent is finished ("shared"), padding beams
    ("padding"), rows with fewer than N edges ("short"), every beam finished."""
    a, d = auto
    x, scores, fin, states, t, cap = C.select_cases(a)[name]
    N = x.shape[0]
    s32 = np.asarray(scores, dtype=np.float32).astype(np.float64)
    masked = C.masked_by_hand(a, x, states)
    tol = C.row_tol(a, x, states)
    row_gap, sel_gap = bm.step_gaps(masked, s32, fin)
    assert row_gap > 4 * (tol + EPS * C.amax(s32)) and sel_gap > 4 * (tol + EPS * C.amax(s32))
    par, tok, lp, sc, nf, done, ns = bm.grammar_beam_step(x, s32, fin, states, a, t, cap, C.EOS, early_stop)
    r = _step(hip, d, x, scores, fin, states, t, cap, early_stop)
    bw, st = r["bw"], r["st"]
    assert bw[16:16 + N].tolist() == par.tolist() and r["out"][:, t].tolist() == tok.tolist()
    assert r["gq"].tolist() == ns.tolist()
    assert bw[8:8 + N].tolist() == nf.astype(int).tolist() == st[8:8 + N].tolist()
    assert st[0] == t + 1 and st[1] == int(done)
    got_sc = bw[:N].copy().view(np.float32).astype(np.float64)
    live = np.isfinite(sc)
    assert np.isneginf(got_sc[~live]).all()
    assert (np.abs(got_sc[live] - sc[live]) <= tol + EPS * C.amax(sc[live])).all(), (got_sc, sc)
    assert (np.abs(r["logp"][:, t].astype(np.float64) - lp) <= tol).all()
    assert np.array_equal(r["out"][:, :t], r["out0"][par][:, :t]) and np.array_equal(r["out"][:, t + 1:], r["out0"][:, t + 1:])
    assert np.array_equal(r["logp"][:, :t].view(np.int32), r["lp0"][par][:, :t].view(np.int32))
    assert np.array_equal(r["logp"][:, t + 1:].view(np.int32), r["lp0"][:, t + 1:].view(np.int32))
    assert bw[25] == r["bw0"][25] + int(par.tolist() != list(range(N)))
    if name == "shared":
        assert par.tolist() == [1, 0, 0, 2]


@pytest.mark.parametrize("t, done", [(9, 0), (12, 0), (3, 1)])
def test_select_past_the_budget_or_done_leaves_gstate(hip, auto, t, done):
    a, d = auto
    x, scores, fin, states, _, cap = C.select_cases(a)["shared"]
    r = _step(hip, d, x, scores, fin, states, t, cap, done=done)
    want = r["st0"].copy()
    want[1] = 1
    assert np.array_equal(r["st"], want) and np.array_equal(r["bw"], r["bw0"]) and np.array_equal(r["out"], r["out0"])
    assert np.array_equal(r["logp"].view(np.int32), r["lp0"].view(np.int32)) and r["gq"].tolist() == states.tolist()


def test_the_plain_select_is_unchanged_beside_the_grammar_one(hip, auto):
    """The same candidates through lap_decode_beam_select and lap_decode_beam_grammar_select: every word both write is equal."""
    a, d = auto
    x, scores, fin, states, t, cap = C.select_cases(a)["short"]
    N = 8
    cl, ci, cn = _cands(N)
    st, bw = _state(hip, t), _beam_words(hip, N, scores, fin)
    hip.decode_beam_grammar_topn(st, bw, torch.from_numpy(states).to(DEV), d.offsets, d.ids, d.next, torch.from_numpy(x).to(DEV), cl, ci, cn, cap)
    res = []
    for grammar in (False, True):
        s, b = st.clone(), bw.clone()
        out = torch.arange(N * cap, dtype=torch.int32, device=DEV).view(N, cap).contiguous()
        lp = -torch.arange(N * cap, dtype=torch.float32, device=DEV).view(N, cap).contiguous()
        if grammar:
            hip.decode_beam_grammar_select(s, b, torch.from_numpy(states).to(DEV), cl, ci, cn, out, lp, C.V, C.EOS)
        else:
            hip.decode_beam_select(s, b, cl, ci, out, lp, C.V, C.EOS)
        res.append((s.cpu(), b.cpu(), out.cpu(), lp.cpu()))
    for x0, x1 in zip(*res):
        assert torch.equal(x0, x1)


# ----------------------------------------------------------------------------------------------------------------- model
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
    """(cfg, model, automaton, device automaton): LAP-3B widths with 2 layers per tower and a 16k vocabulary (the configuration of
    tests/test_beam_gpu.py), as initialised, and the verbose-with-rotation automaton under the tiny tokenizer (EOS 1)."""
    from lap_amd import config as Cf
    from lap_amd import policy_io as pio
    from lap_amd.config import LAPConfig
    from lap_amd.model import LAP
    from oracle import lap_oracle as O
    from tests.common import oracle_cfg, tiny_sentencepiece_proto

    with pytest.MonkeyPatch.context() as mp:
        mp.setitem(Cf._GEMMA, "gemma_2b_x2", Cf.GemmaConfig(2048, 2, 16384, 8, 1, 256))
        mp.setitem(Cf._GEMMA, "gemma_300m_x2", Cf.GemmaConfig(1024, 2, 4096, 8, 1, 256))
        mp.setitem(Cf._SIGLIP, "So400m/14_x2", Cf.SiglipConfig(1152, 2, 4304, 16))
        mp.setitem(O.GEMMA, "gemma_2b_x2", O.GemmaCfg(2048, 2, 16384, 8, 1, 256))
        mp.setitem(O.GEMMA, "gemma_300m_x2", O.GemmaCfg(1024, 2, 4096, 8, 1, 256))
        mp.setitem(O.SIGLIP, "So400m/14_x2", O.SiglipCfg(1152, 2, 4304, 16))
        cfg = LAPConfig(paligemma_variant="gemma_2b_x2", action_expert_variant="gemma_300m_x2", siglip_variant="So400m/14_x2",
                        image_size=224, vocab_size=16384, action_dim=32, action_horizon=50, max_token_len=48,
                        language_loss_weight=0.4, enable_image_augmentation=False, enable_action_training=True)
        model = LAP(cfg, params=O.init_params(oracle_cfg(cfg), seed=13), device=DEV)
        tk = pio.PaligemmaTokenizer(model_proto=tiny_sentencepiece_proto(), max_len=48)
        a = pio.grammar_automaton(tk, "verbose_with_rotation", vocab_size=cfg.vocab_size)
        assert a.eos_token == 1
        model.EOS_TOKEN = 1
        yield cfg, model, a, a.to_device(DEV)
        model.EOS_TOKEN = 1


def _obs1(cfg, seed=0):
    from tests.common import make_inputs, to_observation

    obs, _, _, _ = make_inputs(cfg, B=1, seed=seed, ragged=True)
    so = dict(obs)
    so.pop("tokenized_langact_mask")
    so["image_masks"] = {k: torch.ones_like(m) for k, m in so["image_masks"].items()}
    return to_observation(so | {"tokenized_langact_mask": None}, DEV)


def _accepted_or_cut(a, row, score):
    """A finished beam is a sentence; a beam that the budget or the early stop cut is a path of the automaton (of at least one
    token) with nothing but the zeros of the untouched output after it; a padding beam is neither."""
    if not np.isfinite(score):
        return True
    row = row.tolist()
    if a.eos_token in row:
        return a.accepts(np.asarray(row)) and not any(row[row.index(a.eos_token) + 1:])
    q = 0
    for i, t in enumerate(row):
        if a.step(q, t) < 0:
            return i > 0 and not any(row[i:])
        q = a.step(q, t)
    return True


# The observation of every case is seed 0 of tests/common.py `make_inputs`: under this automaton a state offers at most ten edges and
# the gaps of every step exceed the condition by orders of magnitude (printed).  The condition is asserted, not searched: if a change
# moves the logits, the case fails and says so.
OBS_SEED = {}


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
@pytest.mark.parametrize("budget", [13, 5])
@pytest.mark.parametrize("N", [2, 4, 8])
def test_fused_decode_follows_the_specification_step_by_step(ar, N, budget, weights):
    """The fused grammar beam decode, one step at a time: every step's stored logits go through `beam.grammar_beam_step` in float64
    from the device's own f32 scores and states (under the asserted gap condition), and parents, tokens, gstate, state[0], state[1],
    log-probabilities and scores must be what it says; every finished beam is a sentence of the automaton; the result equals
    `sample_tokens(num_beams=N, grammar=a)` and `beam_decode_fused`.  Budget 13 searches with early_stop=False, so that the decode
    goes on after the rank-0 beam has finished (finished parents, padding); budget 5 with the default."""
    cfg, model, a, d = ar
    _follow(model, cfg, a, d, _obs1(cfg, OBS_SEED.get((N, budget, weights), 0)), N, budget, weights)


def _follow(model, cfg, a, d, o, N, budget, weights, probe=False):
    """probe (choosing OBS_SEED): no assertion on the gaps is made; the smallest of (gap / (4 tol)) over the steps is returned."""
    from lap_amd import ar_decode

    union = a.union()
    early = budget == 5
    with model._serving_weights():
        pre = ar_decode.replicate_prefill(ar_decode.prefill(model, o), N)
        ctx = ar_decode.DecodeCtx(model, N, pre.Pn, budget, weights=weights, beams=N, grammar=d, early_stop=early)
        scores, fin = bm.initial(N)
        states = np.zeros(N, np.int32)
        tokens, logp = np.zeros((N, budget), np.int32), np.zeros((N, budget))
        smax, room, done, worst = 0.0, np.inf, False, 0.0
        for t in range(budget):
            if done:
                break
            ctx.first_token(pre) if t == 0 else ctx.step()
            lg = ctx.logits.cpu().numpy()
            outside = np.ones(cfg.vocab_size, bool)
            outside[union] = False
            assert np.isneginf(lg[:, outside]).all()
            masked = C.masked_by_hand(a, lg, states)
            tol = C.row_tol(a, lg, states) + EPS * max(smax, C.amax(scores))
            row_gap, sel_gap = bm.step_gaps(masked, scores, fin)
            room = min(room, min(row_gap, sel_gap) / (4 * tol))
            assert probe or (row_gap > 4 * tol and sel_gap > 4 * tol), (t, row_gap, sel_gap, tol)
            par, tok, lp, new_scores, fin, done, new_states = bm.grammar_beam_step(lg, scores, fin, states, a, t, budget, model.EOS_TOKEN,
                                                                                   early)
            st, bw = ctx.state.cpu().numpy(), ctx.beam.cpu().numpy()
            if probe and bw[16:16 + N].tolist() != par.tolist():
                return 0.0
            assert bw[16:16 + N].tolist() == par.tolist() and st[0] == t + 1 and st[1] == int(done)
            assert ctx.gstate.cpu().numpy().tolist() == new_states.tolist()
            assert bw[8:8 + N].tolist() == fin.astype(int).tolist() == st[8:8 + N].tolist()
            tokens, logp = tokens[par], logp[par]
            tokens[:, t], logp[:, t] = tok, lp
            assert np.array_equal(ctx.out.cpu().numpy()[:, :t + 1], tokens[:, :t + 1])
            err = np.abs(ctx.logp.cpu().numpy()[:, :t + 1] - logp[:, :t + 1])
            worst = max(worst, float(err.max()))
            assert (err <= tol).all()
            dev_scores = bw[:N].copy().view(np.float32).astype(np.float64)      # the next step adds to the device's own f32 sums
            live = np.isfinite(new_scores)
            assert np.isneginf(dev_scores[~live]).all()
            assert (np.abs(dev_scores[live] - new_scores[live]) <= tol + EPS * C.amax(new_scores[live])).all()
            smax = max(smax, C.amax(new_scores[live]))
            scores, states = dev_scores, new_states
        res = ctx.beam_result()
        tok_f, lp_f, sc_f = ar_decode.beam_decode_fused(model, o, N, max_decoding_steps=budget, weights=weights, grammar=d,
                                                            early_stop=early)
    assert torch.equal(res[0], tok_f) and torch.equal(res[1], lp_f) and torch.equal(res[2], sc_f)
    rows, sc = tok_f.cpu().numpy(), sc_f.cpu().numpy()
    assert all(_accepted_or_cut(a, rows[b], sc[b]) for b in range(N)), rows
    one, lp1 = model.sample_tokens(0, o, max_decoding_steps=budget, decode="fused", decode_weights=weights, num_beams=N, grammar=a,
                                   return_logprobs=True, early_stop=early)
    assert torch.equal(one, tok_f[:1]) and torch.equal(lp1, lp_f[:1])
    print(f"N {N} budget {budget} {weights}: {t + 1} steps, {int(sum(a.eos_token in r.tolist() for r in rows))} finished beams, "
          f"|logp - float64| up to {worst:.3e}, smallest gap / (4 tol) {room:.1f}")
    return room


@pytest.mark.parametrize("weights", ["bf16", "fp8"])
def test_one_beam_is_the_greedy_grammar_decode(ar, weights):
    """N = 1: the tokens of the greedy `grammar=` decode exactly; both log-probabilities are f32 log-softmaxes over the same state's
    set of the same logits, each within tol_lp of the float64 one, so within 2 tol_lp of each other."""
    cfg, model, a, d = ar
    o = _obs1(cfg)
    kw = dict(max_decoding_steps=13, decode="fused", decode_weights=weights, grammar=a, return_logprobs=True)
    col = {}
    want, want_lp = model.sample_tokens(0, o, **kw)
    model.sample_tokens(0, o, collect=col, **kw)
    got, lp = model.sample_tokens(0, o, num_beams=1, **kw)
    assert torch.equal(got, want) and _accepted_or_cut(a, got[0].cpu().numpy(), 0.0)
    A = max(C.amax(v.cpu().numpy()) for v in col.values())
    tol = 2 * C.tol_lp(int(np.diff(a.offsets).max()), A)
    err = float((lp - want_lp).abs().max())
    print(f"{weights}: |logp(beam) - logp(greedy)| up to {err:.3e}, tolerance {tol:.3e}")
    assert err <= tol


ROUTE_REL = 1e-2        # tests/test_beam_gpu.py (tests/test_logprob_gpu.py): the routes' logit rows differ by at most this share of the row's norm
MARGIN = 5e-2           # tests/test_beam_gpu.py: the score margin above which the routes are held to the same choice


def _teacher_forced_logp(model, a, pre, row):
    """(logp float64 [n], d float64 [n]) over the n tokens of `row` up to and including its EOS: the eager log-probability of
    each token given the tokens before it, over the set of the automaton state the tokens before it lead to, from ONE batch-1 chain
    of its own over the batch-1 prefill `pre` (nothing of the beam code is in it), and the route tolerance d = ROUTE_REL |z|_2 of
    the masked logits row each came from."""
    from lap_amd import ar_decode

    logits = ar_decode._lm_logits(model, pre.x_last)
    gen = [(None, None)] * model.v.depth
    lps, ds, q = [], [], 0
    for s, tok in enumerate(row):
        z = logits[0].double().cpu().numpy()[a.allowed(q)]
        ds.append(ROUTE_REL * float(np.sqrt((z * z).sum())))
        lps.append(float(logits[0, int(tok)].double()) - (z.max() + np.log(np.exp(z - z.max()).sum())))
        q = a.step(q, int(tok))
        assert q >= 0, (row, s)
        if int(tok) == a.eos_token or s + 1 == len(row):
            break
        token = torch.tensor([int(tok)], dtype=torch.int32, device=DEV)
        pos = (pre.plen + s).to(torch.int32).view(1, 1).contiguous()
        logits = ar_decode._vlm_decode_step(model, token, pos, s, pre.cache, gen, pre.qinfo_d, pre.kinfo_prefix, 1, pre.Pn)
    return np.asarray(lps), np.asarray(ds)


@pytest.mark.parametrize("budget", [13, 5])
@pytest.mark.parametrize("N", [2, 4, 8])
def test_both_routes_against_teacher_forced_eager_forwards(ar, N, budget):
    """Every beam of the fused route and of the eager route (the host's `grammar_beam_step` on eager logits), scored again token by
    token with a teacher-forced batch-1 eager forward masked to the state's set: a log-probability within 2 d, d = ROUTE_REL |z|_2
    of the masked row, and a score within the sum of those plus the f32 sum's own rounding.  Then the routes against each other,
    tokens and rank order, step by step over the prefix of steps at which the eager side's gaps exceed MARGIN (its length is
    printed, not bounded below)."""
    from lap_amd import ar_decode

    cfg, model, a, d = ar
    o = _obs1(cfg, OBS_SEED.get((N, budget, "bf16"), 0))
    eager_steps = []

    def record(t, masked, scores, finished, res, states):
        prev = eager_steps[-1][1] if eager_steps else np.zeros((N, budget), np.int32)
        hist = prev[res[0]].copy()
        hist[:, t] = res[1]
        eager_steps.append((min(bm.step_gaps(masked, scores, finished)), hist))

    with model._serving_weights():
        pre1 = ar_decode.prefill(model, o)
        tok_e, lp_e, sc_e = ar_decode.beam_decode_eager(model, o, N, max_decoding_steps=budget, grammar=d, on_step=record)
        pre = ar_decode.replicate_prefill(pre1, N)
        ctx = ar_decode.DecodeCtx(model, N, pre.Pn, budget, beams=N, grammar=d)
        fused_steps = []
        for t in range(budget):
            ctx.first_token(pre) if t == 0 else ctx.step()
            if t and int(ctx.state[0]) == len(fused_steps):         # (done: the step wrote nothing)
                break
            fused_steps.append(ctx.out.cpu().numpy().copy())
        tok_f, lp_f, sc_f = ctx.beam_result()
        worst = 0.0
        for name, tok, lp, sc in (("fused", tok_f, lp_f, sc_f), ("eager", tok_e, lp_e, sc_e)):
            tok, lp, sc = tok.cpu().numpy(), lp.cpu().numpy().astype(np.float64), sc.cpu().numpy().astype(np.float64)
            steps = len(fused_steps) if name == "fused" else len(eager_steps)
            assert tok.shape == (N, budget) and np.isfinite(sc[0])
            for b in range(N):
                if not np.isfinite(sc[b]):          # a padding beam: fewer than N candidates ever existed
                    continue
                assert _accepted_or_cut(a, tok[b, :steps], sc[b]), (name, b, tok[b])
                want, dd = _teacher_forced_logp(model, a, pre1, tok[b, :steps])
                n = want.shape[0]
                err = np.abs(lp[b, :n] - want)
                worst = max(worst, float((err / (2 * dd)).max()))
                assert (err <= 2 * dd).all(), (name, b, err, dd)
                assert not lp[b, n:].any() and not tok[b, n:].any()
                # (the f32 sum's own share, as tests/test_beam_gpu.py takes it: tol_lp and one rounded sum per step)
                own = budget * (C.tol_lp(int(np.diff(a.offsets).max()), 0.0) + EPS * abs(want.sum())) + EPS * 64 * budget
                assert abs(sc[b] - want.sum()) <= 2 * dd.sum() + own, (name, b)
    clear = 0
    for t in range(min(len(eager_steps), len(fused_steps))):
        if not eager_steps[t][0] > MARGIN:
            break
        assert np.array_equal(fused_steps[t][:, :t + 1], eager_steps[t][1][:, :t + 1]), t
        clear += 1
    print(f"N {N} budget {budget}: largest |logp - teacher-forced| / (2 d) {worst:.3f}; clear prefix {clear} of {len(eager_steps)} steps")


def test_one_capture_serves_two_observations(ar):
    from lap_amd import ar_decode
    from lap_amd.serve import GraphedTokenDecoder

    cfg, model, a, d = ar
    dec = GraphedTokenDecoder(model, 1, 13, num_beams=4, grammar=a, logprobs=True).capture()
    graphs, ctx = (dec.g_prefill, dec.g_step), dec.ctx
    answers = []
    for seed in (1, 2, 1):
        o = _obs1(cfg, seed)
        tok, lp = dec(o)
        with model._serving_weights():
            want = ar_decode.beam_decode_fused(model, o, 4, max_decoding_steps=13, grammar=d)
        for got, w in zip(dec.last_beams, want):
            assert torch.equal(got.view(torch.int32), w.view(torch.int32))
        assert torch.equal(tok, want[0][:1]) and torch.equal(lp.view(torch.int32), want[1][:1].view(torch.int32))
        rows, sc = want[0].cpu().numpy(), want[2].cpu().numpy()
        assert all(_accepted_or_cut(a, rows[b], sc[b]) for b in range(4))
        answers.append(rows)
    assert (dec.g_prefill, dec.g_step) == graphs and dec.ctx is ctx and ctx.B == 4 and ctx.gstate.shape == (4,)
    assert np.array_equal(answers[0], answers[2])
    with pytest.raises(ValueError, match="allowed_tokens"):
        GraphedTokenDecoder(model, 1, 6, num_beams=4, grammar=a, allowed_tokens=[1, 2, 3])
    with pytest.raises(ValueError, match="jump_forward"):
        GraphedTokenDecoder(model, 1, 6, num_beams=4, grammar=a, jump_forward=4)


@pytest.mark.parametrize("use_graph", [False, True])
def test_ar_policy_answers_with_a_sentence(ar, use_graph):
    from lap_amd import ar_decode, sampling
    from lap_amd.serve import ARPolicy, Policy
    from tests.common import make_inputs

    cfg, model, a, d = ar
    obs, _, _, _ = make_inputs(cfg, B=1, seed=2, ragged=True)
    req = {"image": {k: v[0].numpy() for k, v in obs["images"].items()}, "image_mask": {k: np.array(True) for k in obs["images"]},
           "state": obs["state"][0].numpy(), "tokenized_prompt": obs["tokenized_prompt"][0].numpy(),
           "tokenized_prompt_mask": obs["tokenized_prompt_mask"][0].numpy()}
    pol = ARPolicy(Policy(model, use_graph=False), sample_kwargs={"num_beams": 4, "grammar": a, "select": "sum", "max_decoding_steps": 13},
                   use_graph=use_graph)
    assert (pol._decoder is not None) == use_graph
    res = pol.infer(req)
    o = pol._base._to_observation(req)[0]
    with model._serving_weights():
        tok, lp, sc = (t.cpu().numpy() for t in ar_decode.beam_decode_fused(model, o, 4, max_decoding_steps=13, grammar=d))
    assert np.array_equal(res["candidates"]["tokens"], tok)
    lp = np.where(np.isfinite(sc)[:, None], lp, -np.inf)
    best = sampling.select_best(tok, lp, model.EOS_TOKEN, "sum")
    assert np.array_equal(res["tokens"][0], tok[best]) and _accepted_or_cut(a, res["tokens"][0], sc[best])
