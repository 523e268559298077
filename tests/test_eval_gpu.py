"""Verbose token-accuracy metrics (lap.py:209-289, metrics.py:7-73) and checkpoint evaluation (scripts/eval.py) on the GPU: the fused
cross-entropy + argmax kernel, the token-metrics kernel, the model's verbose metrics against metrics.py restated in torch, and an
end-to-end train -> evaluate run."""
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------ kernels
def _ce_pair(hip, lg_full, targets, chunks):
    R = lg_full.shape[0]
    st = [torch.full((R,), -3.0e38, device="cuda"), torch.zeros(R, device="cuda"), torch.zeros(R, device="cuda")]
    sa = [t.clone() for t in st]
    amax = torch.full((R,), -7, dtype=torch.int32, device="cuda")
    for v0, vc in chunks:
        hip.ce_chunk_update(lg_full[:, v0:v0 + vc], targets, *st, v0)
        hip.ce_chunk_update_argmax(lg_full[:, v0:v0 + vc], targets, *sa, amax, v0)
    torch.cuda.synchronize()
    return st, sa, amax


def test_ce_update_argmax_matches_ce_update_and_argmax_at_full_vocab(hip):
    R, V = 512, 257_152
    g = torch.Generator(device="cuda").manual_seed(0)
    lg = torch.randn((R, V), generator=g, device="cuda") * 3.0
    targets = torch.randint(0, V, (R,), generator=g, device="cuda", dtype=torch.int32)
    big = float(lg.max()) + 1.0
    lg[0, 100] = lg[0, 5000] = big                      # a tie inside one chunk (different waves)
    lg[1, 65535] = lg[1, 65536] = big                   # a tie across the boundary of 64 Ki-column chunks
    lg[2, 70000] = lg[2, 250000] = big                  # a tie between two later chunks
    lg[3, 8] = lg[3, 9] = lg[3, 10] = big               # a tie inside one thread's 4-vector
    lg[4, 0] = lg[4, V - 1] = big                       # the first and the last column
    lg[5, 64 * 4] = lg[5, 4] = big                      # a tie across lanes of one wave
    ref = torch.argmax(lg, dim=1).to(torch.int32)
    assert ref[:6].tolist() == [100, 65535, 70000, 8, 0, 4]
    from lap_amd.loss import vocab_chunks

    for chunks in (vocab_chunks(R, V),                                    # the model's chunking: one chunk at R = 512
                   [(v0, min(65536, V - v0)) for v0 in range(0, V, 65536)]):
        st, sa, amax = _ce_pair(hip, lg, targets, chunks)
        for a, b in zip(st, sa):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))      # bitwise
        assert torch.equal(amax, ref)


def test_ce_update_argmax_odd_width_unaligned_rows(hip):
    R, ld, vc = 37, 1001, 997
    g = torch.Generator(device="cuda").manual_seed(1)
    base = torch.randn((R, ld), generator=g, device="cuda")
    base[:, 1:1 + vc] = torch.round(base[:, 1:1 + vc] * 4)                  # many exact ties
    lg = base[:, 1:1 + vc]                                                   # row starts off 16-byte alignment, odd stride
    targets = torch.randint(0, vc, (R,), generator=g, device="cuda", dtype=torch.int32)
    st, sa, amax = _ce_pair(hip, lg, targets, [(0, vc)])
    for a, b in zip(st, sa):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(amax, torch.argmax(lg, dim=1).to(torch.int32))
    # two chunks of the odd view
    st, sa, amax = _ce_pair(hip, lg, targets, [(0, 500), (500, vc - 500)])
    assert torch.equal(amax, torch.argmax(lg, dim=1).to(torch.int32))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(st, sa))


def _metrics_ref(pred_full, labels, nll_full, lm, crit, num, dirn):
    """metrics.py:7-45 restated in torch (token_mask = lm != 0, per_token_loss = nll * lm)."""
    correct = (pred_full == labels).float()
    tm = lm != 0
    out = {"token_accuracy": (correct * tm).sum() / torch.clamp(tm.float().sum(), min=1.0), "per_token_loss": nll_full * lm}
    for name, mk in (("critical", crit), ("number", num), ("direction", dirn)):
        if mk is not None:
            out[f"{name}_token_accuracy"] = (correct * mk).sum() / torch.clamp(mk.float().sum(), min=1.0)
            out[f"per_sample_{name}_correct"] = (correct * mk).sum(-1)
            out[f"per_sample_{name}_total"] = mk.float().sum(-1)
    return out


@pytest.mark.parametrize("with_sel", [False, True])
def test_token_metrics_kernel_against_torch(hip, with_sel):
    B, Lm = 6, 300
    g = torch.Generator(device="cuda").manual_seed(2)
    rnd = lambda p: torch.rand((B, Lm), generator=g, device="cuda") < p
    lmb = rnd(0.3)
    crit, num = rnd(0.1) & ~lmb, rnd(0.2)
    lmb[3] = crit[3] = num[3] = False                      # a masked-out sample
    row_mask = lmb | crit | num
    labels = torch.randint(0, 20, (B, Lm), generator=g, device="cuda", dtype=torch.int32)
    pred_full = torch.where(rnd(0.5), labels, torch.randint(0, 20, (B, Lm), generator=g, device="cuda", dtype=torch.int32))
    nll_full = torch.rand((B, Lm), generator=g, device="cuda") * 5
    lm = lmb.float()
    if with_sel:
        Ls = int(row_mask.sum(-1).max())
        sel = torch.sort((~row_mask).to(torch.uint8), dim=1, stable=True).indices[:, :Ls].to(torch.int32).contiguous()
        gat = lambda t: t.gather(1, sel.long()).contiguous().view(-1)
        ptl, counts = hip.token_metrics(gat(pred_full), gat(labels), gat(nll_full), lm, sel=sel, critical=crit, number=num)
    else:
        v = lambda t: t.contiguous().view(-1)
        ptl, counts = hip.token_metrics(v(pred_full), v(labels), v(nll_full), lm, critical=crit, number=num)
    ref = _metrics_ref(pred_full, labels, nll_full, lm, crit, num, None)
    assert torch.equal(ptl, ref["per_token_loss"])
    tm = lmb.float()
    assert torch.equal(counts[:, 0, 0], ((pred_full == labels).float() * tm).sum(-1)) and torch.equal(counts[:, 0, 1], tm.sum(-1))
    assert torch.equal(counts[:, 1, 0], ref["per_sample_critical_correct"]) and torch.equal(counts[:, 1, 1], ref["per_sample_critical_total"])
    assert torch.equal(counts[:, 2, 0], ref["per_sample_number_correct"]) and torch.equal(counts[:, 2, 1], ref["per_sample_number_total"])
    assert torch.equal(counts[:, 3], torch.zeros_like(counts[:, 3]))           # absent direction mask
    assert torch.equal(counts[3], torch.zeros_like(counts[3]))


def test_token_metrics_rejects_bad_shapes(hip):
    z = torch.zeros(8, dtype=torch.int32, device="cuda")
    lm = torch.zeros((2, 4), device="cuda")
    with pytest.raises(ValueError):
        hip.token_metrics(z[:6], z[:6], torch.zeros(6, device="cuda"), lm)
    with pytest.raises(TypeError):
        hip.token_metrics(z, z, torch.zeros(8, device="cuda"), lm, critical=torch.zeros((2, 4), device="cuda"))


# ------------------------------------------------------------------------------------------------------------ model
def _batch(cfg, *, dropout=False, B=4, seed=1):
    from lap_amd.observation import CoTObservation
    from tests.common import make_inputs, to_observation

    obs, actions, noise, time = make_inputs(cfg, B=B, seed=seed, ragged=True)
    la, pm = obs["tokenized_langact_mask"], obs["tokenized_prompt_mask"]
    g = torch.Generator().manual_seed(seed + 100)
    crit = la & (torch.rand(la.shape, generator=g) < 0.5)
    num = crit & (torch.rand(la.shape, generator=g) < 0.5)
    dirn = crit & ~num
    tl = obs["token_loss_mask"].clone()
    if dropout:        # reasoning dropout (tokenizer.py:140-206): part of the span, class tokens included, carries no loss
        for b in range(B):
            idx = torch.nonzero(la[b]).view(-1)
            tl[b, idx[: len(idx) // 2]] = False
    loss_rows = (la & pm & tl)[:, 1:].sum(-1).max()
    metric_rows = ((la & pm & tl) | crit | num | dirn)[:, 1:].sum(-1).max()
    o = dataclasses.replace(to_observation({**obs, "token_loss_mask": tl}, "cuda"), critical_token_mask=crit.cuda(),
                            number_token_mask=num.cuda(), direction_token_mask=dirn.cuda(), loss_rows_max=int(loss_rows),
                            metric_rows_max=int(metric_rows))
    assert isinstance(o, CoTObservation)
    return o, actions.cuda(), dict(noise=noise.cuda(), time=time.cuda())


def _model(cfg, seed=3):
    from lap_amd.model import LAP

    return LAP(cfg, seed=seed, device="cuda")


def _restated(hip, model, obs, collect, nll_rows):
    """metrics.py restated from the logits of the engine's own LM-head GEMMs on the collected pre-logits."""
    pl, sel = collect["pl"], collect["sel"]
    R, Dv = pl.shape
    V = model.config.vocab_size
    lg = torch.empty((R, V), dtype=torch.float32, device="cuda")
    hip.gemm(pl, model.W("llm/embed"), lg, M=R, N=V, K=Dv, lda=Dv, ldb=Dv, ldc=V)
    lo = model.ps.w16lo("llm/embed")
    if lo is not None:
        hip.gemm(pl, lo, lg, M=R, N=V, K=Dv, lda=Dv, ldb=Dv, ldc=V, accum=True)
    pred = torch.argmax(lg, dim=1).to(torch.int32)
    B = obs.tokenized_prompt.shape[0]
    Lm = obs.tokenized_prompt.shape[1] - 1
    Ls = R // B
    pos = sel.long() if sel is not None else torch.arange(Ls, device="cuda").expand(B, Ls)
    pred_full = torch.full((B, Lm), -1, dtype=torch.int32, device="cuda").scatter(1, pos, pred.view(B, Ls))
    nll_full = torch.zeros((B, Lm), device="cuda").scatter(1, pos, nll_rows.view(B, Ls))
    labels = obs.tokenized_prompt[:, 1:]
    lm = (obs.tokenized_langact_mask[:, 1:] & obs.tokenized_prompt_mask[:, 1:] & obs.token_loss_mask[:, 1:] & obs.sample_mask[:, None]).float()
    prep = lambda m: m[:, 1:] & obs.sample_mask[:, None]
    return pred, _metrics_ref(pred_full, labels, nll_full, lm, prep(obs.critical_token_mask), prep(obs.number_token_mask),
                              prep(obs.direction_token_mask))


def _nll_rows(model, collect, obs):
    """The per-row cross entropy from the restated logits (reference nll for per_token_loss, to f32 rounding)."""
    pl, sel = collect["pl"], collect["sel"]
    R, Dv = pl.shape
    V = model.config.vocab_size
    from lap_amd import hip

    lg = torch.empty((R, V), dtype=torch.float32, device="cuda")
    hip.gemm(pl, model.W("llm/embed"), lg, M=R, N=V, K=Dv, lda=Dv, ldb=Dv, ldc=V)
    lo = model.ps.w16lo("llm/embed")
    if lo is not None:
        hip.gemm(pl, lo, lg, M=R, N=V, K=Dv, lda=Dv, ldb=Dv, ldc=V, accum=True)
    B = obs.tokenized_prompt.shape[0]
    Ls = R // B
    t = obs.tokenized_prompt[:, 1:]
    t = (t.gather(1, sel.long()) if sel is not None else t[:, :Ls]).reshape(-1).long()
    return torch.logsumexp(lg.double(), 1) - lg.double().gather(1, t.view(-1, 1)).view(-1)


@pytest.mark.parametrize("dropout", [False, True])
def test_verbose_metrics_match_metrics_py(hip, dropout):
    from tests.common import debug_model_cfg

    cfg = debug_model_cfg()
    model = _model(cfg)
    obs, actions, kw = _batch(cfg, dropout=dropout)
    collect = {}
    loss, m = model.compute_loss(0, obs, actions, verbose_mode=True, collect=collect, **kw)
    nll = _nll_rows(model, collect, obs)
    pred, ref = _restated(hip, model, obs, collect, nll.float())
    assert torch.equal(collect["predictions"].view(-1), pred)
    for k in ("token_accuracy", "critical_token_accuracy", "number_token_accuracy", "direction_token_accuracy",
              "per_sample_critical_correct", "per_sample_critical_total", "per_sample_number_correct", "per_sample_number_total",
              "per_sample_direction_correct", "per_sample_direction_total"):
        assert torch.equal(m[k], ref[k]), k
    torch.testing.assert_close(m["per_token_loss"], ref["per_token_loss"], rtol=2e-5, atol=2e-5)
    assert torch.equal(m["labels"], obs.tokenized_prompt[:, 1:])
    psl = cfg.language_loss_weight * collect["per_sample_lang"] + cfg.action_loss_weight * collect["per_sample_action"]
    assert torch.equal(m["per_sample_loss"], psl)
    if dropout:     # class tokens outside the loss mask are scored: the totals are the full mask sums
        crit = obs.critical_token_mask[:, 1:] & obs.sample_mask[:, None]
        lmask = obs.tokenized_langact_mask[:, 1:] & obs.token_loss_mask[:, 1:] & obs.tokenized_prompt_mask[:, 1:]
        assert int((crit & ~lmask).sum()) > 0
        assert torch.equal(m["per_sample_critical_total"], crit.float().sum(-1))
        assert obs.metric_rows_max > obs.loss_rows_max
    assert torch.isfinite(loss)


def test_verbose_is_bitwise_neutral_when_rows_coincide(hip):
    """Class masks inside the loss mask: the same rows run, so loss, metrics and gradients equal the verbose-off call bit for bit."""
    from tests.common import debug_model_cfg

    cfg = debug_model_cfg()
    obs, actions, kw = _batch(cfg)
    assert obs.metric_rows_max == obs.loss_rows_max
    model = _model(cfg)
    l0, m0 = model.compute_loss(0, obs, actions, **kw)
    l1, m1 = model.compute_loss(0, obs, actions, verbose_mode=True, **kw)
    assert torch.equal(l0, l1) and set(m0) < set(m1)
    assert all(torch.equal(m0[k], m1[k]) for k in m0)
    assert "token_accuracy" not in m0 and "per_sample_loss" not in m0

    def grads(verbose):
        model.config = dataclasses.replace(cfg, verbose_mode=verbose)
        for u in model.ps.units:
            model.ps.grad[u.name].zero_()
        loss, met = model.loss_and_grad(0, obs, actions, **kw)
        torch.cuda.synchronize()
        return loss, met, {u.name: model.ps.grad[u.name].clone() for u in model.ps.units}

    la, ma, ga = grads(False)
    _, _, ga2 = grads(False)
    lb, mb, gb = grads(True)
    assert torch.equal(la, lb) and "token_accuracy" in mb and "token_accuracy" not in ma
    assert all(torch.equal(ma[k], mb[k]) for k in ma)
    for n in ga:
        if torch.equal(ga[n], ga2[n]):
            assert torch.equal(ga[n], gb[n]), n
        else:       # units accumulated with f32 atomics (small unit, the table's scatter-add) differ between two verbose-off calls
            run = float((ga[n].float() - ga2[n].float()).norm())
            assert float((ga[n].float() - gb[n].float()).norm()) <= max(10 * run, 1e-6 * float(ga[n].float().norm())), n
    assert sum(torch.equal(ga[n], ga2[n]) for n in ga) >= len(ga) - 2
    model.config = cfg
    # compute_loss(verbose_mode=None) follows the config
    model.config = dataclasses.replace(cfg, verbose_mode=True)
    _, m2 = model.compute_loss(0, obs, actions, **kw)
    assert "token_accuracy" in m2
    model.config = cfg


def test_too_small_metric_hint_poisons_the_loss(hip):
    from tests.common import debug_model_cfg

    cfg = debug_model_cfg()
    obs, actions, kw = _batch(cfg, dropout=True)
    model = _model(cfg)
    loss, _ = model.compute_loss(0, dataclasses.replace(obs, metric_rows_max=obs.metric_rows_max - 1), actions, verbose_mode=True, **kw)
    assert torch.isnan(loss)
    loss, _ = model.compute_loss(0, obs, actions, verbose_mode=True, **kw)
    assert torch.isfinite(loss)


def test_per_vqa_dataset_losses(hip):
    from lap_amd.config import VQA_DATASET_ID_MAP
    from tests.common import debug_model_cfg

    cfg = debug_model_cfg(enable_vqa_training=True, vqa_loss_weight=0.7)
    obs, actions, kw = _batch(cfg, B=4)
    obs = dataclasses.replace(obs, is_vqa_sample=torch.tensor([True, True, False, True], device="cuda"),
                              vqa_dataset_id=torch.tensor([1, 2, 0, 1], dtype=torch.int32, device="cuda"))
    model = _model(cfg)
    collect = {}
    _, m = model.compute_loss(0, obs, actions, collect=collect, **kw)
    lang = collect["per_sample_lang"]
    vqa = obs.is_vqa_sample & obs.sample_mask
    for name, i in VQA_DATASET_ID_MAP.items():
        mk = ((obs.vqa_dataset_id == i) & vqa).float()
        assert float(m[f"vqa_{name}_num_samples"]) == float(mk.sum()), name
        torch.testing.assert_close(m[f"vqa_{name}_loss"], (lang * mk).sum() / torch.clamp(mk.sum(), min=1.0), rtol=1e-6, atol=0)
    assert float(m["vqa_coco_captions_num_samples"]) == float(vqa[[0, 3]].sum())


# ------------------------------------------------------------------------------------------------------------ end to end
def test_train_then_evaluate_all_checkpoints(hip, tmp_path):
    from lap_amd import evaluate as E
    from lap_amd.config import EmaScheduleChoice, get_config
    from lap_amd.model import LAP
    from lap_amd.params import ParamStore
    from lap_amd.train import SyntheticDataLoader, ValidationStepRunner, TrainState, main
    from lap_amd import checkpoints as ck

    tc = dataclasses.replace(get_config("debug"), checkpoint_base_dir=str(tmp_path), exp_name="ev", batch_size=2, num_train_steps=4,
                             save_interval=1, keep_period=1, log_interval=2, seed=5,
                             ema_schedule_choice=EmaScheduleChoice(kind="delayed", start_step=2))
    main(tc, log=lambda s: None)
    mngr = ck.CheckpointManager(tc.checkpoint_dir)
    assert mngr.all_steps() == (1, 2, 3, 4)
    ec = dataclasses.replace(tc, num_eval_batches=2, model=dataclasses.replace(tc.model, verbose_mode=True))
    val = SyntheticDataLoader(ec.model, 2, "cuda", seed=99, num_batches=3)
    lines = []
    res = E.main(ec, data_loaders={"original": val}, log=lines.append, output=tmp_path / "r.json")
    assert any("eval_demo_dataset" in l for l in lines)         # debug data_mix is set, no loader for it: skipped with a line
    for s in (1, 2, 3, 4):
        assert res[f"step_{s}/val_loss/original/eval/val_loss/num_batches"] == 2
        assert res[f"step_{s}/action_prediction_loss/original/eval/action_prediction_loss/num_batches"] == 2
        assert f"step_{s}/val_loss/original/eval/val_loss/token_accuracy" in res
        assert not any(k.startswith(f"step_{s}/val_loss/original/eval/val_loss/per_") for k in res)
        assert not any("per_sample_action_prediction_loss" in k for k in res)
    assert all(k.startswith("step_") and k.split("/")[3] == "eval" for k in res)
    assert any("live" in l for l in lines) and any("EMA" in l for l in lines)
    # by hand: steps 1 and 2 < ... start_step=2 -> step 1 live, steps >= 2 EMA
    model = LAP(ec.model, device="cuda", store=ParamStore(ec.model, "cuda", with_optimizer=False, with_ema=False, with_grads=False))
    runner = ValidationStepRunner(ec)
    for s in (1, 2, 4):
        which = "live" if s < 2 else "ema"
        model.ps.load_reference_tree(ck.restore_eval_params(mngr, s, which, ec.model))
        st = TrainState(step=s, model=model, ema_decay=None)
        vl = [runner(ec.seed, st, b)["val_loss"] for b in iter(val)][:2]
        want = float(torch.stack(vl).mean())
        got = res[f"step_{s}/val_loss/original/eval/val_loss/val_loss"]
        assert abs(got - want) <= 1e-6 * abs(want), (s, got, want)
        seed = ec.seed * 1_000_003 + s
        mse = []
        for i, (o, a) in enumerate(iter(val)):
            if i == 2:
                break
            p = model.sample_actions(seed, o)
            mse.append(((p.float() - a.float()) ** 2).mean(dim=(1, 2)).mean())
        got = res[f"step_{s}/action_prediction_loss/original/eval/action_prediction_loss/action_prediction_loss"]
        assert abs(got - float(torch.stack(mse).mean())) <= 1e-5 * max(1.0, abs(got)), (s, got)
    # the live and EMA weights of a step past the start differ, and the evaluator used the EMA ones
    live4 = ck.restore_eval_params(mngr, 4, "live", ec.model)
    ema4 = ck.restore_eval_params(mngr, 4, "ema", ec.model)
    assert any(not torch.equal(live4[k], ema4[k]) for k in live4)
    import json

    assert json.loads((tmp_path / "r.json").read_text()) == res
