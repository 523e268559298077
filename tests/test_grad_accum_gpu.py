"""Gradient accumulation in the train step (TrainConfig.grad_accum_steps, GPU): an accumulated step over K micro-batches against
the plain step on the whole batch and against the oracle's f32 gradient; the global loss denominators; what the pipeline leaves
behind; the freeze filter.  Debug widths (tests/common.debug_model_cfg, make_inputs).

MARGIN: the accumulated gradient rounds every micro-gradient to bf16 before the f32 sum where the plain step rounds once, so its
relative L2 error against the oracle's f32 gradient may exceed the plain step's.  Measured per tensor on MI355X over seeds 1, 2, 3
(docs/EXPERIMENTS.md, "Gradient accumulation"): see the figures there and next to MARGIN below."""
import dataclasses

import pytest
import torch

from oracle import lap_oracle as O
from tests.common import debug_model_cfg, make_inputs, oracle_cfg, rel, to_observation

pytestmark = pytest.mark.gpu
DEV = "cuda"
# worst err_accumulated / err_plain over every tensor, per (K, seed): K = 2: 1.0086, 1.0121, 1.0039; K = 3: 1.0169, 1.0051, 1.0105.
# Largest 1.0169, spread over the seeds (max - min) 0.0130: 1.0169 + 0.0130 = 1.0299, rounded up
MARGIN = 1.03
# a tensor is held to MARGIN unless the REFERENCE gradient itself is zero up to rounding: only the SigLIP key bias is (a shift of every
# key by one vector leaves the softmax unchanged), max |g| ~ 1e-9 against 1e-3 .. 1e-1 for every other tensor
GRAD_FLOOR = 1e-6
_ORACLE = {}


def _tc(K=1, **kw):
    from lap_amd.config import get_config

    cfg = debug_model_cfg(enable_vqa_training=True, enable_prediction_training=True, vqa_loss_weight=0.1, prediction_loss_weight=0.7)
    return dataclasses.replace(get_config("debug"), model=cfg, grad_accum_steps=K, batch_size=2 * K if K > 1 else 2, **kw)


def _inputs(cfg, K, seed=1):
    """2K samples; sample 1 idle, sample 2 a VQA sample, sample 3 a prediction sample: n_active / n_action per micro-batch of two are
    (1, 2), (2, 1 after the clamp at 0) and, for K = 3, (2, 2) — against (3, 2) or (5, 4) for the whole batch."""
    B = 2 * K
    obs, actions, noise, time = make_inputs(cfg, B=B, ragged=True, seed=seed)
    obs["is_vqa_sample"] = torch.tensor([i == 2 for i in range(B)])
    obs["is_prediction_sample"] = torch.tensor([i == 3 for i in range(B)])
    return obs, actions, noise, time


def _slice(obs, sl):
    return {k: ({kk: vv[sl] for kk, vv in v.items()} if isinstance(v, dict) else (v[sl] if v is not None else None)) for k, v in obs.items()}


def _micro(obs, actions, noise, time, K):
    sls = [slice(2 * k, 2 * k + 2) for k in range(K)]
    return ([(to_observation(_slice(obs, s), DEV), actions[s].to(DEV)) for s in sls], [noise[s].to(DEV) for s in sls], [time[s].to(DEV) for s in sls])


def _oracle(K, seed):
    """(P, f32 gradients of the whole batch, f32 loss, bf16-emulated loss): computed once per (K, seed), never modified."""
    if (K, seed) not in _ORACLE:
        cfg = _tc().model
        oc = oracle_cfg(cfg)
        P = O.init_params(oc, seed=5)
        obs, actions, noise, time = _inputs(cfg, K, seed)
        Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
        loss32, _ = O.compute_loss(Pg, oc, obs, actions, noise, time)
        loss32.backward()
        loss16, _ = O.compute_loss(P, dataclasses.replace(oc, emulate_bf16=True), obs, actions, noise, time)
        _ORACLE[(K, seed)] = (P, {k: v.grad.detach() for k, v in Pg.items() if v.grad is not None}, loss32.item(), loss16.item())
    return _ORACLE[(K, seed)]


def _engine_grads(ps, accumulated):
    """The gradient the optimizer pass reads, in the reference's layout: the f32 accumulators of the big units after an accumulated step."""
    from lap_amd.params import engine_to_reference

    out = {}
    for name in ps.names():
        u = ps.tensor_unit[name]
        buf = ps.gacc[u.name] if (accumulated and u.big) else ps.grad[u.name]
        out[name] = ps._view(buf, name).detach().float().cpu()
    return engine_to_reference(ps.cfg, out)


def _run(K, seed, *, P=None, freeze=None, denominators=True, monkeypatch=None):
    from lap_amd.train import TrainingStepRunner, init_train_state

    tc = _tc(K, **({"freeze_filter": freeze} if freeze is not None else {}))
    P = _oracle(K, seed)[0] if P is None else P
    obs, actions, noise, time = _inputs(tc.model, K, seed)
    state = init_train_state(tc, params=P, device=DEV)
    runner = TrainingStepRunner(tc)
    if not denominators:
        monkeypatch.setattr("lap_amd.loss.global_denominators", lambda *a, **k: None)
    if K > 1:
        batches, nz, tm = _micro(obs, actions, noise, time, K)
        state, info = runner(0, state, batches, 0, noise=nz, time=tm)
    else:
        state, info = runner(0, state, (to_observation(obs, DEV), actions.to(DEV)), 0, noise=noise.to(DEV), time=time.to(DEV))
    state.model.comm.synchronize()
    torch.cuda.synchronize()
    return tc, state, info


def _errors(K, seed):
    """Per tensor: (relative L2 error of the accumulated gradient, of the plain step's gradient) against the oracle's f32 gradient."""
    P, gref, loss32, loss16 = _oracle(K, seed)
    tca, sa, ia = _run(K, seed)
    ga = _engine_grads(sa.model.ps, True)
    tcp, sp, ip = _run_plain(K, seed)
    gp = _engine_grads(sp.model.ps, False)
    return {k: (rel(ga[k], gref[k]), rel(gp[k], gref[k]), float(gref[k].abs().max())) for k in gref}, (sa, ia, ga), (sp, ip, gp)


def _run_plain(K, seed):
    """The plain step (grad_accum_steps = 1) on the whole batch of 2K samples."""
    from lap_amd.train import TrainingStepRunner, init_train_state

    tc = dataclasses.replace(_tc(), batch_size=2 * K)
    P = _oracle(K, seed)[0]
    obs, actions, noise, time = _inputs(tc.model, K, seed)
    state = init_train_state(tc, params=P, device=DEV)
    state, info = TrainingStepRunner(tc)(0, state, (to_observation(obs, DEV), actions.to(DEV)), 0, noise=noise.to(DEV), time=time.to(DEV))
    state.model.comm.synchronize()
    torch.cuda.synchronize()
    return tc, state, info


@pytest.mark.parametrize("K", [2, 3])
def test_accumulated_step_equals_the_plain_step_on_the_whole_batch(hip, K):
    seed = 1
    P, gref, loss32, loss16 = _oracle(K, seed)
    errs, (sa, ia, ga), (sp, ip, gp) = _errors(K, seed)
    for k, (ea, ep, gmax) in sorted(errs.items()):
        print(f"K {K} seed {seed} {k}: accumulated {ea:.3e} plain {ep:.3e} ratio {ea / max(ep, 1e-30):.3f}")
    exempt = {k for k, (_, _, gmax) in errs.items() if gmax < GRAD_FLOOR}
    assert exempt <= {"PaliGemma/img/Transformer/encoderblock/MultiHeadDotProductAttention_0/key/bias"}, exempt
    for k, (ea, ep, gmax) in errs.items():
        assert ea <= MARGIN * ep or k in exempt, (k, ea, ep)
    # no accumulator outside the big units, and the optimizer read them
    ps = sa.model.ps
    assert set(ps.gacc) == {u.name for u in ps.units if u.big} and all(a.dtype == torch.float32 for a in ps.gacc.values())
    assert not sp.model.ps.gacc
    # the summed loss is the whole batch's: the bf16 criterion of the model-parity tests (engine against engine, and each against the oracle)
    la, lp = ia["loss"].item(), ip["loss"].item()
    ref_noise = abs(loss16 - loss32) / abs(loss32)
    print(f"K {K} loss accumulated {la:.6f} plain {lp:.6f} oracle {loss32:.6f} bf16 oracle {loss16:.6f}")
    assert abs(la - lp) / abs(lp) < max(3 * ref_noise, 5e-3), (la, lp)
    assert abs(la - loss32) / abs(loss32) < max(3 * ref_noise, 5e-3), (la, loss32)
    # grad_norm is the norm of the accumulated gradient
    gn = torch.sqrt(sum((g.double() ** 2).sum() for g in ga.values())).item()
    assert abs(ia["grad_norm"].item() - gn) / gn < 1e-5, (ia["grad_norm"].item(), gn)
    assert sa.step == 1 and sp.step == 1
    # the update: (1) clip -> AdamW applied to the accumulated gradient is the oracle's restatement on the same gradient, tensor by tensor
    # (tests/test_model_parity_gpu.py::test_train_step_matches_oracle_adamw, 2e-5 where the update is well conditioned) ...
    tc = _tc(K)
    opt, lr = tc.optimizer, tc.lr_schedule(0)
    cs = O.clip_scale(gn, opt.clip_gradient_norm)
    new_a, new_p = ps.to_reference_tree("master"), sp.model.ps.to_reference_tree("master")
    for k in P:
        p1, _, _ = O.adamw_step(P[k], ga[k], torch.zeros_like(P[k]), torch.zeros_like(P[k]), 1, lr, opt.b1, opt.b2, opt.eps, opt.weight_decay, cs)
        du, dr = new_a[k] - P[k], p1 - P[k]
        big = ga[k].abs() * cs > 1e-5
        if dr.norm() > 0 and big.any():
            assert rel(du[big], dr[big]) < 2e-5, (k, rel(du[big], dr[big]))
    # ... (2) and the two runs' updates agree, EVERY tensor, as two runs of one step do whose gradients differ by bf16 rounding (the
    # rank-parity bound of tests/test_fsdp_gpu.py on the update: Adam's first step is sign-like)
    for k in P:
        upd_a, upd_p = new_a[k] - P[k], new_p[k] - P[k]
        if k in exempt or upd_p.norm() == 0:
            continue
        print(f"K {K} {k}: update accumulated vs plain {rel(upd_a, upd_p):.3e}")
        assert rel(upd_a, upd_p) < 0.1, (k, rel(upd_a, upd_p))


def test_global_denominators_do_work(hip, monkeypatch):
    """The same split with every micro-step dividing by its OWN counts: a different gradient — the input can tell.  Checked on the
    language path: its micro-steps divide by 1 and 2 active samples instead of 3.  (The action expert's gradient coincides at K = 2 on
    this input: micro-batch 1 has no action sample and micro-batch 0 has the whole batch's count of two.)"""
    K, seed = 2, 1
    P, gref, _, _ = _oracle(K, seed)
    _, sa, ia = _run(K, seed)
    ga = _engine_grads(sa.model.ps, True)
    _, sn, inn = _run(K, seed, denominators=False, monkeypatch=monkeypatch)
    gn_ = _engine_grads(sn.model.ps, True)
    for k in ("PaliGemma/llm/layers/mlp/linear", "PaliGemma/img/head/kernel", "PaliGemma/llm/final_norm/scale"):
        print(f"{k}: with {rel(ga[k], gref[k]):.3e} without {rel(gn_[k], gref[k]):.3e}")
        assert rel(ga[k], gref[k]) < 5e-2 and rel(gn_[k], gref[k]) > 0.2, (k, rel(ga[k], gref[k]), rel(gn_[k], gref[k]))
    assert abs(inn["loss"].item() - ia["loss"].item()) > 5e-2 * abs(ia["loss"].item())


_BITS = {}


def _bit_for_bit_runs(tmp_path):
    """One fresh process for both bit-for-bit cases, with LAP_SUMSQ_BLOCKS=1: the gradient norm's partial sums are f32 atomic adds,
    one per block, and land in no fixed order, so two identical steps of this process report grad_norm one f32 ulp apart about every
    other time (and the parameters follow through the clip factor).  One block per norm launch gives the sum one order; the knob is
    read once per process.  Figures and the scenario code: tests/grad_accum_worker.py."""
    if "res" not in _BITS:
        import gc
        import os
        import pathlib
        import subprocess
        import sys

        out = tmp_path / "bits.pt"
        env = {k: v for k, v in os.environ.items() if not k.startswith("LAP_")}
        env["LAP_SUMSQ_BLOCKS"] = "1"
        gc.collect()
        torch.cuda.empty_cache()
        root = pathlib.Path(__file__).resolve().parent.parent
        r = subprocess.run([sys.executable, "-m", "tests.grad_accum_worker", str(out)], cwd=root, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        _BITS["res"] = torch.load(out)
    return _BITS["res"]


def test_plain_step_after_an_accumulated_step_starts_clean(hip, tmp_path):
    """A K = 1 step on the runner state an accumulated step left (learning rate 0: the parameters are the initial ones) against
    the same step on a fresh state, bit for bit: no stale sum of squares, fold_sumsq back on, the small unit zeroed."""
    c = _bit_for_bit_runs(tmp_path)["clean"]
    print(f"(loss, grad_norm) after an accumulated step {c['after']!r} fresh {c['fresh']!r}")
    assert c["fold_restored"] and c["accum"] == (0, 1) and c["fresh_gacc"] == 0
    assert c["after"][1] == c["fresh"][1]
    assert c["after"][0] == c["fresh"][0]


def test_one_micro_batch_through_the_list_argument_is_the_existing_call(hip, tmp_path):
    """Bit for bit in loss, grad_norm and every parameter."""
    plain, as_list = _bit_for_bit_runs(tmp_path)["list"]
    print(f"existing call: loss {plain[0]!r} grad_norm {plain[1]!r}; list of one pair: loss {as_list[0]!r} grad_norm {as_list[1]!r}")
    assert plain[3] == 0 and as_list[3] == 0           # no accumulator either way
    assert plain[0] == as_list[0] and plain[1] == as_list[1], (plain[:2], as_list[:2])
    assert set(plain[2]) == set(as_list[2])
    for k, v in plain[2].items():
        assert torch.equal(v, as_list[2][k]), k


def test_frozen_vlm_accumulates_over_the_trainable_ranges_only(hip):
    K, seed = 2, 1
    cfg = _tc().model
    frz = cfg.get_vlm_freeze_filter()
    P = {k: (v.to(torch.bfloat16).float() if frz(k) else v) for k, v in _oracle(K, seed)[0].items()}
    tc, state, info = _run(K, seed, P=P, freeze=frz)
    ps = state.model.ps
    new = ps.to_reference_tree("master")
    moved = 0
    for k, v in P.items():
        if frz(k):
            assert torch.equal(new[k], v), k
        else:
            moved += int(not torch.equal(new[k], v))
    assert moved > 0 and torch.isfinite(info["grad_norm"]) and info["grad_norm"].item() > 0
    # accumulators: none for a fully frozen unit; inside a unit, nothing outside the trainable ranges was written
    assert set(ps.gacc) == {u.name for u in ps.units if u.big and ps.unit_trainable(u)}
    assert any(not ps.unit_trainable(u) for u in ps.units if u.big)
    for name, acc in ps.gacc.items():
        keep = torch.ones(acc.numel(), dtype=torch.bool, device=acc.device)
        for a, b in ps.local_train_ranges(ps.unit_by_name[name]):
            keep[a:b] = False
            assert bool((acc[a:b] != 0).any()), name
        assert bool((acc[keep] == 0).all()), name
    assert any(len(ps.local_train_ranges(ps.unit_by_name[n])) >= 1 and sum(b - a for a, b in ps.local_train_ranges(ps.unit_by_name[n])) < ps.gacc[n].numel()
               for n in ps.gacc)
