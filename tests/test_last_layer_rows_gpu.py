"""The last joint layer's row-subset path (joint_layers.last_layer_rows, LAP_LAST_LAYER_ROWS): in a train step the prefix stream of the last
layer keeps K / V of every row and runs Q, attention, out projection, FFN and their backward on the language head's rows only.

Kernel level: the indexed kernels against float64 references computed here from the same bf16 inputs (tests/train_reference.py
states the rounding points and the element bounds; the indexed forms add no arithmetic, so the bounds are those of the plain
kernels), 2 x 40 rows with 5 kept rows per sample — not contiguous, different per sample — and once with the first and the last
row of a sample.  Attention with the gathered query segment against the same rows of the full-segment call, bit for bit.

Step level: `loss_and_grad` with the switch on and off against the f32 CPU oracle, on identical state and batch.  The model is the
debug model with 2 Gemma layers, B = 2, a 16-token prompt, 8 action tokens, vocabulary 512, loss_rows_max = 5.  Its prefix has
n0 = 2 x 16 image tokens + 16 = 48 rows: the SigLIP grid is square and there are two cameras, so n0 = 40 with a 16-token prompt
does not exist; 48 is the nearest shape (the kernel-level cases run at 2 x 40).
"""
import dataclasses

import pytest
import torch

from oracle import lap_oracle as O
from tests import train_reference as T
from tests.common import debug_model_cfg, make_inputs, oracle_cfg, rel, to_observation

pytestmark = pytest.mark.gpu
DEV = "cuda"

B, N0, N1, NSEL = 2, 40, 8, 5
IDX_SPREAD = torch.tensor([[3, 7, 8, 21, 38], [0, 12, 30, 31, 33]])      # not contiguous, different per sample
IDX_ENDS = torch.tensor([[0, 5, 17, 18, 39], [39, 2, 0, 20, 9]])         # the first and the last row of a sample; not sorted
INDEXES = {"spread": IDX_SPREAD, "ends": IDX_ENDS}


def _maps(idx, n0=N0):
    """(rowid [B * n_sel] rows of the full tensor, inv [B * n0] compact row of a full row or -1), int32 on the CPU."""
    b, n = idx.shape
    rowid = (torch.arange(b)[:, None] * n0 + idx).reshape(-1)
    inv = torch.full((b * n0,), -1, dtype=torch.int32)
    inv[rowid] = torch.arange(b * n, dtype=torch.int32)
    return rowid.to(torch.int32), inv


def _check(what, got, ref):
    r, bound = ref
    got = got.detach().double().cpu().reshape(r.shape)
    if bound is None:
        assert torch.equal(got, r.double()), (what, "not bit for bit")
        return
    ratio = T.worst_ratio(got, r, bound.clamp(min=1e-300))
    print(f"{what}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)


# ------------------------------------------------------------------------------------------------------------ RoPE
# HD 16 / 256 at 80 rows: one thread per (row, head, chunk); 2 x 2048 rows at HD 256: B T HD / 16 = 65536, the per-row form the
# train step's 17,920 rows take (lap_rope_split_fwd's threshold)
ROPE = [("spread", T.RopeCase(16, 8, B, N0, N0 + N1, 0, 0.25)), ("ends", T.RopeCase(16, 8, B, N0, N0 + N1, 0, 0.25)),
        ("spread", T.RopeCase(256, 8, B, N0, N0 + N1, 0, 1.0 / 16)), ("rowform", T.RopeCase(256, 1, 2, 2048, 2048, 0, 1.0 / 16))]


@pytest.mark.parametrize("which,spec", ROPE, ids=lambda v: v if isinstance(v, str) else f"hd{v.HD}x{v.B * v.T_seg}")
def test_rope_split_with_query_rows(hip, which, spec):
    idx = INDEXES[which] if which in INDEXES else torch.tensor([[0, 5, 1031, 2047, 640], [2047, 3, 0, 99, 1500]])
    rowid, inv = _maps(idx, spec.T_seg)
    n = rowid.numel()
    c = dict(T.rope_case(spec))
    ref = T.ref_rope_fwd(c)
    dev = lambda t: t.to(DEV)
    q, k, v = hip.rope_split_fwd(dev(c["qkv"]), dev(c["pos"]), spec.B, spec.T_seg, spec.T_total, spec.seg_off, spec.NH, spec.HD, spec.q_scale,
                                 q_row=dev(inv), q_rows=n)
    assert q.shape == (n, spec.NH * spec.HD)
    sel = rowid.long()
    _check("rope_split_fwd rows q", q, (ref["q"][0][sel], ref["q"][1][sel]))      # compact, in the index's order
    _check("rope_split_fwd rows k", k, ref["k"])                                  # every row
    _check("rope_split_fwd rows v", v, ref["v"])
    # backward: compact dq (the case's first n rows of dq), whole dk / dv -> whole dqkv with zero q columns elsewhere
    dq_c = c["dq"][:n].contiguous()
    full = torch.zeros_like(c["dq"])
    full[sel] = dq_c
    rb, bb = T.ref_rope_bwd(c | {"dq": full})["dqkv"]
    keep = torch.zeros(spec.B * spec.T_seg, dtype=torch.bool)
    keep[sel] = True
    qcols = spec.NH * spec.HD
    bb = bb.clone()
    bb[~keep, :qcols] = 0.0                # exactly zero: no arithmetic happens there
    dqkv = hip.rope_split_bwd(dev(dq_c), dev(c["dk"]), dev(c["dv"]), dev(c["pos"]), spec.B, spec.T_seg, spec.T_total, spec.seg_off, spec.NH,
                              spec.HD, spec.q_scale, q_row=dev(inv))
    got = dqkv.double().cpu()
    assert bool((got[~keep, :qcols] == 0).all()), "q columns of rows without a dq row must be zero"
    assert T.worst_ratio(got[keep], rb[keep], bb[keep].clamp(min=1e-300)) <= 1.0
    assert T.worst_ratio(got[:, qcols:], rb[:, qcols:], bb[:, qcols:].clamp(min=1e-300)) <= 1.0


# ----------------------------------------------------------------------------------------- RMSNorm backward + rows
@pytest.mark.parametrize("which", ["spread", "ends"])
@pytest.mark.parametrize("D", [64, 2048])      # one / four 8-wide chunks per lane (the D = 2048 variant asks for the addend late)
def test_rmsnorm_bwd_with_scattered_residual(hip, D, which):
    rows = B * N0
    rowid, inv = _maps(INDEXES[which])
    n = rowid.numel()
    spec = T.NormCase("rms", D, rows)
    c = dict(T.norm_case(spec))
    addend = c["old"][:n].contiguous()                   # compact
    old = torch.zeros_like(c["old"])
    old[rowid.long()] = addend
    keep = torch.zeros(rows, dtype=torch.bool)
    keep[rowid.long()] = True
    x = c["x"].to(DEV)
    _, rstd = hip.rmsnorm_fwd(x, scale=c["scale"].to(DEV))
    dscale = c["dscale0"].to(DEV).clone()
    dx = hip.rmsnorm_bwd(x, c["dy"].to(DEV), rstd, scale=c["scale"].to(DEV), dscale=dscale, add_row=inv.to(DEV), addend=addend.to(DEV))
    plain, acc = T.ref_rms_bwd(c, rstd.cpu()), T.ref_rms_bwd(c | {"old": old}, rstd.cpu(), accum=True)
    # a row with an addend: norm backward + addend, rounded once; a row without: the plain kernel's value and bound
    r = torch.where(keep[:, None], acc["dx"][0], plain["dx"][0])
    b = torch.where(keep[:, None], acc["dx"][1], plain["dx"][1])
    _check(f"rmsnorm_bwd rows dx D={D}", dx, (r, b))
    _check(f"rmsnorm_bwd rows dscale D={D}", dscale, plain["dscale"])


def test_gather_rows(hip):
    rowid, _ = _maps(IDX_ENDS)
    src = torch.randn(B * N0, 64, generator=T.gen("gather")).bfloat16()
    out = hip.gather_rows_bf16(src.to(DEV), rowid.to(DEV))
    assert torch.equal(out.cpu(), src[rowid.long()])


# -------------------------------------------------------------------------------------------------------- attention
def _attn_inputs(NH, HD):
    g = T.gen("attn", NH, HD)
    rnd = lambda *s: torch.randn(*s, generator=g)
    q0, q1 = (rnd(B * N0, NH * HD) * HD ** -0.5).bfloat16(), (rnd(B * N1, NH * HD) * HD ** -0.5).bfloat16()
    k0, k1, v0, v1 = rnd(B * N0, HD).bfloat16(), rnd(B * N1, HD).bfloat16(), rnd(B * N0, HD).bfloat16(), rnd(B * N1, HD).bfloat16()
    # the train step's info words (LAP._train_infos): image rows block 0, a causal tail over the last 10 prefix rows, two padding
    # rows (class 0) in sample 1; suffix rows see the prefix rows of class bit 2 and each other
    cls_q = torch.ones(B, N0, dtype=torch.int32); cls_k = torch.full((B, N0), 3, dtype=torch.int32)
    ar = torch.zeros(B, N0, dtype=torch.int32)
    ar[:, N0 - 10:] = torch.arange(1, 11, dtype=torch.int32)
    cls_k[:, N0 - 10:] = 1
    cls_q[1, N0 - 2:] = 0; cls_k[1, N0 - 2:] = 0
    sidx = torch.full((B, N1), 0x800001, dtype=torch.int32)
    qinfo = torch.cat([(cls_q << 24) | ar, (6 << 24) | sidx], 1).to(torch.int32).contiguous()
    kinfo = torch.cat([(cls_k << 24) | ar, (4 << 24) | sidx], 1).to(torch.int32).contiguous()
    return [t.to(DEV) for t in (q0, q1, k0, k1, v0, v1, qinfo, kinfo)]


@pytest.mark.parametrize("which", ["spread", "ends"])
@pytest.mark.parametrize("HD", [16, 256])
def test_attention_with_gathered_query_segment(hip, HD, which):
    """HD = 16 runs the generic kernels: every query row's arithmetic depends on that row and the key tiles alone, so the gathered
    rows equal the full call's bit for bit — output, log-sum-exp and dQ.  HD = 256 runs the LDS-DMA kernels, whose forward moves a
    row's running maximum only when SOME row of its 16-row wave outgrows it by 2^8 (attention_dma.hpp: the lazy maximum): P is
    rounded to bf16 at a scale that depends on the row's wave neighbours, which a gather changes.  There the rows are not equal
    bit for bit; o = sum p v / sum p with every p rounded to bf16 (2^-9 relative) in both calls, so they differ by at most
    2 (numerator and denominator) x 2 (two calls) x 2^-9 max|v|, plus one bf16 spacing of the output for its own rounding."""
    NH = 8
    q0, q1, k0, k1, v0, v1, qinfo, kinfo = _attn_inputs(NH, HD)
    idx = INDEXES[which]
    rowid, _ = _maps(idx)
    sel = rowid.long().to(DEV)
    qinfo_c = torch.cat([qinfo[:, :N0].gather(1, idx.to(DEV)), qinfo[:, N0:]], 1).contiguous()
    o, lse = hip.attention_fwd([q0, q1], [k0, k1], [v0, v1], [N0, N1], [N0, N1], B, NH, 1, HD, qinfo, kinfo)
    oc, lsec = hip.attention_fwd([q0[sel].contiguous(), q1], [k0, k1], [v0, v1], [NSEL, N1], [N0, N1], B, NH, 1, HD, qinfo_c, kinfo)
    lse_rows = torch.cat([lse[:, :, :N0].gather(2, idx.to(DEV)[:, None, :].expand(B, NH, NSEL)), lse[:, :, N0:]], 2)
    if HD == 16:
        assert torch.equal(oc[0], o[0][sel]) and torch.equal(oc[1], o[1]) and torch.equal(lsec, lse_rows)
    else:
        for a, b_, vv in ((oc[0], o[0][sel], v0), (oc[1], o[1], v0)):
            a, b_ = a.double().cpu(), b_.double().cpu()
            bound = 4 * 2.0 ** -9 * float(vv.abs().max()) + T.ulp_bf16(b_.abs() + 4 * 2.0 ** -9 * float(vv.abs().max()))
            assert bool(((a - b_).abs() <= bound).all()), float(((a - b_).abs() / bound).max())
        assert torch.allclose(lsec, lse_rows, rtol=0, atol=1e-4)      # m + log l in f32 at |lse| of a few units
    # backward: dO of the rows that are not kept is zero in the full call, which is what the step's full path computes
    g = T.gen("attn-do", HD)
    do_c = torch.randn(B * NSEL, NH * HD, generator=g).bfloat16().to(DEV)
    do1 = torch.randn(B * N1, NH * HD, generator=g).bfloat16().to(DEV)
    do_f = torch.zeros(B * N0, NH * HD, dtype=torch.bfloat16, device=DEV)
    do_f[sel] = do_c
    if HD == 16:
        dq, dk, dv = hip.attention_bwd([q0, q1], [k0, k1], [v0, v1], o, [do_f, do1], lse, [N0, N1], [N0, N1], B, NH, 1, HD, qinfo, kinfo)
        dqc, dkc, dvc = hip.attention_bwd([q0[sel].contiguous(), q1], [k0, k1], [v0, v1], oc, [do_c, do1], lsec, [NSEL, N1], [N0, N1], B, NH, 1, HD,
                                          qinfo_c, kinfo)
        assert torch.equal(dqc[0], dq[0][sel]) and torch.equal(dqc[1], dq[1])
        assert bool((dq[0][~torch.isin(torch.arange(B * N0, device=DEV), sel)] == 0).all())
        for a, b_ in ((dkc[0], dk[0]), (dvc[0], dv[0]), (dkc[1], dk[1]), (dvc[1], dv[1])):
            # the same products summed over the query tiles in another order: f32 sums (2^-24 per addition, < 64 of them) of terms
            # bounded by the largest, then one bf16 rounding each
            a, b_ = a.double().cpu(), b_.double().cpu()
            slack = 64 * 2.0 ** -24 * float(b_.abs().max()) * (N0 + N1)
            assert bool(((a - b_).abs() <= slack + T.ulp_bf16(b_.abs() + slack)).all())
    else:     # the compact call on the LDS-DMA kernels: finite, and dQ has the kept rows' height
        dqc, dkc, dvc = hip.attention_bwd([q0[sel].contiguous(), q1], [k0, k1], [v0, v1], oc, [do_c, do1], lsec, [NSEL, N1], [N0, N1], B, NH, 1, HD,
                                          qinfo_c, kinfo)
        dq, dk, dv = hip.attention_bwd([q0, q1], [k0, k1], [v0, v1], o, [do_f, do1], lse, [N0, N1], [N0, N1], B, NH, 1, HD, qinfo, kinfo)
        for a, b_ in ((dqc[0], dq[0][sel]), (dqc[1], dq[1]), (dkc[0], dk[0]), (dvc[0], dv[0]), (dkc[1], dk[1]), (dvc[1], dv[1])):
            # P and dS are rounded to bf16 once per product in each call (at wave-dependent scales, see above): 2^-9 relative per
            # term, two roundings per call, two calls, against the L2 norm as the gradient-parity tests measure
            assert bool(torch.isfinite(a).all()) and rel(a, b_) < 8 * 2.0 ** -9, rel(a, b_)


# ------------------------------------------------------------------------------------------------------ step level
def _cfg(mp, **kw):
    from lap_amd import config as C

    mp.setitem(C._GEMMA, "dummy_x2", C.GemmaConfig(64, 2, 128, 8, 1, 16))
    mp.setitem(O.GEMMA, "dummy_x2", O.GemmaCfg(64, 2, 128, 8, 1, 16))
    return debug_model_cfg(paligemma_variant="dummy_x2", action_expert_variant="dummy_x2", max_token_len=16, action_horizon=8, **kw)


def _batch(cfg):
    """B = 2; sample 0: 5 loss rows (tokens 10, 11, 13, 14, 15), sample 1: 3 (tokens 6, 8, 11) and two padding rows, three
    padded prompt tokens.  Not contiguous, different per sample."""
    obs, actions, noise, time = make_inputs(cfg, B=2, ragged=True)
    tl = obs["token_loss_mask"]
    tl[0, 12] = False
    tl[1, [7, 9, 10, 12]] = False
    lm = (obs["tokenized_langact_mask"] & obs["tokenized_prompt_mask"] & tl)[:, 1:]
    assert lm.sum(-1).tolist() == [5, 3]
    return obs, actions, noise, time


def _unit_vectors(model, tensors):
    """engine-named tensors -> one flat f32 vector per parameter unit"""
    out = {}
    for name in model.ps.names():
        out.setdefault(model.ps.tensor_unit[name].name, []).append(tensors[name].detach().float().cpu().reshape(-1))
    return {u: torch.cat(v) for u, v in out.items()}


@pytest.fixture(scope="module")
def step():
    """One oracle pass (f32 autograd on the CPU) and the engine's step with the switch off and on, same state and batch."""
    from lap_amd import hip as H
    from lap_amd.model import LAP
    from lap_amd.params import reference_to_engine

    with pytest.MonkeyPatch.context() as mp:
        cfg = _cfg(mp)
        oc = oracle_cfg(cfg)
        P = O.init_params(oc, seed=23)
        obs, actions, noise, time = _batch(cfg)
        Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
        loss32, _ = O.compute_loss(Pg, oc, obs, actions, noise, time)
        loss32.backward()
        loss16, _ = O.compute_loss(P, dataclasses.replace(oc, emulate_bf16=True), obs, actions, noise, time)
        model = LAP(cfg, params=P, device=DEV)
        want = _unit_vectors(model, reference_to_engine(cfg, {k: v.grad for k, v in Pg.items()}))
        ob = dataclasses.replace(to_observation(obs, DEV), loss_rows_max=5)
        runs = {}
        n0 = model.n_img_tok * len(cfg.image_keys) + cfg.max_token_len
        for on in (False, True):
            model.last_layer_rows = on
            for g in model.ps.grad.values():
                g.zero_()
            seen = []
            orig = H.rope_split_bwd

            def spy(dq, dk, dv, pos, B_, T_seg, *a, **k):
                out = orig(dq, dk, dv, pos, B_, T_seg, *a, **k)
                if T_seg == n0:
                    seen.append(out.clone())
                return out
            mp.setattr(H, "rope_split_bwd", spy)
            before = model.last_rows_steps
            loss, _ = model.loss_and_grad(0, ob, actions.to(DEV), noise=noise.to(DEV), time=time.to(DEV))
            torch.cuda.synchronize()
            mp.setattr(H, "rope_split_bwd", orig)
            runs[on] = dict(loss=loss.item(), grads=_unit_vectors(model, {n: model.ps.g(n) for n in model.ps.names()}), dqkv_last=seen[0],
                            took=model.last_rows_steps - before)
        model.last_layer_rows = True
        lm = (obs["tokenized_langact_mask"] & obs["tokenized_prompt_mask"] & obs["token_loss_mask"])[:, 1:]
        yield dict(cfg=cfg, model=model, ob=ob, obs=obs, actions=actions, noise=noise, time=time, want=want, runs=runs, loss32=loss32.item(),
                   loss16=loss16.item(), n0=n0, lm=lm)


def test_step_values_against_oracle(step):
    """Loss and every parameter unit's gradient, switch on against switch off, each measured against the f32 oracle in the relative
    L2 norm of the gradient-parity tests.  The two paths are not bit-equal (M = B n_sel sends the last layer's products through
    other tiles and K splits), so the new path's deviation must be at most 1.5 x the old path's per unit: another summation
    order at equal precision.  Measured pairs: docs/EXPERIMENTS.md, section P."""
    runs, want = step["runs"], step["want"]
    assert runs[False]["took"] == 0 and runs[True]["took"] == 1
    l32 = step["loss32"]
    d_off, d_on = abs(runs[False]["loss"] - l32) / abs(l32), abs(runs[True]["loss"] - l32) / abs(l32)
    print(f"loss: oracle f32 {l32:.7f} bf16 {step['loss16']:.7f} | off {runs[False]['loss']:.7f} ({d_off:.2e}) on {runs[True]['loss']:.7f} ({d_on:.2e})")
    for u in sorted(want):
        off, on = rel(runs[False]["grads"][u], want[u]), rel(runs[True]["grads"][u], want[u])
        print(f"unit {u}: deviation from the oracle  off {off:.3e}  on {on:.3e}  ratio {on / max(off, 1e-30):.3f}")
    assert d_on <= 1.5 * d_off or abs(runs[True]["loss"] - runs[False]["loss"]) <= 2.0 ** -23 * abs(l32), (d_on, d_off)   # (one f32 spacing)
    for u in sorted(want):
        off, on = rel(runs[False]["grads"][u], want[u]), rel(runs[True]["grads"][u], want[u])
        assert on <= 1.5 * off, (u, on, off)


def test_step_dqkv_of_skipped_rows(step):
    """d(qkv) of the last layer: the Q columns of the rows that are not kept are exactly zero on the new path (the old path computes
    them: zeros too, since nothing reads those rows), dQ of the kept rows and dK / dV of every row equal the old path's up to the
    rounding of the cotangents in front of them.  Between d(x0) at the head and dK / dV lie four bf16 rounding points that the
    M = B n_sel routes may place differently (d(xa), dO, dS inside the attention backward, the store): 4 x 2^-9 in the L2 norm."""
    cfg, model, n0, lm = step["cfg"], step["model"], step["n0"], step["lm"]
    new, old = step["runs"][True]["dqkv_last"].float().cpu(), step["runs"][False]["dqkv_last"].float().cpu()
    qcols = model.v.num_heads * model.v.head_dim
    sel = torch.sort((~lm).to(torch.uint8), dim=1, stable=True).indices[:, :5] + (n0 - cfg.max_token_len)
    keep = torch.zeros(2 * n0, dtype=torch.bool)
    keep[(torch.arange(2)[:, None] * n0 + sel).reshape(-1)] = True
    assert int(keep.sum()) == 10
    assert bool((new[~keep, :qcols] == 0).all())
    assert bool((old[~keep, :qcols] == 0).all())
    assert float(old[:, qcols:].abs().max()) > 0 and float(old[keep, :qcols].abs().max()) > 0
    for what, a, b in (("dK|dV", new[:, qcols:], old[:, qcols:]), ("dQ kept", new[keep, :qcols], old[keep, :qcols])):
        print(f"{what}: new against old {rel(a, b):.3e}")
        assert rel(a, b) <= 4 * 2.0 ** -9, (what, rel(a, b))


def test_fallbacks_keep_every_row(step, monkeypatch):
    """collect, LoRA, no row hint, eval and serving run the old path: the counter of row-subset passes does not move."""
    from lap_amd import config as C
    from lap_amd.model import LAP

    model, ob = step["model"], step["ob"]
    a, nz, tm = step["actions"].to(DEV), step["noise"].to(DEV), step["time"].to(DEV)
    assert model.last_layer_rows

    def moved(fn):
        before = model.last_rows_steps
        fn()
        torch.cuda.synchronize()
        return model.last_rows_steps - before
    assert moved(lambda: model.loss_and_grad(0, ob, a, noise=nz, time=tm)) == 1
    col = {}
    assert moved(lambda: model.loss_and_grad(0, ob, a, noise=nz, time=tm, collect=col)) == 0
    assert col["x0_out"].shape[0] == 2 * step["n0"]          # full height for whoever reads it
    assert moved(lambda: model.loss_and_grad(0, dataclasses.replace(ob, loss_rows_max=None), a, noise=nz, time=tm)) == 0
    assert moved(lambda: model.compute_loss(0, ob, a, train=False, noise=nz, time=tm)) == 0
    assert moved(lambda: model.sample_actions(0, dataclasses.replace(ob, tokenized_langact_mask=None), num_steps=2)) == 0
    monkeypatch.setitem(C._GEMMA, "dummy_lora", dataclasses.replace(C._GEMMA["dummy_lora"], depth=2))
    lcfg = dataclasses.replace(step["cfg"], paligemma_variant="dummy_lora", action_expert_variant="dummy_lora")
    lora = LAP(lcfg, seed=3, device=DEV)
    before = lora.last_rows_steps
    lora.loss_and_grad(0, ob, a, noise=nz, time=tm)
    torch.cuda.synchronize()
    assert lora.last_rows_steps == before
