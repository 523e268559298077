"""Batch-1 LAP_AR token decoding of LAP-3B on one MI355X: eager, fused (csrc/decode.hip issued from Python) and graph-replayed
(GraphedTokenDecoder) ms per token, prefill ms, graphed-vs-eager token agreement, algorithmic bytes per token and the achieved
rate against the 6.29 TB/s measured copy rate.  Random weights, the reference prompt shape, greedy, EOS disabled so that every
run decodes N tokens.  One JSON line.

    python tools/bench_ar.py [--tokens 64] [--config lap_bench] [--kwaves 4] [--temperature T] [--weights bf16 fp8 fp8_layers]
                             [--allowed N] [--logprobs] [--num-samples N] [--speculate S [S ...]] [--grammar verbose]
                             [--jump-forward S [S ...]]

--temperature T > 0 adds the sampled figures: the eager loop with the torch-generator noise (sampler="host"), the eager loop and
the fused steps with the device noise (sampler="device"), and a GraphedTokenDecoder(sampling=True) called sampled and greedy.
--profile-graphed --temperature T replays one sampled decode on the sampling graphs instead of the greedy one.
--weights: the bf16 figures are always measured; every other value named (fp8, fp8_layers: `sample_tokens(decode_weights=)`) adds,
side by side and in the same process, its fused and graphed ms per token, its bytes per token and achieved rate, how many of the
graphed tokens agree with the bf16 graph's, and the relative error of its first and second tokens' logits against bf16's.
--profile-graphed replays the graph of the LAST value named.
--allowed N adds constrained decoding (`allowed_tokens=` the N lowest ids; EOS stays disabled, so the set need not hold it): for
bf16 and every --weights value, in the same process, the graphed ms per token without and with the set (the mean and the
[min, max] of the timed repeats, which is the run-to-run spread to read the difference against), the bytes per token with the
set and whether every constrained token lies in it.  --profile-graphed --allowed N replays the constrained graph.
--logprobs adds the greedy decode with `return_logprobs=True` (the LM head that also leaves the log-sum-exp partials): fused and
graphed ms per token, next to the plain figures of the same process.
--top-k K / --top-p P (with --temperature T > 0) add filtered sampled decoding (`top_k=`, `top_p=`): eager, fused and graphed
(GraphedTokenDecoder(filtering=True)) ms per token, the same graphs called with neutral words, and the ratio to the unfiltered
sampling graph.
--num-samples N adds best-of-N (`num_samples=N`, sampled at --temperature or at 1.0): fused and graphed ms per token of the N
rows, next to one sampled row with log-probabilities on the same kernels, and both prefill graphs (the N-row one ends with the copies).
The fused best-of-N figure subtracts the plain batch-1 prefill, so the copies to N rows and the allocation of the N-row context are
spread into its ms per token; the graphed figures subtract their own prefill graph and are the ones to quote.
--num-beams N [N ...] adds beam search (`num_beams=N`) beside `num_samples=N` at the same N: both graphed, in this process, taking
turns; ms per step of each (mean and [min, max]) after their own prefill graphs, their ratio, the device time of the three beam
launches on their own (events round single launches; the reorder at half the budget with every row moving), and how many steps of
a decode had a non-identity reorder.
--score S [S ...] adds teacher-forced scoring (`LAP.score_tokens(rows=S)`) of the bf16 graph's own answer for bf16 and every
--weights value: ms per scored token and per step next to the plain decode lines of the same process, and the answer's total
log-probability under each weight format.
--speculate S [S ...] adds exact speculative decoding (`speculate=S`) for bf16 and every --weights value, in the same process as
the plain graph of those weights: a GraphedTokenDecoder(speculate=S) called with the answer itself as the draft (full acceptance)
and without a draft (zero acceptance, the price of a wrong guess), each as the mean and [min, max] of the timed repeats; ms per
verify step, ms per token, whether the tokens equal the plain graph's, and the break-even the two imply: the mean tokens per
verify step, and the share of the S - 1 drafts that must be accepted, at which a speculating decode costs what the plain one does.
--grammar verbose adds grammar-constrained decoding (`grammar=`) with the automaton of the verbose-with-rotation format, graphed at
B = 1: ms per token with the automaton and ms per token of `allowed_tokens=` over the same union set, from this process (the two
decoders take turns; each figure is the mean and [min, max] of at least seven timed repeats), Q, E and the size of the union, and
the time per launch of what differs between the two steps (the SUBSET head without and with the logits store, lap_decode_finish
and lap_decode_grammar_finish, each from a captured graph of back-to-back launches).  No tokenizer model is needed: a word is encoded as a
head piece and single-character pieces with ids in order of first use, which gives the automaton the shape a real tokenizer gives
it.  The automaton needs a real EOS id (the model's is set to 1 for this part), so after "gripper" the sentence may start again and a
row ends only when it draws EOS there; the grammar figure is per token actually decoded, which the result reports.
--grammar verbose together with --num-beams N [N ...] adds grammar-constrained beam search (`num_beams=N` + `grammar=`) on the same
automaton, beside the plain beam search and `grammar=` with `num_samples=N` at the same N: the three graphed decoders take turns
in this process; ms per step actually decoded of each (mean and [min, max] of at least seven repeats), the steps each decoded,
the device time of lap_decode_beam_grammar_topn (every row in the state with the most edges) and lap_decode_beam_grammar_select
on their own, and whether every finished beam is a sentence of the automaton.
--jump-forward S [S ...] (with --grammar verbose) adds jump-forward grammar decoding (`grammar=` + `jump_forward=S`), graphed at B = 1
on the automaton of the same synthetic word graph WITHOUT the restart after "gripper", so the greedy answer is one sentence that
ends in its EOS: ms per answer (the call minus the prefill graph) of `grammar=` alone and of every S, without a reference (only
the tokens the grammar forces ride along) and with the answer itself as the reference (every step is full), each as the mean and
[min, max] of the timed repeats with the decoders taking turns; the steps and accepted drafts (`last_stats`), whether tokens and
log-probabilities equal the plain grammar graph's, and the cost of one S-row step relative to one single-row step.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from lap_amd import hip
from lap_amd.config import get_config
from lap_amd.model import LAP
from lap_amd.serve import GraphedTokenDecoder

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="lap_bench")
ap.add_argument("--tokens", type=int, default=64)
ap.add_argument("--kwaves", type=int, default=hip.DECODE_KWAVES_DOWN, help="K split of the down projection (1 or 4)")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--profile-graphed", action="store_true", help="capture, replay one graphed decode and exit (for rocprofv3)")
ap.add_argument("--temperature", type=float, default=0.0, help="> 0: also measure sampled decoding at this temperature")
ap.add_argument("--weights", nargs="+", default=["bf16"], choices=list(LAP.DECODE_WEIGHTS),
                help="decode weights to measure next to bf16 (fp8, fp8_layers)")
ap.add_argument("--allowed", type=int, default=0, help="> 0: also measure constrained decoding over the N lowest token ids")
ap.add_argument("--logprobs", action="store_true", help="also measure greedy decoding that returns token log-probabilities")
ap.add_argument("--num-samples", type=int, default=0, help="N > 0: also measure best-of-N (N rows from one batch-1 prefill); "
                "sampled at --temperature, or at 1.0 when that is 0")
ap.add_argument("--num-beams", type=int, nargs="+", default=[], help="also measure beam search (num_beams=N) beside best-of-N at the same N")
ap.add_argument("--top-k", type=int, default=0, help="with --temperature: also measure filtered sampled decoding (top_k)")
ap.add_argument("--top-p", type=float, default=1.0, help="with --temperature: also measure filtered sampled decoding (top_p)")
ap.add_argument("--grammar", choices=["verbose"], default=None, help="also measure grammar-constrained decoding (verbose-with-rotation)")
ap.add_argument("--jump-forward", type=int, nargs="+", default=[], help="with --grammar: also measure grammar + jump_forward at these step widths")
ap.add_argument("--speculate", type=int, nargs="+", default=[], help="also measure exact speculative decoding at these verify-step widths")
ap.add_argument("--score", type=int, nargs="+", default=[], help="also measure teacher-forced scoring (score_tokens) at these rows per step")
a = ap.parse_args()
if a.jump_forward and not a.grammar:
    ap.error("--jump-forward needs --grammar")
hip.DECODE_KWAVES_DOWN = a.kwaves

cfg = get_config(a.config).model
dev = "cuda"
model = LAP(cfg, seed=0, device=dev, with_grads=False)
model.EOS_TOKEN = -1
N = a.tokens
dec = GraphedTokenDecoder(model, 1, N)
gen = torch.Generator(device="cpu").manual_seed(0)
for k in dec.obs.images:
    dec.obs.images[k].copy_(torch.rand(dec.obs.images[k].shape, generator=gen) * 2 - 1)
dec.obs.tokenized_prompt.copy_(torch.randint(0, cfg.vocab_size, dec.obs.tokenized_prompt.shape, generator=gen, dtype=torch.int32))
o = dec.obs


def timeit(fn, n):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


T = a.temperature
allowed = list(range(a.allowed)) if a.allowed > 0 else None
if a.profile_graphed:
    if T > 0.0:
        filtered = a.top_k > 0 or a.top_p < 1.0
        sdec = GraphedTokenDecoder(model, 1, N, sampling=True, weights=a.weights[-1], allowed_tokens=allowed, filtering=filtered)
        sdec(o, temperature=T, seed=1, **({"top_k": a.top_k or None, "top_p": a.top_p if a.top_p < 1.0 else None} if filtered else {}))
    elif a.weights[-1] != "bf16" or allowed is not None:
        GraphedTokenDecoder(model, 1, N, weights=a.weights[-1], allowed_tokens=allowed)(o)
    else:
        dec(o)
    torch.cuda.synchronize()
    sys.exit(0)
t_pre = timeit(lambda: model.sample_tokens(0, o, max_decoding_steps=1), a.reps)            # prefill + first token
t_eager = timeit(lambda: model.sample_tokens(0, o, max_decoding_steps=N), a.reps)
t_fused = timeit(lambda: model.sample_tokens(0, o, max_decoding_steps=N, decode="fused"), a.reps)
eager = model.sample_tokens(0, o, max_decoding_steps=N)
dec.capture()
t_gpre = timeit(lambda: (dec.g_prefill.replay()), a.reps)
t_graph = timeit(lambda: dec(o), a.reps)
got = dec(o)
agree = int((got == eager).cumprod(1).sum())          # leading tokens that agree

v = model.v
layer = sum(model.W(f"llm/0/{n}").numel() for n in ("wqkv0", "wo0", "wgu0", "wd0")) * 2
head = model.W("llm/embed").numel() * 2 * (2 if model.ps.w16lo("llm/embed") is not None else 1)
bytes_tok = v.depth * layer + head
per = lambda t, t0: (t - t0) / (N - 1)
g_ms = per(t_graph, t_gpre)
quant = {}
for wname in dict.fromkeys(w for w in a.weights if w != "bf16"):
    qdec = GraphedTokenDecoder(model, 1, N, weights=wname).capture()
    t_qpre = timeit(lambda: (qdec.g_prefill.replay()), a.reps)
    t_qgraph = timeit(lambda: qdec(o), a.reps)
    t_qfused = timeit(lambda: model.sample_tokens(0, o, max_decoding_steps=N, decode="fused", decode_weights=wname), a.reps)
    qgot = qdec(o)
    c16, c8 = {}, {}
    model.sample_tokens(0, o, max_decoding_steps=2, decode="fused", collect=c16)
    model.sample_tokens(0, o, max_decoding_steps=2, decode="fused", decode_weights=wname, collect=c8)
    q_bytes = v.depth * layer // 2 + (head // 4 if wname == "fp8" else head)
    q_ms = per(t_qgraph, t_qpre)
    quant[wname] = {
        "fused_ms_per_token": round(per(t_qfused, t_pre), 3), "graphed_ms_per_token": round(q_ms, 3),
        "graphed_speedup_vs_bf16": round(g_ms / q_ms, 3), "algorithmic_bytes_per_token": q_bytes,
        "achieved_GBps_graphed": round(q_bytes / (q_ms * 1e-3) / 1e9, 1), "share_of_6.29TBps": round(q_bytes / (q_ms * 1e-3) / 6.29e12, 3),
        "tokens_equal_to_bf16_graph": int((qgot == got).sum()), "leading_tokens_equal_to_bf16_graph": int((qgot == got).cumprod(1).sum()),
        "first_token_logit_rel_err_vs_bf16": round(float((c8["logit/0"] - c16["logit/0"]).norm() / c16["logit/0"].norm()), 5),
        "second_token_logit_rel_err_vs_bf16": round(float((c8["logit/1"] - c16["logit/1"]).norm() / c16["logit/1"].norm()), 5)}
constrained = {}
if allowed is not None:
    def per_token(d):
        """mean and [min, max] over the timed repeats of the graphed ms per token of decoder `d`"""
        d.capture()
        t0 = timeit(lambda: (d.g_prefill.replay()), a.reps)
        ms = [per(timeit(lambda: d(o), 1), t0) for _ in range(max(a.reps, 3))]
        return round(sum(ms) / len(ms), 3), [round(min(ms), 3), round(max(ms), 3)]

    row = 2 * v.width
    for wname in dict.fromkeys(["bf16", *a.weights]):
        free_ms, free_spread = per_token(GraphedTokenDecoder(model, 1, N, weights=wname))
        cdec = GraphedTokenDecoder(model, 1, N, weights=wname, allowed_tokens=allowed)
        c_ms, c_spread = per_token(cdec)
        cgot = cdec(o)
        f8_head = wname == "fp8"
        layers = v.depth * layer // (1 if wname == "bf16" else 2)
        c_head = a.allowed * (row // 2 if f8_head else row * (2 if model.ps.w16lo("llm/embed") is not None else 1))
        constrained[wname] = {
            "graphed_ms_per_token": free_ms, "graphed_ms_per_token_min_max": free_spread,
            "constrained_graphed_ms_per_token": c_ms, "constrained_graphed_ms_per_token_min_max": c_spread,
            "constrained_speedup": round(free_ms / c_ms, 3),
            "algorithmic_bytes_per_token": layers + (head // 4 if f8_head else head),
            "constrained_algorithmic_bytes_per_token": layers + c_head,
            "constrained_tokens_inside_the_set": bool((cgot < a.allowed).all()),
            "constrained_equals_fused_constrained": bool(torch.equal(cgot, model.sample_tokens(
                0, o, max_decoding_steps=N, decode="fused", decode_weights=wname, allowed_tokens=allowed)))}
sampled = {}
if T > 0.0:
    st = lambda **kw: (lambda: model.sample_tokens(1, o, max_decoding_steps=N, temperature=T, **kw))
    t_host = timeit(st(), a.reps)
    t_edev = timeit(st(sampler="device"), a.reps)
    t_fdev = timeit(st(sampler="device", decode="fused"), a.reps)
    sdec = GraphedTokenDecoder(model, 1, N, sampling=True).capture()
    t_spre = timeit(lambda: (sdec.g_prefill.replay()), a.reps)
    t_sgraph = timeit(lambda: sdec(o, temperature=T, seed=1), a.reps)
    t_sgreedy = timeit(lambda: sdec(o), a.reps)
    sgot = sdec(o, temperature=T, seed=1)
    sampled = {
        "temperature": T,
        "eager_host_sampled_ms_per_token": round(per(t_host, t_pre), 3),
        "eager_device_sampled_ms_per_token": round(per(t_edev, t_pre), 3),
        "fused_sampled_ms_per_token": round(per(t_fdev, t_pre), 3),
        "graphed_sampled_ms_per_token": round(per(t_sgraph, t_spre), 3),
        "graphed_greedy_on_sampling_graph_ms_per_token": round(per(t_sgreedy, t_spre), 3),
        "graphed_sampled_equals_fused_sampled": bool(torch.equal(sgot, st(sampler="device", decode="fused")())),
        "greedy_on_sampling_graph_equals_graphed": bool(torch.equal(sdec(o), got))}
    if a.top_k > 0 or a.top_p < 1.0:        # the same sampled decode through the filter kernel (one more launch per token)
        fkw = {"top_k": a.top_k or None, "top_p": a.top_p if a.top_p < 1.0 else None}
        t_fe = timeit(st(sampler="device", **fkw), a.reps)
        t_ff = timeit(st(sampler="device", decode="fused", **fkw), a.reps)
        fdec = GraphedTokenDecoder(model, 1, N, sampling=True, filtering=True).capture()
        t_fpre = timeit(lambda: (fdec.g_prefill.replay()), a.reps)
        t_fgraph = timeit(lambda: fdec(o, temperature=T, seed=1, **fkw), a.reps)
        t_fneutral = timeit(lambda: fdec(o, temperature=T, seed=1), a.reps)
        sampled["filtered"] = {
            "top_k": a.top_k, "top_p": a.top_p,
            "eager_ms_per_token": round(per(t_fe, t_pre), 3), "fused_ms_per_token": round(per(t_ff, t_pre), 3),
            "graphed_ms_per_token": round(per(t_fgraph, t_fpre), 3),
            "graphed_neutral_words_ms_per_token": round(per(t_fneutral, t_fpre), 3),
            "graphed_ms_per_token_over_unfiltered": round(per(t_fgraph, t_fpre) / per(t_sgraph, t_spre), 4),
            "graphed_equals_fused": bool(torch.equal(fdec(o, temperature=T, seed=1, **fkw), st(sampler="device", decode="fused", **fkw)())),
            "neutral_words_equal_unfiltered_graph": bool(torch.equal(fdec(o, temperature=T, seed=1), sgot))}
logprobs = {}
if a.logprobs:          # the same greedy decode with return_logprobs=True: what the log-sum-exp in the LM head and the finish cost
    t_lfused = timeit(lambda: model.sample_tokens(0, o, max_decoding_steps=N, decode="fused", return_logprobs=True), a.reps)
    ldec = GraphedTokenDecoder(model, 1, N, logprobs=True).capture()
    t_lpre = timeit(lambda: (ldec.g_prefill.replay()), a.reps)
    t_lgraph = timeit(lambda: ldec(o), a.reps)
    ltok, llp = ldec(o)
    logprobs = {"logprobs": {
        "fused_ms_per_token": round(per(t_lfused, t_pre), 3), "graphed_ms_per_token": round(per(t_lgraph, t_lpre), 3),
        "graphed_ms_per_token_over_plain": round(per(t_lgraph, t_lpre) / g_ms, 4),
        "tokens_equal_to_plain_graph": bool(torch.equal(ltok, got)), "mean_token_logprob": round(float(llp.mean()), 4)}}
best_of = {}
if a.num_samples > 0:   # N rows from one batch-1 prefill against one sampled row on the same kernels (both return log-probabilities)
    Tn = T if T > 0.0 else 1.0
    skw = dict(max_decoding_steps=N, temperature=Tn, sampler="device", decode="fused")
    t_one = timeit(lambda: model.sample_tokens(1, o, return_logprobs=True, **skw), a.reps)
    t_n = timeit(lambda: model.sample_tokens(1, o, num_samples=a.num_samples, **skw), a.reps)
    one = GraphedTokenDecoder(model, 1, N, sampling=True, logprobs=True).capture()
    ndec = GraphedTokenDecoder(model, 1, N, sampling=True, num_samples=a.num_samples).capture()
    t_1pre, t_npre = (timeit(lambda d=d: (d.g_prefill.replay()), a.reps) for d in (one, ndec))
    t_1graph = timeit(lambda: one(o, temperature=Tn, seed=1), a.reps)
    t_ngraph = timeit(lambda: ndec(o, temperature=Tn, seed=1), a.reps)
    ntok, _ = ndec(o, temperature=Tn, seed=1)
    best_of = {"best_of": {
        "num_samples": a.num_samples, "temperature": Tn,
        "one_row_fused_ms_per_token": round(per(t_one, t_pre), 3), "fused_ms_per_token": round(per(t_n, t_pre), 3),
        "one_row_graphed_ms_per_token": round(per(t_1graph, t_1pre), 3), "graphed_ms_per_token": round(per(t_ngraph, t_npre), 3),
        "graphed_ms_per_token_over_one_row": round(per(t_ngraph, t_npre) / per(t_1graph, t_1pre), 4),
        "one_row_graphed_prefill_ms": round(t_1pre, 3), "graphed_prefill_ms": round(t_npre, 3),
        "distinct_rows": len({tuple(r) for r in ntok.tolist()})}}
beams = {}
if a.num_beams:     # the beam step against the num_samples=N step at equal batch width: graphed, one process, the decoders taking turns
    def launch_us(fn, reset, n=50):
        """Median device time of one launch of `fn` (events round it), `reset` before each; microseconds."""
        ts = []
        for _ in range(n + 5):
            reset()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return round(sorted(ts[5:])[n // 2], 2)

    one_launch_us = launch_us       # (the grammar part below reuses the name for its own table)
    for NB in a.num_beams:
        bdec = GraphedTokenDecoder(model, 1, N, num_beams=NB, logprobs=True).capture()
        ndec = GraphedTokenDecoder(model, 1, N, sampling=True, num_samples=NB).capture()
        runs = {"beam": [], "best_of": []}
        pre = {"beam": timeit(lambda: bdec.g_prefill.replay(), a.reps), "best_of": timeit(lambda: ndec.g_prefill.replay(), a.reps)}
        for _ in range(max(a.reps, 3)):     # in turns, so that drift hits both alike
            runs["beam"].append(per(timeit(lambda: bdec(o), 1), pre["beam"]))
            runs["best_of"].append(per(timeit(lambda: ndec(o, temperature=1.0, seed=1), 1), pre["best_of"]))
        bdec(o)
        reorders = bdec.ctx.beam_reorders()
        ctx = bdec.ctx
        st, bw = ctx.state.clone(), ctx.beam.clone()
        st0, bw0 = ctx.state.clone(), ctx.beam_init.clone()
        st0[0], st0[1] = N // 2, 0                                  # mid decode, not done
        bw0[:NB] = torch.linspace(0, -1, NB).view(torch.int32) if NB > 1 else bw0[:NB]
        bw0[16:16 + NB] = torch.roll(torch.arange(NB, dtype=torch.int32), 1)     # every row moves

        def reset():
            st.copy_(st0); bw.copy_(bw0)

        out, lp = ctx.out.clone(), ctx.logp.clone()
        mean = lambda xs: sum(xs) / len(xs)
        beams[f"N{NB}"] = {
            "beam_ms_per_step": round(mean(runs["beam"]), 4), "beam_ms_per_step_min_max": [round(min(runs["beam"]), 4), round(max(runs["beam"]), 4)],
            "num_samples_ms_per_step": round(mean(runs["best_of"]), 4),
            "num_samples_ms_per_step_min_max": [round(min(runs["best_of"]), 4), round(max(runs["best_of"]), 4)],
            "beam_over_num_samples": round(mean(runs["beam"]) / mean(runs["best_of"]), 4),
            "beam_prefill_ms": round(pre["beam"], 3), "num_samples_prefill_ms": round(pre["best_of"], 3),
            "topn_us": launch_us(lambda: hip.decode_beam_topn(st, bw, ctx.logits, ctx.cand_logp, ctx.cand_id, N), reset),
            "select_us": launch_us(lambda: hip.decode_beam_select(st, bw, ctx.cand_logp, ctx.cand_id, out, lp, cfg.vocab_size, -1), reset),
            "reorder_us_at_half_budget_every_row_moving": launch_us(lambda: hip.decode_beam_reorder(st, bw, ctx.gen), reset),
            "steps": N, "steps_with_a_non_identity_reorder": reorders}
        del bdec, ndec
speculative = {}
if a.speculate:
    def spread(fn):
        ms = [timeit(fn, 1) for _ in range(max(a.reps, 3))]
        return sum(ms) / len(ms), [round(min(ms), 3), round(max(ms), 3)]

    for wname in dict.fromkeys(["bf16", *a.weights]):
        pdec = GraphedTokenDecoder(model, 1, N, weights=wname).capture()
        t_ppre = timeit(lambda: (pdec.g_prefill.replay()), a.reps)
        t_plain, plain_mm = spread(lambda: pdec(o))
        answer = pdec(o)
        draft = answer[0].tolist()
        plain_ms = per(t_plain, t_ppre)
        rows = {"plain_graphed_ms_per_token": round(plain_ms, 3),
                "plain_graphed_ms_per_token_min_max": [round(per(x, t_ppre), 3) for x in plain_mm]}
        for S in a.speculate:
            sd = GraphedTokenDecoder(model, 1, N, weights=wname, speculate=S).capture()
            t_spre = timeit(lambda: (sd.g_prefill.replay()), a.reps)
            t_full, full_mm = spread(lambda: sd(o, draft_tokens=draft))
            full_tok, full_stats = sd(o, draft_tokens=draft), sd.last_stats
            t_zero, zero_mm = spread(lambda: sd(o))
            zero_tok, zero_stats = sd(o), sd.last_stats
            step_ms = (t_zero - t_spre) / zero_stats[0]       # (every verify step of a decode without a draft emits one token)
            rows[f"S{S}"] = {
                "verify_step_ms": round(step_ms, 3), "verify_step_ms_at_full_acceptance": round((t_full - t_spre) / full_stats[0], 3),
                "full_acceptance_ms_per_token": round(per(t_full, t_spre), 3),
                "full_acceptance_ms_per_token_min_max": [round(per(x, t_spre), 3) for x in full_mm],
                "zero_acceptance_ms_per_token": round(per(t_zero, t_spre), 3),
                "zero_acceptance_ms_per_token_min_max": [round(per(x, t_spre), 3) for x in zero_mm],
                "full_acceptance_verify_steps_accepted": list(full_stats), "zero_acceptance_verify_steps_accepted": list(zero_stats),
                "speedup_at_full_acceptance": round(plain_ms / per(t_full, t_spre), 3),
                "break_even_tokens_per_verify_step": round(step_ms / plain_ms, 3),
                "break_even_draft_acceptance_rate": round((step_ms / plain_ms - 1) / (S - 1), 3),
                "tokens_equal_plain_graph": bool(torch.equal(full_tok, answer) and torch.equal(zero_tok, answer))}
        speculative[wname] = rows
scoring = {}
if a.score:
    # the candidate is the bf16 graph's own answer (--tokens ids); score_tokens launches its steps eagerly, so the line to compare
    # with is the eagerly launched fused decode of this process (fused_ms_per_token), with the graphed one beside it
    cand = got[0].tolist()
    for wname in dict.fromkeys(["bf16", *a.weights]):
        t_wfused = t_fused if wname == "bf16" else timeit(
            lambda: model.sample_tokens(0, o, max_decoding_steps=N, decode="fused", decode_weights=wname), a.reps)
        rows = {"fused_ms_per_token": round(per(t_wfused, t_pre), 3), "graphed_ms_per_token_bf16": round(g_ms, 3)}
        for S in a.score:
            sc = lambda: model.score_tokens(o, cand, rows=S, decode_weights=wname, max_decoding_steps=N)
            ms = [timeit(sc, 1) for _ in range(max(a.reps, 3))]
            t_sc = sum(ms) / len(ms)
            steps = (N - 1 + S - 1) // S
            res = sc()
            rows[f"S{S}"] = {
                "ms_per_scored_token": round(per(t_sc, t_pre), 3),
                "ms_per_scored_token_min_max": [round(per(min(ms), t_pre), 3), round(per(max(ms), t_pre), 3)],
                "step_ms": round((t_sc - t_pre) / steps, 3), "steps": steps, "total_ms": round(t_sc, 3),
                "speedup_vs_fused_decode": round(per(t_wfused, t_pre) / per(t_sc, t_pre), 3),
                "total_logp": round(float(res.total[0]), 4),
                "token_accuracy": round(float((res.greedy[0] == got[0]).float().mean()), 4)}
        scoring[wname] = rows
grammar_res = {}
if a.grammar:
    from lap_amd import grammar as G, lang_actions as LA

    pieces = {}
    encode = lambda w: [pieces.setdefault(p, 2 + len(pieces)) for p in ["\u2581" + w[0], *w[1:]]]
    wg = LA.word_graph(LA.VERBOSE_WITH_ROTATION_FORMAT)
    wg = G.WordGraph(wg.edges | {"end": wg.edges[wg.start]}, wg.start, wg.accepting)        # after "gripper": EOS, or the next sentence
    model.EOS_TOKEN = 1
    auto = G.automaton_from_words(encode, wg, 1, cfg.vocab_size)

    gdec = GraphedTokenDecoder(model, 1, N, grammar=auto).capture()
    adec = GraphedTokenDecoder(model, 1, N, allowed_tokens=auto.union()).capture()
    pre = {d: timeit(lambda d=d: (d.g_prefill.replay()), a.reps) for d in (gdec, adec)}
    runs = {gdec: [], adec: []}
    for _ in range(max(a.reps, 7)):         # the two decoders take turns, so that a drift of the machine reaches both
        for d in (gdec, adec):
            t = timeit(lambda: d(o), 1)
            runs[d].append((t - pre[d]) / max(int(d.ctx.state[0]) - 1, 1))
    res = lambda d: (round(sum(runs[d]) / len(runs[d]), 3), [round(min(runs[d]), 3), round(max(runs[d]), 3)], int(d.ctx.state[0]))
    g_res, a_res = res(gdec), res(adec)
    gtok = gdec(o)

    # the two launches a grammar step has in place of the allowed step's: the SUBSET head with and without the logits store, and
    # the two finishes, each as a captured graph of n launches on the grammar context's buffers (EOS disabled in these launches)
    ctx, dg, n_l = gdec.ctx, gdec.grammar, min(56, N - 2)

    def launches(fn):
        with model._serving_weights():
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fn()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(n_l):
                    fn()
        us = []
        for _ in range(6):
            ctx.state[:3] = torch.tensor([1, 0, 0], dtype=torch.int32, device=dev)
            ctx.gstate.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) / n_l * 1e3)
        return round(sum(us[1:]) / 5, 2)

    gamma, hi, lo = model.F("llm/final_norm"), model.W("llm/embed"), model.ps.w16lo("llm/embed")
    head = lambda lg: (lambda: hip.decode_lm_head(ctx.state, ctx.x, gamma, hi, lo, ctx.pval, ctx.pidx, lg, ids=dg.union))
    launch_us = {
        "subset_head_us": launches(head(None)), "subset_head_with_logits_store_us": launches(head(ctx.logits)),
        "finish_us": launches(lambda: hip.decode_finish(ctx.state, ctx.pval, ctx.pidx, ctx.out, -1)),
        "grammar_finish_us": launches(lambda: hip.decode_grammar_finish(ctx.state, None, ctx.gstate, dg.offsets, dg.ids, dg.next,
                                                                        ctx.logits, ctx.out, -1)),
        "launches_per_graph": n_l}
    gbeams = {}
    if a.num_beams:     # grammar + beams beside the plain beam step and the grammar best-of-N step at the same N: graphed, in turns
        for NB in a.num_beams:
            trio = {"grammar_beam": GraphedTokenDecoder(model, 1, N, num_beams=NB, grammar=auto, logprobs=True).capture(),
                    "plain_beam": GraphedTokenDecoder(model, 1, N, num_beams=NB, logprobs=True).capture(),
                    "grammar_num_samples": GraphedTokenDecoder(model, 1, N, sampling=True, num_samples=NB, grammar=auto).capture()}
            call = {k: ((lambda d=d: d(o, temperature=1.0, seed=1)) if k == "grammar_num_samples" else (lambda d=d: d(o)))
                    for k, d in trio.items()}
            bpre = {k: timeit(lambda d=d: (d.g_prefill.replay()), a.reps) for k, d in trio.items()}
            bruns = {k: [] for k in trio}
            for _ in range(max(a.reps, 7)):
                for k, d in trio.items():
                    t = timeit(call[k], 1)
                    bruns[k].append((t - bpre[k]) / max(int(d.ctx.state[0]) - 1, 1))
            gb = trio["grammar_beam"]
            gb(o)
            btok = gb.last_beams[0].cpu().numpy()
            bctx = gb.ctx
            st, bw, gq = bctx.state.clone(), bctx.beam.clone(), bctx.gstate.clone()
            st0, bw0 = bctx.state.clone(), bctx.beam_init.clone()
            st0[0], st0[1] = N // 2, 0
            bw0[:NB] = torch.linspace(0, -1, NB).view(torch.int32) if NB > 1 else bw0[:NB]
            big = int(np.argmax(np.diff(auto.offsets)))             # every row in the state with the most edges

            def greset():
                st.copy_(st0); bw.copy_(bw0); gq.fill_(big)

            gout, glp = bctx.out.clone(), bctx.logp.clone()
            row = {}
            for k in trio:
                row |= {f"{k}_ms_per_step": round(sum(bruns[k]) / len(bruns[k]), 4),
                        f"{k}_ms_per_step_min_max": [round(min(bruns[k]), 4), round(max(bruns[k]), 4)],
                        f"{k}_steps_decoded": int(trio[k].ctx.state[0]), f"{k}_prefill_ms": round(bpre[k], 3)}
            row |= {"grammar_beam_over_plain_beam": round(row["grammar_beam_ms_per_step"] / row["plain_beam_ms_per_step"], 4),
                    "grammar_topn_us_at_the_largest_state": one_launch_us(lambda: hip.decode_beam_grammar_topn(
                        st, bw, gq, dg.offsets, dg.ids, dg.next, bctx.logits, bctx.cand_logp, bctx.cand_id, bctx.cand_next, N), greset),
                    "grammar_select_us": one_launch_us(lambda: hip.decode_beam_grammar_select(
                        st, bw, gq, bctx.cand_logp, bctx.cand_id, bctx.cand_next, gout, glp, cfg.vocab_size, -1), greset),
                    "largest_state_edges": int(np.diff(auto.offsets).max()),
                    "finished_beams_accepted": bool(all(auto.accepts(r) for r in btok if 1 in r.tolist()))}
            gbeams[f"N{NB}"] = row
            del trio, gb
    model.EOS_TOKEN = -1
    grammar_res = ({"grammar_beams": gbeams} if gbeams else {}) | {"grammar": {
        "format": "verbose_with_rotation", "Q": auto.num_states, "E": auto.num_edges, "union": int(auto.union().shape[0]),
        "grammar_graphed_ms_per_token": g_res[0], "grammar_graphed_ms_per_token_min_max": g_res[1], "grammar_tokens_decoded": g_res[2],
        "allowed_union_graphed_ms_per_token": a_res[0], "allowed_union_graphed_ms_per_token_min_max": a_res[1],
        "allowed_union_tokens_decoded": a_res[2], "plain_graphed_ms_per_token": round(g_ms, 3),
        "grammar_row_is_accepted_or_cut_by_the_budget": bool(auto.accepts(gtok[0].cpu().numpy()) or int((gtok[0] == 1).sum()) == 0),
        "launch_us": launch_us}}
if a.jump_forward:
    model.EOS_TOKEN = 1
    auto1 = G.automaton_from_words(encode, LA.word_graph(LA.VERBOSE_WITH_ROTATION_FORMAT), 1, cfg.vocab_size)      # one sentence, then EOS
    decs = {0: GraphedTokenDecoder(model, 1, N, grammar=auto1, logprobs=True).capture()}
    for S in a.jump_forward:
        decs[S] = GraphedTokenDecoder(model, 1, N, grammar=auto1, logprobs=True, jump_forward=S).capture()
    pre = {S: timeit(lambda d=d: (d.g_prefill.replay()), a.reps) for S, d in decs.items()}
    answer, answer_lp = decs[0](o)
    row = answer[0].tolist()
    ans = row[:row.index(1) + 1] if 1 in row else row
    forced_states, q = 0, 0
    for x in ans:
        forced_states += int(len(auto1.allowed(q)) == 1)
        q = auto1.step(q, x)
    runs = {(S, r): [] for S in decs for r in ("none", "answer") if S or r == "none"}
    stats, equal = {}, {}
    for _ in range(max(a.reps, 7)):         # the decoders take turns, so that a drift of the machine reaches all of them
        for S, r in runs:
            kw = {"draft_tokens": ans if r == "answer" else None} if S else {}
            runs[(S, r)].append(timeit(lambda: decs[S](o, **kw), 1) - pre[S])
            if S:
                jgot = decs[S](o, **kw)
                stats[(S, r)] = list(decs[S].last_stats)
                equal[(S, r)] = bool(torch.equal(jgot[0], answer) and torch.equal(jgot[1].view(torch.int32), answer_lp.view(torch.int32)))
    mean = lambda k: sum(runs[k]) / len(runs[k])
    plain_ms = mean((0, "none"))
    one_row_step_ms = plain_ms / max(len(ans) - 1, 1)
    jf = {"format": "verbose_with_rotation", "Q": auto1.num_states, "E": auto1.num_edges, "union": int(auto1.union().shape[0]),
          "answer_tokens": len(ans), "answer_ends_in_eos": bool(ans[-1] == 1), "tokens_from_single_edge_states": forced_states,
          "grammar_ms_per_answer": round(plain_ms, 3),
          "grammar_ms_per_answer_min_max": [round(min(runs[(0, "none")]), 3), round(max(runs[(0, "none")]), 3)],
          "single_row_step_ms": round(one_row_step_ms, 4)}
    for S in a.jump_forward:
        step_ms = mean((S, "none")) / max(stats[(S, "none")][0], 1)
        jf[f"S{S}"] = {
            "forced_only_ms_per_answer": round(mean((S, "none")), 3),
            "forced_only_ms_per_answer_min_max": [round(min(runs[(S, "none")]), 3), round(max(runs[(S, "none")]), 3)],
            "forced_only_steps_accepted": stats[(S, "none")],
            "answer_as_reference_ms_per_answer": round(mean((S, "answer")), 3),
            "answer_as_reference_ms_per_answer_min_max": [round(min(runs[(S, "answer")]), 3), round(max(runs[(S, "answer")]), 3)],
            "answer_as_reference_steps_accepted": stats[(S, "answer")],
            "step_ms": round(step_ms, 4), "step_cost_over_single_row_step": round(step_ms / one_row_step_ms, 3),
            "forced_only_speedup": round(plain_ms / mean((S, "none")), 3),
            "answer_as_reference_speedup": round(plain_ms / mean((S, "answer")), 3),
            "tokens_and_logprobs_equal_plain_grammar_graph": equal[(S, "none")] and equal[(S, "answer")]}
    model.EOS_TOKEN = -1
    grammar_res["grammar_jump_forward"] = jf
print(json.dumps({
    "metric": "batch-1 LAP_AR decode LAP-3B bf16 (ms per token after the prefill, greedy, EOS disabled)",
    "tokens": N, "prompt_len": cfg.max_token_len,
    "eager_ms_per_token": round(per(t_eager, t_pre), 3), "fused_ms_per_token": round(per(t_fused, t_pre), 3),
    "graphed_ms_per_token": round(g_ms, 3), "prefill_ms": round(t_pre, 3), "graphed_prefill_ms": round(t_gpre, 3),
    "graphed_total_ms": round(t_graph, 3), "eager_total_ms": round(t_eager, 3),
    "graphed_vs_eager_leading_tokens_equal": agree, "graphed_equals_eager": bool(torch.equal(got, eager)),
    "algorithmic_bytes_per_token": bytes_tok, "floor_ms_per_token_at_6.29TBps": round(bytes_tok / 6.29e12 * 1e3, 3),
    "achieved_GBps_graphed": round(bytes_tok / (g_ms * 1e-3) / 1e9, 1),
    "share_of_6.29TBps": round(bytes_tok / (g_ms * 1e-3) / 6.29e12, 3), "down_proj_kwaves": a.kwaves} | sampled | ({"weights": quant} if quant else {})
    | ({"allowed": a.allowed, "constrained": constrained} if constrained else {}) | logprobs | best_of | ({"beams": beams} if beams else {}) | ({"speculate": speculative} if speculative else {})
    | ({"score": scoring} if scoring else {}) | grammar_res))
