"""Gradient accumulation under FSDP on ONE GPU: two ranks (gloo backend, both on cuda:0) running accumulated steps (K = 2) on their
halves of every micro-batch must reproduce the single rank's accumulated steps on the whole micro-batches — the per-micro-step
reduce-scatter into the reduced shard's accumulator, the replicated unit's one all-reduce on the last micro-step, the two norm
slots, and the global loss denominators over a real process group.  Harness, batch and tolerances of tests/test_fsdp_gpu.py
(imported, not edited); fresh spawned processes."""
import dataclasses
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_fsdp_gpu import _batch, _debug_tc, _slice_obs

pytestmark = pytest.mark.gpu
K, PER = 2, 2          # micro-steps per optimizer step; samples per rank and micro-step
KEYS = ("PaliGemma/llm/layers/mlp/linear", "PaliGemma/img/head/kernel", "PaliGemma/llm/embedder/input_embedding", "action_out_proj/kernel")


def _tc(world):
    return dataclasses.replace(_debug_tc(True), grad_accum_steps=K, batch_size=K * PER * 2)


def _micro_batches(cfg, rank, world, dev):
    """Micro-batch k of the whole batch is samples [4k, 4k + 4); rank r of two takes [4k + 2r, 4k + 2r + 2) of it, so the ranks'
    micro-gradients sum to the single rank's."""
    from tests.common import to_observation

    obs, actions, noise, time = _batch(cfg, K * PER * 2)
    per = PER * 2 // world
    sls = [slice(2 * PER * k + per * rank, 2 * PER * k + per * (rank + 1)) for k in range(K)]
    return ([(to_observation(_slice_obs(obs, s), dev), actions[s].to(dev)) for s in sls], [noise[s].to(dev) for s in sls],
            [time[s].to(dev) for s in sls])


def _steps(tc, state, rank, world, dev):
    from lap_amd.train import TrainingStepRunner

    runner = TrainingStepRunner(tc)
    batches, nz, tm = _micro_batches(tc.model, rank, world, dev)
    infos = []
    for step in range(2):      # the second step runs on the all-gathered bf16 mirrors and re-uses the accumulators
        state, info = runner(0, state, batches, step, noise=nz, time=tm)
        infos.append((info["loss"].item(), info["grad_norm"].item()))
    torch.cuda.synchronize()
    return state, infos


def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from lap_amd.train import init_train_state
        from oracle import lap_oracle as O
        from tests.common import oracle_cfg

        dev = "cuda:0"
        tc = _tc(world)
        P = O.init_params(oracle_cfg(tc.model), seed=9)
        state = init_train_state(tc, params=P, device=dev, world_size=world, rank=rank, use_fsdp=True)
        state, infos = _steps(tc, state, rank, world, dev)
        ps = state.model.ps
        shard_sized = all(ps.gacc[n].numel() == ps.shard_numel(ps.unit_by_name[n]) for n in ps.gacc)
        names = sorted(ps.gacc)
        tree = ps.to_reference_tree("master")
        ret[rank] = ("ok", infos, {k: v for k, v in tree.items() if k in KEYS}, (names, shard_sized))
    except Exception:  # noqa: BLE001
        import traceback

        ret[rank] = ("err", traceback.format_exc(), None, None)
    finally:
        dist.destroy_process_group()


def test_two_rank_accumulated_step_equals_single_rank(hip):
    from lap_amd.train import init_train_state
    from oracle import lap_oracle as O
    from tests.common import oracle_cfg, rel

    world = 2
    port = 29950 + os.getpid() % 300
    mgr = mp.get_context("spawn").Manager()   # (a forked manager next to an initialised HIP runtime is not safe)
    ret = mgr.dict()
    procs = [mp.get_context("spawn").Process(target=_worker, args=(r, world, port, ret)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(150)
    for p in procs:
        if p.is_alive():
            p.kill()
    assert all(ret.get(r, ("missing",))[0] == "ok" for r in range(world)), {r: ret.get(r, ("missing",))[:2] for r in range(world)}
    # single rank, K = 2, on the whole micro-batches
    tc = _tc(1)
    P = O.init_params(oracle_cfg(tc.model), seed=9)
    state = init_train_state(tc, params=P, device="cuda:0")
    state, ref_infos = _steps(tc, state, 0, 1, "cuda:0")
    ref_tree = state.model.ps.to_reference_tree("master")
    big = sorted(u.name for u in state.model.ps.units if u.big)
    for r in range(world):
        _, infos, tree, (names, shard_sized) = ret[r]
        assert names == big and shard_sized          # one accumulator per big unit, each the size of the rank's shard
        print(f"rank {r}: (loss, grad_norm) {infos} single rank {ref_infos}")
        for (l, g), (lr, gr) in zip(infos, ref_infos):      # tests/test_fsdp_gpu.py:105
            assert abs(l - lr) / abs(lr) < 2e-3 and abs(g - gr) / gr < 2e-2, (infos, ref_infos)
        for k, v in tree.items():                           # tests/test_fsdp_gpu.py:106-109
            upd, upd_ref = v - P[k], ref_tree[k] - P[k]
            assert rel(upd, upd_ref) < 0.1, (k, rel(upd, upd_ref))
            assert rel(v, ref_tree[k]) < 1e-3, k
    assert torch.equal(ret[0][2]["action_out_proj/kernel"], ret[1][2]["action_out_proj/kernel"])  # replicated unit stays in sync
