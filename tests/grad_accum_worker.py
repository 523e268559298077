"""Worker of the bit-for-bit cases of tests/test_grad_accum_gpu.py, run as `python -m tests.grad_accum_worker <out.pt>` with
LAP_SUMSQ_BLOCKS=1 in the environment (read once per process by csrc/loss_optim.hip, hence a process of its own).

Why: two identical plain train steps do not report the same grad_norm bit for bit.  The norm pass (`lap_sumsq_f32` / `_bf16`) ends
in one f32 atomic add per block, a unit of the debug model takes several blocks, and the order in which their adds land is not
fixed: on MI355X the same step gave 6.187402725219727 or 6.187403202056885 from run to run (5 and 3 of 8 runs in one process), and the
parameters behind the clip factor followed.  With one block per launch the sum has one order: 16 of 16 runs gave 6.187403202056885
and identical parameters.  The gradients themselves do not vary in a way that reaches either figure.

Writes {"list": [(loss, grad_norm, master tree) of the existing call, of the one-pair list call],
        "clean": {"after": (loss, grad_norm), "fresh": (loss, grad_norm), "fold_restored": bool, "accum": tuple, "fresh_gacc": int}}."""
import dataclasses
import sys

import torch


def main(out_path):
    import tests.test_grad_accum_gpu as T
    from lap_amd.config import CosineDecaySchedule
    from lap_amd.train import TrainingStepRunner, init_train_state
    from tests.common import to_observation

    DEV = "cuda"
    seed = 1
    res = {}
    # ---- K = 1: the existing call against a list of one pair
    tc = T._tc(1)
    P = T._oracle(2, seed)[0]
    obs, actions, noise, time = T._inputs(tc.model, 1, seed)
    b = (to_observation(obs, DEV), actions.to(DEV))
    runs = []
    for as_list in (False, True):
        st = init_train_state(tc, params=P, device=DEV)
        st, info = TrainingStepRunner(tc)(0, st, [b] if as_list else b, 0, noise=[noise.to(DEV)] if as_list else noise.to(DEV),
                                          time=[time.to(DEV)] if as_list else time.to(DEV))
        runs.append((info["loss"].item(), info["grad_norm"].item(), st.model.ps.to_reference_tree("master"), len(st.model.ps.gacc)))
    res["list"] = runs
    # ---- a plain step on the state an accumulated step left (learning rate 0: the parameters are the initial ones) against a fresh state
    K = 2
    still = dict(lr_schedule=CosineDecaySchedule(warmup_steps=0, peak_lr=0.0, decay_steps=1, decay_lr=0.0))
    tca, tc1 = T._tc(K, **still), T._tc(1, **still)
    obs, actions, noise, time = T._inputs(tca.model, K, seed)
    batches, nz, tm = T._micro(obs, actions, noise, time, K)
    plain = lambda s: TrainingStepRunner(tc1)(0, s, batches[1], 1, noise=nz[1], time=tm[1])      # noqa: E731
    sa = init_train_state(tca, params=P, device=DEV)
    fold0 = sa.model.comm.fold_sumsq
    sa, _ = TrainingStepRunner(tca)(0, sa, batches, 0, noise=nz, time=tm)
    restored, accum = sa.model.comm.fold_sumsq == fold0, tuple(sa.model.comm.accum)
    _, info_a = plain(sa)
    sf = dataclasses.replace(init_train_state(tc1, params=P, device=DEV), step=1)
    sf2, info_f = plain(sf)
    torch.cuda.synchronize()
    res["clean"] = {"after": (info_a["loss"].item(), info_a["grad_norm"].item()), "fresh": (info_f["loss"].item(), info_f["grad_norm"].item()),
                    "fold_restored": restored, "accum": accum, "fresh_gacc": len(sf2.model.ps.gacc)}
    torch.save(res, out_path)


if __name__ == "__main__":
    main(sys.argv[1])
