"""The inputs of the top-k / top-p kernel tests, shared by tests/test_topk_topp_cpu.py (which checks, without a GPU, that few of them
sit on a cut) and tests/test_topk_topp_gpu.py (which runs the kernel on them).  numpy only."""
import numpy as np

from lap_amd import sampling as S

MARGIN = 5e-2                   # tests/test_logprob_gpu.py's MARGIN on scores (top-2 agreement of a draw)
SHARE = 0.05                    # of the (row, case) pairs, the most that may be left out of a comparison
SCALE = 4.0                     # logits = SCALE * standard normal: a peaked row, as an LM head's is
SEED = 20261020                 # of the draws
STEP = 3
BS, VS, TEMPS = (1, 3, 8), (4097, 16384), (0.7, 2.0)
PS = (1e-6, 0.5, 0.9, 1.0)


def ks(n):
    return (1, 2, 50, n - 1, n, n + 5)


def logits(B, V, ties=False, seed=0):
    """float32 [B, V]; ties: rounded to bf16 (8 significant bits), which leaves many exactly equal entries."""
    rng = np.random.default_rng(1000 * B + V + seed)
    lg = (rng.standard_normal((B, V)) * SCALE).astype(np.float32)
    if ties:
        lg = (lg.view(np.uint32) + np.uint32(0x8000) & np.uint32(0xFFFF0000)).view(np.float32)
    return lg


def grid(B, V):
    """The (top_k, top_p) pairs of one (B, V): the issue's k x p grid."""
    return [(k, p) for k in ks(V) for p in PS]


def host(lg, T, k, p, seed=SEED, step=STEP):
    """What the host says about one case: dict of kept count [rows], smallest kept z [rows], token [rows], clear [rows] (the
    filter margin exceeds FILTER_MARGIN and the top-2 kept scores lie further apart than MARGIN)."""
    keep = S.filter_keep(lg, T, k, p)
    z = (lg * S.inverse_temperature(T)).astype(np.float32)
    sc = np.where(keep, S.scores_from_logits(lg, T, seed, step), -np.inf)
    top2 = np.partition(sc, -2, axis=1)[:, -2:]
    with np.errstate(invalid="ignore"):
        gap = top2[:, 1] - top2[:, 0]                       # inf when one entry is kept
    fm = S.filter_margin(lg, T, k, p)
    return {"kept": keep.sum(1), "cut": np.where(keep, z, np.inf).min(1), "token": S.sample_from_logits(lg, T, seed, step, k, p),
            "filter_clear": fm > S.FILTER_MARGIN, "clear": (fm > S.FILTER_MARGIN) & (gap > MARGIN)}
