"""lap_grad_fold (csrc/grad_fold.hip) element by element against float64 numpy (GPU): three folds of one accumulator — first,
middle, last with the sum of squares — from bf16 and f32 gradient sources, at sizes that exercise the unaligned head, the tail,
one block, several blocks and a grid-stride loop that wraps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
# The kernel's block is 256 threads and a thread folds 8 bf16 (4 f32) values per iteration: 256 CUs x 256 x 8 = 524,288 bf16 values
# per sweep of the whole grid (one block per CU).  1,100,003 > 2 x 524,288: the grid-stride loop wraps twice for bf16 and four
# times for f32, and the odd count leaves a tail.
N_WRAP = 1_100_003
SIZES = (1, 2, 7, 255, 4102, N_WRAP)
GUARD = 3.0e38


def _sources(n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(3):
        big = torch.empty(n + 9, dtype=torch.float32).normal_(0.0, 3.0 ** k, generator=g).to(dtype)
        out.append(big)
    return out


@pytest.mark.parametrize("layout", ["odd-acc+4B", "odd-acc+16B", "aligned", "cut5"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_three_folds_against_float64(hip, n, dtype, layout):
    """odd: the source is a view at an ODD element offset of a larger buffer (bf16: 2-byte aligned); the accumulator sits between guard
    words, 4 or 16 bytes into its allocation.  acc+4B: the head that brings the gradient to a 16-byte boundary (7 bf16 / 3 f32
    elements) aligns the accumulator too: vector loads behind an unaligned head.  acc+16B: no common boundary exists; the accumulator
    alone is aligned and the gradient's values are loaded one by one.  aligned: both 16-byte aligned, as whole unit buffers are (no
    head).  cut5: both views start at element 5 of 16-byte aligned buffers, as a range cut by a freeze filter does: a
    three-element head and vector loads on both."""
    src = _sources(n, dtype, seed=n % 1000 + (7 if dtype == torch.float32 else 0))
    acc_off = {"odd-acc+4B": 1, "cut5": 5}.get(layout, 4)
    off = {"aligned": 0, "cut5": 5}.get(layout, 1 if dtype == torch.bfloat16 or acc_off == 1 else 3)
    buf = torch.full((acc_off + n + 5,), GUARD, dtype=torch.float32, device=DEV)
    acc = buf[acc_off:acc_off + n]
    ss = torch.full((3,), 7.5, dtype=torch.float32, device=DEV)        # [guard, sumsq, guard]
    want32 = None
    sum64 = np.zeros(n, np.float64)
    sumabs = np.zeros(n, np.float64)
    for k in range(3):
        gk = src[k].to(DEV)[off:off + n]
        assert (gk.data_ptr() % 16 == 0) == (layout == "aligned")
        last = k == 2
        if last:
            ss[1] = 0.0
        hip.grad_fold(acc, gk, first=(k == 0), sumsq=ss[1:2] if last else None)
        torch.cuda.synchronize()
        g32 = src[k][off:off + n].float().numpy()
        # the specification: one f32 add per element and fold, in this order -> bit equality
        want32 = g32.copy() if k == 0 else (want32 + g32).astype(np.float32)
        got = acc.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), want32.view(np.uint32)), (n, dtype, k, np.flatnonzero(got != want32)[:8])
        sum64 += g32.astype(np.float64)
        sumabs += np.abs(g32.astype(np.float64))
        assert np.all(np.abs(got.astype(np.float64) - sum64) <= 3 * U * sumabs), (n, dtype, k)      # K 2^-24 sum |g_k|
        host = buf.cpu()
        assert bool((host[:acc_off] == GUARD).all()) and bool((host[acc_off + n:] == GUARD).all()), (n, dtype, k, "guard words")
        if not last:        # a call without `sumsq` leaves the buffer alone
            assert ss.cpu().tolist() == [7.5, 7.5, 7.5]
    # the sum of squares of the values stored: the form of tests/test_kernels_gpu.py:1101 (lap_sumsq_f32), rel. 1e-5 of the float64 sum
    want = float((want32.astype(np.float64) ** 2).sum())
    s = ss.cpu().tolist()
    assert s[0] == 7.5 and s[2] == 7.5
    assert abs(s[1] - want) <= 1e-5 * want, (n, dtype, s[1], want)


def test_fold_adds_to_a_running_sum_of_squares_and_rejects_bad_arguments(hip):
    n = 4102
    g = torch.randn(n, device=DEV).bfloat16()
    acc = torch.zeros(n, device=DEV)
    ss = torch.full((1,), 3.25, device=DEV)
    hip.grad_fold(acc, g, first=True, sumsq=ss)
    want = 3.25 + float((g.double() ** 2).sum())
    assert torch.equal(acc, g.float()) and abs(ss.item() - want) <= 1e-5 * want
    with pytest.raises(ValueError):
        hip.grad_fold(acc, g[:-1], first=True)
    with pytest.raises(TypeError):
        hip.grad_fold(acc.bfloat16(), g, first=True)
    with pytest.raises(hip.LapHipError, match="1001"):
        hip.call("lap_grad_fold", acc.data_ptr(), g.data_ptr(), 1, 0, 1, None)
    with pytest.raises(hip.LapHipError, match="1001"):
        hip.call("lap_grad_fold", acc.data_ptr() + 2, g.data_ptr(), 1, 8, 1, None)
