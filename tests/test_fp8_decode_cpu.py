"""The fp8 weight format of the fused decoder (lap_amd/fp8.py) against an independent statement of it, on the CPU.

Format: codes = e4m3fn(w * 2^e), round to nearest even, e the largest integer with amax_row * 2^e <= 448 (0 for an all-zero
row); the weight a code stands for is code * 2^-e.  The independent statement finds e by exact float64 search instead of frexp.
"""
import math

import pytest
import torch

from lap_amd import fp8

SHAPES = [((2560, 2048), 0.02), ((2048, 16384), 0.01), ((4096, 2048), 0.03)]      # wqkv, wd, a slice of the table; (shape, std)


def _exponent_by_search(amax: float) -> int:
    """The largest integer e with amax * 2^e <= 448, in exact arithmetic (float64 holds every product of a float32 and 2^e)."""
    if amax == 0.0:
        return 0
    e = int(math.floor(math.log2(448.0 / amax)))
    while amax * 2.0 ** (e + 1) <= 448.0:
        e += 1
    while amax * 2.0 ** e > 448.0:
        e -= 1
    return e


def _statement(w):
    """(codes, scales) by the words of the format."""
    amax = w.abs().amax(dim=1).double().tolist()
    e = torch.tensor([_exponent_by_search(a) for a in amax], dtype=torch.float64)
    scales = torch.pow(torch.tensor(2.0, dtype=torch.float64), e).to(torch.float32)
    return (w.to(torch.float32) * scales[:, None]).to(torch.float8_e4m3fn), scales


def _hand_rows(K, dtype):
    """Rows built by hand (every value a bf16 number): all zero; amax an exact power of two; amax exactly on 448 * 2^-9 and one
    bf16 step above it (the exponent changes between them); rounding ties of the normal range (17, 19, 21 ... of spacing 2 lie
    halfway between codes) and the e4m3 subnormal range (multiples of 2^-9 below 2^-6, halves of them are ties)."""
    rows = torch.zeros(6, K, dtype=torch.float32)
    rows[1, :4] = torch.tensor([0.5, -0.25, 0.125, 0.3125])
    rows[2, :3] = torch.tensor([0.875, -0.5, 0.09375])
    rows[3, :3] = torch.tensor([0.87890625, -0.5, 0.09375])
    ties = torch.tensor([17.0, 19.0, 21.0, 23.0, -17.0, -19.0, 34.0, 38.0, 1.0625, 1.1875, 208.0, 240.0, 432.0])
    rows[4, 0] = 0.875                                   # e = 9: the values below are k / 512
    rows[4, 1:1 + ties.numel()] = ties / 512.0
    sub = torch.tensor([0.5, 1.0, 1.5, 2.5, 3.5, 6.5, 7.5, 0.4921875, 0.5078125, 3.3125, -0.5, -1.5, -7.5, 8.0, 8.5]) * 2.0 ** -9
    rows[5, 0] = 0.875
    rows[5, 1:1 + sub.numel()] = sub / 512.0
    assert torch.equal(rows, rows.to(torch.bfloat16).to(torch.float32))
    return rows.to(dtype)


def _inputs(shape, std, dtype):
    g = torch.Generator().manual_seed(shape[0] + shape[1])
    w = (torch.randn(shape, generator=g) * std).to(dtype)
    hand = _hand_rows(shape[1], dtype)
    w[: hand.shape[0]] = hand
    return w


@pytest.mark.parametrize("shape,std", SHAPES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_host_quantiser_is_the_format_byte_for_byte(shape, std, dtype):
    w = _inputs(shape, std, dtype)
    codes, scales = fp8.quantize_rows(w)
    rc, rs = _statement(w)
    assert codes.dtype == torch.float8_e4m3fn and scales.dtype == torch.float32 and tuple(codes.shape) == shape
    assert torch.equal(scales, rs)
    assert torch.equal(codes.view(torch.uint8), rc.view(torch.uint8))
    # the hand-built rows land where the format says
    assert scales[0] == 1.0 and int(codes[0].view(torch.uint8).max()) == 0
    assert scales[1] == 512.0 and scales[2] == 512.0 and scales[3] == 256.0
    assert float(codes[2, 0].float()) == 448.0
    c4 = codes[4, 1:14].float().tolist()
    assert c4 == [16.0, 20.0, 20.0, 24.0, -16.0, -20.0, 32.0, 40.0, 1.0, 1.25, 208.0, 240.0, 448.0]       # ties to even
    c5 = (codes[5, 1:16].float() * 512.0).tolist()
    assert c5 == [0.0, 1.0, 2.0, 2.0, 4.0, 6.0, 8.0, 0.0, 1.0, 3.0, -0.0, -2.0, -8.0, 8.0, 8.0]          # subnormal codes, ties to even


@pytest.mark.parametrize("shape,std", SHAPES)
def test_dequantised_weights_are_bf16_numbers_within_the_e4m3_error(shape, std):
    w = _inputs(shape, std, torch.bfloat16)
    codes, scales = fp8.quantize_rows(w)
    d32 = fp8.dequantize_rows(codes, scales, torch.float32)
    d16 = fp8.dequantize_rows(codes, scales)
    assert d16.dtype == torch.bfloat16 and torch.equal(d16.to(torch.float32), d32)          # survives the bf16 round trip
    assert torch.equal(fp8.dequantize_rows(codes.view(torch.uint8), scales, torch.float32), d32)
    # the dequantised weights are a fixed point: every value is a code of its row (whose exponent can only have grown)
    c2, s2 = fp8.quantize_rows(d16)
    assert bool((s2 >= scales).all()) and torch.equal(fp8.dequantize_rows(c2, s2, torch.float32), d32)
    # the relative error of a Gaussian matrix: 3 mantissa bits round within 2^-4 per weight; 2.6 - 2.7 % in the norm
    w32 = w.to(torch.float32)
    err = float((d32 - w32).norm() / w32.norm())
    assert 0.02 < err < 0.03, err
    normal = w32.abs() * scales[:, None] >= 2.0 ** -6
    assert float(((d32 - w32).abs()[normal] / w32.abs()[normal]).max()) <= 2.0 ** -4


def test_extreme_rows_keep_finite_scales():
    w = torch.zeros(3, 8, dtype=torch.float32)
    w[0, 0] = 2.0 ** -140            # (float32 subnormal: e is capped at 126)
    w[1, 0] = 3.0e38
    w[2, 0] = -448.0
    codes, scales = fp8.quantize_rows(w)
    assert torch.isfinite(scales).all() and torch.isfinite(1.0 / scales).all()
    assert scales.tolist() == [2.0 ** 126, 2.0 ** -120, 1.0]
    assert float(codes[2, 0].float()) == -448.0 and abs(float(codes[1, 0].float())) <= 448.0


def test_sample_tokens_rejects_bad_decode_weights_before_any_device_work():
    from lap_amd.model import LAP
    from lap_amd.params import ParamStore
    from tests.common import debug_model_cfg

    cfg = debug_model_cfg()
    model = LAP(cfg, device="cpu", store=ParamStore(cfg, "cpu", with_optimizer=False, with_ema=False, with_grads=False))
    assert LAP.DECODE_WEIGHTS == ("bf16", "fp8", "fp8_layers")
    with pytest.raises(ValueError, match="decode_weights"):
        model.sample_tokens(0, None, decode="fused", decode_weights="int4")
    for w in ("fp8", "fp8_layers"):
        with pytest.raises(ValueError, match='decode="fused"'):
            model.sample_tokens(0, None, decode_weights=w)
        with pytest.raises(ValueError, match='decode="fused"'):
            model.sample_tokens(0, None, decode="eager", decode_weights=w)
