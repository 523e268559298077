"""The fp8 weight format of the fused LAP_AR decoder (`sample_tokens(decode="fused", decode_weights="fp8")`), restated on the host.

One weight matrix [N, K] (N output features, K contiguous) is stored as
  * codes   OCP e4m3fn, one byte per weight, [N, K];
  * scales  float32 [N], scales[n] = 2^e with e the largest integer such that amax_n * 2^e <= 448 (448 is the largest e4m3
            number); an all-zero row takes e = 0.  e is kept inside [-126, 126] so that 2^e and 2^-e are normal float32 numbers,
            which only rows with amax below 2^-117 can notice.
  * code = e4m3(w * 2^e), round to nearest even (w * 2^e is exact and never exceeds 448, so nothing saturates);
  * the weight a code stands for is code * 2^-e.

The scales are powers of two on purpose.  e4m3 is a floating-point format, so a power of two costs no relative precision against
a free scale; and it makes the decoder exact in two ways: every dequantised weight is a bfloat16 number (3 mantissa bits, an
exponent bfloat16 has), and the scale commutes with float32 accumulation, so the kernels (csrc/decode.hip) accumulate the codes
and multiply the finished row sum by 2^-e once.  "fp8 decoding" is therefore, by definition, the bf16 fused decoder run on
`dequantize_rows(*quantize_rows(w))`.

`quantize_rows` / `dequantize_rows` work on torch tensors of any device (offline use, CPU tests); the device kernel
lap_quantize_fp8_rows (`lap_amd.hip.quantize_fp8_rows`) produces the same bytes.
"""
from __future__ import annotations

import torch

E4M3_MAX = 448.0
E_MIN, E_MAX = -126, 126


def row_exponents(w: torch.Tensor) -> torch.Tensor:
    """int32 [N]: e of every row of the bf16 / f32 matrix w [N, K]."""
    if w.dim() != 2 or w.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"row_exponents: expected a bf16 / f32 matrix, got {w.dtype} {tuple(w.shape)}")
    amax = w.abs().amax(dim=1).to(torch.float32)
    m, x = torch.frexp(amax)                      # amax = m 2^x, 0.5 <= m < 1; 448 = 0.875 * 2^9
    e = torch.where(m <= 0.875, 9, 8).to(torch.int32) - x.to(torch.int32)
    e = e.clamp(E_MIN, E_MAX)
    return torch.where(amax > 0, e, torch.zeros_like(e))


def quantize_rows(w: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """w bf16 / f32 [N, K] -> (codes float8_e4m3fn [N, K], scales f32 [N] = 2^e)."""
    e = row_exponents(w)
    scales = torch.ldexp(torch.ones_like(e, dtype=torch.float32), e)
    codes = (w.to(torch.float32) * scales[:, None]).to(torch.float8_e4m3fn)
    return codes, scales


def dequantize_rows(codes: torch.Tensor, scales: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """code * 2^-e as `dtype` (exact in bfloat16 and float32)."""
    if codes.dtype == torch.uint8:
        codes = codes.view(torch.float8_e4m3fn)
    return (codes.to(torch.float32) / scales.to(torch.float32)[:, None]).to(dtype)
