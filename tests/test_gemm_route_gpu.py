"""The plan is what runs (GPU): for one shape per route class of lap_gemm_bf16_ex, the automatic call launches exactly the assembly
kernels its plan (hip.gemm_plan) names, and running the plan's legs by hand, each as a call of its own on the sub-views with the
leg's tile and K split forced, gives the same bits.

The shapes are the smallest by operand bytes that the planner routes to each class, searched on the CPU over M in {8 .. 512, 256 i,
65536 + 8}, N in {8, 16, 64, 128 i}, K in {8, 64, 512, 768, 1024, 1536, 2048, 2176, 4096, 4224, 8192, 16384} with the scratch
lap_amd.hip lends; the rules' own thresholds (128 tiles for the assembly kernels, a full round for the cuts, 65536 rows for the
ragged-M cut) set their size, K stays at each rule's minimum."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
FWD, DGRAD, WGRAD = (True, True), (True, False), (False, False)
# class: (M, N, K, layout, f32 output, bias (f32), residual, engines of the plan)
CASES = {
    "asm_plain_forward": (2048, 4096, 512, FWD, False, False, False, [32]),
    "asm_plain_dgrad": (3328, 4096, 512, DGRAD, False, False, False, [32]),
    "asm_plain_wgrad": (3328, 4096, 512, WGRAD, True, False, False, [32]),
    "asm_bias": (5888, 2176, 512, FWD, False, True, False, [33]),
    "asm_residual": (3328, 4096, 512, FWD, False, False, True, [34]),
    "m_cut_plain": (4352, 4096, 512, FWD, False, False, False, [32, 6]),
    "m_cut_residual": (4352, 4096, 512, FWD, False, False, True, [34, 6]),
    "ragged_m_cut": (65544, 256, 512, WGRAD, True, False, False, [32, 6]),
    "n_cut": (7424, 2176, 2048, FWD, False, False, False, [32, 6]),
    "long_k_split": (8, 8, 16384, FWD, False, False, False, [10]),
    "serving_tile": (264, 1024, 8, FWD, False, False, False, [17]),
    "two_phase_tile_6": (8, 8, 1024, FWD, False, False, False, [6]),
    "tail_split": (26368, 640, 768, FWD, False, False, False, [10, 6]),
}
ASM_NAME = {(32, FWD): "nt", (32, DGRAD): "nn", (33, FWD): "nt_bias", (34, FWD): "nt_res"}


def _rnd(rows, cols, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(rows, cols, generator=g).bfloat16().to(DEV)


def _call(hip, a, b, c, bias, res, M, N, K, layout, tile, ksplit, scratch, offs=(0, 0, 0, 0, 0)):
    flags = (hip.GEMM_OUT_F32 if c.dtype == torch.float32 else 0) | (hip.GEMM_BIAS_F32 if bias is not None else 0)
    ptr = lambda t, off: None if t is None else t.data_ptr() + off * t.element_size()
    hip.call("lap_gemm_bf16_ex", ptr(a, offs[0]), ptr(b, offs[1]), ptr(c, offs[2]), ptr(bias, offs[3]), ptr(res, offs[4]), M, N, K, a.stride(0), b.stride(0),
             c.stride(0), res.stride(0) if res is not None else 0, 1.0, int(layout[0]), int(layout[1]), flags, tile, ksplit, scratch.data_ptr(), scratch.numel() * 4)


@pytest.mark.parametrize("name", list(CASES))
def test_the_plan_is_what_runs(hip, name):
    M, N, K, layout, f32, biased, with_res, engines = CASES[name]
    a_kc, b_kc = layout
    a = _rnd(M, K, 1) if a_kc else _rnd(K, M, 1)
    b = _rnd(N, K, 2) if b_kc else _rnd(K, N, 2)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(3)).to(DEV) if biased else None
    res = _rnd(M, N, 4) if with_res else None
    scratch = hip._gemm_scratch(a.device)
    flags = (hip.GEMM_OUT_F32 if f32 else 0) | (hip.GEMM_BIAS_F32 if biased else 0)
    legs = hip.gemm_plan(M=M, N=N, K=K, lda=a.stride(0), ldb=b.stride(0), ldc=N, ldr=N if with_res else 0, a_kc=a_kc, b_kc=b_kc, flags=flags,
                         a=a.data_ptr(), b=b.data_ptr(), c=256, bias=None if bias is None else bias.data_ptr(), residual=None if res is None else res.data_ptr(),
                         scratch=scratch.data_ptr(), scratch_bytes=scratch.numel() * 4)
    assert [l.engine for l in legs] == engines, name            # the class this shape was chosen for
    want = {}
    for l in legs:
        if l.engine >= hip.LEG_ASM:
            k = ("tn_t" if l.M > l.N else "tn") if layout == WGRAD else ASM_NAME[(l.engine, layout)]
            want[k] = want.get(k, 0) + 1
    auto = torch.full((M, N), 3.0, device=DEV, dtype=torch.float32 if f32 else torch.bfloat16)
    before = hip.gemm_asm_launch_counts()
    _call(hip, a, b, auto, bias, res, M, N, K, layout, -1, 0, scratch)
    ran = {k: v - before[k] for k, v in hip.gemm_asm_launch_counts().items() if v != before[k]}
    assert ran == want, (name, ran, want)
    if any(l.tile_count for l in legs):      # a tail split's legs share one tile grid: not expressible as calls of their own
        ref = (a.float() if a_kc else a.float().t()) @ (b.float().t() if b_kc else b.float())
        assert ((auto.float() - ref).norm() / ref.norm()).item() < 4e-3
        return
    hand = torch.full_like(auto, 3.0)
    for l in legs:
        _call(hip, a, b, hand, bias, res, l.M, l.N, K, layout, 14 if l.engine >= hip.LEG_ASM else l.engine, l.ksplit, scratch,
              (l.off_a, l.off_b, l.off_c, l.off_bias, l.off_res))
    assert torch.equal(auto, hand), name
