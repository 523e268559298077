"""The outputs of the HIP GEMM kernels (csrc/gemm.hip, csrc/gemm_fp8.hip) pinned bit for bit (GPU).

tests/test_kernels_gpu.py holds the tiles to a float32 product within a tolerance and to each other bitwise; neither says that an
output is the bits it was before a change to an epilogue, a launcher or a staging offset.  This module does:
tests/golden/gemm_bits_v1.json holds, per case, the sha256 of the bytes of the whole output buffer (padding columns included) as
the kernels wrote it at the commit the fixture names, before the epilogue arithmetic, the 256 x 256 launchers and the operand
staging were each brought to one place, and the kernels of the tree must reproduce them.  A change that means to move the bits
re-records the fixture (tests/golden/make_gemm_bits_golden.py) and says so.

Every bf16 case first asks hip.gemm_plan what its arguments launch and asserts the legs it is meant to reach: per leg
(engine, ksplit, reduce, sub256, part_compact).  A case that routes elsewhere fails there instead of passing on another kernel.
Atomic split-K (ksplit > 1 without scratch) is left out: its summation order is not fixed.

Inputs are drawn on the CPU from seeded generators and copied to the device; operands with more than BLOCK rows repeat a seeded
block of BLOCK rows.  The fixture holds the sha256 of every drawn block, and a platform whose generators do not reproduce them
fails with that message.  Cases (all with ldc = N + 8 and, with a residual, ldr = N + 8):
  direct epilogue   tiles 0, 2, 6 at 200 x 136 x 72 in all three layouts, tiles 16-19 at 520 x 392 x 200 (forward), every option
  staged epilogue   requested tiles 5, 10, 12 at 520 x 392 x 192 in all three layouts (a requested 5 runs as 10 or 12 when
                    K % 8 == 0), the 16-wave kernel itself (engine 5) at K = 196 in the weight-gradient layout, every option;
                    520 x 396 x 192 for the fallback to direct stores (N % 8 != 0)
  GeGLU             tile 15 through linear_geglu, M 300, H 256, K 128, tanhf and exp2
  full reduce       100 x 1024 x 2048 forward (tile 6 split 8): residual, bias + GELU; 136 x 200 x 16384 data gradient,
                    f32 accumulating (tile 12 split 8)
  tail reduce       16384 x 1152 x 4352, requested tile 5 with scratch (256 tiles unsplit + 64 tiles split 4): forward plain
                    and bias + residual, weight-gradient layout f32 accumulating
  quadrant tail     10760 x 1288 x 768 forward, requested tile 5 with scratch: 258 tiles, the last 2 as quadrants on the
                    128 x 128 kernel (sub256), both on the ragged right edge
  fp8               300 x 264 x 256 (staged) and 300 x 260 x 256 (direct): bf16 + residual, f32 accumulating
"""
import functools
import hashlib
import json
import os
import pathlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIXTURE = pathlib.Path(__file__).parent / "golden" / "gemm_bits_v1.json"
BLOCK = 521                            # rows of a seeded block; taller operands repeat it
SCRATCH_FLOATS = 32 * 1024 * 1024      # 128 MiB: the tail split's 4 x 64 slabs of 256 x 256 f32 need 64 MiB
LAYOUTS = {"fwd": (1, 1), "dgrad": (1, 0), "wgrad": (0, 0)}     # (a_kc, b_kc)
NONE, SPLITK, TAIL = 0, 1, 2           # LAP_LEG_REDUCE_*
OPTS = {
    "none": {}, "bias16": {"bias": "b16"}, "bias32": {"bias": "b32"}, "bias_gelu": {"bias": "b32", "gelu": 1},
    "bias_gelu_bf16": {"bias": "b32", "gelu": 2}, "residual": {"res": True}, "bias_residual": {"bias": "b16", "res": True},
    "alpha": {"alpha": 0.5}, "f32": {"f32": True}, "f32_accum": {"f32": True, "accum": True}, "f32_bias32": {"f32": True, "bias": "b32"},
}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def _case(group, M, N, K, lay, opt, tile, legs, scratch=False, ksplit=1):
    return {"name": f"{group}/t{tile}/{M}x{N}x{K}/{lay}/{opt}", "group": group, "shape": (M, N, K), "lay": lay, "opt": opt, "tile": tile,
            "ksplit": ksplit, "scratch": scratch, "legs": legs}


def _big(lay):   # what a requested tile 5 runs as when K % 8 == 0 (csrc/gemm_route.hpp)
    return 10 if lay == "fwd" else 12


def gemm_cases():
    cs = []
    for tile in (0, 2, 6):
        cs += [_case(f"direct-t{tile}", 200, 136, 72, lay, o, tile, [(tile, 1, NONE, 0, 0)]) for lay in LAYOUTS for o in OPTS]
    for tile in (16, 17, 18, 19):
        cs += [_case(f"direct-t{tile}", 520, 392, 200, "fwd", o, tile, [(tile, 1, NONE, 0, 0)]) for o in OPTS]
    for tile in (5, 10, 12):
        cs += [_case(f"staged-t{tile}", 520, 392, 192, lay, o, tile, [(_big(lay) if tile == 5 else tile, 1, NONE, 0, 0)])
               for lay in LAYOUTS for o in OPTS]
    cs += [_case("staged-16wave", 520, 392, 196, "wgrad", o, 5, [(5, 1, NONE, 0, 0)]) for o in OPTS]
    cs += [_case("fallback", 520, 396, 192, "fwd", o, 5, [(10, 1, NONE, 0, 0)]) for o in OPTS]
    cs += [_case("reduce", 100, 1024, 2048, "fwd", o, -1, [(6, 8, SPLITK, 0, 0)], scratch=True, ksplit=0) for o in ("residual", "bias_gelu")]
    cs += [_case("reduce", 136, 200, 16384, "dgrad", "f32_accum", -1, [(12, 8, SPLITK, 0, 0)], scratch=True, ksplit=0)]
    cs += [_case("tail", 16384, 1152, 4352, lay, o, 5, [(_big(lay), 1, NONE, 0, 0), (_big(lay), 4, TAIL, 0, 1)], scratch=True, ksplit=0)
           for lay, o in (("fwd", "none"), ("fwd", "bias_residual"), ("wgrad", "f32_accum"))]
    cs += [_case("sub256", 10760, 1288, 768, "fwd", o, 5, [(10, 1, NONE, 0, 0), (6, 1, NONE, 1, 0)], scratch=True, ksplit=0)
           for o in ("none", "bias_residual")]
    return cs


GEGLU = (300, 256, 128)                                   # M, H, K
FP8_SHAPES = ((300, 264, 256), (300, 260, 256))           # staged / direct
GROUPS = sorted({c["group"] for c in gemm_cases()}) + ["geglu", "fp8"]


def block(seed, rows, cols, dtype=torch.bfloat16, scale=1.0):
    """The seeded block an operand [rows][cols] is made of (at most BLOCK rows)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(min(rows, BLOCK), cols, generator=g) * scale).to(dtype)


def tiled(blk, rows):
    return blk if blk.shape[0] >= rows else blk.repeat((rows + blk.shape[0] - 1) // blk.shape[0], 1)[:rows].contiguous()


def operand_blocks(M, N, K, lay):
    a_kc, b_kc = LAYOUTS[lay]
    return {"a": block(1, *((M, K) if a_kc else (K, M))), "b": block(2, *((N, K) if b_kc else (K, N)), scale=K ** -0.5),
            "b16": block(3, 1, N), "b32": block(4, 1, N, torch.float32), "res": block(5, M, N + 8), "c0": block(6, M, N + 8, torch.float32)}


def fp8_blocks(M, N, K):
    g = torch.Generator().manual_seed(7)
    code = lambda r: (torch.randint(0, 0x48, (r, K), generator=g) | (torch.randint(0, 2, (r, K), generator=g) << 7)).to(torch.uint8)
    return {"a8": code(M), "b8": code(N), "res": block(5, M, N + 8), "c0": block(6, M, N + 8, torch.float32)}


@functools.lru_cache(maxsize=2)
def operands(M, N, K, lay):
    a_kc, b_kc = LAYOUTS[lay]
    rows = {"a": M if a_kc else K, "b": N if b_kc else K, "b16": 1, "b32": 1, "res": M, "c0": M}
    return {n: tiled(t, rows[n]).to(DEV) for n, t in operand_blocks(M, N, K, lay).items()}


def input_hashes():
    out = {}
    for M, N, K, lay in sorted({(*c["shape"], c["lay"]) for c in gemm_cases()}):
        out.update({f"{M}x{N}x{K}/{lay}/{n}": sha(t) for n, t in operand_blocks(M, N, K, lay).items()})
    M, H, K = GEGLU
    out.update({"geglu/x": sha(block(1, M, K)), "geglu/wgu": sha(block(2, 2 * H, K, scale=K ** -0.5))})
    for s in FP8_SHAPES:
        out.update({"fp8/%dx%dx%d/%s" % (*s, n): sha(t) for n, t in fp8_blocks(*s).items()})
    return out


def _switches(hip):
    return sum(bit for name, bit in hip.ROUTE_SWITCHES.items() if os.environ.get(name) is not None)


def _assert_route(hip, name, want, **plan_args):
    legs = hip.gemm_plan(switches=_switches(hip), **plan_args)
    got = [(l.engine, l.ksplit, l.reduce, l.sub256, l.part_compact) for l in legs]
    assert got == want, f"{name}: routed to {got} (engine, ksplit, reduce, sub256, part_compact), the case is meant for {want}"


def run_gemm(hip, c, scratch):
    (M, N, K), (a_kc, b_kc), o = c["shape"], LAYOUTS[c["lay"]], OPTS[c["opt"]]
    d = operands(M, N, K, c["lay"])
    f32 = o.get("f32", False)
    out = d["c0"].clone() if o.get("accum") else torch.zeros(M, N + 8, dtype=torch.float32 if f32 else torch.bfloat16, device=DEV)
    bias = d[o["bias"]][0] if "bias" in o else None
    res = d["res"] if o.get("res") else None
    flags = ((hip.GEMM_OUT_F32 if f32 else 0) | (hip.GEMM_ACCUM if o.get("accum") else 0) | (hip.GEMM_BIAS_F32 if o.get("bias") == "b32" else 0)
             | (hip.GEMM_GELU if o.get("gelu") else 0) | (hip.GEMM_GELU_BF16 if o.get("gelu") == 2 else 0))
    p = lambda t: None if t is None else t.data_ptr()
    sc = scratch if c["scratch"] else None
    args = dict(M=M, N=N, K=K, lda=d["a"].stride(0), ldb=d["b"].stride(0), ldc=N + 8, ldr=N + 8 if res is not None else 0, alpha=o.get("alpha", 1.0),
                a_kc=a_kc, b_kc=b_kc, flags=flags, tile=c["tile"], ksplit=c["ksplit"])
    _assert_route(hip, c["name"], c["legs"], a=p(d["a"]), b=p(d["b"]), c=p(out), bias=p(bias), residual=p(res), scratch=p(sc),
                  scratch_bytes=sc.numel() * 4 if sc is not None else 0, **args)
    hip.call("lap_gemm_bf16_ex", p(d["a"]), p(d["b"]), p(out), p(bias), p(res), M, N, K, args["lda"], args["ldb"], args["ldc"], args["ldr"],
             float(args["alpha"]), a_kc, b_kc, flags, c["tile"], c["ksplit"], p(sc), sc.numel() * 4 if sc is not None else 0)
    return {"out": sha(out)}


def geglu_results(hip):
    M, H, K = GEGLU
    x, wgu = block(1, M, K).to(DEV), block(2, 2 * H, K, scale=K ** -0.5).to(DEV)
    out = {}
    for exp2 in (False, True):
        name = f"geglu/exp2={int(exp2)}"
        _assert_route(hip, name, [(15, 1, NONE, 0, 0)], M=M, N=2 * H, K=K, lda=K, ldb=K, ldc=H, a=x.data_ptr(), b=wgu.data_ptr(),
                      flags=hip.GEMM_GEGLU | (hip.GEMM_GELU_EXP2 if exp2 else 0))
        out[name] = {"act": sha(hip.linear_geglu(x, wgu, exp2=exp2))}
    return out


def fp8_results(hip):
    out = {}
    sa, sb = torch.tensor([3.0], device=DEV), torch.tensor([5.0], device=DEV)
    for M, N, K in FP8_SHAPES:
        d = {n: t.to(DEV) for n, t in fp8_blocks(M, N, K).items()}
        y = torch.zeros(M, N + 8, dtype=torch.bfloat16, device=DEV)
        hip.gemm_fp8(d["a8"], sa, d["b8"], sb, out=y[:, :N], residual=d["res"][:, :N])
        acc = d["c0"].clone()
        hip.gemm_fp8(d["a8"], sa, d["b8"], sb, out=acc[:, :N], accum=True, alpha=0.5)
        out[f"fp8/{M}x{N}x{K}"] = {"bf16_residual": sha(y), "f32_accum": sha(acc)}
    return out


def group_results(hip, group, scratch):
    if group == "geglu":
        return geglu_results(hip)
    if group == "fp8":
        return fp8_results(hip)
    return {c["name"]: run_gemm(hip, c, scratch) for c in gemm_cases() if c["group"] == group}


def make_scratch():
    return torch.empty(SCRATCH_FLOATS, dtype=torch.float32, device=DEV)


@pytest.fixture(scope="module")
def golden():
    g = json.loads(FIXTURE.read_text())
    got = input_hashes()
    bad = sorted(k for k in g["inputs"] if got.get(k) != g["inputs"][k])
    assert not bad and len(got) == len(g["inputs"]), (
        f"the CPU generators of torch {torch.__version__} do not reproduce the inputs the fixture was recorded on (torch {g['torch']}): {bad}")
    yield g["results"]
    operands.cache_clear()


@pytest.fixture(scope="module")
def scratch(hip):
    return make_scratch()


def test_fixture_is_complete(golden):
    names = [c["name"] for c in gemm_cases()] + ["geglu/exp2=0", "geglu/exp2=1"] + ["fp8/%dx%dx%d" % s for s in FP8_SHAPES]
    assert len(set(names)) == len(names) and sorted(golden) == sorted(names)


@pytest.mark.parametrize("group", GROUPS)
def test_gemm_bits(hip, golden, scratch, group):
    got = group_results(hip, group, scratch)
    bad = [f"{case}: {name}" for case, arrays in got.items() for name, v in arrays.items() if golden.get(case, {}).get(name) != v]
    assert not bad, f"outputs that are no longer the recorded bits (case: array): {bad}"
    assert all(set(golden[case]) == set(arrays) for case, arrays in got.items())
