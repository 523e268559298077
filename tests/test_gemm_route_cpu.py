"""The GEMM router on the CPU: lap_gemm_plan (csrc/gemm_route.hpp) against the routes recorded before the planner existed
(tests/golden/gemm_routes_v1.json, written by tests/golden/make_gemm_routes_golden.py), and properties every plan must have."""
import ctypes as C
import functools
import json
import pathlib

ROOT = pathlib.Path(__file__).resolve().parent.parent
F32, BIAS_F32, PARTIALS = 1, 8, 16
ASM, ASM_BIAS, ASM_RES, ASM_WGRAD_SUMSQ = 32, 33, 34, 35
WGRAD_SUMSQ = 65536
MAX_LEGS = 6
BASE = {"A": 1 << 32, "B": 2 << 32, "C": 3 << 32, "bias": 4 << 32, "res": 5 << 32, "scratch": 6 << 32}
LEG_FIELDS = ("engine", "M", "N", "off_a", "off_b", "off_c", "off_bias", "off_res", "ksplit", "tile_base", "tile_count", "sub256", "part_compact",
              "f32_tile", "part", "reduce")


class Leg(C.Structure):
    _fields_ = [(n, C.c_longlong) for n in ("off_a", "off_b", "off_c", "off_bias", "off_res")] + [
        (n, C.c_int) for n in ("engine", "M", "N", "ksplit", "tile_base", "tile_count", "sub256", "part_compact", "f32_tile", "part", "reduce")]


@functools.lru_cache(maxsize=None)
def _lib():
    from lap_amd.build import build

    lib = C.CDLL(str(build(verbose=False)))
    vp, i = C.c_void_p, C.c_int
    lib.lap_gemm_plan.argtypes = [vp] * 5 + [i] * 7 + [C.c_float] + [i] * 5 + [vp, C.c_longlong, C.c_uint, C.POINTER(Leg), i, C.POINTER(i)]
    for name in ("lap_gemm_asm_ok", "lap_gemm_asm_bias_ok", "lap_gemm_asm_res_ok"):
        getattr(lib, name).argtypes = [i] * {"lap_gemm_asm_ok": 9, "lap_gemm_asm_bias_ok": 6, "lap_gemm_asm_res_ok": 7}[name]
    return lib


@functools.lru_cache(maxsize=None)
def _rows():
    return json.loads((ROOT / "tests" / "golden" / "gemm_routes_v1.json").read_text())


def _plan(row, max_legs=MAX_LEGS):
    """(rc, legs as lists in LEG_FIELDS order, the call as a dict)"""
    M, N, K, lda, ldb, ldc, ldr, a_kc, b_kc, flags, tile, ksplit, bias, res, scratch, sw, mis, alpha = row[:18]
    call = dict(M=M, N=N, K=K, lda=lda or (K if a_kc else M), ldb=ldb or (K if b_kc else N), ldc=ldc or N, a_kc=a_kc, b_kc=b_kc, flags=flags,
                bias=bias, res=res, scratch=scratch, sw=sw)
    legs, n = (Leg * MAX_LEGS)(), C.c_int(-1)
    rc = _lib().lap_gemm_plan(BASE["A"] + mis, BASE["B"], BASE["C"], BASE["bias"] if bias else None, BASE["res"] if res else None, M, N, K, call["lda"],
                              call["ldb"], call["ldc"], ldr, alpha, a_kc, b_kc, flags, tile, ksplit, BASE["scratch"] if scratch else None, scratch, sw, legs,
                              max_legs, C.byref(n))
    return rc, [[getattr(legs[j], f) for f in LEG_FIELDS] for j in range(max(n.value, 0))], call


def test_fixture_covers_the_routes():
    rows = _rows()
    assert len(rows) > 2000 and all(len(r) == 20 for r in rows)
    engines = {leg[0] for r in rows for leg in r[19]}
    assert engines >= {0, 2, 5, 6, 10, 12, 15, 16, 17, 18, 19, ASM, ASM_BIAS, ASM_RES, ASM_WGRAD_SUMSQ}
    assert {(leg + [0] * 16)[15] for r in rows for leg in r[19]} == {0, 1, 2}        # no reduce, split-K reduce, tail reduce
    assert any((leg + [0] * 16)[11] for r in rows for leg in r[19])                   # the tail as quadrants of the 128 x 128 kernel
    assert {r[18] for r in rows} == {0, 1001} and {r[15] & 0xffff for r in rows} >= {0, 1, 2, 4, 8, 16, 32, 64, 128, 256}


def test_plan_reproduces_every_recorded_route():
    bad = []
    for row in _rows():
        rc, legs, _ = _plan(row)
        want = [leg + [0] * (16 - len(leg)) for leg in row[19]]
        if rc != row[18] or legs != want:
            bad.append((row[:18], rc, legs, row[18], want))
    assert not bad, f"{len(bad)} routes changed, first: {bad[0]}"


def _asm_ok(lib, leg, call):
    engine, M, N = leg[:3]
    K, lda, ldb, ldc = call["K"], call["lda"], call["ldb"], call["ldc"]
    if engine == ASM_BIAS:
        return lib.lap_gemm_asm_bias_ok(M, N, K, lda, ldb, ldc)
    if engine == ASM_RES:
        return lib.lap_gemm_asm_res_ok(call["bias"], M, N, K, lda, ldb, ldc)
    return lib.lap_gemm_asm_ok(call["a_kc"], call["b_kc"], call["flags"] & F32, M, N, K, lda, ldb, ldc)


def test_every_plan_is_sound():
    """Properties that need no fixture: the legs tile [0, M) x [0, N) exactly once, every assembly leg is eligible for its kernel,
    no leg needs more scratch than the caller lent, the leg count stays within the capacity."""
    lib = _lib()
    for row in _rows():
        rc, legs, call = _plan(row)
        if rc:
            continue
        assert 1 <= len(legs) <= MAX_LEGS
        M, N, ldc, ldr, a_kc, b_kc = call["M"], call["N"], call["ldc"], row[6], call["a_kc"], call["b_kc"]
        # sub-products as rectangles (m0, n0, m, n) read off the C offsets; all other offsets must name the same rectangle
        rects = {}
        for leg in legs:
            engine, m, n, off_a, off_b, off_c, off_bias, off_res, ksplit, tile_base, tile_count, sub256, part_compact, f32_tile, part, reduce = leg
            m0, n0 = divmod(off_c, ldc)
            assert off_a == (m0 * call["lda"] if a_kc else m0) and off_b == (n0 * call["ldb"] if b_kc else n0), (row, leg)
            assert off_bias == (n0 if call["bias"] else 0) and off_res == (m0 * ldr + n0 if call["res"] else 0), (row, leg)
            assert 0 <= m0 and m0 + m <= M and 0 <= n0 and n0 + n <= N and m > 0 and n > 0, (row, leg)
            t5 = -(-m // 256) * -(-n // 256)
            lo, hi = (tile_base, tile_base + tile_count) if tile_count else (0, t5)      # a launch covers tiles [lo, hi) of its rectangle
            assert 0 <= lo < hi <= t5 and (tile_count > 0 or not (tile_base or sub256 or part_compact)), (row, leg)
            rects.setdefault((m0, n0, m, n), []).append((lo, hi))
            if engine >= ASM:
                assert _asm_ok(lib, leg, call), (row, leg)
                assert engine != ASM_WGRAD_SUMSQ or (call["sw"] & WGRAD_SUMSQ and len(legs) == 1), (row, leg)
            need = 4 * ksplit * (tile_count * 65536 if part_compact else m * n) if part else 0
            assert need <= call["scratch"], (row, leg)
            assert (reduce != 0) <= bool(part) and (reduce == 2) == bool(part_compact) and (not part or f32_tile), (row, leg)
        for (m0, n0, m, n), spans in rects.items():           # each rectangle's tiles exactly once
            spans.sort()
            assert spans[0][0] == 0 and spans[-1][1] == -(-m // 256) * -(-n // 256) and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), (row, spans)
        # the rectangles: disjoint and of the whole area -> [0, M) x [0, N) exactly once
        rs = list(rects)
        assert sum(m * n for _, _, m, n in rs) == M * N, (row, rs)
        for i, (am, an, a_m, a_n) in enumerate(rs):
            for bm, bn, b_m, b_n in rs[i + 1:]:
                assert am + a_m <= bm or bm + b_m <= am or an + a_n <= bn or bn + b_n <= an, (row, rs)


def test_capacity_overflow_is_an_error_not_a_write():
    row = next(r for r in _rows() if len(r[19]) == 2)
    rc, legs, _ = _plan(row, max_legs=1)
    assert rc == 1001 and legs == []
    assert _plan(row, max_legs=2)[0] == 0
