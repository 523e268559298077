"""Writes the cases of tests/golden/gemm_routes_v1.json and packs a recorder's answers into it.

The fixture records what lap_gemm_bf16_ex / lap_gemm_wgrad_* launched for each case at the commit BEFORE the routing moved into
csrc/gemm_route.hpp: that commit's launch functions were replaced (in a scratch copy) by lines that print what they were asked to
launch, and a small host program fed it the case lines below, one process per switch mask (the switches were per-process statics).
It is not meant to be regenerated from the current tree: a routing change edits the rows it means to change, by hand or with
tools/gemm_route_plan.cpp after review (same input and output format as the recorder).

  python tests/golden/make_gemm_routes_golden.py cases > cases.txt        # columns: tools/gemm_route_plan.cpp
  <recorder> < cases.txt > answers.txt
  python tests/golden/make_gemm_routes_golden.py pack cases.txt answers.txt

Row of the fixture: [M, N, K, lda, ldb, ldc, ldr, a_kc, b_kc, flags, tile, ksplit, bias, residual, scratch_bytes, switches, misalign,
alpha, rc, legs] with lda / ldb / ldc = 0 for a contiguous operand, bias / residual 0 (null) or 1, misalign = bytes added to A, and
each leg [engine, M, N, off_a, off_b, off_c, off_bias, off_res, ksplit, tile_base, tile_count, sub256, part_compact, f32_tile, part,
reduce] (include/lap_hip.h: lap_gemm_leg) with its trailing zeros left out.
"""
import json
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

F32, ACCUM, GELU, BIAS_F32, PARTIALS, GELU_BF16, GEGLU, EXP2 = 1, 2, 4, 8, 16, 32, 64, 128
SW = {"NO_ASM": 1, "NO_ASM_NN": 2, "NO_ASM_RES": 4, "NO_MSPLIT": 8, "NO_MSPLIT_LONGK": 16, "NO_NSPLIT": 32, "NO_SERVING_TILES": 64,
      "NO_PINGPONG": 128, "NO_KTAIL": 256}
WGRAD_SUMSQ = 65536
BASE = {"A": 1 << 32, "B": 2 << 32, "C": 3 << 32, "bias": 4 << 32, "res": 5 << 32, "scratch": 6 << 32}
BIG = 160 * 1024 * 1024 * 4     # the scratch lap_amd.hip lends
FWD, DGRAD, WGRAD = (1, 1), (1, 0), (0, 0)


def case(M, N, K, layout=FWD, flags=0, tile=-1, ksplit=0, bias=0, res=0, scratch=BIG, sw=0, lda=0, ldb=0, ldc=0, ldr=None, mis=0, alpha=1):
    a_kc, b_kc = layout
    return [M, N, K, lda, ldb, ldc, (N if res else 0) if ldr is None else ldr, a_kc, b_kc, flags, tile, ksplit, bias, res, scratch, sw, mis, alpha]


def lds(row):
    M, N, K, lda, ldb, ldc = row[:6]
    a_kc, b_kc = row[7], row[8]
    return lda or (K if a_kc else M), ldb or (K if b_kc else N), ldc or N


def line(row):
    M, N, K, _, _, _, ldr, a_kc, b_kc, flags, tile, ksplit, bias, res, scratch, sw, mis, alpha = row
    lda, ldb, ldc = lds(row)
    return " ".join(str(v) for v in (BASE["A"] + mis, BASE["B"], BASE["C"], BASE["bias"] if bias else 0, BASE["res"] if res else 0, M, N, K, lda, ldb, ldc,
                                     ldr, alpha, a_kc, b_kc, flags, tile, ksplit, BASE["scratch"] if scratch else 0, scratch, sw))


def linear(rows, d_in, d_out, *, bias=0, res=0):
    """the three products of a linear layer d_in -> d_out over `rows` rows, f32 and bf16 weight gradients (+ folded sum of squares)"""
    out = [case(rows, d_out, d_in, FWD, BIAS_F32 if bias else 0, bias=bias, res=res), case(rows, d_in, d_out, DGRAD)]
    for f in (F32, 0):
        out += [case(d_out, d_in, rows, WGRAD, f), case(d_out, d_in, rows, WGRAD, f, sw=WGRAD_SUMSQ)]
    return out


def train_step(B):
    from lap_amd.config import get_config, get_gemma_config, get_siglip_config

    m = get_config("lap_bench").model
    g, a, s = get_gemma_config("gemma_2b"), get_gemma_config("gemma_300m"), get_siglip_config("So400m/14")
    patches = (m.image_size // s.patch) ** 2
    out = []
    for cfg, rows in ((g, B * (2 * patches + m.max_token_len)), (a, B * m.action_horizon)):
        qkv = (cfg.num_heads + 2 * cfg.num_kv_heads) * cfg.head_dim
        out += linear(rows, cfg.width, qkv) + linear(rows, cfg.num_heads * cfg.head_dim, cfg.width, res=1)
        out += linear(rows, cfg.width, 2 * cfg.mlp_dim) + linear(rows, cfg.mlp_dim, cfg.width, res=1)
    rows, mlp = B * 2 * patches, (s.mlp_dim + 127) // 128 * 128          # 4304 -> 4352
    out += linear(rows, s.width, 3 * s.width, bias=1) + linear(rows, s.width, s.width, bias=1, res=1)
    out += linear(rows, s.width, mlp, bias=1) + linear(rows, mlp, s.width, bias=1, res=1) + linear(rows, s.width, g.width, bias=1)
    return out


def cases():
    out = []
    for B in (32, 16, 2):
        out += train_step(B)
    for sc in (BIG, 0):
        # LM head: logits, data gradient (f32, accumulated hi / lo), embedding weight gradient
        out += [case(1504, 257152, 2048, FWD, scratch=sc), case(1504, 2048, 257152, DGRAD, scratch=sc), case(1504, 2048, 257152, DGRAD, F32 | ACCUM, scratch=sc),
                case(257152, 2048, 1504, WGRAD, F32, scratch=sc), case(257152, 2048, 1536, WGRAD, F32, scratch=sc), case(257152, 2048, 1536, WGRAD, 0, scratch=sc)]
        # serving prefill: 512 SigLIP rows, 560 Gemma rows
        for M in (512, 560):
            for N, K in ((3456, 1152), (1152, 1152), (4352, 1152), (1152, 4352), (2048, 1152), (2560, 2048), (2048, 2048), (32768, 2048), (2048, 16384), (8192, 1024)):
                out.append(case(M, N, K, scratch=sc))
            out += [case(M, 2048, 2048, res=1, scratch=sc), case(M, 3456, 1152, flags=BIAS_F32, bias=1, scratch=sc), case(M, 2048, 1152, flags=F32, scratch=sc)]
            out += [case(M, 32768, 2048, flags=GEGLU, ldc=16384, scratch=0), case(M, 32768, 2048, flags=GEGLU | EXP2, ldc=16384, scratch=0)]
    # thresholds, one below / at / above each
    Ms = [248, 256, 264, 504, 512, 520, 632, 640, 648, 760, 768, 776, 1016, 1024, 1032, 3840, 4088, 4096, 4104, 4352, 7936, 8192, 8448]
    Ks = [504, 512, 520, 1016, 1024, 1032, 1536, 1544, 2040, 2048, 2056, 2080, 2552, 2560, 2568, 4088, 4096, 4104, 16376, 16384, 16392]
    for sc in (BIG, 0):
        for layout, f in ((FWD, 0), (DGRAD, 0), (WGRAD, F32), (WGRAD, 0), (FWD, F32)):
            main = f == (F32 if layout == WGRAD else 0)
            for M in Ms:
                for N, K in ((2048, 2048), (1024, 4096))[:2 if main else 1]:
                    out.append(case(M, N, K, layout, f, scratch=sc))
            for K in Ks + ([2052, 4100] if layout == WGRAD else []):        # K % 8 != 0 exists where no operand is K-contiguous
                for M, N in ((17920, 2048), (560, 2048), (4096, 1152))[:3 if layout == FWD and main else 2 if main else 1]:
                    out.append(case(M, N, K, layout, f, scratch=sc))
        # t5 around 128 and 256, fill around 0.8 (204.8 of 256, 409.6 of 512) and 0.9 (230.4) on N = 256 columns of tiles
        for layout, f in ((FWD, 0), (DGRAD, 0), (WGRAD, F32)):
            for t in (127, 128, 129, 204, 205, 230, 231, 255, 256, 257, 409, 410, 460, 461):
                for K in (2048, 8192)[:2 if t in (204, 205, 409, 410, 460, 461) else 1]:
                    out.append(case(t * 256, 256, K, layout, f, scratch=sc))
                out.append(case(t * 256, 256, 2048, layout, f, scratch=sc, sw=WGRAD_SUMSQ) if layout == WGRAD else case(t * 256, 256, 2048, res=1, scratch=sc))
            for tm in (25, 26, 51, 52, 64, 70, 102, 128, 140):       # eight columns of tiles: the M cut needs (rounds * 256) % 8 == 0
                for K in (2048, 4096, 4224, 16384):
                    out.append(case(tm * 256, 2048, K, layout, f, scratch=sc))
            for tm in (68, 70, 77, 102):
                out.append(case(tm * 256, 1792, 2048, layout, f, scratch=sc))      # seven columns: (rounds * 256) % 7 != 0
        for tm in (26, 64, 70, 102, 140):
            for K in (2048, 4096, 16384):
                out += [case(tm * 256, 2048, K, res=1, scratch=sc), case(tm * 256, 2048, K, flags=BIAS_F32, bias=1, res=1, scratch=sc)]
        # ragged M with many rows
        for M in (65528, 65536, 65544, 65664, 65792, 131080, 257152):
            for layout, f in ((WGRAD, F32), (WGRAD, 0), (FWD, 0)):
                out.append(case(M, 1024, 1536, layout, f, scratch=sc))
        # N = 256 j + 128
        for N in (384, 640, 896, 1152, 1408, 1664, 1920, 2176, 2432):
            for M in (4088, 4096, 16384, 17920):
                for K in (2040, 2048, 4352):
                    out.append(case(M, N, K, scratch=sc))
            out += [case(16384, N, 4352, DGRAD, scratch=sc), case(16384, N, 4352, flags=BIAS_F32, bias=1, scratch=sc),
                    case(16384, N, 4352, flags=BIAS_F32, bias=1, res=1, scratch=sc), case(16384, N, 4352, bias=1, res=1, ldr=N + 8, scratch=sc)]
        # an N cut whose whole-tile part (6 x 116 = 696 tiles) leaves a 184-tile tail: too long a tail to split, the plan stays at two legs
        out += [case(29696, 1664, 8192, DGRAD, scratch=sc), case(29696, 1664, 8192, bias=1, scratch=sc)]
        # tail split: tails below / above 128 and 200 tiles, small scratch
        for t5m in (33, 40, 48, 56, 57, 58):                                         # x 8 columns: tails 8, 64, 128, 192, 200, 208
            for K in (1024, 2048, 2304, 8192):
                out.append(case(t5m * 256, 2048, K, DGRAD, scratch=sc))
            out += [case(t5m * 256, 2048, 8192, DGRAD, scratch=sc and 64 << 20), case(t5m * 256, 2040, 8192, DGRAD, ldc=2048, scratch=sc)]
    # epilogues
    for M, N, K in ((17920, 2048, 2048), (1600, 1024, 4096), (560, 2048, 2048), (16384, 1152, 4352)):
        for sc in (BIG, 0):
            out += [case(M, N, K, bias=1, scratch=sc), case(M, N, K, flags=BIAS_F32, bias=1, scratch=sc), case(M, N, K, res=1, scratch=sc),
                    case(M, N, K, res=1, ldr=N + 64, scratch=sc), case(M, N, K, flags=GELU | BIAS_F32, bias=1, scratch=sc),
                    case(M, N, K, flags=GELU | GELU_BF16, bias=1, scratch=sc), case(M, N, K, flags=F32 | ACCUM, scratch=sc),
                    case(M, N, K, WGRAD, F32 | ACCUM, scratch=sc), case(M, N, K, alpha=0.5, scratch=sc), case(M, N, K, lda=K + 64, ldc=N + 64, scratch=sc)]
        for ks in (1, 2, 4):
            out.append(case(M, N, K, flags=PARTIALS, ksplit=ks))
        # forced tile and ksplit
        for tile in (0, 2, 5, 6, 10, 12, 14, 15, 16, 17, 18, 19):
            out += [case(M, N, K, tile=tile), case(M, N, K, DGRAD, tile=tile, scratch=0)]
        for ks in (1, 2, 3, 8):
            out += [case(M, N, K, ksplit=ks), case(M, N, K, tile=6, ksplit=ks), case(M, N, K, WGRAD, F32 | ACCUM, ksplit=ks, scratch=0)]
        out += [case(M, N, K, tile=14, res=1), case(M, N, K, tile=14, flags=BIAS_F32, bias=1), case(M, N, K, tile=14, flags=BIAS_F32, bias=1, res=1)]
    # each switch, alone, over the shapes it can move
    shapes = [case(17920, 2048, 2048), case(17920, 2048, 2048, DGRAD), case(17920, 2048, 16384, res=1), case(17920, 32768, 2048), case(17920, 2048, 32768, DGRAD),
              case(16384, 2048, 2048, DGRAD), case(16384, 1152, 4352), case(16384, 3456, 1152, flags=BIAS_F32, bias=1), case(560, 2560, 2048), case(512, 3456, 1152),
              case(14592, 2048, 8192, DGRAD), case(14592, 2048, 8224, DGRAD), case(2048, 16384, 17920, WGRAD, F32), case(2048, 16384, 17920, WGRAD, F32, sw=WGRAD_SUMSQ),
              case(257152, 2048, 1536, WGRAD, F32), case(17920, 2048, 2048, res=1), case(16384, 2048, 2048, res=1)]
    for bit in SW.values():
        for r in shapes:
            out.append(r[:15] + [r[15] | bit] + r[16:])
    # rejected calls
    M, N, K = 1024, 1024, 1024
    out += [case(0, N, K), case(M, 0, K), case(M, N, 0), case(M, 1022, K), case(M, N, K, ldc=1026), case(M, N, K, lda=1028), case(M, N, K, ldb=1028),
            case(M, N, 1028), case(1028, N, K, WGRAD, F32), case(M, 1028, K, DGRAD), case(M, N, K, res=1, ldr=1026), case(M, N, K, mis=8),
            case(1 << 20, N, K), case(M, N, K, WGRAD, F32, lda=1 << 21), case(M, N, K, flags=ACCUM), case(M, N, K, flags=F32 | GELU), case(M, N, K, tile=20),
            case(M, N, K, tile=-2), case(M, N, K, ksplit=-1), case(M, N, K, flags=GEGLU, scratch=0), case(512, N, K, flags=GEGLU | F32, scratch=0),
            case(512, N, K, flags=GEGLU, bias=1, scratch=0), case(512, 1152, K, flags=GEGLU, scratch=0), case(512, N, K, flags=GEGLU, tile=16, scratch=0),
            case(512, N, K, DGRAD, flags=GEGLU, scratch=0), case(512, N, K, flags=GEGLU, ksplit=2, scratch=0), case(512, N, K, flags=GEGLU, alpha=2.0, scratch=0),
            case(M, N, K, tile=14, bias=1), case(M, N, K, tile=14, flags=F32), case(M, N, 1088, tile=14), case(M, N, K, ksplit=2, scratch=0),
            case(M, N, K, flags=F32 | ACCUM, ksplit=2, bias=1, scratch=0), case(M, N, K, ksplit=4, scratch=1 << 20), case(M, N, K, flags=PARTIALS, scratch=0),
            case(M, N, K, flags=PARTIALS, ksplit=0), case(M, N, K, flags=PARTIALS, ksplit=2, scratch=1 << 20), case(M, N, K, DGRAD, tile=15), case(M, N, K, WGRAD, F32, tile=17),
            case(M, N, 1028, WGRAD, F32, tile=10), case(M, N, 1028, WGRAD, F32, tile=12), case(M, N, 1028, WGRAD, F32, tile=5), case(M, N, K, tile=7), case(M, N, K, tile=13),
            case(M, N, K, tile=1), case(M, N, K, tile=3), case(M, N, K, tile=4), case(M, N, K, tile=8), case(M, N, K, tile=9), case(M, N, K, tile=11)]
    seen, uniq = set(), []
    for r in out:
        if tuple(r) not in seen:
            seen.add(tuple(r))
            uniq.append(r)
    return uniq


def _trim(leg):
    while leg and leg[-1] == 0:
        leg = leg[:-1]
    return leg


def main():
    if sys.argv[1] == "cases":
        for r in cases():
            print(line(r))
        return
    rows = cases()
    lines, answers = pathlib.Path(sys.argv[2]).read_text().splitlines(), pathlib.Path(sys.argv[3]).read_text().splitlines()
    assert lines == [line(r) for r in rows] and len(answers) == len(rows)
    packed = []
    for r, a in zip(rows, answers):
        v = [int(x) for x in a.split()]
        assert len(v) == 2 + 16 * v[1]
        packed.append(r + [v[0], [_trim(v[2 + 16 * i:18 + 16 * i]) for i in range(v[1])]])
    text = "[\n" + ",\n".join(json.dumps(p, separators=(",", ":")) for p in packed) + "\n]\n"
    (ROOT / "tests" / "golden" / "gemm_routes_v1.json").write_text(text)
    print(len(packed), "rows,", len(text), "bytes")


if __name__ == "__main__":
    main()
