// Stand-alone driver of the GEMM route planner (lap_amd/csrc/gemm_route.hpp), for runs under host sanitizers and for recording
// tests/golden/gemm_routes_v1.json (tests/golden/make_gemm_routes_golden.py writes the case lines):
//   c++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -g tools/gemm_route_plan.cpp -o gemm_route_plan
// stdin, one call per line: A B C bias residual (pointer values, 0 = null) M N K lda ldb ldc ldr alpha a_kc b_kc flags tile ksplit
// scratch (pointer value) scratch_bytes switches.  stdout, one line per call: rc n_legs, then 16 integers per leg: engine M N off_a
// off_b off_c off_bias off_res ksplit tile_base tile_count sub256 part_compact f32_tile part reduce.
#include <cstdio>

#include "../lap_amd/csrc/gemm_route.hpp"

int main() {
  char line[1024];
  while (fgets(line, sizeof line, stdin)) {
    lap_route::Call c = {};
    unsigned long long A, B, C, bias, res, scratch;
    if (sscanf(line, "%llu %llu %llu %llu %llu %d %d %d %d %d %d %d %f %d %d %d %d %d %llu %lld %u", &A, &B, &C, &bias, &res, &c.M, &c.N, &c.K, &c.lda,
               &c.ldb, &c.ldc, &c.ldr, &c.alpha, &c.a_kc, &c.b_kc, &c.flags, &c.tile, &c.ksplit, &scratch, &c.scratch_bytes, &c.sw) != 21) {
      fprintf(stderr, "bad line: %s", line);
      return 2;
    }
    c.A = (uintptr_t)A; c.B = (uintptr_t)B; c.C = (uintptr_t)C; c.bias = (uintptr_t)bias; c.res = (uintptr_t)res; c.scratch = scratch != 0;
    lap_route::Plan plan;
    const int rc = lap_route::plan_call(c, plan);
    printf("%d %d", rc, rc ? 0 : plan.n);
    for (int i = 0; !rc && i < plan.n; ++i) {
      const lap_gemm_leg& l = plan.legs[i];
      printf(" %d %d %d %lld %lld %lld %lld %lld %d %d %d %d %d %d %d %d", l.engine, l.M, l.N, l.off_a, l.off_b, l.off_c, l.off_bias, l.off_res, l.ksplit,
             l.tile_base, l.tile_count, l.sub256, l.part_compact, l.f32_tile, l.part, l.reduce);
    }
    printf("\n");
  }
  return 0;
}
