"""tools/gen_gemm_asm.py as a module: its output is the committed lap_amd/csrc/gemm_asm_kernels.s, every schedule option still
writes what the generator of commit a8e35a8 wrote (tests/golden/gemm_asm_variants_v1.json, made by that commit's script:
tests/golden/make_gemm_asm_variants_golden.py), the kernel table rejects what cannot be emitted, and the register map is checked."""
import ast
import dataclasses
import hashlib
import importlib.util
import json
import pathlib
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
SCRIPT = ROOT / "tools" / "gen_gemm_asm.py"
COMMITTED = (ROOT / "lap_amd" / "csrc" / "gemm_asm_kernels.s").read_text()
GOLDEN = json.loads((ROOT / "tests" / "golden" / "gemm_asm_variants_v1.json").read_text())


def _load(name="gen_gemm_asm_under_test"):
    spec = importlib.util.spec_from_file_location(name, SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod         # (dataclasses looks the defining module up by name)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gen():
    return _load()


def test_default_output_is_the_committed_file_and_repeats(gen):
    first = gen.generate()
    assert first == COMMITTED
    assert gen.generate() == first          # no state survives a call (label numbers, emitted lines)
    assert gen.generate(gen.Options()) == first


@pytest.mark.parametrize("variant", sorted(GOLDEN))
def test_every_kept_option_writes_what_the_parent_wrote(gen, variant):
    assert len(GOLDEN) == 15
    env = {} if variant == "default" else dict([variant.split("=", 1)])
    out = gen.generate(gen.Options.from_env(env))
    assert hashlib.sha256(out.encode()).hexdigest() == GOLDEN[variant], variant
    if variant != "default":
        assert out != COMMITTED             # a kept option changes the output


def test_removed_ablations_are_rejected(gen):
    for token in ("noepi", "fullline"):
        with pytest.raises(ValueError):
            gen.Options(abl={token})


def test_kernel_table(gen):
    K, L, O, Ep = gen.KernelSpec, gen.Layout, gen.Out, gen.Epilogue
    assert [k.name for k in gen.KERNELS] == [
        "lap_gemm_asm_nt", "lap_gemm_asm_nn", "lap_gemm_asm_tn", "lap_gemm_asm_nt_bias", "lap_gemm_asm_tn_t", "lap_gemm_asm_nt_res",
        "lap_gemm_asm_nt_bias_res", "lap_gemm_asm_nn_geglu_bwd", "lap_gemm_asm_nt_geglu", "lap_gemm_asm_nn_gelu_bwd",
        "lap_gemm_asm_nt_bias_gelu", "lap_gemm_asm_tn_b16", "lap_gemm_asm_tn_t_b16"]
    for k in gen.KERNELS:                   # every spec constructs again from its own fields
        assert K(**dataclasses.asdict(k)) == k
    with pytest.raises(TypeError):
        K("lap_gemm_asm_nt", L.NT)          # keyword-only
    illegal = {
        "ring with a K-contiguous operand": dict(layout=L.NT, ring=True),
        "geglu_fwd on a layout other than nt": dict(layout=L.NN, epilogue=Ep.GEGLU_FWD),
        "sum of squares with a fused epilogue": dict(layout=L.NT, epilogue=Ep.BIAS, sumsq=True),
        "f32 output with a second operand": dict(layout=L.NT, out=O.F32, epilogue=Ep.RES),
        "transposed stores with a bias": dict(layout=L.TN, epilogue=Ep.BIAS, transposed_out=True),
    }
    for why, fields in illegal.items():
        try:
            K(name="illegal", **fields)
        except ValueError:
            continue
        pytest.fail(f"accepted: {why}")
    nvgpr = {k.name: k.nvgpr for k in gen.KERNELS}
    assert nvgpr.pop("lap_gemm_asm_nn_geglu_bwd") == 256 and set(nvgpr.values()) == {224}
    assert {k.name for k in gen.KERNELS if k.ragged_n} == {"lap_gemm_asm_nt_bias", "lap_gemm_asm_nt_bias_res", "lap_gemm_asm_nt_bias_gelu"}
    assert {k.name for k in gen.KERNELS if k.second_operand} == {
        "lap_gemm_asm_nt_res", "lap_gemm_asm_nt_bias_res", "lap_gemm_asm_nn_geglu_bwd", "lap_gemm_asm_nn_gelu_bwd"}
    assert {k.name for k in gen.KERNELS if k.stages_f32} == {k.name for k in gen.KERNELS if k.second_operand or k.f32}


def test_register_map_is_checked(gen):
    for k in gen.KERNELS:
        gen.check_register_map(k)
    nt = gen.KERNELS[0]
    # a main-loop name on the register of the lane's store offset (live from the epilogue-address step to the end)
    with pytest.raises(gen.RegisterOverlap, match="V_BAD"):
        gen.check_register_map(nt, vgprs=gen.VGPRS + (gen.Reg("V_BAD", gen.V_CO, 1, "main loop"),))
    # the same registers in a scope that is over before V_CO is written: no overlap
    gen.check_register_map(nt, vgprs=gen.VGPRS + (gen.Reg("V_EARLY", gen.V_CO, 1, "args+clear"),))
    # a variant's register only counts in the kernels that have it
    bad = gen.VGPRS + (gen.Reg("V_BAD", gen.V_CO, 1, "epilogue", "geglu_fwd"),)
    gen.check_register_map(nt, vgprs=bad)
    with pytest.raises(gen.RegisterOverlap):
        gen.check_register_map(next(k for k in gen.KERNELS if k.geglu_fwd), vgprs=bad)
    with pytest.raises(gen.RegisterOverlap, match="224"):
        gen.check_register_map(nt, vgprs=gen.VGPRS + (gen.Reg("V_HIGH", 224, 1, "always"),))
    with pytest.raises(gen.RegisterOverlap, match="102"):
        gen.check_register_map(nt, sgprs=gen.SGPRS + (gen.Reg("S_HIGH", 102, 1, "always"),))
    # the stated exceptions are overlaps the check does see
    assert gen.EXCEPTIONS
    with pytest.raises(gen.RegisterOverlap):
        gen.check_register_map(next(k for k in gen.KERNELS if k.bias_res), exceptions={})


def test_environment_is_read_in_main_only(monkeypatch):
    monkeypatch.setenv("ASM_ABL", "nodma")
    monkeypatch.setenv("ASM_RING", "0")
    assert _load("gen_gemm_asm_env_probe").generate() == COMMITTED
    tree = ast.parse(SCRIPT.read_text())
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    inside = {id(n) for n in ast.walk(main)}
    for n in ast.walk(tree):
        uses_os = (isinstance(n, ast.Name) and n.id == "os") or (isinstance(n, ast.Import) and any(a.name == "os" for a in n.names)) \
            or (isinstance(n, ast.ImportFrom) and n.module == "os")
        if uses_os:
            assert id(n) in inside, f"line {n.lineno}: the environment is main()'s business"
