"""The training step's norm, elementwise, loss and optimizer kernels (csrc/norm.hip, csrc/elementwise.hip, csrc/loss_optim.hip)
element by element against float64 (GPU).

The references, the derivation of every bound and the inputs are in tests/train_reference.py; nothing there calls lap_amd.hip.
Every case puts all its buffers into one allocation between NaN guards and sentinels (train_reference.Arena), calls the C entry
point on views of it, and asserts: each element within its bound (or bit for bit where the reference is exact); every output
finite; the allocation byte for byte unchanged outside what the kernel owns: padding columns of the _ld forms, rows past
`rows`, the gate third of dmod, an EMA buffer whose flag is off.  Backward cases are fed the reference's own float32 rstd /
mean; one case per family chains the device's forward output instead.  Shapes are the smallest at which each mechanism exists.

The cases assume LAP_NORM_BWD_ROWS, LAP_SUMSQ_BLOCKS, LAP_ADAMW_BLOCKS, LAP_ADAMW_THREADS and LAP_STREAM_NT unset."""
import os

import pytest
import torch

from tests import train_reference as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}
BF, F32, I32, U8 = torch.bfloat16, torch.float32, torch.int32, torch.uint8
KNOBS = ("LAP_NORM_BWD_ROWS", "LAP_SUMSQ_BLOCKS", "LAP_ADAMW_BLOCKS", "LAP_ADAMW_THREADS", "LAP_STREAM_NT")


@pytest.fixture(scope="module", autouse=True)
def _module():
    set_ = [k for k in KNOBS if k in os.environ]
    if set_:
        pytest.skip(f"tuning knobs set: {set_}")
    yield
    for k, r in sorted(WORST.items()):        # docs/EXPERIMENTS.md quotes these
        print(f"{k}: worst error / bound {r:.3f}")
    T.drop_caches()
    torch.cuda.empty_cache()


class Session:
    """One arena on the device.  run(fn, written): calls fn(view) and asserts that only the named regions (and windows) changed."""

    def __init__(self, arena):
        self.host, self.reg = arena.build()
        self.dev = self.host.to(DEV)

    def v(self, name):
        return T.view(self.dev, self.reg[name])

    def p(self, name, col0=0):
        t = self.v(name)
        return t.data_ptr() + col0 * t.element_size()

    def run(self, fn, written, windows=(), tag=""):
        fn()
        torch.cuda.synchronize()
        got = self.dev.cpu()
        assert T.untouched(self.host, got, self.reg, written, windows), (tag, "wrote outside", written)
        self.host = got
        return got

    def out(self, name):
        return T.view(self.host, self.reg[name]).double()


def check(kernel, got, ref, tag):
    r, b = ref
    got = got.reshape(r.shape)
    assert bool(torch.isfinite(got).all()) or not bool(torch.isfinite(r).all()), (tag, "not finite")
    if b is None:
        assert torch.equal(got.double(), r.double()), (tag, "not bit for bit")
        ratio = 0.0
    else:
        ratio = T.worst_ratio(got, r, b.clamp(min=1e-300))
        print(f"{tag}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0, (tag, ratio)
    WORST[kernel] = max(WORST.get(kernel, 0.0), ratio)


def _id(s):
    return "-".join(str(x) for x in s)


# ===================================================================================================== normalisation
def _norm_arena(c, accum):
    s = c["spec"]
    a = T.Arena()
    for n in ("x", "dy"):
        a.add(n, BF, s.rows, s.D, data=c[n])
    a.add("y", BF, s.rows, s.D, out=True).add("dx", BF, s.rows, s.D, out=True, data=c["old"] if accum else None)
    a.add("rstd", F32, 1, s.rows, out=True).add("mean", F32, 1, s.rows, out=True)
    if s.kind == "rms":
        a.add("scale", F32, 1, s.D, data=c["scale"]).add("dscale", F32, 1, s.D, out=True, data=c["dscale0"])
    elif s.kind == "ada":
        a.add("mod", BF, s.B, 3 * s.D, rs=3 * s.D + s.pad, data=c["mod"]).add("dmod", F32, s.B, 3 * s.D, out=True, data=c["dmod0"])
    else:
        a.add("gamma", F32, 1, s.D, data=c["gamma"]).add("beta", F32, 1, s.D, data=c["beta"])
        for n in ("dgamma", "dbeta", "dxsum"):
            a.add(n, F32, 1, s.D, out=True, data=c[n + "0"])
    return a


def _rms(hip, spec, chain=False):
    c = T.norm_case(spec)
    ada = spec.kind == "ada"
    fam = "rmsnorm_ada" if ada else "rmsnorm"
    for accum in T.accum_modes(spec.D):
        S = Session(_norm_arena(c, accum))
        tag = f"{spec} accum {accum}"
        sc, mod = (None, S.p("mod")) if ada else (S.p("scale"), None)
        ld = S.reg["mod"].rs if ada else 0
        S.run(lambda: hip.call("lap_rmsnorm_fwd", S.p("x"), sc, mod, S.p("y"), S.p("rstd"), spec.rows, spec.D, spec.rps, ld, 1e-6), ["y", "rstd"], tag=tag)
        ref = T.ref_rms_fwd(c)
        check(fam + "_fwd y", S.out("y"), ref["y"], tag + " y")
        check(fam + "_fwd rstd", S.out("rstd"), ref["rstd"], tag + " rstd")
        rstd32 = S.out("rstd").float().view(-1) if chain else ref["rstd"][0].float()
        S.v("rstd").copy_(rstd32.view(1, -1))
        S.host = S.dev.cpu()
        if ada:
            S.run(lambda: hip.call("lap_rmsnorm_bwd", S.p("x"), None, mod, S.p("rstd"), S.p("dy"), S.p("dx"), None, S.p("dmod"), spec.rows, spec.D,
                                   spec.rps, ld, 3 * spec.D, int(accum)), ["dx"], [T.sub(S.reg["dmod"], width=2 * spec.D)], tag)     # the gate third stays
        else:
            S.run(lambda: hip.call("lap_rmsnorm_bwd", S.p("x"), sc, None, S.p("rstd"), S.p("dy"), S.p("dx"), S.p("dscale"), None, spec.rows, spec.D,
                                   0, 0, 0, int(accum)), ["dx", "dscale"], tag=tag)
        ref = T.ref_rms_bwd(c, rstd32, accum)
        check(fam + "_bwd dx", S.out("dx"), ref["dx"], tag + " dx")
        n = "dmod" if ada else "dscale"
        check(fam + "_bwd " + n, S.out(n), ref[n], tag + " " + n)


@pytest.mark.parametrize("spec", T.norm_specs("rms"), ids=_id)
def test_rmsnorm(hip, spec):
    _rms(hip, spec)


@pytest.mark.parametrize("spec", T.norm_specs("ada"), ids=_id)
def test_rmsnorm_adaptive(hip, spec):
    _rms(hip, spec)


@pytest.mark.parametrize("D", [64, 1152, 2048])
def test_rmsnorm_adaptive_shared_row(hip, D):
    """mod_ld = 0: every sample reads modulation row 0 (forward only: the backward has one dmod row per sample)."""
    spec = T.NormCase("ada", D, 15, 3, 5, 8)
    c = T.norm_case(spec)
    S = Session(_norm_arena(c, False))
    S.run(lambda: hip.call("lap_rmsnorm_fwd", S.p("x"), None, S.p("mod"), S.p("y"), S.p("rstd"), spec.rows, D, spec.rps, 0, 1e-6), ["y", "rstd"])
    check("rmsnorm_ada_fwd y", S.out("y"), T.ref_rms_fwd(c, shared=True)["y"], f"{spec} shared")


@pytest.mark.parametrize("spec", [T.NormCase("rms", 1152, 67), T.NormCase("ada", 1152, 15, 3, 5, 8)], ids=_id)
def test_rmsnorm_backward_chained_to_device_forward(hip, spec):
    _rms(hip, spec, chain=True)


def _ln(hip, spec, chain=False):
    c = T.norm_case(spec)
    D, rows = spec.D, spec.rows
    for accum in T.accum_modes(D):
        for with_sum in (False, True) if D <= 1152 else (False,):
            S = Session(_norm_arena(c, accum))
            tag = f"{spec} accum {accum} dxsum {with_sum}"
            S.run(lambda: hip.call("lap_layernorm_fwd", S.p("x"), S.p("gamma"), S.p("beta"), S.p("y"), S.p("mean"), S.p("rstd"), rows, D, 1e-6),
                  ["y", "mean", "rstd"], tag=tag)
            ref = T.ref_ln_fwd(c)
            for n in ("y", "mean", "rstd"):
                check("layernorm_fwd " + n, S.out(n), ref[n], f"{tag} {n}")
            if rows > 1:        # the constant row: variance clamped at 0, exactly
                assert float(S.out("mean")[0, 1]) == 1.5 and abs(float(S.out("rstd")[0, 1]) - 1000.0) <= 1000.0 * 4 * T.U
            mean32, rstd32 = (S.out(n).float().view(-1) for n in ("mean", "rstd")) if chain else (ref["mean"][0].float(), ref["rstd"][0].float())
            S.v("mean").copy_(mean32.view(1, -1))
            S.v("rstd").copy_(rstd32.view(1, -1))
            S.host = S.dev.cpu()
            S.run(lambda: hip.call("lap_layernorm_bwd_sum", S.p("x"), S.p("gamma"), S.p("mean"), S.p("rstd"), S.p("dy"), S.p("dx"), S.p("dgamma"),
                                   S.p("dbeta"), S.p("dxsum") if with_sum else None, rows, D, int(accum)),
                  ["dx", "dgamma", "dbeta"] + (["dxsum"] if with_sum else []), tag=tag)
            ref = T.ref_ln_bwd(c, mean32, rstd32, accum)
            for n in ("dx", "dgamma", "dbeta"):
                check("layernorm_bwd " + n, S.out(n), ref[n], f"{tag} {n}")
            if with_sum:        # the column sums of the dx as stored
                check("layernorm_bwd dxsum", S.out("dxsum"), T.ref_dxsum(S.out("dx"), c["dxsum0"], rows), tag + " dxsum")


@pytest.mark.parametrize("spec", T.norm_specs("ln"), ids=_id)
def test_layernorm(hip, spec):
    _ln(hip, spec)


def test_layernorm_backward_chained_to_device_forward(hip):
    _ln(hip, T.NormCase("ln", 1152, 35), chain=True)


def test_norm_argument_checks(hip):
    """dxsum needs 3 x 4 x D floats of shared memory: above 64 KiB (D = 1536, 2048) the call is rejected; D = 2056 (a fifth chunk
    per lane) is rejected by every entry point.  Nothing is written."""
    for D in (1536, 2048):
        S = Session(_norm_arena(T.norm_case(T.NormCase("ln", D, 5)), False))
        with pytest.raises(hip.LapHipError, match="1001"):
            S.run(lambda: hip.call("lap_layernorm_bwd_sum", S.p("x"), S.p("gamma"), S.p("mean"), S.p("rstd"), S.p("dy"), S.p("dx"), S.p("dgamma"),
                                   S.p("dbeta"), S.p("dxsum"), 5, D, 0), [])
        S.run(lambda: None, [])
    D = 2056
    x = T.norm_case(T.NormCase("rms", 2048, 5))["x"]          # 5 x 2048 elements hold 4 rows of 2056
    a = T.Arena()
    for n in ("x", "dy", "y", "dx"):
        a.add(n, BF, 5, 2048, data=x, out=n in ("y", "dx"))
    for n in ("p0", "p1", "g0", "g1", "st0", "st1"):
        a.add(n, F32, 1, D, data=torch.ones(D), out=n[0] == "g")
    S = Session(a)
    calls = [("lap_rmsnorm_fwd", (S.p("x"), S.p("p0"), None, S.p("y"), S.p("st0"), 4, D, 0, 0, 1e-6)),
             ("lap_rmsnorm_bwd", (S.p("x"), S.p("p0"), None, S.p("st0"), S.p("dy"), S.p("dx"), S.p("g0"), None, 4, D, 0, 0, 0, 0)),
             ("lap_layernorm_fwd", (S.p("x"), S.p("p0"), S.p("p1"), S.p("y"), S.p("st0"), S.p("st1"), 4, D, 1e-6)),
             ("lap_layernorm_bwd_sum", (S.p("x"), S.p("p0"), S.p("st0"), S.p("st1"), S.p("dy"), S.p("dx"), S.p("g0"), S.p("g1"), None, 4, D, 0))]
    for name, args in calls:
        with pytest.raises(hip.LapHipError, match="1001"):
            hip.call(name, *args)
    S.run(lambda: None, [])


# ============================================================================================================== RoPE
def _rope_arena(c):
    s = c["spec"]
    rows = s.B * s.T_seg
    a = T.Arena().add("qkv", BF, rows, (s.NH + 2) * s.HD, data=c["qkv"]).add("pos", I32, s.B, s.T_total, data=c["pos"])
    a.add("q", BF, rows, s.NH * s.HD, out=True).add("k", BF, rows, s.HD, out=True).add("v", BF, rows, s.HD, out=True)
    for n in ("dq", "dk", "dv"):
        a.add(n, BF, rows, c[n].shape[1], data=c[n])
    return a.add("dqkv", BF, rows, (s.NH + 2) * s.HD, out=True)


def _rope(hip, spec, backward=True):
    c = T.rope_case(spec)
    S = Session(_rope_arena(c))
    geo = (spec.B, spec.T_seg, spec.T_total, spec.seg_off, spec.NH, spec.HD, float(spec.q_scale))
    S.run(lambda: hip.call("lap_rope_split_fwd", S.p("qkv"), S.p("pos"), S.p("q"), S.p("k"), S.p("v"), *geo), ["q", "k", "v"], tag=str(spec))
    ref = T.ref_rope_fwd(c)
    for n in ("q", "k", "v"):
        check("rope_split_fwd " + n, S.out(n), ref[n], f"{spec} {n}")
    if backward:
        S.run(lambda: hip.call("lap_rope_split_bwd", S.p("dq"), S.p("dk"), S.p("dv"), S.p("pos"), S.p("dqkv"), *geo), ["dqkv"], tag=str(spec))
        check("rope_split_bwd dqkv", S.out("dqkv"), T.ref_rope_bwd(c)["dqkv"], f"{spec} dqkv")
    return S


@pytest.mark.parametrize("spec", T.ROPE_SMALL, ids=_id)
def test_rope_split(hip, spec):
    _rope(hip, spec)


def test_rope_split_row_form_and_switch(hip):
    """4096 rows x HD 256 is the smallest shape of the per-row forward form (B T_seg HD / 16 = 65536).  The same rows in two calls of
    2048 run the per-(row, head) form below the switch: both sides must agree bit for bit."""
    spec = T.ROPE_ROWFORM
    S = _rope(hip, spec)
    c = T.rope_case(spec)
    half = T.RopeCase(spec.HD, spec.NH, 1, 2048, 4096, 0, spec.q_scale)
    outs = []
    for h in range(2):
        ch = dict(c, spec=half, qkv=c["qkv"][h * 2048:(h + 1) * 2048], dq=c["dq"][:2048], dk=c["dk"][:2048], dv=c["dv"][:2048])
        Sh = Session(_rope_arena(ch))
        Sh.run(lambda: hip.call("lap_rope_split_fwd", Sh.p("qkv"), Sh.p("pos", h * 2048), Sh.p("q"), Sh.p("k"), Sh.p("v"), 1, 2048, 2048, 0, spec.NH,
                                spec.HD, float(spec.q_scale)), ["q", "k", "v"])
        outs.append([Sh.out(n) for n in ("q", "k", "v")])
    for i, n in enumerate(("q", "k", "v")):
        assert torch.equal(torch.cat([outs[0][i], outs[1][i]]), S.out(n)), n


# ===================================================================================================== GeGLU / GELU
@pytest.mark.parametrize("padded", [False, True])
@pytest.mark.parametrize("H,rows", T.GEGLU_SHAPES)
def test_geglu(hip, H, rows, padded):
    c = T.geglu_case(H, rows)
    lg, la, ld = (2 * H + 8, H + 16, 2 * H + 24) if padded else (2 * H, H, 2 * H)
    S = Session(T.Arena().add("gu", BF, rows, 2 * H, rs=lg, data=c["gu"]).add("dact", BF, rows, H, rs=la, data=c["dact"])
                .add("act", BF, rows, H, rs=la, out=True).add("dgu", BF, rows, 2 * H, rs=ld, out=True))
    tag = f"geglu H {H} rows {rows} padded {padded}"
    if padded:
        S.run(lambda: hip.call("lap_geglu_fwd_ld", S.p("gu"), S.p("act"), rows, H, lg, la), ["act"], tag=tag)
    else:
        S.run(lambda: hip.call("lap_geglu_fwd", S.p("gu"), S.p("act"), rows, H), ["act"], tag=tag)
    check("geglu_fwd", S.out("act"), T.ref_geglu_fwd(c)["act"], tag + " act")
    if padded:
        S.run(lambda: hip.call("lap_geglu_bwd_ld", S.p("gu"), S.p("dact"), S.p("dgu"), rows, H, lg, la, ld), ["dgu"], tag=tag)
    else:
        S.run(lambda: hip.call("lap_geglu_bwd", S.p("gu"), S.p("dact"), S.p("dgu"), rows, H), ["dgu"], tag=tag)
    check("geglu_bwd", S.out("dgu"), T.ref_geglu_bwd(c)["dgu"], tag + " dgu")


@pytest.mark.parametrize("H,rows", T.GEGLU_SHAPES)
def test_gelu(hip, H, rows):
    c = T.geglu_case(H, rows)
    x = c["gu"][:, :H].contiguous()
    S = Session(T.Arena().add("x", BF, rows, H, data=x).add("dy", BF, rows, H, data=c["dact"]).add("y", BF, rows, H, out=True).add("dx", BF, rows, H, out=True))
    S.run(lambda: hip.call("lap_gelu_fwd", S.p("x"), S.p("y"), rows * H), ["y"])
    check("gelu_fwd", S.out("y"), T.ref_gelu_fwd(x)["y"], f"gelu {H} {rows} y")
    S.run(lambda: hip.call("lap_gelu_bwd", S.p("x"), S.p("dy"), S.p("dx"), rows * H), ["dx"])
    check("gelu_bwd", S.out("dx"), T.ref_gelu_bwd(x, c["dact"])["dx"], f"gelu {H} {rows} dx")


# =================================================================================================== gated residual
@pytest.mark.parametrize("rps", T.GATED_RPS)
@pytest.mark.parametrize("D", [8, 264])
def test_gated_residual(hip, D, rps):
    c = T.gated_case(D, rps)
    rows, B = c["rows"], c["B"]
    a = T.Arena()
    for n in ("x", "u", "dy"):
        a.add(n, BF, rows, D, data=c[n])
    a.add("gate", BF, B, D, rs=3 * D + 8, data=c["gate"])
    a.add("y", BF, rows, D, out=True).add("du", BF, rows, D, out=True).add("dgate", F32, B, D, rs=D + 4, out=True)
    S = Session(a)
    tag = f"gated D {D} rps {rps}"
    S.run(lambda: hip.call("lap_gated_residual_fwd", S.p("x"), S.p("u"), S.p("gate"), S.p("y"), rows, D, rps, 3 * D + 8), ["y"], tag=tag)
    check("gated_residual_fwd", S.out("y"), T.ref_gated_fwd(c)["y"], tag + " y")
    S.run(lambda: hip.call("lap_gated_residual_fwd", S.p("x"), S.p("u"), None, S.p("y"), rows, D, 0, 0), ["y"], tag=tag)
    check("gated_residual_fwd", S.out("y"), T.ref_gated_fwd(c, False)["y"], tag + " y, no gate")
    S.run(lambda: hip.call("lap_gated_residual_bwd", S.p("dy"), S.p("u"), S.p("gate"), S.p("du"), S.p("dgate"), rows, D, rps, 3 * D + 8, D + 4),
          ["du", "dgate"], tag=tag)
    ref = T.ref_gated_bwd(c)
    check("gated_residual_bwd du", S.out("du"), ref["du"], tag + " du")
    check("gated_residual_bwd dgate", S.out("dgate"), ref["dgate"], tag + " dgate")


# ============================================================================= embedding, column sums, row copies
@pytest.mark.parametrize("D", [8, 264])
def test_embedding(hip, D):
    c = T.embed_case(D)
    rows = c["B"] * c["T"]
    S = Session(T.Arena().add("table", F32, c["hi"] - c["lo"], D, data=c["table"]).add("tok", I32, 1, rows, data=c["tok"])
                .add("stok", I32, 1, rows, data=c["stok"]).add("out", BF, c["B"] * c["rps"], D, out=True)
                .add("dout", BF, c["B"] * c["rps"], D, data=c["dout"]).add("dtable", F32, 6, D, out=True, data=c["dtable0"]))
    src = T.embed_src_rows(c)
    wins = [T.sub(S.reg["out"], int(r), 1) for r in src]
    S.run(lambda: hip.call("lap_embed_gather", S.p("table"), S.p("tok"), S.p("out"), rows, c["T"], D, c["rps"], c["off"], float(c["scale"]), c["lo"], c["hi"]),
          [], wins, "embed gather")
    check("embed_gather", S.out("out")[src], T.ref_embed_gather(c)["out"], f"embed_gather D {D}")
    S.run(lambda: hip.call("lap_embed_scatter_add", S.p("dtable"), S.p("stok"), S.p("dout"), rows, c["T"], D, c["rps"], c["off"], float(c["scale"])),
          ["dtable"], tag="embed scatter")
    check("embed_scatter_add", S.out("dtable"), T.ref_embed_scatter(c)["dtable"], f"embed_scatter_add D {D}")


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("rows,cols", T.colsum_shapes())
def test_colsum(hip, rows, cols, dtype):
    """A 16-byte aligned view (lanes whose 8 columns fit take the vector path, the last lane the scalar one when cols % 8 != 0)
    and views offset by 4 elements (bf16: 8 bytes, the scalar path; float32: still aligned) and by 2 (float32: the scalar path)."""
    c = T.colsum_case(rows, cols, dtype)
    ld = (cols + 7) // 8 * 8 + 8
    name = "lap_colsum_bf16" if dtype == BF else "lap_colsum_f32"
    for shift in (0, 4) + ((2,) if dtype == F32 else ()):
        S = Session(T.Arena().add("x", dtype, rows, cols, rs=ld, data=c["x"], shift=shift).add("out", F32, 1, cols, out=True, data=c["out0"]))
        S.run(lambda: hip.call(name, S.p("x"), S.p("out"), rows, cols, ld), ["out"], tag=f"colsum {rows} {cols} {shift}")
        check("colsum " + ("bf16" if dtype == BF else "f32"), S.out("out"), T.ref_colsum(c)["out"], f"colsum {rows}x{cols} {dtype} shift {shift}")


def test_copy_rows_and_copy2d(hip):
    g = T.gen("copies")
    B, Tn, D, srps, soff, drps, doff = 2, 3, 264, 7, 2, 5, 1
    src, dst0 = torch.randn(B * srps, D, generator=g).bfloat16(), torch.randn(B * drps, D, generator=g).bfloat16()
    r = torch.arange(B * Tn)
    srow, drow = (r // Tn) * srps + soff + r % Tn, (r // Tn) * drps + doff + r % Tn
    for accumulate in (False, True):
        S = Session(T.Arena().add("src", BF, B * srps, D, data=src).add("dst", BF, B * drps, D, out=True, data=dst0))
        S.run(lambda: hip.call("lap_copy_rows_bf16", S.p("src"), S.p("dst"), B * Tn, Tn, D, srps, soff, drps, doff, int(accumulate)), [],
              [T.sub(S.reg["dst"], int(x), 1) for x in drow], "copy_rows")
        ref = T.ref_copy_rows_accumulate(src[srow], dst0[drow]) if accumulate else (src[srow].double(), None)
        check("copy_rows_bf16", S.out("dst")[drow], ref, f"copy_rows accumulate {accumulate}")
    S = Session(T.Arena().add("src", BF, 37, 264, rs=272, data=torch.randn(37, 264, generator=g).bfloat16())
                .add("dst", BF, 37, 264, rs=288, out=True))
    want = S.v("src").cpu().double()
    S.run(lambda: hip.call("lap_copy2d_bf16", S.p("src"), S.p("dst"), 37, 264, 272, 288), ["dst"], tag="copy2d")
    check("copy2d_bf16", S.out("dst"), (want, None), "copy2d lds 272 ldd 288")


# =========================================================================================================== cross-entropy
def _ce_arena(c):
    R, V, ld = c["R"], c["V"], c["ld"]
    a = T.Arena().add("logits", F32, R, V, rs=ld, data=c["logits"]).add("target", I32, 1, R, data=c["target"]).add("w", F32, 1, R, data=c["w"])
    for tag in ("", "_a"):
        a.add("m" + tag, F32, 1, R, out=True, data=torch.full((R,), T.M_INIT)).add("l" + tag, F32, 1, R, out=True, data=torch.zeros(R))
        a.add("tl" + tag, F32, 1, R, out=True, data=torch.full((R,), T.TL_INIT))
    a.add("amax", I32, 1, R, out=True)
    return a.add("hi", BF, R, V, rs=ld + 3, out=True).add("lo", BF, R, V, rs=ld + 3, out=True).add("hi1", BF, R, V, rs=ld + 3, out=True)


@pytest.mark.parametrize("name", ["main", "odd"])
def test_cross_entropy_chunks(hip, name):
    """Chunk update with and without the argmax, then the gradient in both forms from the reference's own float32 (m, l): aligned
    f32x4 loads, the width-513 tail, a misaligned scalar chunk; widths 3, 1 and 2051; ties inside a thread, across lanes, waves and
    chunks; a target outside every chunk leaves tl alone; w = 0 rows give zeros."""
    c = T.ce_case(name)
    R, ld = c["R"], c["ld"]
    S = Session(_ce_arena(c))
    for v0, vc in c["chunks"]:
        S.run(lambda: hip.call("lap_ce_chunk_update", S.p("logits", v0), ld, S.p("target"), S.p("m"), S.p("l"), S.p("tl"), R, v0, vc), ["m", "l", "tl"], tag=name)
        S.run(lambda: hip.call("lap_ce_chunk_update_argmax", S.p("logits", v0), ld, S.p("target"), S.p("m_a"), S.p("l_a"), S.p("tl_a"), S.p("amax"), R, v0, vc),
              ["m_a", "l_a", "tl_a", "amax"], tag=name)
    ref = T.ref_ce_update(c)
    for n in ("m", "l", "tl"):
        check("ce_chunk_update " + n, S.out(n).view(-1), ref[n], f"ce {name} {n}")
        assert torch.equal(T.view(S.host, S.reg[n]), T.view(S.host, S.reg[n + "_a"])), (n, "the two instantiations differ")
    assert torch.equal(T.view(S.host, S.reg["amax"]).view(-1), ref["amax"][0]), (T.view(S.host, S.reg["amax"]), ref["amax"][0])
    WORST["ce_chunk_update_argmax amax"] = 0.0
    m32, l32 = ref["m"][0].float(), ref["l"][0].float()
    S.v("m").copy_(m32.view(1, -1))
    S.v("l").copy_(l32.view(1, -1))
    S.host = S.dev.cpu()
    ldd = ld + 3
    for v0, vc in c["chunks"]:
        wins = [T.sub(S.reg[n], col0=v0, width=vc) for n in ("hi", "lo", "hi1")]
        S.run(lambda: hip.call("lap_ce_chunk_grad", S.p("logits", v0), ld, S.p("target"), S.p("m"), S.p("l"), S.p("w"), S.p("hi1", v0), ldd, R, v0, vc), [], wins[2:], name)
        S.run(lambda: hip.call("lap_ce_chunk_grad_hilo", S.p("logits", v0), ld, S.p("target"), S.p("m"), S.p("l"), S.p("w"), S.p("hi", v0), S.p("lo", v0), ldd, R, v0, vc),
              [], wins[:2], name)
        ref_g = T.ref_ce_grad(c, m32, l32, v0, vc)
        hi, lo, hi1 = (S.out(n)[:, v0:v0 + vc] for n in ("hi", "lo", "hi1"))
        check("ce_chunk_grad", hi1, ref_g["hi"], f"ce {name} grad [{v0}, {v0 + vc})")
        check("ce_chunk_grad_hilo hi", hi, ref_g["hi"], f"ce {name} hilo hi [{v0}, {v0 + vc})")
        check("ce_chunk_grad_hilo hi+lo", hi + lo, ref_g["sum"], f"ce {name} hilo hi + lo [{v0}, {v0 + vc})")
        assert torch.equal(hi, hi1) and bool((hi[2] == 0).all()) and bool((lo[2] == 0).all())


@pytest.mark.parametrize("with_sel,with_masks", [(False, True), (True, True), (False, False)])
@pytest.mark.parametrize("Lm", T.METRIC_LM)
def test_token_metrics(hip, Lm, with_sel, with_masks):
    c = T.metrics_case(Lm, with_sel, with_masks)
    B, Ls = c["B"], c["Ls"]
    a = T.Arena().add("pred", I32, 1, B * Ls, data=c["pred"]).add("target", I32, 1, B * Ls, data=c["target"]).add("nll", F32, 1, B * Ls, data=c["nll"])
    a.add("lm", F32, B, Lm, data=c["lm"]).add("ptl", F32, B, Lm, out=True).add("counts", F32, B, 8, out=True)
    if with_sel:
        a.add("sel", I32, B, Ls, data=c["sel"])
    for n in ("crit", "num"):
        if c[n] is not None:
            a.add(n, U8, B, Lm, data=c[n].to(U8))
    S = Session(a)
    opt = lambda n: S.p(n) if n in S.reg else None      # noqa: E731
    S.run(lambda: hip.call("lap_token_metrics", S.p("pred"), S.p("target"), S.p("nll"), opt("sel"), Ls, S.p("lm"), opt("crit"), opt("num"), None, B, Lm,
                           S.p("ptl"), S.p("counts")), ["ptl", "counts"], tag=f"metrics {Lm}")
    ptl, counts = T.ref_token_metrics(c)
    check("token_metrics per_token_loss", S.out("ptl"), (ptl.double(), None), f"metrics Lm {Lm} sel {with_sel}")
    check("token_metrics counts", S.out("counts").view(B, 4, 2), (counts.double(), None), f"metrics Lm {Lm} counts")


@pytest.mark.parametrize("n", T.ARGMAX_N)
def test_argmax_rows(hip, n):
    x = T.argmax_case(n)
    S = Session(T.Arena().add("x", F32, 6, n, rs=n + 3, data=x).add("out", I32, 1, 6, out=True))
    S.run(lambda: hip.call("lap_argmax_rows_f32", S.p("x"), 6, n, n + 3, S.p("out")), ["out"], tag=f"argmax {n}")
    got = T.view(S.host, S.reg["out"]).view(-1)
    assert torch.equal(got, T.first_argmax(x)) and int(got[4]) == 0, (got, T.first_argmax(x))
    WORST["argmax_rows"] = 0.0


# ============================================================================================== sum of squares, AdamW
@pytest.mark.parametrize("n,dtype", [(n, F32) for n in T.SUMSQ_F32] + [(n, BF) for n in T.SUMSQ_BF16], ids=lambda x: str(x))
def test_sumsq(hip, n, dtype):
    c = T.sumsq_case(n, dtype)
    S = Session(T.Arena().add("x", dtype, 1, n, data=c["x"]).add("out", F32, 1, 1, out=True, data=c["out0"]))
    S.run(lambda: hip.call("lap_sumsq_f32" if dtype == F32 else "lap_sumsq_bf16", S.p("x"), n, S.p("out")), ["out"], tag=f"sumsq {n}")
    check("sumsq " + ("f32" if dtype == F32 else "bf16"), S.out("out").view(()), T.ref_sumsq(c)["out"], f"sumsq {n} {dtype}")


ADAM_MODES = [("clipped", "on", "f32"), ("below", "flag0", "f32"), ("off", "none", "f32"), ("clipped", "on", "bf16"), ("below", "on", "hilo"),
              ("off", "flag0", "nop16")]


@pytest.mark.parametrize("clip,ema,form", ADAM_MODES)
@pytest.mark.parametrize("n", T.ADAM_N)
def test_adamw_ema(hip, n, clip, ema, form):
    """form: the gradient as float32 / bf16; hilo: float32 gradient with the p16 / p16lo planes; nop16: p16 = NULL."""
    c = T.adam_case(n, clip, ema, BF if form == "bf16" else F32)
    h = T.ADAM_HP
    a = T.Arena()
    for k in ("p", "m", "v", "ema"):
        a.add(k, F32, 1, n, out=True, data=c[k])
    a.add("g", c["g"].dtype, 1, n, data=c["g"]).add("sc", F32, 1, 8, data=c["sc"]).add("p16", BF, 1, n, out=True).add("p16lo", BF, 1, n, out=True)
    S = Session(a)
    hp = (float(h["b1"]), float(h["b2"]), float(h["eps"]), float(h["wd"]), float(c["max_norm"]))
    e = None if ema == "none" else S.p("ema")
    tag = f"adamw n {n} {clip} {ema} {form}"
    written = ["p", "m", "v"] + (["ema"] if ema == "on" else []) + {"nop16": [], "hilo": ["p16", "p16lo"]}.get(form, ["p16"])
    if form == "hilo":
        fn = lambda: hip.call("lap_adamw_ema_hilo", S.p("p"), S.p("m"), S.p("v"), e, S.p("g"), S.p("p16"), S.p("p16lo"), n, S.p("sc"), *hp)      # noqa: E731
    else:
        fn = lambda: hip.call("lap_adamw_ema_g16" if form == "bf16" else "lap_adamw_ema", S.p("p"), S.p("m"), S.p("v"), e, S.p("g"),      # noqa: E731
                              None if form == "nop16" else S.p("p16"), n, S.p("sc"), *hp)
    S.run(fn, written, tag=tag)
    ref = T.ref_adamw(c)
    for k in ("p", "m", "v") + (("ema",) if ema == "on" else ()):
        check("adamw_ema " + k, S.out(k).view(-1), ref[k], f"{tag} {k}")
    hi, lo = T.p16_planes(T.view(S.host, S.reg["p"]).view(-1))
    if form != "nop16":
        check("adamw_ema p16", S.out("p16").view(-1), (hi, None), tag + " p16")
    if form == "hilo":
        check("adamw_ema_hilo p16lo", S.out("p16lo").view(-1), (lo, None), tag + " p16lo")
    if form == "bf16":      # the same pass on the widened gradient, bit for bit
        c2 = dict(c, g=c["g"].float())
        a2 = T.Arena()
        for k in ("p", "m", "v", "ema"):
            a2.add(k, F32, 1, n, out=True, data=c2[k])
        a2.add("g", F32, 1, n, data=c2["g"]).add("sc", F32, 1, 8, data=c["sc"]).add("p16", BF, 1, n, out=True)
        S2 = Session(a2)
        S2.run(lambda: hip.call("lap_adamw_ema", S2.p("p"), S2.p("m"), S2.p("v"), S2.p("ema"), S2.p("g"), S2.p("p16"), n, S2.p("sc"), *hp), ["p", "m", "v", "ema", "p16"])
        for k in ("p", "m", "v", "ema", "p16"):
            assert torch.equal(T.view(S.host, S.reg[k]), T.view(S2.host, S2.reg[k])), (tag, k, "bf16 pass differs from the widened float32 pass")
