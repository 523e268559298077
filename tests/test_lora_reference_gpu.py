"""The five kernels of csrc/lora.hip element by element against float64 (GPU).

The references, the derivation of every bound and cap and the seeded cases are in tests/lora_reference.py; nothing there calls
lap_amd.hip.  Every case puts all its buffers into one allocation between NaN guards and sentinels (train_reference.Arena), calls
the C entry point on pointers into it, and asserts: (a) each element of each output within its bound and finite, (b) for bf16
outputs the share of elements that differ from the reference at all under the case's cap, and the allocation byte for byte
unchanged outside the output window: guards, padding columns of every leading dimension, the inputs, and for lap_lora_wgrad a
scratch of exactly S * G*R * Ng floats.  One test per launcher walks its argument check clause by clause."""
import pytest
import torch

from tests import lora_reference as L

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _module():
    yield
    for k, (r, s) in sorted(WORST.items()):        # docs/EXPERIMENTS.md quotes these
        print(f"{k}: worst error / bound {r:.3f}" + ("" if s is None else f", largest differing share {s:.2e}"))
    L.drop_caches()
    torch.cuda.empty_cache()


class Session:
    """One arena on the device.  run(fn, written): calls fn() and asserts that only the named regions changed."""

    def __init__(self, arena):
        self.host, self.reg = arena.build()
        self.dev = self.host.to(DEV)

    def p(self, name):
        return L.view(self.dev, self.reg[name]).data_ptr()

    def run(self, fn, written, tag=""):
        fn()
        torch.cuda.synchronize()
        got = self.dev.cpu()
        assert L.untouched(self.host, got, self.reg, written), (tag, "wrote outside", written)
        self.host = got
        return got

    def out(self, name):
        return L.view(self.host, self.reg[name]).double()

    def bits(self, name):
        return L.view(self.host, self.reg[name]).clone()


def check(kernel, spec, out, got, ref):
    r, b = ref
    cap = L.cap(spec, out, r.numel())
    ratio, share = L.check_elementwise(got.reshape(r.shape), r, b.clamp(min=1e-300), cap, L.case_id(spec, out))
    w = WORST.get(kernel, (0.0, None if cap is None else 0.0))
    WORST[kernel] = (max(w[0], ratio), None if cap is None else max(w[1], share))


def _ids(cases):
    return [L.case_id(c) for c in cases]


# ================================================================================================================ down
@pytest.mark.parametrize("spec", L.DOWN_CASES, ids=_ids(L.DOWN_CASES))
def test_lora_down(hip, spec):
    """M = 1, K = 8: three of the four k-groups masked.  K = 48 / 72 / 88: K % 32 = 16 / 8 / 24, one column chunk with nt = 3; the
    same with ldx = K + 8, ldw = K + 16, ldt = G*R + 3.  R = 80 / 128: two column chunks, the second with nt = 1 / 4.  xg > 0: the
    data-gradient form (G = 3 with ldx wider than (G - 1) xg + K; G = 10 at the debug model's head width).  nsum = 8."""
    p, c = spec, L.make_case(spec)
    xw = (p.G - 1) * p.xg + p.K
    ldx, ldw, ldt = xw + p.px, p.K + p.pw, p.G * p.R + p.pt
    S = Session(L.Arena().add("x", BF, p.M, xw, rs=ldx, data=c["x"]).add("w", BF, p.nsum * p.G * p.R, p.K, rs=ldw, data=c["w"])
                .add("t", BF, p.M, p.G * p.R, rs=ldt, out=True))
    S.run(lambda: hip.call("lap_lora_down", S.p("x"), ldx, p.xg, S.p("w"), ldw, p.nsum, S.p("t"), ldt, p.M, p.K, p.G, p.R, float(p.s)), ["t"],
          L.case_id(p))
    check("lora_down", p, "t", S.out("t"), L.ref_down(c)["t"])


# ============================================================================================================== up_add
@pytest.mark.parametrize("spec", L.UP_CASES, ids=_ids(L.UP_CASES))
def test_lora_up_add(hip, spec):
    """M = 1 / 17 / 70: the last live thread row holds 1 / 1 / 2 of its 4 rows (the clamp and the break).  Ng = 8, G = 1: one column chunk.  G = 3,
    Ng = 40: 15 chunks in a 64-thread row (the early return).  G*Ng = 520: a second column block with one chunk.  R = 16, 24 (no
    multiple of 16), 320 (the dx-add form).  tw = 16: t wider than G*R behind a padded ldt.  ldy = G*Ng + 8, ldb = Ng + 8."""
    p, c = spec, L.make_case(spec)
    ldt, ldb, ldy = p.G * p.R + p.tw + p.pt, p.Ng + p.pb, p.G * p.Ng + p.py
    S = Session(L.Arena().add("t", BF, p.M, p.G * p.R, rs=ldt, data=c["t"]).add("b", BF, p.nsum * p.G * p.R, p.Ng, rs=ldb, data=c["b"])
                .add("y", BF, p.M, p.G * p.Ng, rs=ldy, out=True, data=c["y0"]))
    S.run(lambda: hip.call("lap_lora_up_add", S.p("t"), ldt, S.p("b"), ldb, p.nsum, S.p("y"), ldy, p.M, p.Ng, p.G, p.R, float(p.s)), ["y"],
          L.case_id(p))
    check("lora_up_add", p, "y", S.out("y"), L.ref_up_add(c)["y"])


# =============================================================================================================== wgrad
@pytest.mark.parametrize("f32_out", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("spec", L.WGRAD_CASES, ids=_ids(L.WGRAD_CASES))
def test_lora_wgrad(hip, spec, f32_out):
    """M = 1 / 31 / 32 / 33: the last MFMA step short.  M = 100, msplit = 1 .. 4: mchunk = 128 / 64 / 64 / 32, S = 1 / 2 / 2 / 4 (the last
    chunk holds 4 rows); the split and the unsplit result both meet their bounds.  Ng = 8 / 40 / 72: the c < Ng guards, a second
    column block with one live wave.  G = 3 with bg = Ng; R = 48: three row tiles in one group; ldo = Ng + 5 with padded lda / ldb.
    Every copy is bit-equal to copy 0, and a repeated call reproduces the bits."""
    p, c = spec, L.make_case(spec)
    GR, bw = p.G * p.R, (p.G - 1) * p.bg + p.Ng
    lda, ldb, ldo = GR + p.pa, bw + p.pb, p.Ng + p.po
    _, Sn = L.wgrad_split(p.M, p.msplit)
    a = L.Arena().add("a", BF, p.M, GR, rs=lda, data=c["a"]).add("b", BF, p.M, bw, rs=ldb, data=c["b"])
    a.add("out", F32 if f32_out else BF, p.ncopy * GR, p.Ng, rs=ldo, out=True)
    n_scratch = Sn * GR * p.Ng if Sn > 1 else 0
    if n_scratch:
        a.add("scratch", F32, 1, n_scratch, out=True)
    S = Session(a)
    written = ["out"] + (["scratch"] if n_scratch else [])
    fn = lambda: hip.call("lap_lora_wgrad", S.p("a"), lda, S.p("b"), ldb, p.bg, S.p("out"), ldo, p.ncopy, int(f32_out), p.M, p.Ng, p.G, p.R,      # noqa: E731
                          float(p.s), p.msplit, S.p("scratch") if n_scratch else None, n_scratch)
    S.run(fn, written, L.case_id(p))
    name = "out_f32" if f32_out else "out_bf16"
    check("lora_wgrad" + ("" if Sn == 1 else " + reduce") + (" f32" if f32_out else " bf16"), p, name, S.out("out"), L.ref_wgrad(c)[name])
    first = S.bits("out")
    for n in range(1, p.ncopy):
        assert torch.equal(first[n * GR:(n + 1) * GR], first[:GR]), (L.case_id(p), "copy", n)
    S.run(fn, written, L.case_id(p))
    assert torch.equal(S.bits("out"), first), (L.case_id(p), "a repeated call gave other bits")


# =============================================================================================================== merge
@pytest.mark.parametrize("spec", L.MERGE_CASES, ids=_ids(L.MERGE_CASES))
def test_lora_merge(hip, spec):
    """I = 4: one thread.  I = 1028: a second block with one thread.  Ng = 3, G = 2, R = 5: no alignment in Ng or R.  R = 16.  All four
    leading dimensions padded by the least the launcher accepts."""
    p, c = spec, L.make_case(spec)
    ldw, lda, ldb, ldo = p.I + p.pw, p.I + p.pa, p.Ng + p.pb, p.I + p.po
    S = Session(L.Arena().add("w", F32, p.G * p.Ng, p.I, rs=ldw, data=c["w"]).add("a", F32, p.G * p.R, p.I, rs=lda, data=c["a"])
                .add("b", F32, p.nsum * p.G * p.R, p.Ng, rs=ldb, data=c["b"]).add("weff", BF, p.G * p.Ng, p.I, rs=ldo, out=True))
    S.run(lambda: hip.call("lap_lora_merge", S.p("w"), ldw, S.p("a"), lda, S.p("b"), ldb, p.nsum, S.p("weff"), ldo, p.I, p.Ng, p.G, p.R, float(p.s)),
          ["weff"], L.case_id(p))
    check("lora_merge", p, "weff", S.out("weff"), L.ref_merge(c)["weff"])


# ===================================================================================================== argument checks
def _walk(hip, S, name, order, base, clauses):
    """The unchanged arguments are accepted; every clause alone is rejected on the host (LAP_ERR_ARG), nothing is launched and
    the arena stays byte for byte what it was."""
    for what, change in clauses:
        args = dict(base, **change)
        with pytest.raises(hip.LapHipError, match="1001"):
            hip.call(name, *[args[k] for k in order])
        S.run(lambda: None, [], f"{name}: {what}")
    return len(clauses)


def _sizes(names):
    return [(f"{n} = {v}", {n: v}) for n in names for v in (0, -16)]


def test_lora_down_argument_checks(hip):
    g = L.gen("args", "down")
    S = Session(L.Arena().add("x", BF, 5, 40, data=torch.randn(5, 40, generator=g)).add("w", BF, 64, 24, data=torch.randn(64, 24, generator=g))
                .add("t", BF, 5, 64, out=True))
    order = "X ldx xg W ldw nsum T ldt M K G R s".split()
    base = dict(X=S.p("x"), ldx=32, xg=16, W=S.p("w"), ldw=16, nsum=1, T=S.p("t"), ldt=64, M=5, K=16, G=2, R=16, s=1.0)
    clauses = [(f"{n} null", {n: None}) for n in "XWT"] + _sizes(["M", "K", "G", "R", "nsum"]) + [
        ("R % 16", dict(R=24)), ("K % 8", dict(K=12)), ("ldx % 8", dict(ldx=36)), ("xg % 8", dict(xg=12)), ("ldw % 8", dict(ldw=20)),
        ("ldx < (G - 1) xg + K", dict(ldx=24)), ("ldw < K", dict(ldw=8)), ("ldt < G R", dict(ldt=31)),
        ("X misaligned", dict(X=base["X"] + 2)), ("W misaligned", dict(W=base["W"] + 2))]
    assert _walk(hip, S, "lap_lora_down", order, base, clauses) == 23
    S.run(lambda: hip.call("lap_lora_down", *[base[k] for k in order]), ["t"])


def test_lora_up_add_argument_checks(hip):
    g = L.gen("args", "up_add")
    S = Session(L.Arena().add("t", BF, 5, 64, data=torch.randn(5, 64, generator=g)).add("b", BF, 64, 24, data=torch.randn(64, 24, generator=g))
                .add("y", BF, 5, 40, out=True, data=torch.randn(5, 40, generator=g)))
    order = "T ldt B ldb nsum Y ldy M Ng G R s".split()
    base = dict(T=S.p("t"), ldt=32, B=S.p("b"), ldb=16, nsum=1, Y=S.p("y"), ldy=32, M=5, Ng=16, G=2, R=16, s=1.0)
    clauses = [(f"{n} null", {n: None}) for n in "TBY"] + _sizes(["M", "Ng", "G", "R", "nsum"]) + [
        ("Ng % 8", dict(Ng=12)), ("ldb % 8", dict(ldb=20)), ("ldy % 8", dict(ldy=36)), ("ldb < Ng", dict(ldb=8)), ("ldy < G Ng", dict(ldy=24)),
        ("ldt < G R", dict(ldt=31)), ("B misaligned", dict(B=base["B"] + 2)), ("Y misaligned", dict(Y=base["Y"] + 2))]
    assert _walk(hip, S, "lap_lora_up_add", order, base, clauses) == 21
    S.run(lambda: hip.call("lap_lora_up_add", *[base[k] for k in order]), ["y"])


def test_lora_wgrad_argument_checks(hip):
    """M = 70, msplit = 2: mchunk = 64, S = 2, so the call needs 2 * 32 * 16 floats of scratch."""
    g = L.gen("args", "wgrad")
    S = Session(L.Arena().add("a", BF, 70, 72, data=torch.randn(70, 72, generator=g)).add("b", BF, 70, 40, data=torch.randn(70, 40, generator=g))
                .add("out", F32, 48, 16, out=True).add("scratch", F32, 1, 1024, out=True))
    order = "A lda B ldb bg out ldo ncopy out_f32 M Ng G R s msplit scratch scratch_floats".split()
    base = dict(A=S.p("a"), lda=32, B=S.p("b"), ldb=32, bg=16, out=S.p("out"), ldo=16, ncopy=1, out_f32=1, M=70, Ng=16, G=2, R=16, s=1.0, msplit=2,
                scratch=S.p("scratch"), scratch_floats=1024)
    clauses = [(f"{n} null", {n: None}) for n in ("A", "B", "out")] + _sizes(["M", "Ng", "G", "R", "ncopy", "msplit"]) + [
        ("R % 16", dict(R=24, lda=64)), ("Ng % 8", dict(Ng=12)), ("lda % 8", dict(lda=36)), ("ldb % 8", dict(ldb=36)), ("bg % 8", dict(bg=12)),
        ("lda < G R", dict(lda=24)), ("ldb < (G - 1) bg + Ng", dict(ldb=24)), ("ldo < Ng", dict(ldo=15)),
        ("A misaligned", dict(A=base["A"] + 2)), ("B misaligned", dict(B=base["B"] + 2)),
        ("scratch missing", dict(scratch=None)), ("scratch short", dict(scratch_floats=1023))]
    assert _walk(hip, S, "lap_lora_wgrad", order, base, clauses) == 27
    S.run(lambda: hip.call("lap_lora_wgrad", *[base[k] for k in order]), ["out", "scratch"])


def test_lora_merge_argument_checks(hip):
    g = L.gen("args", "merge")
    S = Session(L.Arena().add("w", F32, 6, 12, data=torch.randn(6, 12, generator=g)).add("a", F32, 10, 12, data=torch.randn(10, 12, generator=g))
                .add("b", F32, 10, 4, data=torch.randn(10, 4, generator=g)).add("weff", BF, 6, 12, out=True))
    order = "W ldw A lda B ldb nsum out ldo I Ng G R s".split()
    base = dict(W=S.p("w"), ldw=8, A=S.p("a"), lda=8, B=S.p("b"), ldb=3, nsum=1, out=S.p("weff"), ldo=8, I=8, Ng=3, G=2, R=5, s=1.0)
    clauses = [(f"{n} null", {n: None}) for n in ("W", "A", "B", "out")] + _sizes(["I", "Ng", "G", "R", "nsum"]) + [
        ("I % 4", dict(I=6)), ("ldw % 4", dict(ldw=10)), ("lda % 4", dict(lda=10)), ("ldo % 4", dict(ldo=10)), ("ldw < I", dict(ldw=4)),
        ("lda < I", dict(lda=4)), ("ldo < I", dict(ldo=4)), ("ldb < Ng", dict(ldb=2)), ("W misaligned", dict(W=base["W"] + 4)),
        ("A misaligned", dict(A=base["A"] + 4)), ("out misaligned", dict(out=base["out"] + 4))]
    assert _walk(hip, S, "lap_lora_merge", order, base, clauses) == 25
    S.run(lambda: hip.call("lap_lora_merge", *[base[k] for k in order]), ["weff"])
