"""Generator of lap_amd/csrc/gemm_asm_kernels.s: the bf16 GEMM main loop as hand-scheduled gfx950 assembly, one kernel per
operand layout and epilogue.  The HIP kernels of csrc/gemm.hip stop at 1.15-1.35 PF because hipcc cannot be made to keep ONE
wave per SIMD fed; here the instruction stream is fixed by this script:

  256 x 256 x 64 tile, 4 waves (2 x 2), one per SIMD, each 128 x 128 = 8 x 8 MFMA 16x16x32 tiles in 256 AGPRs;
  PERSISTENT blocks (256, one per CU).  Tiles are handed out per XCD: round r of XCD x covers logical tiles r * 256 + 32 x .. + 31;
  a block's first tile is static (block b: 32 (b % 8) + b / 8), every further one is a ticket of its XCD's counter (the XCD
  is read from HW_REG_XCC_ID), drawn by wave 0 one k-tile before the operand stream needs it and passed to the other waves
  through an LDS mailbox — a block that starts late or shares its CU simply takes fewer tiles, and neighbours in the tile
  order stay on one L2.  The operand stream (LDS-DMA) runs two k-tiles ahead of the MFMAs and straight across tile seams,
  so a tile's epilogue overlaps the next tile's first fetches;
  LDS: 2 stages x [A tile 32 KiB | B tile 32 KiB].  A K-contiguous operand tile is [256 rows][128 B], 16-byte chunks
  XOR-swizzled with (row >> 1) & 7 and read with ds_read_b128; an M- / N-contiguous operand tile is [64 k-rows][512 B],
  chunks XOR-swizzled with mc_swz(k) << 1 and read with ds_read_b64_tr_b16 (the images of csrc/common.hpp kc_tile_off /
  mc_tile_off: conflict free); both are filled by `buffer_load_dwordx4 ... lds` (16 one-KiB pieces per wave and k-tile), the
  swizzle applied to the SOURCE address;
  two fragment register sets (k-step 0 / 1 of a k-tile): every LDS read and every DMA piece is threaded between the MFMAs of
  the other set; one barrier per k-tile.

Per k-tile kt (stage s = kt & 1):
  P0   64 MFMA on set 0                 | fragment reads (kt, k-step 1) -> set 1
  MID  s_waitcnt vmcnt(0) lgkmcnt(0); s_barrier      (tile kt+1 has landed everywhere; stage s is no longer read)
  P1   64 MFMA on set 1                 | fragment reads (kt+1, k-step 0) -> set 0, 16 DMA pieces of k-tile kt+2 -> stage s
The accumulation order per output element (k-tiles ascending, k-step 0 then 1) is that of every other tile of the library,
so results are bitwise equal.  Output: D' = B A^T per MFMA, i.e. a lane owns 4 consecutive n of one m.  C leaves through a
per-wave LDS staging buffer as full 256-byte rows (Kernel.epilogue).

Layout of this file:
  Options       the schedule parameters (defaults = the committed file); main() reads them from the ASM_* environment
  KernelSpec    what a kernel is: layout, output type, Epilogue; KERNELS is the table of the 13 kernels that are built
  SGPRS, VGPRS  the register map: name, first register, count, the steps in which the register is live, the kernels that
                have it; check_register_map() asserts that no two live names overlap (the names are module constants)
  Kernel        one kernel's instruction stream: Kernel.emit() is the list of steps
  generate()    the whole file as a string; nothing here reads the environment or keeps state between two calls

Constraints checked by the launcher (csrc/gemm_asm.hip): M % 256 == 0, N % 256 == 0 (N % 16 == 0 for the bias kernels),
K % 128 == 0, K >= 512, strides % 8 == 0.

Usage: python tools/gen_gemm_asm.py > lap_amd/csrc/gemm_asm_kernels.s
       ASM_RING=0 | ASM_STORE_NT=0 | ASM_RD_STRIDE=x | ASM_DMA_STRIDE=n | ASM_ABL=token+token: schedule variants for timing
       (tools/probes/asm_variants.sh builds them into code objects that LAP_ASM_HSACO loads)
"""
import dataclasses
import enum
import re
import sys

# timing ablations (ASM_ABL): every one of them produces WRONG results on purpose
ABLATIONS = {
    "m32": "a phase's 64 MFMA 16x16x32 as 32 MFMA 32x32x16 (same flops, garbage operands)",
    "nodma": "no LDS-DMA pieces",
    "noread": "no fragment reads",
    "gll": "the DMA pieces as global_load_lds (no range check: the parked stream reads real memory)",
    "spread": "half of a k-tile's DMA pieces issued in P0 (races on the stage being read)",
    "nowait": "no vmcnt wait before the k-tile's barrier",
    "nobar": "no barrier per k-tile",
    "nomath": "the fused GeGLU-backward epilogue without its arithmetic",
    "nostore": "the plain epilogues without their C stores",
}


@dataclasses.dataclass(frozen=True)
class Options:
    ring: bool = True           # weight-gradient kernels: LDS as a ring of four half k-tiles (Kernel.phase_ring)
    # nontemporal C stores: full rows stream past the L2 (+5 % at K = 2048, +12 % at 8192^3)
    store_nt: bool = True
    rd_stride: float = 2.0      # MFMAs between two fragment reads (K-contiguous count)
    dma_stride: int = 4         # MFMAs between two DMA pieces
    abl: frozenset = frozenset()

    def __post_init__(self):
        object.__setattr__(self, "abl", frozenset(self.abl))
        if self.abl - set(ABLATIONS):
            raise ValueError(f"unknown ablation {sorted(self.abl - set(ABLATIONS))}; known: {sorted(ABLATIONS)}")

    @classmethod
    def from_env(cls, env):
        return cls(ring=env.get("ASM_RING", "1") == "1", store_nt=env.get("ASM_STORE_NT", "1") == "1",
                   rd_stride=float(env.get("ASM_RD_STRIDE", "2")), dma_stride=int(env.get("ASM_DMA_STRIDE", "4")),
                   abl=frozenset(env.get("ASM_ABL", "").split("+")) - {""})


class Emitter:
    """the lines of one generate() call and its counter for unique local labels"""

    def __init__(self):
        self.lines = []
        self._uid = 0

    def line(self, text):
        """one instruction or directive (indented by a tab) or one label (`name:`, not indented)"""
        self.lines.append(text if text.endswith(":") else "\t" + text)

    def raw(self, text):
        self.lines.append(text)

    def uid(self):
        self._uid += 1
        return self._uid

    def text(self):
        return "\n".join(self.lines) + "\n"


# ---- what a kernel is ------------------------------------------------------------------------------------------------
class Layout(enum.Enum):
    """(A K-contiguous, B K-contiguous)"""
    NT = (True, True)       # A [M,K], B [N,K]: forward
    NN = (True, False)      # A [M,K], B [K,N]: data gradient
    TN = (False, False)     # A [K,M], B [K,N]: weight gradient


class Out(enum.Enum):
    BF16 = "bf16"
    F32 = "f32"


class Epilogue(enum.Enum):
    PLAIN = "plain"
    # f32 bias per output column + ragged N (the last n-tile may hold fewer than 256 valid columns; N % 16 == 0): the last
    # n-tile's missing rows of B read as zeros, its missing columns of C are masked out of the stores
    BIAS = "bias"
    # + a bf16 residual R [M][ldc] (same leading dimension as C) added in f32 before the one rounding: the accumulators
    # are staged as f32 (two 64-column halves per row group), read back 8 columns per lane, and leave as 128-byte rows
    RES = "res"
    BIAS_RES = "bias_res"
    # the product is d(act) [M][N] of a GeGLU MLP's down projection and never leaves the kernel: the epilogue reads the
    # forward's gate | up values GU [M][2N] (C's leading dimension), rounds d(act) to bf16 as the stand-alone product
    # would, and stores d(gate) = d(act) * up * gelu'(gate) and d(up) = d(act) * bf16(gelu(gate)) into C [M][2N]
    # (csrc/elementwise.hip geglu_bwd_kernel; gemma.py:308-312 backward).  GELU' through v_exp / v_rcp (sigmoid form).
    # (a backward kernel: no optimizer waves to share the register file with; 256 VGPRs hold a third set of gate | up values)
    GEGLU_BWD = "geglu_bwd"
    # (forward layout) B = W [2F][K] holds the gate rows [0, F) and the up rows [F, 2F) of a GeGLU MLP; a tile pairs 128 gate
    # columns with their 128 up columns (every wave: 64 + 64), C = gate | up [M][2F] is stored as by the plain kernel and
    # ACT [M][F] = bf16(bf16(gelu(gate)) * up) (csrc/elementwise.hip geglu_fwd_kernel; gemma.py:308-312) leaves with it
    GEGLU_FWD = "geglu_fwd"
    # the product is d(a) [M][N] of an MLP's second Dense and never leaves the kernel: the epilogue reads the first Dense's
    # pre-activation H [M][N] (C's leading dimension) and stores d(h) = bf16(d(a)) * gelu'(h) (csrc/elementwise.hip gelu_bwd_kernel)
    GELU_BWD = "gelu_bwd"
    # (with the bias) C = H = bf16(x W^T + bias) and a second output A = bf16(gelu(H)) with C's leading dimension (kernarg
    # 0x68): the accumulators are walked twice, the second pass zeroes them (siglip_gemma3.py MlpBlock; gelu_fwd_kernel)
    BIAS_GELU = "bias_gelu"


@dataclasses.dataclass(frozen=True, kw_only=True)
class KernelSpec:
    name: str
    layout: Layout
    out: Out = Out.BF16
    epilogue: Epilogue = Epilogue.PLAIN
    # (both operands M- / N-contiguous) the 128 KiB of LDS as a ring of four 32-deep half k-tiles [A 16 KiB | B 16 KiB]
    # instead of two 64-deep stages: phase p (64 MFMAs on half p) reads the fragments of half p + 1 and requests half p + 4
    # into the slot half p left, so every phase carries 8 DMA pieces (instead of none / 16) and a request has two phases
    # to land (counted vmcnt(16) + one barrier per phase)
    ring: bool = False
    # the product is stored TRANSPOSED (C is [N][ldc]): a tall weight gradient dW [out, in] = dy^T x runs as the wide
    # product x^T dy (whose operand panels stream much better, tools/bench_asm_gemm.py) and lands in dW's layout
    transposed_out: bool = False
    # the kernel also adds the sum of squares of everything it stores to the f32 word at kernarg 0x68 (null: no) — a weight
    # gradient's contribution to the global gradient norm (scripts/train.py:363-371 via optax clip_by_global_norm), so that
    # no second pass has to read the gradient back.  Per lane across the block's tiles in V_SS, one atomic per wave when
    # the block is out of tiles.
    sumsq: bool = False

    def __post_init__(self):
        plain = self.epilogue is Epilogue.PLAIN
        if self.ring and self.layout is not Layout.TN:
            raise ValueError(f"{self.name}: the ring reads both operands with ds_read_b64_tr_b16 (layout tn only)")
        if self.geglu_fwd and self.layout is not Layout.NT:
            raise ValueError(f"{self.name}: geglu_fwd pairs gate and up ROWS of a K-contiguous B (layout nt only)")
        if self.sumsq and not plain:
            raise ValueError(f"{self.name}: the running sum of squares lives in the register the other epilogues use (v13)")
        if self.f32 and not plain:
            raise ValueError(f"{self.name}: the bias mask and the second-operand epilogues address bf16 columns")
        if self.transposed_out and not plain:
            raise ValueError(f"{self.name}: with transposed stores a lane's four values are one COLUMN of the product")

    a_kc = property(lambda self: self.layout.value[0])
    b_kc = property(lambda self: self.layout.value[1])
    kc = property(lambda self: self.layout.value)
    f32 = property(lambda self: self.out is Out.F32)
    bias = property(lambda self: self.epilogue in (Epilogue.BIAS, Epilogue.BIAS_RES, Epilogue.BIAS_GELU))
    ragged_n = bias
    residual = property(lambda self: self.epilogue in (Epilogue.RES, Epilogue.BIAS_RES))
    bias_res = property(lambda self: self.epilogue is Epilogue.BIAS_RES)
    geglu_bwd = property(lambda self: self.epilogue is Epilogue.GEGLU_BWD)
    geglu_fwd = property(lambda self: self.epilogue is Epilogue.GEGLU_FWD)
    gelu_bwd = property(lambda self: self.epilogue is Epilogue.GELU_BWD)
    bias_gelu = property(lambda self: self.epilogue is Epilogue.BIAS_GELU)
    # reads a second operand in the epilogue (R, GU or H: same rows and leading dimension as C, 8 bf16 columns per lane)
    second_operand = property(lambda self: self.residual or self.geglu_bwd or self.gelu_bwd)
    # kernarg 0x68 is a second tensor addressed through C's offsets (the second operand, or bias_gelu's second output)
    second_pointer = property(lambda self: self.second_operand or self.bias_gelu)
    stages_f32 = property(lambda self: self.f32 or self.second_operand)      # the staging buffer holds f32
    stages_bf16 = property(lambda self: not self.stages_f32)
    nvgpr = property(lambda self: 256 if self.geglu_bwd else 224)


KERNELS = (
    KernelSpec(name="lap_gemm_asm_nt", layout=Layout.NT),
    KernelSpec(name="lap_gemm_asm_nn", layout=Layout.NN),
    KernelSpec(name="lap_gemm_asm_tn", layout=Layout.TN, out=Out.F32, ring=True, sumsq=True),
    KernelSpec(name="lap_gemm_asm_nt_bias", layout=Layout.NT, epilogue=Epilogue.BIAS),
    KernelSpec(name="lap_gemm_asm_tn_t", layout=Layout.TN, out=Out.F32, ring=True, transposed_out=True, sumsq=True),
    KernelSpec(name="lap_gemm_asm_nt_res", layout=Layout.NT, epilogue=Epilogue.RES),
    KernelSpec(name="lap_gemm_asm_nt_bias_res", layout=Layout.NT, epilogue=Epilogue.BIAS_RES),
    KernelSpec(name="lap_gemm_asm_nn_geglu_bwd", layout=Layout.NN, epilogue=Epilogue.GEGLU_BWD),
    KernelSpec(name="lap_gemm_asm_nt_geglu", layout=Layout.NT, epilogue=Epilogue.GEGLU_FWD),
    KernelSpec(name="lap_gemm_asm_nn_gelu_bwd", layout=Layout.NN, epilogue=Epilogue.GELU_BWD),
    KernelSpec(name="lap_gemm_asm_nt_bias_gelu", layout=Layout.NT, epilogue=Epilogue.BIAS_GELU),
    # the weight-gradient layouts with BF16 stores (the reference's cast boundary `w.astype(bf16)` hands the f32 master a
    # bf16-rounded cotangent, gemma.py:307,318): same ring main loop, the bf16 staged epilogue of the forward kernels
    KernelSpec(name="lap_gemm_asm_tn_b16", layout=Layout.TN, ring=True, sumsq=True),
    KernelSpec(name="lap_gemm_asm_tn_t_b16", layout=Layout.TN, ring=True, transposed_out=True, sumsq=True),
)

# ---- register map -----------------------------------------------------------------------------------------------------
# A kernel runs through STEPS in this order, then loop / prelude / units / tail once per tile.  A register's scope names
# the steps in which it holds a value somebody still reads:
#   "always"            every step            "from <step>"   that step and every later one (written once during setup)
#   "main loop"         loop                  "epilogue"      prelude + units
#   "<step>+<step>"     those steps only (a temporary that is dead at the end of each of them)
# `when` names the KernelSpec properties (a|b: either) of the kernels that have the register: "epilogue of <variant>".
STEPS = ("args", "clear", "first_tile", "descriptors", "dma_offsets", "frag_addrs", "epi_addrs", "prologue",
         "loop", "prelude", "units", "tail")
NSGPR = 102                 # next_free_sgpr of the kernel descriptor


@dataclasses.dataclass(frozen=True)
class Reg:
    name: str
    first: int
    count: int
    scope: str
    when: str = ""

    def live(self):
        if self.scope == "always":
            return set(STEPS)
        if self.scope.startswith("from "):
            return set(STEPS[STEPS.index(self.scope[5:]):])
        steps = set({"main loop": "loop", "epilogue": "prelude+units"}.get(self.scope, self.scope).split("+"))
        assert steps <= set(STEPS), self
        return steps

    def applies(self, spec):
        return not self.when or any(getattr(spec, p) for p in self.when.split("|"))


R = Reg
SGPRS = (
    R("S_KARG", 0, 2, "args"), R("S_WG", 2, 1, "args+clear+first_tile"),
    R("S_XCC", 3, 1, "always"),                 # XCC id of the CU this block runs on
    R("S_A", 4, 2, "always"), R("S_B", 6, 2, "always"),        # pointers (pairs) after the kernarg load
    R("RQ", 8, 4, "always"),                    # descriptor of the 8 per-XCD tile counters
    R("S_M", 12, 1, "always"), R("S_N", 13, 1, "always"), R("S_K", 14, 1, "always"), R("S_LDA", 15, 1, "always"),
    R("S_LDB", 16, 1, "always"), R("S_LDC", 17, 1, "always"), R("S_TN", 18, 1, "always"), R("S_MAGIC", 19, 1, "always"),
    # s20..s34 scratch of every step but the epilogue's units, which keep named values in it:
    R("S_T", 20, 15, "args+clear+first_tile+descriptors+dma_offsets+frag_addrs+epi_addrs+prologue+loop+prelude+tail"),
    R("S_SOFF", 20, 8, "units"),                # soffsets of the four stores of two row groups
    R("RR", 28, 4, "epilogue", "second_pointer"),       # descriptor of the second operand / output of this tile
    R("S_ASOFF", 28, 4, "units", "geglu_fwd"),  # soffsets of the two ACT stores of two row groups
    R("S_WAVE", 35, 1, "always"),               # wave id
    R("RBI", 36, 4, "from args", "bias"),       # bias descriptor (the pointer pair is loaded into its first two words)
    R("RACT", 36, 4, "from descriptors", "geglu_fwd"),      # ACT descriptor of the tile in its epilogue
    R("S_W8K", 40, 1, "from dma_offsets"),      # wave * 8192: LDS byte base of this wave's DMA pieces
    R("S_LOOP", 41, 1, "main loop"),
    R("S_TM", 42, 1, "always"), R("S_GML", 43, 1, "always"), R("S_MAGL", 44, 1, "always"), R("S_NT", 45, 1, "always"),
    R("S_ONE", 46, 1, "always"), R("S_GSH", 47, 1, "always"), R("S_G", 48, 1, "always"),
    R("S_XOFF", 49, 1, "from first_tile"),      # byte offset of this XCD's counter
    R("S_HAVE", 50, 1, "from first_tile"),      # the stream has moved on to a valid next tile of this block
    R("S_TDMA", 51, 1, "from first_tile"), R("S_DLEFT", 52, 1, "from descriptors"), R("S_NKT", 53, 1, "from descriptors"),
    R("S_BUMPA", 54, 1, "from descriptors"), R("S_BUMPB", 55, 1, "from descriptors"),       # bytes per k-tile along each operand
    R("S_C", 56, 2, "always"),                  # C pointer pair
    R("S_RDL", 58, 1, "always", "second_pointer"), R("S_RDH", 91, 1, "always", "second_pointer"),    # R - C in bytes
    R("S_ACTNL", 58, 1, "from descriptors", "geglu_fwd"), R("S_ACTNH", 91, 1, "from descriptors", "geglu_fwd"),   # the next tile's ACT base
    R("S_REQ", 59, 1, "from first_tile"),       # wave 0: a ticket request is in flight
    R("RA", 60, 4, "from descriptors"), R("RB", 64, 4, "from descriptors"), R("RC", 68, 4, "from descriptors"),   # buffer descriptors
    R("S_OFFA", 72, 8, "from dma_offsets"), R("S_OFFB", 80, 8, "from dma_offsets"),         # soffset of the 8 pieces per operand
    R("S_STEPA", 89, 1, "from descriptors"), R("S_STEPB", 90, 1, "from descriptors"),       # the live values of S_BUMPA / S_BUMPB (0 once the stream is parked)
    R("RCN", 92, 4, "from descriptors"),        # C descriptor of the tile the DMA stream is already fetching
    R("S_C16", 96, 1, "from epi_addrs"),        # FOUR rows of C in bytes
    R("S_NREM", 97, 1, "from prologue", "bias"), R("S_NREMN", 98, 1, "from descriptors", "bias"),    # N - n0 of the current tile / of the tile the stream is fetching
    R("S_LDACT", 99, 1, "always", "geglu_fwd"), # ACT's leading dimension in bytes
    R("S_SSP", 100, 2, "always", "sumsq"),      # where the sum of squares goes (0: nowhere)
    R("S_ACT", 100, 2, "always", "geglu_fwd"),  # ACT pointer pair
)
VGPRS = (
    R("V_TID", 0, 1, "args"), R("V_LANE", 1, 1, "from args"),
    R("V_DA", 2, 4, "from dma_offsets"), R("V_DB", 6, 4, "from dma_offsets"),     # DMA lane offsets: up to 4 classes of pieces per operand
    R("V_T", 10, 2, "args+dma_offsets"),        # scratch
    R("V_SW", 10, 1, "from epi_addrs"), R("V_SR", 11, 1, "from epi_addrs"),       # the lane's write / read-back address in its wave's staging buffer (fc = 0 / j = 0)
    R("V_CO", 12, 1, "from epi_addrs"),         # the lane's store offset inside a C tile
    # v13: one per-lane value that each epilogue variant keeps for the whole kernel
    R("V_NCOL", 13, 1, "from epi_addrs", "bias"),       # wn*128 + 4 g (column of the lane's first output inside the tile)
    R("V_COU", 13, 1, "from epi_addrs", "geglu_bwd"),   # V_CO of the up half (+ N columns)
    R("V_SS", 13, 1, "from args", "sumsq"),     # the lane's running sum of squares over the block's tiles
    R("V_CA", 13, 1, "from epi_addrs", "geglu_fwd"),    # the lane's offset in ACT
    R("V_TK", 14, 1, "from prologue"), R("V_MB", 15, 1, "from first_tile"),       # ticket (wave 0: the atomic's return value); LDS address of the ticket mailbox
    R("V_ZERO", 16, 5, "clear"),                # block 0: the zeros that clear the next launch's counters
    R("V_RA", 16, 16, "from frag_addrs"), R("V_RB", 32, 16, "from frag_addrs"),   # fragment read addresses: up to 16 per operand
    # fragment sets: A frags at FA[set] + 4 f, B frags at FB[set] + 4 f.  Set 0 holds the next tile's first fragments
    # across the epilogue (the last P1 read them); set 1 is idle there and carries the epilogue's addresses and temporaries
    R("V_FA0", 48, 32, "from prologue"), R("V_FB0", 80, 32, "from prologue"),
    R("V_FA1", 112, 32, "main loop"), R("V_FB1", 144, 32, "main loop"),
    R("V_RS0", 112, 8, "units", "residual"), R("V_RS1", 168, 8, "units", "residual"),       # two sets of 2 x 4 registers for the residual values
    R("V_GX", 112, 4, "units", "geglu_bwd|gelu_bwd|geglu_fwd"), R("V_GU_", 116, 4, "units", "geglu_bwd|gelu_bwd|geglu_fwd"),     # 4 registers each:
    R("V_GX2", 124, 4, "units", "geglu_bwd|gelu_bwd"), R("V_GP", 164, 4, "units", "geglu_bwd|gelu_bwd|geglu_fwd"),      # the GELU arithmetic of one row piece
    R("V_GG", 168, 4, "units", "geglu_bwd"), R("V_GO", 172, 4, "units", "geglu_bwd|gelu_bwd"),
    R("V_WA", 120, 4, "epilogue"), R("V_WA4", 124, 4, "epilogue", "stages_bf16"),   # V_SW per fc (f32 staging: 4 tiles per unit, bf16: 8)
    R("V_RT", 124, 2, "units", "residual"),     # two residual values widened to f32
    R("V_RD", 128, 4, "epilogue"),              # V_SR per j
    R("V_CS", 132, 32, "units+tail"),           # two sets of 4 x 4 read-back registers (tail: the waves' sums of squares)
    R("V_COM", 164, 1, "epilogue", "bias"), R("V_COM1", 165, 1, "epilogue", "bias_res"),    # V_CO with the ragged-N mask folded in (residual: per 64-column half)
    R("V_KG", 165, 1, "epilogue", "bias_gelu"), # -2 log2(e) sqrt(2/pi)
    R("V_WAA", 168, 4, "epilogue", "geglu_fwd"),        # V_SWA per fc
    R("V_E", 176, 16, "dma_offsets+frag_addrs+epi_addrs+loop+tail"),      # scratch (loop: the gll ablation)
    R("V_EP", 176, 4, "prelude"),               # the prelude's share of the scratch registers
    R("V_ACC0", 176, 6, "units"), R("V_ACC1", 184, 6, "units"),   # two sets: an accumulator tile read out (4) and packed to bf16 (2)
    R("V_GK0", 182, 1, "epilogue", "geglu_bwd|gelu_bwd|geglu_fwd"), R("V_GK1", 183, 1, "epilogue", "geglu_bwd|gelu_bwd"),  # -2 log2(e) sqrt(2/pi), sqrt(2/pi)
    R("V_GT", 182, 2, "units", "bias_gelu"), R("V_GT2", 190, 2, "units", "bias_gelu"),      # four temporaries of gelu_packed
    R("V_BIAS", 192, 32, "epilogue", "bias"),   # the lane's 8 x 4 bias values of the tile
    R("V_GUL", 192, 48, "units", "geglu_bwd"),  # three sets of 2 x (4 gate, 4 up) registers
    R("V_HL", 192, 24, "units", "gelu_bwd"),    # three sets of 2 x 4 registers of pre-activations
    R("V_OUT", 216, 4, "units", "gelu_bwd"),    # a row piece's 8 packed d(h)
    R("V_OG", 240, 4, "units", "geglu_bwd"), R("V_OU", 244, 4, "units", "geglu_bwd"),       # a row piece's 8 packed d(gate) / d(up)
    R("V_GPK", 192, 8, "units", "geglu_fwd"),   # the unit's 4 gate tiles, packed bf16
    R("V_AS", 200, 16, "units", "geglu_fwd"),   # two sets of 2 x 4 read-back registers of the ACT staging buffer
    R("V_SWA", 216, 1, "from epi_addrs", "geglu_fwd"), R("V_SRA", 217, 1, "from epi_addrs", "geglu_fwd"),   # V_SW / V_SR of the ACT staging buffer
    R("V_SRA1", 218, 1, "epilogue", "geglu_fwd"),       # V_SRA of the second row piece
)
# Pairs of names that overlap while both are live, and why the kernels may rely on it:
EXCEPTIONS = {
    # the prelude computes the bias offset (s30) and the second half's mask bound (s31) first and writes RR behind their last use
    ("S_T", "RR"): "s30 / s31 are consumed before the prelude sets RR up",
}
globals().update({r.name: r.first for r in SGPRS + VGPRS})
FA = {0: V_FA0, 1: V_FA1}       # noqa: F821  (the names come from the tables above)
FB = {0: V_FB0, 1: V_FB1}       # noqa: F821


class RegisterOverlap(AssertionError):
    pass


def check_register_map(spec, sgprs=SGPRS, vgprs=VGPRS, exceptions=EXCEPTIONS):
    """asserts for one kernel: no two registers that can be live together overlap; the VGPRs stay below the kernel's nvgpr,
    the SGPRs below the NSGPR of the kernel descriptor"""
    for regs, limit, what in ((sgprs, NSGPR, "SGPR"), (vgprs, spec.nvgpr, "VGPR")):
        mine = [r for r in regs if r.applies(spec)]
        for r in mine:
            if r.first + r.count > limit:
                raise RegisterOverlap(f"{spec.name}: {r.name} ends at {what} {r.first + r.count - 1}, the kernel has {limit}")
        for i, a in enumerate(mine):
            for b in mine[i + 1:]:
                if a.first < b.first + b.count and b.first < a.first + a.count and a.live() & b.live() \
                        and (a.name, b.name) not in exceptions and (b.name, a.name) not in exceptions:
                    raise RegisterOverlap(f"{spec.name}: {a.name} and {b.name} overlap in {sorted(a.live() & b.live())}")


# ---- LDS map ---------------------------------------------------------------------------------------------------------
STAGE = 65536               # bytes per stage [A tile | B tile]
BOFF = 32768                # the B tile inside a stage
CSTAGE = 131072             # the epilogue's staging buffers: 4 KiB per wave ([16 rows][256 B], chunks XOR row)
ASTAGE = 131072 + 16384     # the ACT staging buffers: 2 KiB per wave ([16 rows][128 B], chunk XOR (row >> 1))
MAILBOX = 131072 + 24576    # the ticket mailbox (behind the stages and the staging buffers)


def acc(fm, fn):
    return (fm * 8 + fn) * 4


def mfma(fm, fn, st, swap=False):
    """D' = B A^T (a lane owns 4 consecutive n of one m); swap: D = A B^T (4 consecutive m of one n: transposed stores)"""
    a = acc(fm, fn)
    x, y = (FA[st] + 4 * fm, FB[st] + 4 * fn) if swap else (FB[st] + 4 * fn, FA[st] + 4 * fm)
    return f"v_mfma_f32_16x16x32_bf16 a[{a}:{a+3}], v[{x}:{x+3}], v[{y}:{y+3}], a[{a}:{a+3}]"


def order():
    """MFMA order of a k-step: serpentine over (fm, fn) so consecutive instructions share one operand."""
    o = []
    for fm in range(8):
        fns = range(8) if fm % 2 == 0 else range(7, -1, -1)
        o += [(fm, fn) for fn in fns]
    return o


class Kernel:
    """the instruction stream of one KernelSpec under one set of Options, written to one Emitter"""

    def __init__(self, spec, opt, em):
        check_register_map(spec)
        self.spec, self.opt, self.E, self.uid = spec, opt, em.line, em.uid
        self.ring = spec.ring and opt.ring
        self.abl = opt.abl
        self.st_nt = " nt" if opt.store_nt else ""
        # the epilogue works in units of one staging buffer: a 16-row group of the wave's C tile (bf16 staging, 8 accumulator
        # tiles) or one 64-column half h of it (f32 staging, 4 tiles); bias_gelu walks every row group twice (h = the pass)
        self.nfc = 4 if spec.stages_f32 else 8
        self.two = 2 if (spec.stages_f32 or spec.bias_gelu) else 1
        self.units = [(fr, h) for fr in range(8) for h in range(self.two)]

    def __getattr__(self, name):        # the spec's fields and derived facts read as the kernel's own
        return getattr(self.spec, name)

    def lines(self, texts):
        for x in texts:
            self.E(x)

    # ---- fragment reads of k-step kk from `stage` into register set st
    def reads(self, kk, stage, st):
        per = []
        for op, (F, VR) in enumerate(((FA, V_RA), (FB, V_RB))):
            ops = []
            for f in range(8):
                d = F[st] + 4 * f
                if self.kc[op]:     # address registers: VR + 2 * stage + kk; fragment f: + 2048 f
                    # (geglu_fwd, B: fragments 0-3 = the wave's 64 gate columns, 4-7 = their up columns, 128 tile rows further)
                    extra = 8192 if (self.geglu_fwd and op == 1 and f >= 4) else 0
                    ops.append([f"ds_read_b128 v[{d}:{d+3}], v{VR + 2*stage + kk} offset:{f*2048 + extra}"])
                else:               # address registers: VR + 8 * stage + f; k-step: + 16384 kk; second half: k-row + 4
                    ops.append([f"ds_read_b64_tr_b16 v[{d}:{d+1}], v{VR + 8*stage + f} offset:{kk*16384}",
                                f"ds_read_b64_tr_b16 v[{d+2}:{d+3}], v{VR + 8*stage + f} offset:{kk*16384 + 2048}"])
            per.append(ops)
        r = []
        for f in range(8):
            r += per[0][f] + per[1][f]
        return r

    def dma(self, stage):
        """16 LDS-DMA pieces of the stream's next k-tile into `stage`; each = (m0 write, load)."""
        r = []
        for j in range(8):
            for op, (rs, soff, vd, boff) in enumerate(((RA, S_OFFA, V_DA, 0), (RB, S_OFFB, V_DB, BOFF))):
                cls = (j & 1) if self.kc[op] else ((j & 1) + 2 * ((j >> 2) & 1))
                lds = stage * STAGE + boff + j * 1024
                r.append((f"s_add_u32 m0, s{S_W8K}, {lds}", f"buffer_load_dwordx4 v{vd + cls}, s[{rs}:{rs+3}], s{soff+j} offen lds"))
        return r

    def reads_ring(self, slot, st):
        """fragment reads of the half k-tile in `slot` into register set st (address registers: VR + 8 * (slot >> 1) + f)"""
        r = []
        for f in range(8):
            for F, VR in ((FA, V_RA), (FB, V_RB)):
                d = F[st] + 4 * f
                base = (slot & 1) * 32768
                r.append(f"ds_read_b64_tr_b16 v[{d}:{d+1}], v{VR + 8*(slot >> 1) + f} offset:{base}")
                r.append(f"ds_read_b64_tr_b16 v[{d+2}:{d+3}], v{VR + 8*(slot >> 1) + f} offset:{base + 2048}")
        return r

    def dma_ring(self, slot):
        """8 LDS-DMA pieces of the stream's next half k-tile into `slot`; piece j of wave w: k-rows 8 w + 2 j, + 1 of the half"""
        r = []
        for j in range(4):
            for rs, soff, vd, boff in ((RA, S_OFFA, V_DA, 0), (RB, S_OFFB, V_DB, 16384)):
                lds = slot * 32768 + boff + j * 1024
                r.append((f"s_add_u32 m0, s{S_W8K}, {lds}", f"buffer_load_dwordx4 v{vd + (j & 1)}, s[{rs}:{rs+3}], s{soff+j} offen lds"))
        return r

    def phase_ring(self, p):
        """phase p of the ring: half p is in register set p & 1"""
        E, u = self.E, self.uid()
        E("s_waitcnt vmcnt(16)")                        # this wave's pieces of half p + 1 (behind them: halves p + 2, p + 3)
        E(f"s_cmp_eq_u32 s{S_REQ}, 0")                  # wave 0: the ticket drawn three phases ago is back (16 requests behind it were counted out)
        E(f"s_cbranch_scc1 .Lno_pub{u}")
        E(f"s_sub_u32 s{S_REQ}, s{S_REQ}, 1")
        E(f"s_cmp_lg_u32 s{S_REQ}, 0")
        E(f"s_cbranch_scc1 .Lno_pub{u}")
        E("s_mov_b64 exec, 1")
        E(f"ds_write_b32 v{V_MB}, v{V_TK}")
        E("s_mov_b64 exec, -1")
        E("s_waitcnt lgkmcnt(0)")
        E(f".Lno_pub{u}:")
        E("s_barrier")
        side = [(2 * n, txt) for n, txt in enumerate(self.reads_ring((p + 1) & 3, (p + 1) & 1))]
        for n, (m0w, ld) in enumerate(self.dma_ring(p & 3)):
            slot = 3 + 8 * n
            side += [(slot, m0w), (slot, "s_nop 0"), (slot, ld)]
        side += [(63, txt) for txt in self.stream_step()]
        self.phase(p & 1, side)
        E("s_waitcnt lgkmcnt(0)")

    def bump(self):
        r = []
        for rs, step in ((RA, S_STEPA), (RB, S_STEPB)):
            r += [f"s_add_u32 s{rs}, s{rs}, s{step}", f"s_addc_u32 s{rs+1}, s{rs+1}, 0", f"s_sub_u32 s{rs+2}, s{rs+2}, s{step}",
                  f"s_max_i32 s{rs+2}, s{rs+2}, 0"]
        return r

    def setup(self, treg):
        """SALU: logical tile id in s{treg} -> (tm, tn) (groups of 2^gsh m-tiles sweep n: csrc/gemm_common.hpp tile_coords),
        then the DMA descriptors RA / RB of its operand panels and the C descriptor RCN.  Scratch s20..s34."""
        t = S_T
        r = [f"s_mul_hi_u32 s{t+10}, s{treg}, s{S_MAGIC}",        # group = tile / (GM tiles_n)
             f"s_lshl_b32 s{t+11}, s{S_TN}, s{S_GSH}",
             f"s_mul_i32 s{t+12}, s{t+10}, s{t+11}",
             f"s_sub_u32 s{t+12}, s{treg}, s{t+12}",              # rem
             f"s_lshl_b32 s{t+10}, s{t+10}, s{S_GSH}",            # first_m
             f"s_lshl_b32 s{t+14}, 1, s{S_GSH}",
             f"s_add_u32 s{t+11}, s{t+10}, s{t+14}",
             f"s_sub_u32 s{t+14}, s{t+14}, 1",
             f"s_lshr_b32 s{t+9}, s{t+12}, s{S_GSH}",             # full group: tn = rem >> gsh, tm = first_m + (rem & (GM - 1))
             f"s_and_b32 s{t+8}, s{t+12}, s{t+14}",
             f"s_mul_hi_u32 s{t+13}, s{t+12}, s{S_MAGL}",         # partial group: tn = rem / gm_last
             f"s_mul_i32 s{t+14}, s{t+12}, s{S_ONE}",
             f"s_add_u32 s{t+13}, s{t+13}, s{t+14}",
             f"s_mul_i32 s{t+14}, s{t+13}, s{S_GML}",
             f"s_sub_u32 s{t+14}, s{t+12}, s{t+14}",
             f"s_cmp_le_u32 s{t+11}, s{S_TM}",
             f"s_cselect_b32 s{t+9}, s{t+9}, s{t+13}",
             f"s_cselect_b32 s{t+8}, s{t+8}, s{t+14}",
             f"s_add_u32 s{t+8}, s{t+8}, s{t+10}",                # tm
             f"s_lshl_b32 s{t+8}, s{t+8}, 8",                     # m0
             f"s_lshl_b32 s{t+9}, s{t+9}, {7 if self.geglu_fwd else 8}"]   # n0 (geglu_fwd: of the gate half; the up half sits N / 2 further)
        for op, (rs, ptr, row0, ld) in enumerate(((RA, S_A, t + 8, S_LDA), (RB, S_B, t + 9, S_LDB))):
            if self.kc[op]:     # panel rows row0 .. row0 + 255, all of K: base + row0 * ld; range 255 ld + K bytes
                r += [f"s_mul_i32 s{t+10}, s{row0}, s{ld}", f"s_mul_hi_u32 s{t+11}, s{row0}, s{ld}",
                      f"s_add_u32 s{rs}, s{ptr}, s{t+10}", f"s_addc_u32 s{rs+1}, s{ptr+1}, s{t+11}", f"s_and_b32 s{rs+1}, s{rs+1}, 0xffff"]
                if self.ragged_n and op == 1:    # rows past N read as zeros (range = (rows - 1) ld + K bytes)
                    r += [f"s_sub_u32 s{S_NREMN}, s{S_N}, s{row0}", f"s_min_u32 s{t+10}, s{S_NREMN}, 256", f"s_sub_u32 s{t+10}, s{t+10}, 1",
                          f"s_mul_i32 s{rs+2}, s{ld}, s{t+10}", f"s_add_u32 s{rs+2}, s{rs+2}, s{S_K}"]
                elif self.geglu_fwd and op == 1:   # rows n0 .. n0 + 127 and N / 2 + n0 .. + 127
                    r += [f"s_lshr_b32 s{t+10}, s{S_N}, 1", f"s_add_u32 s{t+10}, s{t+10}, 127",
                          f"s_mul_i32 s{rs+2}, s{ld}, s{t+10}", f"s_add_u32 s{rs+2}, s{rs+2}, s{S_K}"]
                else:
                    r += [f"s_mul_i32 s{rs+2}, s{ld}, 255", f"s_add_u32 s{rs+2}, s{rs+2}, s{S_K}"]
            else:               # panel columns row0 .. row0 + 255 of all K rows: base + row0 * 2; range (K - 1) ld + 512 bytes
                r += [f"s_lshl_b32 s{t+10}, s{row0}, 1",
                      f"s_add_u32 s{rs}, s{ptr}, s{t+10}", f"s_addc_u32 s{rs+1}, s{ptr+1}, 0", f"s_and_b32 s{rs+1}, s{rs+1}, 0xffff",
                      f"s_lshr_b32 s{t+10}, s{S_K}, 1", f"s_sub_u32 s{t+10}, s{t+10}, 1",
                      f"s_mul_i32 s{rs+2}, s{t+10}, s{ld}", f"s_add_u32 s{rs+2}, s{rs+2}, 512"]
        sh = 2 if self.f32 else 1
        cr, cc = (t + 9, t + 8) if self.transposed_out else (t + 8, t + 9)      # C row / column origin of the tile
        r += [f"s_mul_i32 s{t+10}, s{cr}, s{S_LDC}", f"s_mul_hi_u32 s{t+11}, s{cr}, s{S_LDC}", f"s_lshl_b32 s{t+12}, s{cc}, {sh}",
              f"s_add_u32 s{t+10}, s{t+10}, s{t+12}", f"s_addc_u32 s{t+11}, s{t+11}, 0",
              f"s_add_u32 s{RCN}, s{S_C}, s{t+10}", f"s_addc_u32 s{RCN+1}, s{S_C+1}, s{t+11}", f"s_and_b32 s{RCN+1}, s{RCN+1}, 0xffff"]
        if self.geglu_fwd:       # ACT tile: rows m0 .., columns n0 ..
            r += [f"s_mul_i32 s{t+10}, s{cr}, s{S_LDACT}", f"s_mul_hi_u32 s{t+11}, s{cr}, s{S_LDACT}", f"s_lshl_b32 s{t+12}, s{cc}, 1",
                  f"s_add_u32 s{t+10}, s{t+10}, s{t+12}", f"s_addc_u32 s{t+11}, s{t+11}, 0",
                  f"s_add_u32 s{S_ACTNL}, s{S_ACT}, s{t+10}", f"s_addc_u32 s{S_ACTNH}, s{S_ACT+1}, s{t+11}", f"s_and_b32 s{S_ACTNH}, s{S_ACTNH}, 0xffff"]
        return r

    def stream_step(self):
        """after a k-tile's DMA pieces: advance the descriptors.  One k-tile before the tile's last request wave 0 draws the
        block's next ticket from its XCD's counter (returned by the time of the next barrier, where it is put into the LDS
        mailbox); when the last k-tile has been requested every wave reads the mailbox and moves the stream on to that tile
        (or parks it: every further request then falls outside the range: zero fill)."""
        u = self.uid()
        t = S_T
        r = self.bump()
        # (ring: a unit is a half k-tile; the ticket is drawn four units before the seam and published three phases later)
        r += [f"s_sub_u32 s{S_DLEFT}, s{S_DLEFT}, 1",
              f"s_cmp_lg_u32 s{S_DLEFT}, {4 if self.ring else 1}", f"s_cbranch_scc1 .Lno_req{u}",
              f"s_cmp_lg_u32 s{S_WAVE}, 0", f"s_cbranch_scc1 .Lstream_done{u}",               # (DLEFT == 1: nothing else to do)
              "s_mov_b64 exec, 1", f"v_mov_b32 v{V_TK}, 1",
              f"buffer_atomic_add v{V_TK}, off, s[{RQ}:{RQ+3}], s{S_XOFF} sc0",
              "s_mov_b64 exec, -1", f"s_mov_b32 s{S_REQ}, {3 if self.ring else 1}", f"s_branch .Lstream_done{u}",
              f".Lno_req{u}:",
              f"s_cmp_lg_u32 s{S_DLEFT}, 0", f"s_cbranch_scc1 .Lstream_done{u}",
              f"ds_read_b32 v{V_TK}, v{V_MB}", "s_waitcnt lgkmcnt(0)", f"v_readfirstlane_b32 s{t+10}, v{V_TK}",
              f"s_add_u32 s{t+10}, s{t+10}, 32",                                               # tickets count from the second round
              f"s_lshr_b32 s{t+11}, s{t+10}, 5", f"s_lshl_b32 s{t+11}, s{t+11}, 8",            # round * 256
              f"s_and_b32 s{t+10}, s{t+10}, 31", f"s_add_u32 s{t+11}, s{t+11}, s{t+10}",
              f"s_lshl_b32 s{t+10}, s{S_XCC}, 5", f"s_add_u32 s{S_TDMA}, s{t+11}, s{t+10}",    # + 32 xcc
              f"s_cmp_lt_u32 s{S_TDMA}, s{S_NT}", f"s_cbranch_scc0 .Lstream_park{u}"]
        r += self.setup(S_TDMA)
        r += [f"s_mov_b32 s{S_DLEFT}, s{S_NKT}", f"s_mov_b32 s{S_HAVE}, 1", f"s_branch .Lstream_done{u}", f".Lstream_park{u}:",
              f"s_mov_b32 s{RA+2}, 0", f"s_mov_b32 s{RB+2}, 0", f"s_mov_b32 s{S_STEPA}, 0", f"s_mov_b32 s{S_STEPB}, 0",
              f"s_mov_b32 s{S_DLEFT}, 0x7fffffff", f".Lstream_done{u}:"]
        return r

    def phase(self, st, side):
        """64 MFMAs of register set st with the side instructions threaded in: side = list of (slot, text)."""
        E, abl = self.E, self.abl
        byslot = {}
        for slot, txt in side:
            byslot.setdefault(slot, []).append(txt)
        if "m32" in abl:
            merged = {}
            for slot, lst in byslot.items():
                merged.setdefault(slot // 2, []).extend(lst)
            byslot = merged
        for n, (fm, fn) in enumerate(order() if "m32" not in abl else [(k % 4, k // 4 % 4) for k in range(32)]):
            if "m32" in abl:
                a = (n % 16) * 16
                E(f"v_mfma_f32_32x32x16_bf16 a[{a}:{a+15}], v[{FB[st] + 4*fn}:{FB[st] + 4*fn + 3}], v[{FA[st] + 4*fm}:{FA[st] + 4*fm + 3}], a[{a}:{a+15}]")
            else:
                E(mfma(fm, fn, st, self.transposed_out))
            for txt in byslot.get(n, []):
                if ("nodma" in abl and ("lds" in txt.split() or txt.startswith("s_add_u32 m0") or txt == "s_nop 0")) or \
                        ("noread" in abl and txt.startswith("ds_read_b")):
                    continue
                if "gll" in abl and txt.startswith("buffer_load_dwordx4") and txt.endswith("lds"):
                    m = re.match(r"buffer_load_dwordx4 v(\d+), s\[(\d+):(\d+)\], s(\d+) offen lds", txt)
                    vd, rs, _, soff = (int(x) for x in m.groups())
                    E(f"v_add_u32 v{V_E+15}, s{soff}, v{vd}")
                    E(f"global_load_lds_dwordx4 v{V_E+15}, s[{rs}:{rs+1}]")
                    continue
                E(txt)

    def ktile(self, stage):
        E, abl = self.E, self.abl
        DS = self.opt.dma_stride
        rd = self.reads(1, stage, 1)
        rs = self.opt.rd_stride * 16 / len(rd)
        side0 = [(min(int(rs * n), 63), t) for n, t in enumerate(rd)]
        pieces = self.dma(stage)
        if "spread" in abl:
            for n, (m0w, ld) in enumerate(pieces[:8]):
                side0 += [(3 + n * 8, m0w), (3 + n * 8, "s_nop 0"), (3 + n * 8, ld)]
            pieces = pieces[8:]
            DS = 8
        self.phase(0, side0)
        E("s_waitcnt lgkmcnt(0)" if "nowait" in abl else ("s_waitcnt vmcnt(8) lgkmcnt(0)" if "spread" in abl else "s_waitcnt vmcnt(0) lgkmcnt(0)"))
        u = self.uid()
        E(f"s_cmp_eq_u32 s{S_REQ}, 0")                  # wave 0, a ticket has just come back: into the mailbox before the barrier
        E(f"s_cbranch_scc1 .Lno_pub{u}")
        E("s_mov_b64 exec, 1")
        E(f"ds_write_b32 v{V_MB}, v{V_TK}")
        E("s_mov_b64 exec, -1")
        E("s_waitcnt lgkmcnt(0)")
        E(f"s_mov_b32 s{S_REQ}, 0")
        E(f".Lno_pub{u}:")
        if "nobar" not in abl:
            E("s_barrier")
        rd = self.reads(0, stage ^ 1, 0)
        side = [(min(int(rs * n), 63), t) for n, t in enumerate(rd)]
        for n, (m0w, ld) in enumerate(pieces):
            slot = min(1 + n * DS, 62)
            side += [(slot, m0w), (slot, "s_nop 0"), (slot, ld)]
        side += [(63, t) for t in self.stream_step()]
        self.phase(1, side)
        E("s_waitcnt lgkmcnt(0)")

    # ---- epilogue.  Each 16-row group of the wave's C tile goes through the wave's 4 KiB staging buffer and leaves as 4 rows x 256
    # contiguous bytes per store instruction (stored straight from the accumulator layout they would be 16 rows x 32 bytes:
    # partial lines the L2 has to merge, and keeps in place of operand panels).  LDS operations of one wave execute in order,
    # so one buffer is enough: the read-back of unit u is queued before the writes of unit u + 1; the stores of unit u are
    # issued behind the writes and reads of unit u + 1 (lgkmcnt counts them out).  Second-operand variants: the unit's values
    # are requested before its accumulators are staged and used after the read-back, 8 columns per lane -> rows of 128 bytes
    # per store (dwordx4 loads / stores: half the VMEM instructions of 4 columns per lane).
    def epilogue(self):
        self.epilogue_prelude()
        self.epilogue_units()

    def epilogue_prelude(self):
        """bias values, ragged-N mask, second descriptor, constants, staging addresses per tile of a unit"""
        E, t, V = self.E, S_T, V_EP
        if self.bias:
            # the lane's bias values: column n0 + wn*128 + 16 fn + 4 g .. + 3 (past N: zeros); n0 = N - S_NREM
            E(f"s_sub_u32 s{t+10}, s{S_N}, s{S_NREM}")
            E(f"s_lshl_b32 s{t+10}, s{t+10}, 2")
            E(f"v_lshlrev_b32 v{V}, 2, v{V_NCOL}")
            for fn in range(8):
                E(f"buffer_load_dwordx4 v[{V_BIAS+4*fn}:{V_BIAS+4*fn+3}], v{V}, s[{RBI}:{RBI+3}], s{t+10} offen offset:{fn*64}")
            # ragged N: the lane stores columns wn*128 + (l & 15) * 8 .. + 7 of the tile (residual variant: for each 64-column half
            # h, wn*128 + 64 h + (l & 7) * 8 .. + 7); past N -> an out-of-range offset (dropped / read as zero)
            E(f"v_and_b32 v{V+1}, {7 if self.second_operand else 15}, v{V_LANE}")
            E(f"v_lshlrev_b32 v{V+1}, 3, v{V+1}")
            E(f"v_and_b32 v{V+2}, -128, v{V_NCOL}")                 # wn * 128
            E(f"v_add_u32 v{V+1}, v{V+1}, v{V+2}")
            E(f"v_mov_b32 v{V+2}, 0x80000000")
            E(f"v_cmp_gt_i32 vcc, s{S_NREM}, v{V+1}")
            E(f"v_cndmask_b32 v{V_COM}, v{V+2}, v{V_CO}, vcc")
            if self.second_operand:     # second half: + 64 columns
                E(f"s_sub_i32 s{t+11}, s{S_NREM}, 64")
                E(f"v_cmp_gt_i32 vcc, s{t+11}, v{V+1}")
                E(f"v_cndmask_b32 v{V_COM1}, v{V+2}, v{V_CO}, vcc")
        if self.second_pointer:
            E(f"s_add_u32 s{RR}, s{RC}, s{S_RDL}")
            E(f"s_addc_u32 s{RR+1}, s{RC+1}, s{S_RDH}")
            E(f"s_and_b32 s{RR+1}, s{RR+1}, 0xffff")
            E(f"s_mov_b32 s{RR+2}, s{RC+2}")
            E(f"s_mov_b32 s{RR+3}, s{RC+3}")
        if self.geglu_bwd or self.gelu_bwd:
            E(f"v_mov_b32 v{V_GK0}, 0xc0135761")       # -2 log2(e) sqrt(2/pi) = -2.3022082
            E(f"v_mov_b32 v{V_GK1}, 0x3f4c422a")       # sqrt(2/pi) = 0.7978846
        if self.bias_gelu:
            E(f"v_mov_b32 v{V_KG}, 0xc0135761")
        if self.geglu_fwd:
            E(f"v_mov_b32 v{V_GK0}, 0xc0135761")
            for fc in range(4):
                E(f"v_xor_b32 v{V_WAA+fc}, {fc * 32}, v{V_SWA}")
            E(f"v_xor_b32 v{V_SRA1}, 64, v{V_SRA}")
        for fc in range(self.nfc):
            E(f"v_xor_b32 v{V_WA+fc}, {fc * (64 if self.stages_f32 else 32)}, v{V_SW}")
        if self.second_operand:
            # read back 8 columns per lane: lane -> row 8 j' + (l >> 3), chunks 2 (l & 7) + c (c = 0, 1) of the [16 rows][16 chunks] buffer,
            # chunk XOR row: V_RD + 2 j' + c (j' = 1: XOR 128, + 2048 in the instruction)
            E(f"v_lshrrev_b32 v{V}, 3, v{V_LANE}")
            E(f"v_and_b32 v{V+1}, 7, v{V_LANE}")
            E(f"v_lshlrev_b32 v{V+1}, 1, v{V+1}")
            E(f"v_lshlrev_b32 v{V+2}, 8, v{V}")
            E(f"s_lshl_b32 s{t+12}, s{S_WAVE}, 12")
            E(f"s_add_u32 s{t+12}, s{t+12}, {CSTAGE}")
            E(f"v_add_u32 v{V+2}, s{t+12}, v{V+2}")
            for c in range(2):
                E(f"v_or_b32 v{V+3}, {c}, v{V+1}")
                E(f"v_xor_b32 v{V+3}, v{V+3}, v{V}")
                E(f"v_lshlrev_b32 v{V+3}, 4, v{V+3}")
                E(f"v_add_u32 v{V_RD+c}, v{V+2}, v{V+3}")
                E(f"v_xor_b32 v{V_RD+2+c}, 128, v{V_RD+c}")
        else:
            for j in range(4):
                E(f"v_xor_b32 v{V_RD+j}, {j * 64}, v{V_SR}")
        E("s_nop 15")
        E("s_nop 15")
        if self.bias:
            E("s_waitcnt vmcnt(0)")      # the bias values (and the stream's k-tile 1, which the next barrier would wait for anyway)

    def epilogue_units(self):
        """the unit pipeline: accumulator tile n + 1 is read out while tile n is staged; a unit's loads go out at its first
        tile (two units ahead where a miss costs more than a unit, ~1.4 us), its read-back and the previous unit's stores at its last"""
        E, nfc = self.E, self.nfc
        seq = [(fr, h, fcl) for fr, h in self.units for fcl in range(nfc)]
        sets = (V_ACC0, V_ACC1)
        self.read_out(*seq[0], sets[0])
        for n, (fr, h, fcl) in enumerate(seq):
            u = fr * self.two + h
            if fcl == 0:
                self.unit_loads(u)
            if n + 1 < len(seq):
                self.read_out(*seq[n + 1], sets[(n + 1) & 1])
            self.stage_tile(u, fcl, sets[n & 1])
            if fcl == nfc - 1:
                self.unit_read_back(u)
        E("s_waitcnt lgkmcnt(0)")
        if self.second_operand:
            E("s_nop 0")
        self.stores(len(self.units) - 1)
        if self.geglu_fwd:
            self.act_stores(len(self.units) - 1)

    def fc_of(self, h, fcl):
        """the column group of C that tile fcl of a unit holds"""
        return fcl if self.bias_gelu else h * 4 + fcl

    def vco(self, h):
        return (V_COM + (h if self.second_operand else 0)) if self.bias else V_CO

    def read_out(self, fr, h, fcl, base):
        """(fr, fc): 16-row group / 16-column group of C; the accumulator tile is (fm, fn) = (fr, fc), or (fc, fr) when transposed.
        The tile is zeroed behind its last read-out (bias_gelu: the second pass)."""
        fc = self.fc_of(h, fcl)
        a = acc(*((fc, fr) if self.transposed_out else (fr, fc)))
        for r in range(4):
            self.E(f"v_accvgpr_read_b32 v{base+r}, a{a+r}")
        if h == 1 or not self.bias_gelu:
            for r in range(4):
                self.E(f"v_accvgpr_write_b32 a{a+r}, 0")

    def soff(self, fr, j):
        return S_SOFF + 4 * (fr & 1) + j

    def soffs(self, fr):
        """soffsets of this row group's four stores: (fr*16 + 4 j) rows of C"""
        b = self.soff(fr, 0)
        self.E(f"s_mul_i32 s{b}, s{S_C16}, {4*fr}")
        for j in range(1, 4):
            self.E(f"s_add_u32 s{b+j}, s{b+j-1}, s{S_C16}")

    def unit_loads(self, u):
        fr, h = self.units[u]
        if not (self.geglu_bwd or self.gelu_bwd):
            if h == 0:
                self.soffs(fr)
            if self.second_operand:
                self.operand_loads(u)
            return
        if u == 0:
            self.soffs(0)
            self.operand_loads(0)
        if u + 1 < len(self.units):
            if self.units[u + 1][1] == 0:
                self.soffs(self.units[u + 1][0])      # (the set of row group fr + 1 = that of fr - 1: its stores are out)
            self.operand_loads(u + 1)

    def operand_loads(self, u):
        """the unit's second-operand values: two row pieces (rows fr*16 + 8 j' + (l >> 3)) x 8 columns per lane"""
        E = self.E
        fr, h = self.units[u]
        off = f" offset:{h*128}" if h else ""
        for jp in range(2):
            so = self.soff(fr, 2 * jp)
            if self.gelu_bwd:
                hl = V_HL + 8 * (u % 3) + 4 * jp
                E(f"buffer_load_dwordx4 v[{hl}:{hl+3}], v{V_CO}, s[{RR}:{RR+3}], s{so} offen{off}")
            elif self.geglu_bwd:
                gl = V_GUL + 16 * (u % 3) + 8 * jp
                E(f"buffer_load_dwordx4 v[{gl}:{gl+3}], v{V_CO}, s[{RR}:{RR+3}], s{so} offen{off}")
                E(f"buffer_load_dwordx4 v[{gl+4}:{gl+7}], v{V_COU}, s[{RR}:{RR+3}], s{so} offen{off}")
            else:
                rs = (V_RS0, V_RS1)[u & 1] + 4 * jp
                E(f"buffer_load_dwordx4 v[{rs}:{rs+3}], v{self.vco(h)}, s[{RR}:{RR+3}], s{so} offen{off}")

    def stage_tile(self, u, fcl, cur):
        """one accumulator tile (f32 in cur .. cur + 3) -> the wave's staging buffer"""
        E = self.E
        fr, h = self.units[u]
        fc = self.fc_of(h, fcl)
        if self.bias:
            for r in range(4):
                E(f"v_add_f32 v{cur+r}, v{cur+r}, v{V_BIAS+4*fc+r}")
        if self.stages_f32:
            if self.sumsq:
                for r in range(4):
                    E(f"v_fmac_f32 v{V_SS}, v{cur+r}, v{cur+r}")
            E(f"ds_write_b128 v{V_WA+fcl}, v[{cur}:{cur+3}]")
        elif self.geglu_fwd:
            if fcl == 0:            # soffsets of the unit's two ACT stores: (fr*16 + 8 j) rows of ACT
                E(f"s_mul_i32 s{self.act_soff(fr, 0)}, s{S_LDACT}, {16*fr}")
                E(f"s_lshl_b32 s{self.act_soff(fr, 1)}, s{S_LDACT}, 3")
                E(f"s_add_u32 s{self.act_soff(fr, 1)}, s{self.act_soff(fr, 0)}, s{self.act_soff(fr, 1)}")
            dst = (V_GPK + 2 * fc) if fc < 4 else (cur + 4)       # the gate tiles wait for their up tiles
            E(f"v_cvt_pk_bf16_f32 v{dst}, v{cur}, v{cur+1}")
            E(f"v_cvt_pk_bf16_f32 v{dst+1}, v{cur+2}, v{cur+3}")
            E(f"ds_write_b64 v{V_WA+fcl}, v[{dst}:{dst+1}]")
            if fc >= 4:
                geglu_fwd_piece(E, V_GPK + 2 * (fc - 4), cur + 4)
                E(f"ds_write_b64 v{V_WAA + fc - 4}, v[{V_GP}:{V_GP+1}]")
        else:
            if self.sumsq:      # (bf16 stores: the squares of the f32 accumulator values, 2^-9 relative rounding noise of either sign
                for r in range(4):      #  on each term: the sum differs from the stored values' by ~1e-6 relative)
                    E(f"v_fmac_f32 v{V_SS}, v{cur+r}, v{cur+r}")
            E(f"v_cvt_pk_bf16_f32 v{cur+4}, v{cur}, v{cur+1}")
            E(f"v_cvt_pk_bf16_f32 v{cur+5}, v{cur+2}, v{cur+3}")
            if self.bias_gelu and h == 1:
                gelu_packed(E, cur + 4, cur, (V_GT, V_GT + 1, V_GT2, V_GT2 + 1), V_KG)
            E(f"ds_write_b64 v{V_WA+fcl}, v[{cur+4}:{cur+5}]")

    def unit_read_back(self, u):
        """the unit is written: queue its read-back, store the previous unit"""
        E, nfc = self.E, self.nfc
        cs = V_CS + (u & 1) * 16
        if self.geglu_fwd:      # (12 LDS writes per unit: the previous unit's stores go out before this unit's read-back is queued)
            if u > 0:
                E("s_waitcnt lgkmcnt(12)")
                self.stores(u - 1)
                self.act_stores(u - 1)
            for j in range(4):
                E(f"ds_read_b128 v[{cs+4*j}:{cs+4*j+3}], v{V_RD+j} offset:{j*1024}")
            a = V_AS + (u & 1) * 8
            E(f"ds_read_b128 v[{a}:{a+3}], v{V_SRA}")
            E(f"ds_read_b128 v[{a+4}:{a+7}], v{V_SRA1} offset:1024")
            return
        for j in range(4):
            ro = (j >> 1) * 2048 if self.second_operand else j * 1024
            E(f"ds_read_b128 v[{cs+4*j}:{cs+4*j+3}], v{V_RD+j} offset:{ro}")
        if u > 0:
            E(f"s_waitcnt lgkmcnt({nfc + 4})")
            self.stores(u - 1)

    def stores(self, u):
        """unit u's values are back in V_CS: the epilogue's arithmetic and the stores"""
        E, nu = self.E, len(self.units)
        fr, h = self.units[u]
        cs = V_CS + (u & 1) * 16
        off = f" offset:{h*128}" if h else ""
        # vmcnt: this unit's loaded values; issued behind them are the loads of the units ahead and the stores of as many units before
        if self.gelu_bwd:
            hl = V_HL + 8 * (u % 3)
            E(f"s_waitcnt vmcnt({2 * ((u > 1) + (u > 0) + (u + 1 < nu) + (u + 2 < nu))})")
            for jp in range(2):
                for c in range(2):
                    gelu_bwd_piece(E, cs + 8 * jp + 4 * c, hl + 4 * jp + 2 * c, V_OUT + 2 * c)
                E(f"buffer_store_dwordx4 v[{V_OUT}:{V_OUT+3}], v{V_CO}, s[{RC}:{RC+3}], s{self.soff(fr, 2*jp)} offen{off}{self.st_nt}")
        elif self.geglu_bwd:
            gl = V_GUL + 16 * (u % 3)
            E(f"s_waitcnt vmcnt({4 * ((u > 1) + (u > 0) + (u + 1 < nu) + (u + 2 < nu))})")
            for jp in range(2):
                for c in range(2):
                    if "nomath" not in self.abl:
                        geglu_bwd_piece(E, cs + 8 * jp + 4 * c, gl + 8 * jp + 2 * c, gl + 8 * jp + 4 + 2 * c, V_OG + 2 * c, V_OU + 2 * c)
                E(f"buffer_store_dwordx4 v[{V_OG}:{V_OG+3}], v{V_CO}, s[{RC}:{RC+3}], s{self.soff(fr, 2*jp)} offen{off}{self.st_nt}")
                E(f"buffer_store_dwordx4 v[{V_OU}:{V_OU+3}], v{V_COU}, s[{RC}:{RC+3}], s{self.soff(fr, 2*jp)} offen{off}{self.st_nt}")
        elif self.residual:
            rs = (V_RS0, V_RS1)[u & 1]
            E(f"s_waitcnt vmcnt({2 * ((u > 0) + (u + 1 < nu))})")
            for jp in range(2):
                c = cs + 8 * jp
                for k in range(4):      # 8 residual values of the row piece, two at a time
                    E(f"v_lshlrev_b32 v{V_RT}, 16, v{rs+4*jp+k}")
                    E(f"v_and_b32 v{V_RT+1}, 0xffff0000, v{rs+4*jp+k}")
                    E(f"v_add_f32 v{c+2*k}, v{c+2*k}, v{V_RT}")
                    E(f"v_add_f32 v{c+2*k+1}, v{c+2*k+1}, v{V_RT+1}")
                for k in range(4):
                    E(f"v_cvt_pk_bf16_f32 v{c+k}, v{c+2*k}, v{c+2*k+1}")
                E(f"buffer_store_dwordx4 v[{c}:{c+3}], v{self.vco(h)}, s[{RC}:{RC+3}], s{self.soff(fr, 2*jp)} offen{off}{self.st_nt}")
        else:
            for j in range(4):      # rows fr*16 + 4 j .. + 3
                off = f" offset:{h*256}" if (h and not self.bias_gelu) else ""
                dsc = RR if (self.bias_gelu and h) else RC
                if "nostore" not in self.abl:
                    E(f"buffer_store_dwordx4 v[{cs+4*j}:{cs+4*j+3}], v{self.vco(0 if self.bias_gelu else h)}, s[{dsc}:{dsc+3}], s{self.soff(fr, j)} offen{off}{self.st_nt}")

    def act_soff(self, fr, j):
        return S_ASOFF + 2 * (fr & 1) + j

    def act_stores(self, u):
        fr, h = self.units[u]
        a = V_AS + (u & 1) * 8
        for j in range(2):      # rows fr*16 + 8 j .. + 7 of ACT
            self.E(f"buffer_store_dwordx4 v[{a+4*j}:{a+4*j+3}], v{V_CA}, s[{RACT}:{RACT+3}], s{self.act_soff(fr, j)} offen{self.st_nt}")

    # ---- the kernel, step by step (the names of STEPS)
    def emit(self):
        nm, E = self.name, self.E
        E(".text")
        E(f".protected\t{nm}")
        E(f".globl\t{nm}")
        E(".p2align\t8")
        E(f".type\t{nm},@function")
        E(f"{nm}:")
        self.kernarg_loads()
        self.clear_next_counters()
        self.first_tile()
        self.descriptors()
        for op in (0, 1):
            self.dma_offsets(op)
        for op in (0, 1):
            self.fragment_addresses(op)
        self.epilogue_addresses()
        self.prologue()
        self.main_loop()
        # The stream is two k-tiles into this block's next tile (k-tile 0 landed at the last barrier, k-tile 1 is in flight
        # and is waited for, together with the epilogue's stores, by the vmcnt(0) of the next tile's first barrier)
        self.epilogue()
        self.tail()
        self.kernel_descriptor()

    def kernarg_loads(self):
        """arguments (csrc/gemm_asm.hip AsmArgs): A B C | M N K lda ldb ldc tiles_n magic_group | tiles_m gm_last magic_last
        ntiles | last_is_one gm_shift grid pad; lane and wave id"""
        E = self.E
        E(f"s_load_dwordx4 s[{S_A}:{S_A+3}], s[{S_KARG}:{S_KARG+1}], 0x0")
        E(f"s_load_dwordx2 s[{S_C}:{S_C+1}], s[{S_KARG}:{S_KARG+1}], 0x10")
        E(f"s_load_dwordx8 s[{S_M}:{S_M+7}], s[{S_KARG}:{S_KARG+1}], 0x18")
        E(f"s_load_dwordx2 s[{S_TM}:{S_TM+1}], s[{S_KARG}:{S_KARG+1}], 0x38")
        E(f"s_load_dwordx2 s[{S_MAGL}:{S_MAGL+1}], s[{S_KARG}:{S_KARG+1}], 0x40")
        E(f"s_load_dwordx2 s[{S_ONE}:{S_ONE+1}], s[{S_KARG}:{S_KARG+1}], 0x48")
        E(f"s_load_dword s{S_G}, s[{S_KARG}:{S_KARG+1}], 0x50")
        E(f"s_load_dwordx2 s[{RQ}:{RQ+1}], s[{S_KARG}:{S_KARG+1}], 0x70")
        E(f"s_load_dwordx2 s[{S_T+12}:{S_T+13}], s[{S_KARG}:{S_KARG+1}], 0x78")     # the counters of this stream's NEXT launch (or 0)
        E(f"s_getreg_b32 s{S_XCC}, hwreg(HW_REG_XCC_ID)")
        if self.bias:
            E(f"s_load_dwordx2 s[{RBI}:{RBI+1}], s[{S_KARG}:{S_KARG+1}], 0x60")
        if self.second_pointer:
            E(f"s_load_dwordx2 s[{S_T+8}:{S_T+9}], s[{S_KARG}:{S_KARG+1}], 0x68")
        if self.sumsq:
            E(f"s_load_dwordx2 s[{S_SSP}:{S_SSP+1}], s[{S_KARG}:{S_KARG+1}], 0x68")
            E(f"v_mov_b32 v{V_SS}, 0")
        if self.geglu_fwd:
            E(f"s_load_dwordx2 s[{S_ACT}:{S_ACT+1}], s[{S_KARG}:{S_KARG+1}], 0x68")
            E(f"s_load_dword s{S_LDACT}, s[{S_KARG}:{S_KARG+1}], 0x54")
        E(f"v_and_b32 v{V_LANE}, 63, v{V_TID}")
        E(f"v_lshrrev_b32 v{V_T}, 6, v{V_TID}")
        E("s_nop 1")                                           # VALU write -> v_readfirstlane of the same VGPR: wait state
        E(f"v_readfirstlane_b32 s{S_WAVE}, v{V_T}")
        E("s_nop 4")
        E("s_waitcnt lgkmcnt(0)")
        if self.second_pointer:
            E(f"s_sub_u32 s{S_RDL}, s{S_T+8}, s{S_C}")
            E(f"s_subb_u32 s{S_RDH}, s{S_T+9}, s{S_C+1}")

    def clear_next_counters(self):
        """block 0 clears the counters the next launch on this stream will draw from (nobody uses them now: the launch that
        did is over, the one that will has not started), so the host does not have to memset between launches"""
        E, nm, nxt = self.E, self.name, f"s[{S_T+12}:{S_T+13}]"
        E(f"s_cmp_lg_u32 s{S_WG}, 0")
        E(f"s_cbranch_scc1 .Lzeroed_{nm}")
        E(f"s_cmp_eq_u64 {nxt}, 0")
        E(f"s_cbranch_scc1 .Lzeroed_{nm}")
        E("s_mov_b64 exec, 1")
        for r in range(5):
            E(f"v_mov_b32 v{V_ZERO+r}, 0")
        E(f"global_store_dwordx4 v{V_ZERO+4}, v[{V_ZERO}:{V_ZERO+3}], {nxt}")
        E(f"global_store_dwordx4 v{V_ZERO+4}, v[{V_ZERO}:{V_ZERO+3}], {nxt} offset:16")
        E("s_waitcnt vmcnt(0)")
        E("s_mov_b64 exec, -1")
        E(f".Lzeroed_{nm}:")

    def first_tile(self):
        """this block's first tile (static): 32 (b % 8) + b / 8 — the blocks of an XCD (round-robin dispatch) start on
        consecutive tiles; every further tile is a ticket of the XCD the block really runs on"""
        E, nm, t = self.E, self.name, S_T
        E(f"s_and_b32 s{t}, s{S_WG}, 7")
        E(f"s_lshl_b32 s{t}, s{t}, 5")
        E(f"s_lshr_b32 s{t+1}, s{S_WG}, 3")
        E(f"s_add_u32 s{S_TDMA}, s{t}, s{t+1}")
        E(f"s_cmp_lt_u32 s{S_TDMA}, s{S_NT}")
        E(f"s_cbranch_scc1 .Lhave_work_{nm}")
        E("s_endpgm")
        E(f".Lhave_work_{nm}:")
        E(f"s_and_b32 s{S_XCC}, s{S_XCC}, 7")
        E(f"s_lshl_b32 s{S_XOFF}, s{S_XCC}, 2")
        E(f"s_and_b32 s{RQ+1}, s{RQ+1}, 0xffff")
        E(f"s_mov_b32 s{RQ+2}, 32")
        E(f"s_mov_b32 s{RQ+3}, 0x00020000")
        E(f"s_mov_b32 s{S_HAVE}, 0")
        E(f"s_mov_b32 s{S_REQ}, 0")
        E(f"v_mov_b32 v{V_MB}, {MAILBOX}")

    def descriptors(self):
        """everything in bytes, k-tiles per tile, the buffer descriptors of the first tile"""
        E, t = self.E, S_T
        E(f"s_lshl_b32 s{S_LDA}, s{S_LDA}, 1")         # leading dimensions and K in bytes from here on
        E(f"s_lshl_b32 s{S_LDB}, s{S_LDB}, 1")
        E(f"s_lshl_b32 s{S_LDC}, s{S_LDC}, {2 if self.f32 else 1}")
        E(f"s_lshl_b32 s{S_K}, s{S_K}, 1")
        if self.geglu_fwd:
            E(f"s_lshl_b32 s{S_LDACT}, s{S_LDACT}, 1")
        E(f"s_lshr_b32 s{S_NKT}, s{S_K}, {6 if self.ring else 7}")      # k-tiles (ring: half k-tiles) per tile
        E(f"s_mov_b32 s{S_DLEFT}, s{S_NKT}")
        for op, (bump, ld) in enumerate(((S_BUMPA, S_LDA), (S_BUMPB, S_LDB))):
            if self.kc[op]:
                E(f"s_mov_b32 s{bump}, 128")
            else:
                E(f"s_lshl_b32 s{bump}, s{ld}, {5 if self.ring else 6}")
        E(f"s_mov_b32 s{S_STEPA}, s{S_BUMPA}")
        E(f"s_mov_b32 s{S_STEPB}, s{S_BUMPB}")
        for rs in (RA, RB, RC, RCN):
            E(f"s_mov_b32 s{rs+3}, 0x00020000")
        E(f"s_mul_i32 s{RC+2}, s{S_LDC}, 255")
        E(f"s_add_u32 s{RC+2}, s{RC+2}, {1024 if self.f32 else 512}")
        if self.geglu_bwd:      # C (and GU) rows hold 2 N columns: the up half sits N columns behind the gate half
            E(f"s_lshl_b32 s{t+14}, s{S_N}, 1")
            E(f"s_add_u32 s{RC+2}, s{RC+2}, s{t+14}")
        if self.geglu_fwd:      # a tile's up columns sit N / 2 columns (N bytes) behind its gate columns; ACT descriptor: 256 rows x 128 columns
            E(f"s_add_u32 s{RC+2}, s{RC+2}, s{S_N}")
            E(f"s_mul_i32 s{RACT+2}, s{S_LDACT}, 255")
            E(f"s_add_u32 s{RACT+2}, s{RACT+2}, 256")
            E(f"s_mov_b32 s{RACT+3}, 0x00020000")
        E(f"s_mov_b32 s{RCN+2}, s{RC+2}")
        if self.bias:
            E(f"s_and_b32 s{RBI+1}, s{RBI+1}, 0xffff")
            E(f"s_lshl_b32 s{RBI+2}, s{S_N}, 2")
            E(f"s_mov_b32 s{RBI+3}, 0x00020000")
        self.lines(self.setup(S_TDMA))

    def dma_offsets(self, op):
        """DMA lane offsets (V_DA / V_DB) and piece soffsets (S_OFFA / S_OFFB) of operand op"""
        E, t, W = self.E, S_T, S_WAVE
        soff, ld, vd = ((S_OFFA, S_LDA, V_DA), (S_OFFB, S_LDB, V_DB))[op]
        if op == 0:
            E(f"s_lshl_b32 s{S_W8K}, s{W}, {12 if self.ring else 13}")
        if self.kc[op]:
            # piece j of wave w covers tile rows (8w + j) * 8 .. + 7; lane l: row l >> 3, physical chunk l & 7,
            # logical chunk = physical ^ swz, swz = (row >> 1) & 7 = (l >> 4) [even piece] or (l >> 4) ^ 4 [odd piece]
            E(f"s_lshl_b32 s{t+12}, s{W}, 6")
            if self.geglu_fwd and op == 1:     # tile rows 128 .. 255 (waves 2, 3) are the up rows: N / 2 - 128 rows further on
                E(f"s_lshr_b32 s{t+13}, s{S_N}, 1")
                E(f"s_sub_u32 s{t+13}, s{t+13}, 128")
                E(f"s_cmp_ge_u32 s{W}, 2")
                E(f"s_cselect_b32 s{t+13}, s{t+13}, 0")
                E(f"s_add_u32 s{t+12}, s{t+12}, s{t+13}")
            for j in range(8):
                E(f"s_add_u32 s{t+13}, s{t+12}, {8*j}")
                E(f"s_mul_i32 s{soff+j}, s{t+13}, s{ld}")
            E(f"v_lshrrev_b32 v{V_T}, 3, v{V_LANE}")
            E(f"v_lshrrev_b32 v{V_T+1}, 4, v{V_LANE}")
            E(f"v_and_b32 v{V_E}, 7, v{V_LANE}")
            E(f"v_xor_b32 v{V_E}, v{V_E}, v{V_T+1}")
            E(f"v_xor_b32 v{V_E+1}, 4, v{V_E}")
            E(f"v_lshlrev_b32 v{V_E}, 4, v{V_E}")
            E(f"v_lshlrev_b32 v{V_E+1}, 4, v{V_E+1}")
            E(f"v_mul_lo_u32 v{V_E+2}, v{V_T}, s{ld}")
            E(f"v_add_u32 v{vd}, v{V_E+2}, v{V_E}")
            E(f"v_add_u32 v{vd+1}, v{V_E+2}, v{V_E+1}")
            return
        # piece j of wave w covers k-rows (8w + j) * 2 .. + 1; lane l: row hi = l >> 5, physical chunk l & 31,
        # logical chunk = physical ^ (mc_swz(k) << 1), mc_swz(k) = (k & 3) | (((k >> 3) & 1) << 2) with
        # k & 3 = 2 (j & 1) + hi and (k >> 3) & 1 = (j >> 2) & 1: four classes of pieces c = (j & 1) + 2 ((j >> 2) & 1)
        # (ring: piece j of wave w covers k-rows 8 w + 2 j, + 1 of the 32-deep half: k & 3 = 2 (j & 1) + hi, (k >> 3) & 1 = w & 1:
        # two classes of pieces c = j & 1, the wave's parity folded into both)
        E(f"s_lshl_b32 s{t+12}, s{W}, {3 if self.ring else 4}")
        for j in range(4 if self.ring else 8):
            E(f"s_add_u32 s{t+13}, s{t+12}, {2*j}")
            E(f"s_mul_i32 s{soff+j}, s{t+13}, s{ld}")
        E(f"v_lshrrev_b32 v{V_T}, 5, v{V_LANE}")              # hi
        E(f"v_and_b32 v{V_T+1}, 31, v{V_LANE}")               # physical chunk
        E(f"v_mul_lo_u32 v{V_E+2}, v{V_T}, s{ld}")
        if self.ring:
            E(f"s_and_b32 s{t+13}, s{W}, 1")
            E(f"s_lshl_b32 s{t+13}, s{t+13}, 2")
        for c in range(2 if self.ring else 4):
            swz0 = 2 * (c & 1) + 4 * (c >> 1)                   # + hi
            E(f"v_add_u32 v{V_E}, {swz0}, v{V_T}")
            if self.ring:
                E(f"v_add_u32 v{V_E}, s{t+13}, v{V_E}")
            E(f"v_lshlrev_b32 v{V_E}, 1, v{V_E}")
            E(f"v_xor_b32 v{V_E}, v{V_E}, v{V_T+1}")
            E(f"v_lshlrev_b32 v{V_E}, 4, v{V_E}")
            E(f"v_add_u32 v{vd+c}, v{V_E+2}, v{V_E}")

    def fragment_addresses(self, op):
        """fragment read addresses (V_RA / V_RB) of operand op; lane (i = l & 15, g = l >> 4)"""
        E, t = self.E, S_T
        if op == 0:
            E(f"s_lshr_b32 s{t+12}, s{S_WAVE}, 1")                          # wm
            E(f"s_and_b32 s{t+13}, s{S_WAVE}, 1")                           # wn
        VR, wreg, boff = ((V_RA, t + 12, 0), (V_RB, t + 13, 16384 if self.ring else BOFF))[op]
        if self.kc[op]:
            # rows w?*128 + 16 f + i, chunk (4 kk + g) ^ ((i >> 1) & 7): registers VR + 2 stage + kk
            E(f"v_and_b32 v{V_E}, 15, v{V_LANE}")
            E(f"v_lshrrev_b32 v{V_E+1}, 4, v{V_LANE}")
            E(f"v_bfe_u32 v{V_E+2}, v{V_LANE}, 1, 3")
            E(f"v_xor_b32 v{V_E+3}, v{V_E+1}, v{V_E+2}")
            E(f"v_xor_b32 v{V_E+4}, 4, v{V_E+3}")
            E(f"v_lshlrev_b32 v{V_E+3}, 4, v{V_E+3}")
            E(f"v_lshlrev_b32 v{V_E+4}, 4, v{V_E+4}")
            E(f"v_lshlrev_b32 v{V_E}, 7, v{V_E}")
            E(f"s_lshl_b32 s{t+14}, s{wreg}, {13 if (self.geglu_fwd and op == 1) else 14}")    # (geglu_fwd: the wave's 64 gate rows)
            if boff:
                E(f"s_add_u32 s{t+14}, s{t+14}, {boff}")
            for kk in (0, 1):
                E(f"v_add_u32 v{VR+kk}, v{V_E}, v{V_E+3+kk}")
                E(f"v_add_u32 v{VR+kk}, s{t+14}, v{VR+kk}")
                E(f"v_add_u32 v{VR+2+kk}, {STAGE}, v{VR+kk}")
            return
        # k-row 8 g + (i >> 2) (+ 32 kk, + 4 for the second half), columns w?*128 + 16 f + 4 (i & 3):
        # chunk = (16 w? + 2 f + ((i & 3) >> 1)) ^ (mc_swz << 1), mc_swz = (i >> 2) | ((g & 1) << 2); + 8 bytes if i & 1.
        # registers VR + 8 stage + f  (f enters by XOR of f << 5)
        E(f"v_and_b32 v{V_E}, 15, v{V_LANE}")                  # i
        E(f"v_lshrrev_b32 v{V_E+1}, 4, v{V_LANE}")             # g
        E(f"v_lshrrev_b32 v{V_E+2}, 2, v{V_E}")                # i >> 2
        E(f"v_lshlrev_b32 v{V_E+3}, 3, v{V_E+1}")              # 8 g
        E(f"v_add_u32 v{V_E+3}, v{V_E+3}, v{V_E+2}")           # k-row
        E(f"v_lshlrev_b32 v{V_E+3}, 9, v{V_E+3}")              # * 512
        E(f"v_and_b32 v{V_E+4}, 1, v{V_E+1}")                  # g & 1
        E(f"v_lshlrev_b32 v{V_E+4}, 2, v{V_E+4}")
        E(f"v_or_b32 v{V_E+4}, v{V_E+4}, v{V_E+2}")            # mc_swz
        E(f"v_lshlrev_b32 v{V_E+4}, 1, v{V_E+4}")              # << 1
        E(f"v_bfe_u32 v{V_E+5}, v{V_LANE}, 1, 1")              # (i & 3) >> 1
        E(f"s_lshl_b32 s{t+14}, s{wreg}, 4")                   # 16 w?
        E(f"v_or_b32 v{V_E+5}, s{t+14}, v{V_E+5}")
        E(f"v_xor_b32 v{V_E+5}, v{V_E+5}, v{V_E+4}")           # chunk of f = 0
        E(f"v_lshlrev_b32 v{V_E+5}, 4, v{V_E+5}")
        E(f"v_and_b32 v{V_E+6}, 1, v{V_LANE}")                 # i & 1
        E(f"v_lshlrev_b32 v{V_E+6}, 3, v{V_E+6}")
        E(f"v_add_u32 v{V_E+5}, v{V_E+5}, v{V_E+6}")
        E(f"v_add_u32 v{V_E+5}, v{V_E+5}, v{V_E+3}")
        if boff:
            E(f"v_add_u32 v{V_E+5}, {boff}, v{V_E+5}")
        for f in range(8):
            E(f"v_xor_b32 v{VR+f}, {f << 5}, v{V_E+5}")
            E(f"v_add_u32 v{VR+8+f}, {STAGE}, v{VR+f}")

    def epilogue_addresses(self):
        """the lane's addresses in the wave's staging buffer (V_SW, V_SR) and its store offset in a C tile (V_CO).
        Accumulator tile (fr, fc) of the wave: lane (i = l & 15, g = l >> 4) holds C row fr*16 + i, columns fc*16 + 4 g .. + 3.
        Staging buffer of the wave: [16 rows][256 B], 16-byte chunk c of row r at chunk c ^ r.  bf16: one buffer = a whole row
        group (128 columns), the lane's 8 bytes of tile fc are chunk 2 fc + (g >> 1), half g & 1; f32: one buffer = half a
        row group (64 columns), the lane's 16 bytes of tile fc (fc & 3) are chunk 4 (fc & 3) + g.  Read back as 4 rows x 256 B
        per instruction: lane -> row 4 j + (l >> 4), chunk l & 15; stored as 4 full rows of 256 contiguous bytes."""
        E, t = self.E, S_T
        wrow, wcol = (t + 13, t + 12) if self.transposed_out else (t + 12, t + 13)      # (wm, wn of fragment_addresses)
        E(f"v_and_b32 v{V_E}, 15, v{V_LANE}")                      # i
        E(f"v_lshrrev_b32 v{V_E+1}, 4, v{V_LANE}")                 # g
        if self.stages_f32:
            E(f"v_xor_b32 v{V_E+2}, v{V_E+1}, v{V_E}")             # g ^ i
            E(f"v_lshlrev_b32 v{V_E+2}, 4, v{V_E+2}")
        else:
            E(f"v_lshrrev_b32 v{V_E+2}, 1, v{V_E+1}")              # g >> 1
            E(f"v_xor_b32 v{V_E+2}, v{V_E+2}, v{V_E}")
            E(f"v_lshlrev_b32 v{V_E+2}, 4, v{V_E+2}")
            E(f"v_and_b32 v{V_E+3}, 1, v{V_E+1}")
            E(f"v_lshlrev_b32 v{V_E+3}, 3, v{V_E+3}")
            E(f"v_add_u32 v{V_E+2}, v{V_E+2}, v{V_E+3}")
        E(f"v_lshlrev_b32 v{V_E+3}, 8, v{V_E}")                    # i * 256
        E(f"v_add_u32 v{V_E+2}, v{V_E+2}, v{V_E+3}")
        E(f"s_lshl_b32 s{t+14}, s{S_WAVE}, 12")
        E(f"s_add_u32 s{t+14}, s{t+14}, {CSTAGE}")
        E(f"v_add_u32 v{V_SW}, s{t+14}, v{V_E+2}")
        E(f"v_xor_b32 v{V_E+2}, v{V_E}, v{V_E+1}")                 # (l & 15) ^ (l >> 4)
        E(f"v_lshlrev_b32 v{V_E+2}, 4, v{V_E+2}")
        E(f"v_lshlrev_b32 v{V_E+3}, 8, v{V_E+1}")                  # (l >> 4) * 256
        E(f"v_add_u32 v{V_E+2}, v{V_E+2}, v{V_E+3}")
        E(f"v_add_u32 v{V_SR}, s{t+14}, v{V_E+2}")
        # store offset: row w?*128 + (l >> 4), bytes w?*(128 elements) + (l & 15) * 16
        # (second-operand epilogues: row w?*128 + (l >> 3), bytes w?*256 + (l & 7) * 16: 8 bf16 columns per lane)
        if self.second_operand:
            E(f"v_and_b32 v{V_E}, 7, v{V_LANE}")
            E(f"v_lshrrev_b32 v{V_E+1}, 3, v{V_LANE}")
        E(f"s_lshl_b32 s{t+14}, s{wrow}, 7")
        E(f"v_add_u32 v{V_E+1}, s{t+14}, v{V_E+1}")
        E(f"v_mul_lo_u32 v{V_E+1}, v{V_E+1}, s{S_LDC}")
        E(f"v_lshlrev_b32 v{V_E}, 4, v{V_E}")
        E(f"s_lshl_b32 s{t+14}, s{wcol}, {9 if self.f32 else 8}")
        E(f"v_add_u32 v{V_E}, v{V_E}, v{V_E+1}")
        E(f"v_add_u32 v{V_CO}, s{t+14}, v{V_E}")
        if self.geglu_bwd:
            E(f"s_lshl_b32 s{t+14}, s{S_N}, 1")
            E(f"v_add_u32 v{V_COU}, s{t+14}, v{V_CO}")
        if self.geglu_fwd:
            self.geglu_fwd_addresses(wrow, wcol)
        E(f"s_lshl_b32 s{S_C16}, s{S_LDC}, 2")                     # FOUR rows of C in bytes
        if self.bias:
            E(f"v_lshrrev_b32 v{V_NCOL}, 4, v{V_LANE}")
            E(f"v_lshlrev_b32 v{V_NCOL}, 2, v{V_NCOL}")
            E(f"s_lshl_b32 s{t+14}, s{t+13}, 7")
            E(f"v_add_u32 v{V_NCOL}, s{t+14}, v{V_NCOL}")

    def geglu_fwd_addresses(self, wrow, wcol):
        """geglu_fwd: V_CO of the gate | up stores, V_CA of the ACT stores, V_SWA / V_SRA in the ACT staging buffer"""
        E, t = self.E, S_T
        # gate | up stores: lane -> row (l >> 4) (+ wm * 128), chunk l & 15 of the unit's [64 gate | 64 up] columns:
        # bytes wn*128 + (l & 7) * 16, + N (= N / 2 columns) for the up chunks 8 .. 15.   (v{V_E+1} = row * ldc)
        E(f"v_and_b32 v{V_E}, 7, v{V_LANE}")
        E(f"v_lshlrev_b32 v{V_E}, 4, v{V_E}")
        E(f"v_bfe_u32 v{V_E+2}, v{V_LANE}, 3, 1")
        E(f"v_mul_lo_u32 v{V_E+2}, v{V_E+2}, s{S_N}")
        E(f"v_add_u32 v{V_E}, v{V_E}, v{V_E+2}")
        E(f"s_lshl_b32 s{t+14}, s{wcol}, 7")
        E(f"v_add_u32 v{V_E}, s{t+14}, v{V_E}")
        E(f"v_add_u32 v{V_CO}, v{V_E}, v{V_E+1}")
        # ACT stores: lane -> row (l >> 3) (+ wm * 128), bytes wn*128 + (l & 7) * 16
        E(f"v_lshrrev_b32 v{V_E+2}, 3, v{V_LANE}")
        E(f"s_lshl_b32 s{t+14}, s{wrow}, 7")
        E(f"v_add_u32 v{V_E+2}, s{t+14}, v{V_E+2}")
        E(f"v_mul_lo_u32 v{V_E+2}, v{V_E+2}, s{S_LDACT}")
        E(f"v_and_b32 v{V_E}, 7, v{V_LANE}")
        E(f"v_lshlrev_b32 v{V_E}, 4, v{V_E}")
        E(f"s_lshl_b32 s{t+14}, s{wcol}, 7")
        E(f"v_add_u32 v{V_E}, s{t+14}, v{V_E}")
        E(f"v_add_u32 v{V_CA}, v{V_E}, v{V_E+2}")
        # ACT staging buffer of the wave: [16 rows][128 B], 16-byte chunk c of row r at chunk c ^ ((r >> 1) & 7).
        # write: lane (i, g) -> row i, chunk 2 fc + (g >> 1), half g & 1 (fc enters by XOR of fc * 32)
        E(f"v_and_b32 v{V_E}, 15, v{V_LANE}")                      # i
        E(f"v_lshrrev_b32 v{V_E+1}, 4, v{V_LANE}")                 # g
        E(f"v_lshrrev_b32 v{V_E+2}, 1, v{V_E+1}")                  # g >> 1
        E(f"v_bfe_u32 v{V_E+3}, v{V_LANE}, 1, 3")                  # (i >> 1) & 7
        E(f"v_xor_b32 v{V_E+2}, v{V_E+2}, v{V_E+3}")
        E(f"v_lshlrev_b32 v{V_E+2}, 4, v{V_E+2}")
        E(f"v_and_b32 v{V_E+3}, 1, v{V_E+1}")
        E(f"v_lshlrev_b32 v{V_E+3}, 3, v{V_E+3}")
        E(f"v_add_u32 v{V_E+2}, v{V_E+2}, v{V_E+3}")
        E(f"v_lshlrev_b32 v{V_E+3}, 7, v{V_E}")                    # i * 128
        E(f"v_add_u32 v{V_E+2}, v{V_E+2}, v{V_E+3}")
        E(f"s_lshl_b32 s{t+14}, s{S_WAVE}, 11")
        E(f"s_add_u32 s{t+14}, s{t+14}, {ASTAGE}")
        E(f"v_add_u32 v{V_SWA}, s{t+14}, v{V_E+2}")
        # read back: lane -> row 8 j + (l >> 3), chunk (l & 7) ^ (l >> 4) ^ 4 j  (j enters by XOR of 64 and + 1024)
        E(f"v_and_b32 v{V_E+2}, 7, v{V_LANE}")
        E(f"v_xor_b32 v{V_E+2}, v{V_E+2}, v{V_E+1}")
        E(f"v_lshlrev_b32 v{V_E+2}, 4, v{V_E+2}")
        E(f"v_lshrrev_b32 v{V_E+3}, 3, v{V_LANE}")
        E(f"v_lshlrev_b32 v{V_E+3}, 7, v{V_E+3}")
        E(f"v_add_u32 v{V_E+2}, v{V_E+2}, v{V_E+3}")
        E(f"v_add_u32 v{V_SRA}, s{t+14}, v{V_E+2}")

    def take_next_tile(self):
        """the tile the stream has been fetching becomes the tile of the coming loop and epilogue"""
        E = self.E
        for r in range(3):
            E(f"s_mov_b32 s{RC+r}, s{RCN+r}")
        if self.geglu_fwd:
            E(f"s_mov_b32 s{RACT}, s{S_ACTNL}")
            E(f"s_mov_b32 s{RACT+1}, s{S_ACTNH}")
        if self.bias:
            E(f"s_mov_b32 s{S_NREM}, s{S_NREMN}")

    def prologue(self):
        """k-tiles 0 and 1 of the first tile in flight (ring: half k-tiles 0 .. 3), accumulators cleared, first fragments read"""
        E = self.E
        for stage in ((0, 1, 2, 3) if self.ring else (0, 1)):
            for m0w, ld in (self.dma_ring(stage) if self.ring else self.dma(stage)):
                E(m0w)
                E("s_nop 0")
                E(ld)
            self.lines(self.stream_step())
        for a in range(256):
            E(f"v_accvgpr_write_b32 a{a}, 0")
        self.take_next_tile()
        E("s_waitcnt vmcnt(24)" if self.ring else "s_waitcnt vmcnt(16)")
        E("s_barrier")
        self.lines(self.reads_ring(0, 0) if self.ring else self.reads(0, 0, 0))
        E("s_waitcnt lgkmcnt(0)")

    def main_loop(self):
        E, nm = self.E, self.name
        E(f".Ltile_{nm}:")
        E(f"s_lshr_b32 s{S_LOOP}, s{S_NKT}, {2 if self.ring else 1}")
        E(f".Lloop_{nm}:")
        if self.ring:
            for ph in range(4):
                self.phase_ring(ph)
        else:
            self.ktile(0)
            self.ktile(1)
        E(f"s_sub_u32 s{S_LOOP}, s{S_LOOP}, 1")
        E(f"s_cmp_lg_u32 s{S_LOOP}, 0")
        E(f"s_cbranch_scc1 .Lloop_{nm}")

    def tail(self):
        """on to the block's next tile, or out of tiles: the sum of squares, end"""
        E, nm, t = self.E, self.name, S_T
        E(f"s_cmp_lg_u32 s{S_HAVE}, 0")
        E(f"s_cbranch_scc1 .Lnext_{nm}")
        if self.sumsq:
            # the wave's 64 running sums through its staging buffer, added up in lane order by every lane, one atomic
            E(f"s_cmp_eq_u64 s[{S_SSP}:{S_SSP+1}], 0")
            E(f"s_cbranch_scc1 .Lno_ss_{nm}")
            E(f"s_lshl_b32 s{t+12}, s{S_WAVE}, 12")
            E(f"s_add_u32 s{t+12}, s{t+12}, {CSTAGE}")
            E(f"v_lshlrev_b32 v{V_E}, 2, v{V_LANE}")
            E(f"v_add_u32 v{V_E}, s{t+12}, v{V_E}")
            E("s_waitcnt lgkmcnt(0)")
            E(f"ds_write_b32 v{V_E}, v{V_SS}")
            E(f"v_mov_b32 v{V_E+1}, s{t+12}")
            E("s_waitcnt lgkmcnt(0)")
            for k in range(16):
                E(f"ds_read_b128 v[{V_CS+4*(k % 8)}:{V_CS+4*(k % 8)+3}], v{V_E+1} offset:{16*k}")
                if k % 8 == 7:
                    E("s_waitcnt lgkmcnt(0)")
                    if k == 7:
                        E(f"v_mov_b32 v{V_E+2}, 0")
                    for q in range(32):
                        E(f"v_add_f32 v{V_E+2}, v{V_E+2}, v{V_CS+q}")
            E(f"v_mov_b32 v{V_E+3}, 0")
            E("s_mov_b64 exec, 1")
            E(f"global_atomic_add_f32 v{V_E+3}, v{V_E+2}, s[{S_SSP}:{S_SSP+1}]")
            E("s_mov_b64 exec, -1")
            E("s_waitcnt vmcnt(0)")
            E(f".Lno_ss_{nm}:")
        E("s_endpgm")
        E(f".Lnext_{nm}:")     # (register set 0 already holds the next tile's first fragments: the last P1 read them)
        E(f"s_mov_b32 s{S_HAVE}, 0")
        self.take_next_tile()
        E(f"s_branch .Ltile_{nm}")

    def kernel_descriptor(self):
        E = self.E
        E(".section\t.rodata,\"a\",@progbits")
        E(".p2align\t6, 0x0")
        E(f".amdhsa_kernel {self.name}")
        for k, v in (("group_segment_fixed_size", MAILBOX + 64), ("private_segment_fixed_size", 0), ("kernarg_size", 128),
                     ("user_sgpr_count", 2), ("user_sgpr_dispatch_ptr", 0), ("user_sgpr_queue_ptr", 0), ("user_sgpr_kernarg_segment_ptr", 1),
                     ("user_sgpr_dispatch_id", 0), ("user_sgpr_kernarg_preload_length", 0), ("user_sgpr_kernarg_preload_offset", 0),
                     ("user_sgpr_private_segment_size", 0), ("uses_dynamic_stack", 0), ("enable_private_segment", 0),
                     ("system_sgpr_workgroup_id_x", 1), ("system_sgpr_workgroup_id_y", 0), ("system_sgpr_workgroup_id_z", 0),
                     ("system_sgpr_workgroup_info", 0), ("system_vgpr_workitem_id", 0), ("next_free_vgpr", self.nvgpr + 256), ("next_free_sgpr", NSGPR),
                     ("accum_offset", self.nvgpr), ("reserve_vcc", 1), ("float_round_mode_32", 0), ("float_round_mode_16_64", 0),
                     ("float_denorm_mode_32", 3), ("float_denorm_mode_16_64", 3), ("dx10_clamp", 1), ("ieee_mode", 1), ("fp16_overflow", 0),
                     ("tg_split", 0), ("exception_fp_ieee_invalid_op", 0), ("exception_fp_denorm_src", 0), ("exception_fp_ieee_div_zero", 0),
                     ("exception_fp_ieee_overflow", 0), ("exception_fp_ieee_underflow", 0), ("exception_fp_ieee_inexact", 0),
                     ("exception_int_div_zero", 0)):
            E(f"\t.amdhsa_{k} {v}")
        E(".end_amdhsa_kernel")

    def meta(self):
        return f"""  - .agpr_count:     256
    .args:
      - .offset:         0
        .size:           128
        .value_kind:     by_value
    .group_segment_fixed_size: {MAILBOX + 64}
    .kernarg_segment_align: 8
    .kernarg_segment_size: 128
    .max_flat_workgroup_size: 256
    .name:           {self.name}
    .private_segment_fixed_size: 0
    .sgpr_count:     106
    .sgpr_spill_count: 0
    .symbol:         {self.name}.kd
    .uniform_work_group_size: 1
    .uses_dynamic_stack: false
    .vgpr_count:     {self.nvgpr + 256}
    .vgpr_spill_count: 0
    .wavefront_size: 64"""


# ---- the arithmetic of the fused epilogues: E = the emitter's line method; inputs and outputs are the arguments, the temporaries
# V_GX .. V_GO of the register map.  With k0 = sqrt(2/pi), k1 = 0.044715 and s = sigmoid(2 k0 (x + k1 x^3)):
# gelu(x) = x s,  gelu'(x) = s + 2 x s (1 - s) k0 (1 + 3 k1 x^2).
K1P, C3 = "0xbdd2d3e8", "0x3ddb33b6"      # -2 log2(e) k0 k1 = -0.10294324, 3 k0 k1 = 0.10703222


def unpack_bf16(E, dst, src):
    """src, src+1 = 4 bf16 values (pairs) -> f32 in dst .. dst+3"""
    for k in range(2):
        E(f"v_lshlrev_b32 v{dst+2*k}, 16, v{src+k}")
        E(f"v_and_b32 v{dst+2*k+1}, 0xffff0000, v{src+k}")


def gelu_bwd_piece(E, c, hl, out):
    """4 outputs of one row piece: c..c+3 = d(a) (f32, unrounded), hl, hl+1 = 4 pre-activations (bf16 pairs); leaves
    d(h) = bf16(d(a)) * gelu'(h) packed in out, out+1."""
    X, U, X2, P, O = V_GX, V_GU_, V_GX2, V_GP, V_GO
    E(f"v_cvt_pk_bf16_f32 v{P}, v{c}, v{c+1}")
    E(f"v_cvt_pk_bf16_f32 v{P+1}, v{c+2}, v{c+3}")
    unpack_bf16(E, X, hl)
    unpack_bf16(E, c, P)
    for e in range(4): E(f"v_mul_f32 v{X2+e}, v{X+e}, v{X+e}")
    for e in range(4): E(f"v_fmamk_f32 v{P+e}, v{X2+e}, {K1P}, v{V_GK0}")
    for e in range(4): E(f"v_mul_f32 v{P+e}, v{X+e}, v{P+e}")
    for e in range(4): E(f"v_exp_f32 v{P+e}, v{P+e}")
    for e in range(4): E(f"v_add_f32 v{P+e}, 1.0, v{P+e}")
    for e in range(4): E(f"v_rcp_f32 v{P+e}, v{P+e}")                              # s
    for e in range(4): E(f"v_fmamk_f32 v{X2+e}, v{X2+e}, {C3}, v{V_GK1}")
    for e in range(4): E(f"v_sub_f32 v{O+e}, 1.0, v{P+e}")
    for e in range(4): E(f"v_mul_f32 v{O+e}, v{X+e}, v{O+e}")
    for e in range(4): E(f"v_mul_f32 v{O+e}, v{O+e}, v{X2+e}")
    for e in range(4): E(f"v_add_f32 v{O+e}, v{O+e}, v{O+e}")
    for e in range(4): E(f"v_fma_f32 v{O+e}, v{P+e}, v{O+e}, v{P+e}")              # gelu'
    for e in range(4): E(f"v_mul_f32 v{U+e}, v{c+e}, v{O+e}")
    E(f"v_cvt_pk_bf16_f32 v{out}, v{U}, v{U+1}")
    E(f"v_cvt_pk_bf16_f32 v{out+1}, v{U+2}, v{U+3}")


def geglu_bwd_piece(E, c, gl, ul, outg, outu):
    """4 outputs of one row piece: c..c+3 = d(act) (f32, unrounded), gl, gl+1 = 4 gate values (bf16 pairs), ul, ul+1 = 4 up values.
    Leaves d(gate) packed in outg, outg+1 and d(up) packed in outu, outu+1."""
    X, U, X2, P, G, O = V_GX, V_GU_, V_GX2, V_GP, V_GG, V_GO
    E(f"v_cvt_pk_bf16_f32 v{P}, v{c}, v{c+1}")             # d(act) as the stand-alone product stores it
    E(f"v_cvt_pk_bf16_f32 v{P+1}, v{c+2}, v{c+3}")
    for k in range(2):
        E(f"v_lshlrev_b32 v{X+2*k}, 16, v{gl+k}")
        E(f"v_and_b32 v{X+2*k+1}, 0xffff0000, v{gl+k}")
        E(f"v_lshlrev_b32 v{U+2*k}, 16, v{ul+k}")
        E(f"v_and_b32 v{U+2*k+1}, 0xffff0000, v{ul+k}")
    unpack_bf16(E, c, P)
    for e in range(4): E(f"v_mul_f32 v{X2+e}, v{X+e}, v{X+e}")
    for e in range(4): E(f"v_fmamk_f32 v{P+e}, v{X2+e}, {K1P}, v{V_GK0}")          # -2 log2(e) k0 (1 + k1 x^2)
    for e in range(4): E(f"v_mul_f32 v{P+e}, v{X+e}, v{P+e}")
    for e in range(4): E(f"v_exp_f32 v{P+e}, v{P+e}")                              # exp(-2 u)
    for e in range(4): E(f"v_add_f32 v{P+e}, 1.0, v{P+e}")
    for e in range(4): E(f"v_rcp_f32 v{P+e}, v{P+e}")                              # s
    for e in range(4): E(f"v_fmamk_f32 v{X2+e}, v{X2+e}, {C3}, v{V_GK1}")          # k0 (1 + 3 k1 x^2)
    for e in range(4): E(f"v_mul_f32 v{G+e}, v{X+e}, v{P+e}")                      # gelu
    for e in range(4): E(f"v_sub_f32 v{O+e}, 1.0, v{P+e}")
    for e in range(4): E(f"v_mul_f32 v{O+e}, v{X+e}, v{O+e}")
    for e in range(4): E(f"v_mul_f32 v{O+e}, v{O+e}, v{X2+e}")
    for e in range(4): E(f"v_add_f32 v{O+e}, v{O+e}, v{O+e}")
    for e in range(4): E(f"v_fma_f32 v{O+e}, v{P+e}, v{O+e}, v{P+e}")              # gelu'
    for e in range(4): E(f"v_mul_f32 v{U+e}, v{c+e}, v{U+e}")
    for e in range(4): E(f"v_mul_f32 v{U+e}, v{U+e}, v{O+e}")                      # d(gate)
    E(f"v_cvt_pk_bf16_f32 v{X}, v{G}, v{G+1}")                                      # bf16(gelu)
    E(f"v_cvt_pk_bf16_f32 v{X+1}, v{G+2}, v{G+3}")
    unpack_bf16(E, G, X)
    for e in range(4): E(f"v_mul_f32 v{G+e}, v{c+e}, v{G+e}")                      # d(up)
    E(f"v_cvt_pk_bf16_f32 v{outg}, v{U}, v{U+1}")
    E(f"v_cvt_pk_bf16_f32 v{outg+1}, v{U+2}, v{U+3}")
    E(f"v_cvt_pk_bf16_f32 v{outu}, v{G}, v{G+1}")
    E(f"v_cvt_pk_bf16_f32 v{outu+1}, v{G+2}, v{G+3}")


def geglu_fwd_piece(E, gp, up):
    """4 outputs: gp, gp+1 = 4 gate values (packed bf16), up, up+1 = 4 up values; leaves bf16(bf16(gelu(gate)) * up) packed in
    V_GP, V_GP+1."""
    X, U, P = V_GX, V_GU_, V_GP
    for k in range(2):
        E(f"v_lshlrev_b32 v{X+2*k}, 16, v{gp+k}")
        E(f"v_and_b32 v{X+2*k+1}, 0xffff0000, v{gp+k}")
        E(f"v_lshlrev_b32 v{U+2*k}, 16, v{up+k}")
        E(f"v_and_b32 v{U+2*k+1}, 0xffff0000, v{up+k}")
    for e in range(4): E(f"v_mul_f32 v{P+e}, v{X+e}, v{X+e}")
    for e in range(4): E(f"v_fmamk_f32 v{P+e}, v{P+e}, {K1P}, v{V_GK0}")
    for e in range(4): E(f"v_mul_f32 v{P+e}, v{X+e}, v{P+e}")
    for e in range(4): E(f"v_exp_f32 v{P+e}, v{P+e}")
    for e in range(4): E(f"v_add_f32 v{P+e}, 1.0, v{P+e}")
    for e in range(4): E(f"v_rcp_f32 v{P+e}, v{P+e}")
    for e in range(4): E(f"v_mul_f32 v{P+e}, v{X+e}, v{P+e}")                      # gelu
    E(f"v_cvt_pk_bf16_f32 v{X}, v{P}, v{P+1}")
    E(f"v_cvt_pk_bf16_f32 v{X+1}, v{P+2}, v{P+3}")
    unpack_bf16(E, P, X)
    for e in range(4): E(f"v_mul_f32 v{P+e}, v{P+e}, v{U+e}")
    E(f"v_cvt_pk_bf16_f32 v{P}, v{P}, v{P+1}")
    E(f"v_cvt_pk_bf16_f32 v{P+1}, v{P+2}, v{P+3}")


def gelu_packed(E, pk, X, P, kg):
    """pk, pk+1 = 4 bf16 values h -> bf16(gelu(h)) in place; X: the first of four scratch registers, P: four more, kg: the
    register that holds -2 log2(e) k0"""
    unpack_bf16(E, X, pk)
    for e in range(4): E(f"v_mul_f32 v{P[e]}, v{X+e}, v{X+e}")
    for e in range(4): E(f"v_fmamk_f32 v{P[e]}, v{P[e]}, {K1P}, v{kg}")
    for e in range(4): E(f"v_mul_f32 v{P[e]}, v{X+e}, v{P[e]}")
    for e in range(4): E(f"v_exp_f32 v{P[e]}, v{P[e]}")
    for e in range(4): E(f"v_add_f32 v{P[e]}, 1.0, v{P[e]}")
    for e in range(4): E(f"v_rcp_f32 v{P[e]}, v{P[e]}")
    for e in range(4): E(f"v_mul_f32 v{P[e]}, v{X+e}, v{P[e]}")
    E(f"v_cvt_pk_bf16_f32 v{pk}, v{P[0]}, v{P[1]}")
    E(f"v_cvt_pk_bf16_f32 v{pk+1}, v{P[2]}, v{P[3]}")


def generate(options=Options()):
    """the whole of gemm_asm_kernels.s"""
    em = Emitter()
    kernels = [Kernel(spec, options, em) for spec in KERNELS]
    em.line('.amdgcn_target "amdgcn-amd-amdhsa--gfx950"')
    em.line(".amdhsa_code_object_version 6")
    for k in kernels:
        k.emit()
    em.line(".text")
    em.raw("\t.amdgpu_metadata\n---\namdhsa.kernels:")
    for k in kernels:
        em.raw(k.meta())
    em.raw("amdhsa.target:   amdgcn-amd-amdhsa--gfx950\namdhsa.version:\n  - 1\n  - 2\n...\n\n\t.end_amdgpu_metadata")
    return em.text()


def main():
    import os

    sys.stdout.write(generate(Options.from_env(os.environ)))


if __name__ == "__main__":
    main()
