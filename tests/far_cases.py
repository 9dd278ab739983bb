"""Far-offset cases: the GEMM and attention launchers at the far end of their 32-bit byte offsets (include/dinov2_hip_ops.h, "Far operands").
Imported by tests/test_far_probes.py (CPU: the pattern, the byte products, the planner, the break-it check of the samples) and
tests/test_gpu_far.py (the kernels).  Plain module, no fixtures.

The limits.  launch_gemm refuses M * lda * 2 >= 2^32 and N * ldw * 2 >= 2^32 (stamp_args, csrc/gemm.hip); launch_attention refuses
B * T * 3H * 2 >= 2^32; a pass of the forward keeps rows * widest_row * 2 < 2^31 (dinov2_max_pass_batch).  Every case below sits at such a
limit in BYTES and is as small as it can be otherwise: small N and K, a row stride instead of dense rows.

The operands come from far_value (csrc/far_pattern.h, restated here): multiples of 1/64 in [-1, 1), exact in f16 and bf16.  With both GEMM
operands on that grid and K <= 4096 every product is a multiple of 2^-12 of magnitude <= 1 and every partial sum has 12 fraction bits and at
most 12 integer bits: exact in f32 in any summation order.
"""
from dataclasses import dataclass, field

import numpy as np

F16, BF16 = 0, 1
DT_NAME = {F16: "f16", BF16: "bf16"}
EPI_QKV, EPI_RESID, EPI_GELU, EPI_SWIGLU, EPI_PLAIN_F32 = 1, 2, 3, 4, 5
EPI_NAME = {EPI_QKV: "qkv", EPI_RESID: "resid", EPI_GELU: "gelu", EPI_SWIGLU: "swiglu", EPI_PLAIN_F32: "plain_f32"}
ALL_EPIS = (EPI_QKV, EPI_RESID, EPI_GELU, EPI_SWIGLU, EPI_PLAIN_F32)
PANEL = 256  # rows of the tallest GEMM tile: the unit the sampled row ranges are made of
KT = 64      # keys per attention tile
B31, B32 = 1 << 31, 1 << 32
SEED_A, SEED_OUT, SEED_W, SEED_BIAS, SEED_QKV = 11, 12, 13, 14, 15
N_RANDOM = 64

_C = [np.uint64(c) for c in (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB)]


# ------------------------------------------------------------------------------------------------------------- the pattern
def far_q(seed, rows, cols):
    """far_value_q of csrc/far_pattern.h for every (row, col) pair: int64 [len(rows), len(cols)] in [-64, 64)."""
    r = np.asarray(rows, np.uint64).reshape(-1, 1)
    c = np.asarray(cols, np.uint64).reshape(1, -1)
    with np.errstate(over="ignore"):
        h = r * _C[0] + (c + np.uint64(1)) * _C[1] + np.uint64((int(seed) + 1) * 0x165667B19E3779F9 & (B32 * B32 - 1))
        h ^= h >> np.uint64(29)
        h *= _C[3]
        h ^= h >> np.uint64(32)
        h *= _C[4]
        h ^= h >> np.uint64(29)
    return (h >> np.uint64(57)).astype(np.int64) - 64


def far_value(seed, rows, cols):
    """far_value: float32 [len(rows), len(cols)], multiples of 1/64 in [-1, 1)."""
    return (far_q(seed, rows, cols) / 64.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- GEMM cases
@dataclass(frozen=True)
class GemmCase:
    name: str
    M: int
    N: int
    K: int
    lda: int = 0  # 0 = K
    ldw: int = 0
    epis: tuple = ALL_EPIS
    # (gemm_gen, dtype) -> nothing; the runs of the case.  gemm_gen 0 = the planner's own choice
    runs: tuple = ((0, F16),)
    # gemm_gen -> {epilogue or None (any other) -> plan text}
    plans: dict = field(default_factory=dict, hash=False, compare=False)
    limit: str = "A"  # what sits at 2^32: "A" (M * lda * 2 just below), "W" (N * ldw * 2 just below) or "out" (the output passes it; A is small)

    @property
    def a_row_bytes(self):
        return (self.lda or self.K) * 2

    @property
    def w_row_bytes(self):
        return (self.ldw or self.K) * 2

    def width(self, epi):
        return self.N // 2 if epi == EPI_SWIGLU else self.N

    def out_row_bytes(self, epi):
        return self.width(epi) * (4 if epi in (EPI_RESID, EPI_PLAIN_F32) else 2)

    def plan(self, gen, epi):
        p = self.plans[gen]
        return p.get(epi, p[None])

    def device_bytes(self, epi):
        """What dinov2_hip_op_gemm_far allocates: A, W, the output with its guard bands, and the small buffers (rounded up generously)."""
        return self.M * self.a_row_bytes + self.N * self.w_row_bytes + (self.M + 2 * 128) * self.out_row_bytes(epi) + (64 << 20)


_G1_PLANS = {0: {None: "gemm4<256>", EPI_RESID: "gemm2<256>"}, 2: {None: "gemm2<256>"}, 4: {None: "gemm4<256>"}}
GEMM_CASES = [
    # G1: dense A at the launcher's limit, every epilogue, the planner's own choice and both forced generations
    GemmCase("G1", 2097151, 256, 1024, runs=((0, F16), (0, BF16), (2, F16), (4, F16)), plans=_G1_PLANS),
    # G2: the two-height and the split plans with their far end at the limit: M * lda * 2 = 4 293 120 000
    GemmCase("G2-mixed", 2080000, 256, 1024, lda=1032, epis=(EPI_GELU, EPI_RESID), runs=((0, F16), (2, F16)),
             plans={0: {None: "gemm4_mixed<256+192>", EPI_RESID: "gemm2_mixed<256+192>"}, 2: {None: "gemm2_mixed<256+192>"}}),
    GemmCase("G2-split", 2080000, 768, 1024, lda=1032, epis=(EPI_GELU, EPI_RESID), runs=((0, F16),),
             plans={0: {None: "gemm4<256>;small<64x128,w2x2,st2,ks1>", EPI_RESID: "gemm2<256>;small<64x128,w2x2,st2,ks1>"}}),
    # G3: strided A with few rows -- the cheap case
    GemmCase("G3", 131071, 512, 1024, lda=16384, epis=(EPI_QKV, EPI_GELU, EPI_RESID), runs=((0, F16), (0, BF16)),
             plans={0: {None: "gemm4<256>", EPI_RESID: "gemm2<256>"}}),
    # G4: the small-tile kernel with A at the limit and an output past 2^32 bytes (the EPI_PLAIN_F32 form dense_stage launches)
    GemmCase("G4-64", 33554431, 64, 64, epis=(EPI_PLAIN_F32, EPI_GELU), plans={0: {None: "small<128x128,w2x2,st2,ks1>"}}),
    GemmCase("G4-128", 11184810, 128, 192, epis=(EPI_PLAIN_F32, EPI_GELU), plans={0: {None: "small<128x128,w2x2,st2,ks1>"}}),
    # G5: W at the limit
    GemmCase("G5", 4096, 512, 256, ldw=4194296, epis=(EPI_QKV, EPI_RESID), runs=((0, F16), (0, BF16)), limit="W",
             plans={0: {None: "small<64x128,w2x2,st3,ks1>"}}),
    # G6: an f32 read-modify-write output past 2^32 bytes through a persistent kernel
    GemmCase("G6", 1100000, 1024, 256, epis=(EPI_RESID,), runs=((0, F16), (0, BF16)), limit="out",
             plans={0: {None: "gemm2<256>;small<64x128,w2x2,st3,ks1>"}}),
]
GEMM_BY_NAME = {c.name: c for c in GEMM_CASES}
# the leaves the GPU file must reach across its cases (tests/test_far_probes.py checks the table above against this list)
LEAVES_WANTED = ("gemm4<256>", "gemm4_mixed", "gemm2<256>", "gemm2_mixed", "small<128x128,w2x2,st2,ks1>", "small<64x128,w2x2,st")


def gemm_runs():
    """(case, epilogue, gemm_gen, dtype) of every GPU run, with an id."""
    out = []
    for c in GEMM_CASES:
        for epi in c.epis:
            for gen, dt in c.runs:
                out.append((c, epi, gen, dt, "%s-%s-gen%d-%s" % (c.name, EPI_NAME[epi], gen, DT_NAME[dt])))
    return out


def _panel(row, M):
    lo = row // PANEL * PANEL
    return range(lo, min(M, lo + PANEL))


def _aliases(rows, row_bytes, M):
    """Where a truncated offset would land: the rows 2^31 and 2^32 bytes away from `rows`, either way, rounded both ways when the row size does
    not divide the distance; those inside [0, M)."""
    out = set()
    for dist in (B31, B32):
        for d in {dist // row_bytes, -(-dist // row_bytes)}:
            for r in rows:
                for a in (r - d, r + d):
                    if 0 <= a < M:
                        out.add(a)
    return out


def gemm_sample(c, epi):
    """The output rows a GEMM case reads back: the first panel, the last with its ragged end, the panels that straddle byte 2^31 and 2^32 of A
    and of the output (those that exist), the alias rows of all of these under a 2^31 sign flip and a 2^32 wrap of either offset, and 64 seeded
    random rows.  Sorted, unique."""
    M, ab, ob = c.M, c.a_row_bytes, c.out_row_bytes(epi)
    base = set(_panel(0, M)) | set(_panel(M - 1, M))
    for rb in (ab, ob):
        for byte in (B31, B32):
            if M * rb > byte:
                base |= set(_panel(byte // rb, M))
    rows = set(base) | _aliases(base, ab, M) | _aliases(base, ob, M)
    rng = np.random.default_rng(len(c.name) * 1000 + epi)
    rows |= set(int(r) for r in rng.integers(0, M, N_RANDOM))
    return np.array(sorted(rows), np.int64)


def gemm_operands(c, epi):
    """W [N, K], bias [N], aux [N] or None, qcols, qscale of a case's run: host operands on exact grids.
    W: the pattern.  bias: a multiple of 1/64 in [-1, 1) -- plus 2^-13 for EPI_RESID, which puts it OFF the 2^-12 grid of the accumulator, so
    acc + bias is never 0.  aux (EPI_RESID: LayerScale): a power of two in {1, 1/2, 1/4}."""
    W = far_value(SEED_W, np.arange(c.N), np.arange(c.K))
    bias = far_value(SEED_BIAS, [0], np.arange(c.N))[0].astype(np.float32)
    aux = None
    if epi == EPI_RESID:
        bias = (bias.astype(np.float64) + 2.0 ** -13).astype(np.float32)
        aux = (2.0 ** -(np.arange(c.N) % 3)).astype(np.float32)
    qcols, qscale = (c.N // 2, 0.125) if epi == EPI_QKV else (0, 1.0)
    return W, bias, aux, qcols, qscale


# ------------------------------------------------------------------------------------------------------------- attention cases
@dataclass(frozen=True)
class AttnCase:
    name: str
    B: int
    T: int
    nh: int
    runs: tuple  # (attn_v, dtype)
    bound: int   # the limit the case sits under: B * T * 3H * 2 < bound

    @property
    def H(self):
        return 64 * self.nh

    @property
    def row_bytes(self):
        return 3 * self.H * 2

    @property
    def image_bytes(self):
        return self.T * self.row_bytes

    def device_bytes(self):
        return self.B * self.T * (self.row_bytes + self.H * 2) + 2 * 128 * self.H * 2 + (64 << 20)


ATTN_CASES = [
    # A1: far image bases: B * T * 3H * 2 = 4 294 717 440
    AttnCase("A1", 10754, 65, 16, runs=((1, F16), (1, BF16), (2, F16), (2, BF16)), bound=B32),
    # A2: one image at the limit of a pass: T * 3H * 2 = 2 147 475 456 < 2^31
    AttnCase("A2", 1, 174762, 32, runs=((0, F16), (0, BF16)), bound=B31),
    # A3: one image at the launcher's limit: 4 294 963 200 < 2^32
    AttnCase("A3", 1, 349525, 32, runs=((1, F16),), bound=B32),
]
ATTN_BY_NAME = {c.name: c for c in ATTN_CASES}
A_HEADS = (0, 17, 31)  # the heads A2 and A3 read back


def attn_runs():
    return [(c, v, dt, "%s-v%d-%s" % (c.name, v, DT_NAME[dt])) for c in ATTN_CASES for v, dt in c.runs]


def attn_sample(c):
    """(images, queries): A1 -- images 0, 1, the one that straddles byte 2^31 of qkv and the next, the last two; every query.
    A2 / A3 -- the one image; the first 128-query block, the last ragged block and 64 seeded random queries."""
    if c.B > 1:
        b31 = B31 // c.image_bytes
        return sorted({0, 1, b31, b31 + 1, c.B - 2, c.B - 1}), np.arange(c.T, dtype=np.int64)
    rng = np.random.default_rng(c.T)
    q = set(range(128)) | set(range((c.T - 1) // 128 * 128, c.T)) | set(int(x) for x in rng.integers(0, c.T, N_RANDOM))
    return [0], np.array(sorted(q), np.int64)


def attn_rows(c):
    """The rows of out [B * T, H] the sample reads back, image-major."""
    images, queries = attn_sample(c)
    return np.concatenate([b * c.T + queries for b in images]).astype(np.int64)


def attn_heads(c):
    return tuple(range(c.nh)) if c.B > 1 else A_HEADS


# ------------------------------------------------------------------------------------------------------------- address mutants
# Integer models of the address errors the far cases exist to catch.  Each maps the offset a correct kernel uses to the one a defective kernel
# would use; "hit" means the two differ.
#   a_signed32:  an operand row's byte offset r * row_bytes, or the cursor at the end of its tile (below), held or compared as signed 32-bit
#   a_wrap32:    the operand cursor wrapped at 2^32.  A row's own offset is below 2^32 by the launcher's guard; what passes 2^32 is the cursor
#                that runs a whole tile ahead before its clamp (the next-tile delta of gemm4.hip, `stoff += KT * rowb` in attention.hip):
#                the end of the row's tile, (r // tile + 1) * tile * row_bytes
#   out_wrap32:  the output row's byte offset wrapped at 2^32
#   base32:      the base of a row's tile (GEMM: panel) or image (attention) as a signed 32-bit product
MUTANTS = ("a_signed32", "a_wrap32", "out_wrap32", "base32")


def _sext32(x):
    x = np.asarray(x, np.int64) & (B32 - 1)
    return np.where(x >= B31, x - B32, x)


def mutant_hits(mutant, rows, row_bytes, out_row_bytes, tile, group):
    """Which of `rows` (int64) a mutant sends to another address.  row_bytes: of the operand the rows index; tile: rows per staging tile;
    group: rows per base (the panel, or the image)."""
    rows = np.asarray(rows, np.int64)
    if mutant == "a_signed32":
        off, end = rows * row_bytes, (rows // tile + 1) * tile * row_bytes
        return (_sext32(off) != off) | (_sext32(end) != end)
    if mutant == "a_wrap32":
        end = (rows // tile + 1) * tile * row_bytes
        return (end & (B32 - 1)) != end
    if mutant == "out_wrap32":
        off = rows * out_row_bytes
        return (off & (B32 - 1)) != off
    if mutant == "base32":
        off = rows // group * group * row_bytes
        return _sext32(off) != off
    raise ValueError(mutant)


def gemm_mutant_view(c, epi):
    """(all rows' descriptor, sampled rows) of a GEMM case for mutant_hits: the operand at the limit is A (indexed by output row) or, for G5,
    W (indexed by output column: every column of a sampled row is checked, so every W row is sampled)."""
    if c.limit == "W":
        n = np.arange(c.N, dtype=np.int64)
        return dict(all_rows=n, rows=n, row_bytes=c.w_row_bytes, out_row_bytes=0, tile=PANEL, group=PANEL)
    return dict(all_rows=None, M=c.M, rows=gemm_sample(c, epi), row_bytes=c.a_row_bytes, out_row_bytes=c.out_row_bytes(epi), tile=PANEL,
                group=PANEL)


def attn_mutant_view(c):
    """For attention a sampled query reads EVERY key row of its image, so the operand rows the sample touches are all rows of the sampled
    images; the rows it writes are the sampled rows."""
    images, _ = attn_sample(c)
    read = np.concatenate([np.arange(b * c.T, (b + 1) * c.T, dtype=np.int64) for b in images])
    return dict(M=c.B * c.T, read_rows=read, write_rows=attn_rows(c), row_bytes=c.row_bytes, out_row_bytes=c.H * 2, tile=KT, group=c.T)


def any_row_hit(mutant, M, row_bytes, out_row_bytes, tile, group):
    """Whether the mutant moves ANY row of [0, M): the hits are monotone in the row (an offset only grows), so the last row decides."""
    return bool(mutant_hits(mutant, [M - 1], row_bytes, out_row_bytes, tile, group)[0])
