"""Far-row cases: dinov2_hip_match_tokens, dinov2_hip_bank_add / _topk and dinov2_hip_kmeans_tokens at the far end of their row offsets
(include/dinov2_hip_ops.h, "Far rows").  Imported by tests/test_rows_far_probes.py (CPU: the selection rule against its C++ original, the
expectation builders against brute force, the byte products, the address mutants in integers) and tests/test_gpu_rows_far.py (the entry
points).  Plain module, no fixtures.

The operands.  Row r of a far operand is entry far_rows_entry(seed, r) of a small dictionary (csrc/far_pattern.h, restated in `sel` /
`entries`): a hash of the full 64-bit row index onto the D_COMMON common entries, overridden for a short list of planted rows, each of which
holds a rare entry that occurs nowhere else.  Every dictionary entry has exactly 4, 16 or 64 non-zeros of +-1 (kmeans_cases.pm_rows), so its
normalised f16 row is +-2^-1, +-2^-2 or +-2^-3 exactly, every similarity is a short dyadic sum and every cluster sum over <= 2^20 rows is a
multiple of 2^-3 of magnitude <= 2^19: 22 bits, exact in f32 in any order.  Everything is therefore compared bit for bit; no tolerance appears.
The host never holds a far operand: every expectation comes from the D x (other side) similarities, exact in float64, and the integer array
of the rows' entries.
"""
from dataclasses import dataclass

import numpy as np

import bank_cases as bc
import far_cases as fc
import kmeans_cases as kc
import match_cases as mc

SEED = 31
D_COMMON = 131          # >= 128 and not a power of two
MAX_PLANTS = 256
TILE = 128
B31, B32, B33 = 1 << 31, 1 << 32, 1 << 33
BIG = np.iinfo(np.int64).max
# the interface limits (csrc/resident.cpp) and the pass sizes (csrc/kernels.h)
MATCH_N_MAX, KMEANS_N_MAX, BANK_CAP_MAX, BANK_NQ_MAX, H_MAX = 1 << 20, 1 << 20, 1 << 24, 1 << 20, 4096
MATCH_PASS_ROWS, BANK_PASS_ROWS = mc.PASS, bc.PASS


# ------------------------------------------------------------------------------------------------------------- the selection rule
def sel(seed, rows, d_common=D_COMMON):
    """far_rows_sel of csrc/far_pattern.h for every row: int64 in [0, d_common)."""
    rows = np.asarray(rows, np.uint64).ravel()
    out = np.empty(len(rows), np.int64)
    step = 1 << 20
    for a in range(0, len(rows), step):
        q = fc.far_q(seed, rows[a:a + step], [0, 1]) + 64
        out[a:a + step] = (q[:, 0] * 128 + q[:, 1]) % d_common
    return out


def entries(seed, n, plants, d_common=D_COMMON, row0=0):
    """far_rows_entry for rows [row0, row0 + n): the hash, overridden by the plants [(row, entry)]."""
    e = sel(seed, np.arange(row0, row0 + n, dtype=np.uint64), d_common)
    for r, ent in plants:
        if row0 <= r < row0 + n:
            e[r - row0] = ent
    return e


def dictionary(H, n_rare, seed=7):
    """[D_COMMON + n_rare, H] f32: distinct rows of +-1 in exactly 4, 16 or 64 positions (those that fit H).  With H >= 16 entries 0 .. 3
    have four non-zeros each on disjoint supports: their sum (tie_row) is a 16-non-zero row at similarity exactly 1/2 from all four."""
    rng = np.random.default_rng(seed + H)
    rows, seen = [], set()
    if H >= 16:
        pos = rng.choice(H, 16, replace=False)
        for i in range(4):
            x = np.zeros(H, np.float32)
            x[pos[4 * i:4 * i + 4]] = rng.choice([-1.0, 1.0], 4)
            rows.append(x)
            seen.add(x.tobytes())
    while len(rows) < D_COMMON + n_rare:
        x = kc.pm_rows(rng, 1, H)[0]
        if x.tobytes() not in seen:
            seen.add(x.tobytes())
            rows.append(x)
    return np.stack(rows)


def tie_row(dic):
    return dic[0] + dic[1] + dic[2] + dic[3]


def plant_rows(n, byte_strides=(), extra=(), tile=TILE):
    """The planted rows of an operand of n rows: row 0, row n - 1 and the first row of the last tile; for every byte stride of a row
    (the f16 operand's, the f32 source's) and every boundary 2^31 / 2^32 / 2^33 the operand reaches, the rows on both sides of it and the first
    and last row of their tiles; `extra` rows (a pass boundary).  Sorted, unique."""
    rows = {0, n - 1, (n - 1) // tile * tile} | set(extra)
    for rb in byte_strides:
        for byte in (B31, B32, B33):
            if n * rb > byte:
                r = byte // rb  # the row that holds byte `byte`
                for x in (r - 1, r):
                    rows |= {x, x // tile * tile, x // tile * tile + tile - 1}
    rows = sorted(r for r in rows if 0 <= r < n)
    assert len(rows) <= MAX_PLANTS
    return rows


# ------------------------------------------------------------------------------------------------------------- the cases
@dataclass(frozen=True)
class Case:
    name: str
    kind: str      # "match", "bank", "kmeans"
    far: str       # which operand is far: "a" / "b" (match), "bank" / "queries" (bank), "x" (k-means)
    n: int         # rows of the far operand
    small: int     # rows of the other side: nb / na, nq / count, K
    H: int
    ks: tuple = ()     # bank: the k of each search
    adds: tuple = ()   # bank with a far bank: the rows of each add call
    host: bool = False  # M0: host arrays through dinov2_hip_op_match; nothing far in bytes
    extra: tuple = ()   # further planted rows
    rares: int = 0      # 0 = a rare entry of its own for every planted row

    @property
    def hpad(self):
        return -(-self.H // 64) * 64

    @property
    def strides(self):
        """(bytes of a row of the f16 operand, bytes of a row of the f32 source)."""
        return (self.hpad * 2, self.H * 4)

    @property
    def plant_rows(self):
        """The planted rows.  A far bank is filled add by add from one reused source buffer: the f16 boundaries are those of the whole bank,
        the f32 source's those of each add's own rows (which also plants the first and last row of every add)."""
        if self.host:
            return plant_rows(self.n, (), self.extra)
        f16, src = self.strides
        if self.far != "bank":
            return plant_rows(self.n, (f16, src), self.extra)
        rows, at = set(plant_rows(self.n, (f16,))), 0
        for a in self.adds:
            rows |= {at + r for r in plant_rows(a, (src,))}
            at += a
        assert at == self.n and len(rows) <= MAX_PLANTS
        return sorted(rows)

    @property
    def n_rare(self):
        """Rare entries: one per planted row, or `rares` of them dealt out in turn (B1: five queries cannot name every planted row, so two rare
        entries hold them all, each with fewer copies than k = 64 -- every planted row is in its entry's top-64)."""
        return self.rares or len(self.plant_rows)

    @property
    def plant_list(self):
        """[(row, rare entry)]: planted row i holds entry D_COMMON + i % n_rare."""
        return [(r, D_COMMON + i % self.n_rare) for i, r in enumerate(self.plant_rows)]

    def dictionary(self):
        return dictionary(self.H, self.n_rare)

    def entries(self):
        return entries(SEED, self.n, self.plant_list)

    def device_bytes(self):
        """What the case holds on the device at its peak, rounded up generously: the far f32 rows (for a far bank: one add's rows), the f16
        operands and the workspaces of the call."""
        pad = -(-self.n // TILE) * TILE
        f16 = pad * self.hpad * 2
        slack = 256 << 20
        if self.kind == "kmeans":
            return self.n * self.H * 4 + f16 + pad * (-(-self.H // 128) * 128) * 2 + slack
        if self.far == "bank":
            return f16 + max(self.adds) * self.H * 4 + slack
        if self.far == "queries":
            return self.n * self.H * 4 + f16 + self.n * max(self.ks) * 8 + slack
        return self.n * self.H * 4 + f16 + slack


CASES = [
    # both sides in two passes: the first-flags of both reduces inside launch_match's double loop
    Case("M0", "match", "a", MATCH_PASS_ROWS + 1, MATCH_PASS_ROWS + 1, 8, host=True, extra=(MATCH_PASS_ROWS - 1, MATCH_PASS_ROWS)),
    # f16 A just past 2^32 bytes, the f32 source past 2^33
    Case("M1", "match", "a", (1 << 19) + 257, 300, 4096),
    # the B side at the interface limit, the scalar-load normaliser (H % 4 != 0), the column-direction reduce over 64 passes
    Case("M2", "match", "b", 1 << 20, 300, 4094),
    # the row index at the interface limit, the f16 bank past 2^32 bytes, add at a far count
    Case("B1", "bank", "bank", 1 << 24, 5, 136, ks=(1, 64), adds=(1 << 23, (1 << 23) - 1, 1), rares=2),
    # wide rows past 2^32 bytes; two query tiles
    Case("B2", "bank", "bank", (1 << 19) + 257, 130, 4096, ks=(64,), adds=(1 << 17,) * 4 + (257,)),
    # the query operand and the per-pass output offset idx + r0 * k over 256 passes
    Case("B3", "bank", "queries", 1 << 20, 300, 4096, ks=(5,)),
    # x16 and XT just past 2^32 bytes; two centre tiles
    Case("K1", "kmeans", "x", (1 << 19) + 257, 130, 4096),
    # the interface limit, the scalar-load normaliser
    Case("K2", "kmeans", "x", 1 << 20, 3, 4094),
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]


def small_rows(c, dic):
    """The other side of a case, [c.small, H] f32: every rare entry (as many as fit), a zero row and the tie row (bank queries and match, where
    they fit), then the common entries 0, 1, 2, ... over and over -- so the small side repeats entries too, and its own lowest index decides.
    k-means: the init centre vectors -- no zero row, and the LAST centre repeats centre 0, so it never gets a member (an empty cluster)."""
    m, H = c.small, c.H
    if c.host:  # M0: the other side is an entry list of its own, with the rare entries planted at both ends and around the pass boundary
        rare = [e for _, e in c.plant_list][::-1]  # (reversed: the partner of a row of the first pass sits in the second)
        rows = plant_rows(m, (), c.extra)
        eb = entries(SEED + 1, m, list(zip(rows, rare)))
        return dic[eb]
    out = []
    if c.kind == "kmeans":
        m -= 1
    out += list(dic[D_COMMON:D_COMMON + c.n_rare])[:max(m - 2, 1)]
    if c.kind != "kmeans" and H >= 16 and len(out) + 2 <= m:
        out += [np.zeros(H, np.float32), tie_row(dic)]
    i = 0
    while len(out) < m:
        out.append(dic[i % D_COMMON])
        i += 1
    if c.kind == "kmeans":
        out.append(out[0])
    return np.stack(out[:c.small]).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- expectations
def exact_sims(dic, other):
    """[D, m] float64: the cosine similarity of every dictionary entry with every row of the other side; asserted exact in f32 (so the
    kernel's f32 accumulation of the f16 products gives these bits in any order)."""
    S = mc.reference(dic, other)
    assert np.array_equal(S.astype(np.float32).astype(np.float64), S), "a similarity is not exact in f32"
    return S


def _f32(S):
    return S.astype(np.float32) + np.float32(0.0)  # (a -0 becomes +0, as in the kernels)


def first_rows(ent, D):
    """[D] int64: the lowest row that holds each entry; BIG for an entry that occurs nowhere."""
    first = np.full(D, BIG, np.int64)
    u, i = np.unique(ent, return_index=True)
    first[u] = i
    return first


def expected_match(S, ent):
    """Both directions of a match of the far rows (entries `ent`) with the other side, from S = exact_sims(dictionary, other side).
    far -> other: the answer of a row depends on its entry alone (np.argmax returns the first maximum: the lowest index).  other -> far: among
    ALL rows whose entry attains the maximum -- entries of equal similarity included -- the lowest row index."""
    D, m = S.shape
    S32 = _f32(S)
    j = S.argmax(1)
    first = first_rows(ent, D)
    T = np.where((first < BIG)[:, None], S, -np.inf)
    best = T.max(0)
    cand = np.where(T == best[None, :], first[:, None], BIG)
    return {"idx_far": j[ent].astype(np.int32), "sim_far": S32[np.arange(D), j][ent],
            "idx_other": cand.min(0).astype(np.int32), "sim_other": _f32(best)}


def match_result_keys(far):
    """(key of idx far->other, sim far->other, idx other->far, sim other->far) in the result dict of Session.match."""
    return ("idx_ab", "sim_ab", "idx_ba", "sim_ba") if far == "a" else ("idx_ba", "sim_ba", "idx_ab", "sim_ab")


def expected_topk_far_bank(S, ent, k):
    """Top-k of every query against a far bank, from S = exact_sims(dictionary, queries) [D, nq].  The candidates of a query are
    (S[entry(r)], r), ordered by value descending, then row ascending: value group by value group, the merged sorted row lists of the group's
    entries (only the first k rows of an entry can matter)."""
    D, nq = S.shape
    e16 = np.asarray(ent).astype(np.int16)
    order = np.argsort(e16, kind="stable")
    count = np.bincount(ent, minlength=D)
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    firstk = [order[start[d]:start[d] + min(int(count[d]), k)] for d in range(D)]
    idx = np.full((nq, k), -1, np.int32)
    sim = np.full((nq, k), -np.inf, np.float32)
    present = count > 0
    for q in range(nq):
        have = 0
        for v in np.unique(S[present, q])[::-1]:
            grp = np.flatnonzero(present & (S[:, q] == v))
            rows = np.sort(np.concatenate([firstk[d] for d in grp]))[:k - have]
            idx[q, have:have + len(rows)] = rows
            sim[q, have:have + len(rows)] = _f32(np.float64(v).reshape(1))[0]
            have += len(rows)
            if have >= k:
                break
    return {"idx": idx, "sim": sim}


def expected_topk_far_queries(S, ent, k):
    """Top-k of far queries against a small bank, from S = exact_sims(dictionary, bank rows) [D, count]: a query's list depends on its entry
    alone (bank_cases.expected_topk per entry, gathered)."""
    t = bc.expected_topk(_f32(S), k)
    return {"idx": t["idx"][ent], "sim": t["sim"][ent]}


def exact_assign(dic, vec):
    """Per dictionary entry: (label, sim) against dyadic centre vectors, from the exact similarities."""
    S = exact_sims(dic, vec)
    lab = S.argmax(1).astype(np.int32)
    return {"labels": lab, "sim": _f32(S)[np.arange(len(dic)), lab]}


def expected_kmeans(dic, ent, init, max_iter, assign_fn):
    """Contract 5 (kmeans_cases.emulate_run) on the dictionary with multiplicities: assign_fn(dictionary, centre vectors) -> per-ENTRY labels and
    sim (the first assignment's centres are dictionary entries: exact_assign; later ones are normalised sums, no longer dyadic: the
    assignment kernel on the dictionary alone -- the contract of sim_tile.h is that a pair's bits depend on hpad alone).  The update is exact:
    S_c = sum_d mult[d] * xhat_d over the entries labelled c, asserted representable in f32, so any chunking gives these bits; an empty cluster
    keeps its vector.  Returns the dict of Session.kmeans plus `first`: the first assignment per row."""
    D, K, n = len(dic), len(init), len(ent)
    mult = np.bincount(ent, minlength=D).astype(np.int64)
    xhat = mc.normalise_f16(dic).astype(np.float64)
    vec = np.asarray(init, np.float32).copy()
    counts = np.zeros(K, np.int32)
    prev, it, conv, first = None, 0, False, None
    while True:
        a = assign_fn(dic, vec)
        lab, sim = np.asarray(a["labels"]), np.asarray(a["sim"])
        if first is None:
            first = {"labels": lab[ent], "sim": sim[ent]}
        changed = n if prev is None else int(mult[lab != prev].sum())
        prev = lab
        if changed == 0:
            conv = True
            break
        if it == max_iter:
            counts = np.bincount(lab, weights=mult, minlength=K).astype(np.int32)
            break
        for c in range(K):
            m = (lab == c) & (mult > 0)
            counts[c] = mult[m].sum()
            if counts[c] > 0:
                s = (mult[m, None] * xhat[m]).sum(0)
                assert np.array_equal(s.astype(np.float32).astype(np.float64), s), "a cluster sum is not exact in f32"
                assert np.abs(s).max() <= 2.0 ** 19 and np.array_equal(s * 8, np.round(s * 8))
                vec[c] = s.astype(np.float32)
        it += 1
    return {"labels": lab[ent].astype(np.int32), "sim": sim[ent], "centers": vec, "counts": counts, "iterations": it, "converged": conv,
            "first": first}


# ------------------------------------------------------------------------------------------------------------- address mutants
# far_cases.MUTANTS applied to the two stages that touch a far operand's rows:
#   "normalise"  match_normalise_kernel reads the f32 source (H * 4 bytes a row; four rows a workgroup) and writes the f16 operand (hpad * 2
#                bytes a row) -- the bank itself for bank_add, at rows + count * hpad
#   "tile"       the tile kernels read the f16 operand (128 rows a tile, a pass of rows a base) and write a few bytes per row (never far)
STAGES = ("normalise", "tile")


def stage_view(c, stage):
    """The arguments of far_cases.mutant_hits for a stage of a case."""
    f16, src = c.strides
    group = {"match": MATCH_PASS_ROWS, "bank": BANK_PASS_ROWS if c.far == "queries" else TILE, "kmeans": TILE}[c.kind]
    if stage == "normalise":
        return dict(row_bytes=src, out_row_bytes=f16, tile=4, group=4)
    return dict(row_bytes=f16, out_row_bytes=4 * (max(c.ks) if c.far == "queries" else 1), tile=TILE, group=group)


def alias_rows(mutant, rows, row_bytes, out_row_bytes, tile, group):
    """Where the mutant sends each of `rows`: the row whose place the defective offset falls in (int64; -1 = outside the operand or inside
    another row: other data in any case), and whether the offset moved at all."""
    rows = np.asarray(rows, np.int64)
    rb = out_row_bytes if mutant == "out_wrap32" else row_bytes
    off = rows * rb
    if mutant == "a_signed32":
        bad = fc._sext32(off)
    elif mutant in ("a_wrap32", "out_wrap32"):
        bad = off & (B32 - 1)
    elif mutant == "base32":
        base = rows // group * group * rb
        bad = fc._sext32(base) + (off - base)
    else:
        raise ValueError(mutant)
    moved = bad != off
    to = np.where((bad >= 0) & (bad % rb == 0), bad // rb, -1)
    return to, moved
