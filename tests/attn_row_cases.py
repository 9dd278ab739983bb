"""Attention-row test helpers (attn_rows_kernel, csrc/attn_rows.hip; dinov2_hip_predict_attention): the shapes, query sets and key views,
exact probes, a float64 reference with the error bound derived from the kernel's arithmetic, and a numpy emulation of that arithmetic with
planted bugs.  Imported by tests/test_gpu_attn_rows.py, tests/test_gpu_attention_maps.py (the HIP kernel) and tests/test_attn_row_probes.py
(the emulation and its mutants, no GPU).  Built on the code pool and helpers of tests/attention_cases.py.  Plain module, no fixtures.

Layout, as in attention_cases: qkv [B*T, 3H] f32 holding values of the compute type, row = [q | k | v], head h at columns h*64 ..; q carries
0.125 log2(e) already, so a score is q.k in the kernel's own units and a weight is 2^(s - m).  Rows come back as [B, nh, nq, nkeys] f32:
columns [key0, key0 + nkeys) of the softmax over ALL T keys.
"""
import numpy as np

import attention_cases as ac

F16, BF16 = ac.F16, ac.BF16
QSCALE = np.float32(0.125 * 1.44269504088896340736)  # what the forward's QKV epilogue multiplies q by
SLOTS = 256  # denominator slots of the kernel (its workgroup size)

SHAPES = [(1, 1, 1), (3, 2, 2), (1, 63, 1), (3, 64, 6), (1, 65, 2), (1, 129, 6), (3, 261, 2), (1, 1374, 2), (1, 4101, 1)]


def shape_id(s):
    return "B%d-T%d-nh%d" % s


def query_sets(T):
    """[0], [0, T-1], [1, T//2] and, for T <= 261, all T -- those that are valid (strictly ascending, inside [0, T)), without duplicates."""
    sets = [[0], [0, T - 1], [1, T // 2]] + ([list(range(T))] if T <= 261 else [])
    out = []
    for q in sets:
        if all(0 <= v < T for v in q) and all(a < b for a, b in zip(q, q[1:])) and q not in out:
            out.append(q)
    return out


def key_views(T):
    """(key0, nkeys): every column, and columns 5 .. where there are any."""
    return [(0, T)] + ([(5, T - 5)] if T > 5 else [])


def _split(qkv, B, T, nh, dtype=np.float32):
    x = np.asarray(qkv, dtype).reshape(B, T, 3, nh, 64)
    return x[:, :, 0].transpose(0, 2, 1, 3), x[:, :, 1].transpose(0, 2, 1, 3)  # q, k as [B, nh, T, 64]


# ------------------------------------------------------------------------------------------------------------- emulation
MUTANTS = ("drop_last_key", "drop_key_64", "leak_tail", "exp_natural", "q_scaled_twice", "heads_swapped", "query_off_by_one",
           "image_offset_wrong", "renormalised_over_written")


def _tree(a):
    """Pairwise sum over the last axis (a power of two long), neighbours first, in f32."""
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def emulate(qkv, B, T, nh, dt, queries, key0=0, nkeys=None, mutant=None):
    """numpy restatement of the kernel's documented arithmetic (csrc/attn_rows.hip, header): f32 products of the stored T-typed q and k (exact);
    a score = 8 slices of 8 consecutive d summed in ascending d from 0, the slice sums by a pairwise tree; f32 maximum; p = exp2(s - m);
    denominator = 256 slots, slot t summing keys t, t + 256, ... in ascending order, the slots by a pairwise tree; out = p * (1 / l).
    `mutant` plants one bug of MUTANTS."""
    f = np.float32
    nkeys = T - key0 if nkeys is None else nkeys
    q, k = _split(ac.round_t(qkv, dt), B, T, nh)
    qs = np.asarray(queries, np.int64)
    if mutant == "query_off_by_one":
        qs = np.minimum(qs + 1, T - 1)
    if mutant == "q_scaled_twice":
        q = ac.round_t(q * QSCALE, dt)
    qq = q[:, :, qs]  # [B, nh, nq, 64]
    q8, k8 = qq.reshape(B, nh, len(qs), 1, 8, 8), k.reshape(B, nh, 1, T, 8, 8)  # [..., slice, d within the slice]
    acc = np.zeros((B, nh, len(qs), T, 8), f)
    for d in range(8):
        acc = acc + q8[..., d] * k8[..., d]
    s = _tree(acc)  # [B, nh, nq, T]
    dead = np.zeros(T, bool)
    if mutant == "drop_last_key":
        dead[T - 1] = True
    if mutant == "drop_key_64" and T > 64:
        dead[64] = True
    s = np.where(dead, f(-np.inf), s)
    m = s.max(-1, keepdims=True)
    ex = (lambda z: np.exp(z, dtype=f)) if mutant == "exp_natural" else (lambda z: np.exp2(z, dtype=f))
    with np.errstate(invalid="ignore"):
        p = ex(s - m)
    pad = (-T) % SLOTS
    pp = np.concatenate([p, np.zeros(p.shape[:-1] + (pad,), f)], -1)
    if mutant == "leak_tail":  # the clamped copies of key T - 1 that fill the last group of 32 keys counted as keys
        pp[..., T:T + (-T) % 32] = p[..., T - 1:T]
    pp = pp.reshape(p.shape[:-1] + (-1, SLOTS))
    slots = np.zeros(p.shape[:-1] + (SLOTS,), f)
    for r in range(pp.shape[-2]):
        slots = slots + pp[..., r, :]
    inv = f(1) / _tree(slots)
    out = (p * inv[..., None])[..., key0:key0 + nkeys]
    if mutant == "renormalised_over_written" and nkeys < T:
        out = out / out.sum(-1, keepdims=True, dtype=f)
    if mutant == "heads_swapped" and nh > 1:
        out = out[:, [1, 0] + list(range(2, nh))]
    if mutant == "image_offset_wrong" and B > 1:
        out = np.roll(out, 1, axis=0)
    return np.ascontiguousarray(out, f)


# ------------------------------------------------------------------------------------------------------------- exact probes
def _codes63(rng, T):
    """T random +-1 codes of length 63 with pairwise Hamming distance >= 11: a random isometric image of attention_cases' pool (distance
    >= 12 over 64 columns) with one column dropped."""
    c = ac._head_codes(rng, ac.code_pool(T), T)[:, :63]
    return c


def probe_permutation(B, T, nh, seed, pairs=False):
    """Keys (4 c_j, -1008), queries (4 c_pi(i), 1) with 63-long +-1 codes c: query i scores 16 * 63 - 1008 = 0 on key pi(i) and
    16 * (63 - 2 hd) - 1008 = -32 hd <= -352 on every other key (hd >= 11), all sums of integers below 2^24, exact in f32 in any order.
    2^-352 is 0 in f32, so row i is exactly one-hot at pi(i) -- per image and head its own permutation: the row identifies key, head and
    image.  pairs: the keys of each attention_cases.pair_keys() pair share one code, and a query aimed at either scores 0 on both: exactly
    0.5 and 0.5.  Returns (qkv f32, expected [B, nh, T, T])."""
    rng = np.random.default_rng(seed)
    H = nh * 64
    x = np.zeros((B, T, 3, nh, 64), np.float32)
    exp = np.zeros((B, nh, T, T), np.float32)
    pk = ac.pair_keys(T, rng) if pairs else []
    for b in range(B):
        for h in range(nh):
            c = _codes63(rng, T)
            partner = np.arange(T)
            for a, bb in pk:
                c[bb] = c[a]
                partner[a], partner[bb] = bb, a
            pi = rng.permutation(T)
            x[b, :, 1, h, :63] = 4.0 * c
            x[b, :, 1, h, 63] = -1008.0
            x[b, :, 0, h, :63] = 4.0 * c[pi]
            x[b, :, 0, h, 63] = 1.0
            w = np.where(partner[pi] != pi, 0.5, 1.0)
            exp[b, h, np.arange(T), pi] = w
            exp[b, h, np.arange(T), partner[pi]] = w
    x[:, :, 2] = rng.standard_normal((B, T, nh, 64))  # v is not read
    return x.reshape(B * T, 3 * H), exp


def ladder_levels(T):
    """n levels 0, -1, ..., -(n - 1) with 2^k keys at level -k: 2^n - 1 keys whose weights sum to n; n the largest of 1, 2, 4, 8 that fits T."""
    return max(n for n in (1, 2, 4, 8) if 2 ** n - 1 <= T)


def probe_ladder(B, T, nh, seed):
    """Integer scores 0, -1, -1, -2, -2, -2, -2, ... (2^k keys at -k, n = ladder_levels(T) levels), every other key at -200: the weights sum
    to n, a power of two, every partial sum is a multiple of 2^-7 below 16 (exact in f32 in any order), so every entry is exactly
    2^-k / n, or 0.  q = a +-1 sign vector, k_j = sign * score / 64 (multiples of 1/64 with at most 5 significant bits: exact in f16 and
    bf16, as are their partial sums); the ladder keys sit at random positions, different per image and head.  Returns (qkv, expected
    [B, nh, T, T]) -- every query has the same row."""
    rng = np.random.default_rng(seed)
    H = nh * 64
    n = ladder_levels(T)
    level = np.concatenate([np.full(2 ** k, float(k)) for k in range(n)])
    x = np.zeros((B, T, 3, nh, 64), np.float32)
    exp = np.zeros((B, nh, T, T), np.float32)
    for b in range(B):
        for h in range(nh):
            sgn = rng.choice(np.array([-1.0, 1.0], np.float32), 64)
            score = np.full(T, 200.0)
            pos = rng.permutation(T)[:len(level)]
            score[pos] = level
            x[b, :, 0, h] = sgn
            x[b, :, 1, h] = sgn[None, :] * (-score[:, None] / 64.0)
            row = np.zeros(T)
            row[pos] = 2.0 ** -level / n
            exp[b, h] = row[None, :]
    return x.reshape(B * T, 3 * H), exp


def probe_uniform(B, T, nh, seed):
    """q = 0: every score is exactly 0 whatever k (random), every weight exactly 1, l = T exactly: every entry is 1/T within one ulp of f32."""
    rng = np.random.default_rng(seed)
    x = np.zeros((B, T, 3, nh, 64), np.float32)
    x[:, :, 1] = rng.standard_normal((B, T, nh, 64))
    return x.reshape(B * T, 3 * nh * 64), np.full((B, nh, T, T), 1.0 / T)


PROBES = ("permutation", "pairs", "ladder", "uniform")


def build_probe(kind, B, T, nh, seed):
    if kind == "permutation":
        return probe_permutation(B, T, nh, seed)
    if kind == "pairs":
        return probe_permutation(B, T, nh, seed, pairs=True)
    if kind == "ladder":
        return probe_ladder(B, T, nh, seed)
    return probe_uniform(B, T, nh, seed)


def expected_view(exp, queries, key0, nkeys):
    return exp[:, :, np.asarray(queries)][..., key0:key0 + nkeys]


def check_probe(kind, out, exp, what=""):
    """(ok, message).  permutation / pairs / ladder: bit for bit; uniform: within one ulp of f32."""
    out = np.asarray(out, np.float32)
    if out.shape != exp.shape:
        return False, "%s %s probe: shape %s, expected %s" % (what, kind, out.shape, exp.shape)
    if not np.isfinite(out).all():
        bad = np.argwhere(~np.isfinite(out))
        return False, "%s %s probe: %d non-finite entries (unwritten?), first at %s" % (what, kind, len(bad), tuple(bad[0]))
    if kind == "uniform":
        e32 = np.asarray(exp, np.float32)
        d = np.abs(out.view(np.int32).astype(np.int64) - e32.view(np.int32).astype(np.int64))
        bad = d > 1
    else:
        bad = out != np.asarray(exp, np.float32)
    if not bad.any():
        return True, "%s %s probe: exact" % (what, kind)
    i = tuple(np.argwhere(bad)[0])
    return False, "%s %s probe: %d mismatches, first at (image, head, query, column) %s: got %r expected %r" % (
        what, kind, int(bad.sum()), i, float(out[i]), float(exp[i]))


def check_exact(a, b, what):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False, "%s: shapes %s vs %s" % (what, a.shape, b.shape)
    bad = a.view(np.uint32) != b.view(np.uint32)
    if not bad.any():
        return True, what + ": identical"
    i = tuple(np.argwhere(bad)[0])
    return False, "%s: %d of %d entries differ, first at %s: %r vs %r" % (what, int(bad.sum()), bad.size, i, float(a[i]), float(b[i]))


# ------------------------------------------------------------------------------------------------------------- reference
def reference(qkv, B, T, nh, queries):
    """float64 softmax rows of the stored q and k, log2 units.  Returns (P, S, M): P [B, nh, nq, T]; per row (as [B, nh, nq, 1])
    S = max_j sum_d |q_d k_jd| and M = max_j s_j, the score-rounding terms of the bound."""
    q, k = _split(qkv, B, T, nh, np.float64)
    qq = q[:, :, np.asarray(queries)]
    s = qq @ k.transpose(0, 1, 3, 2)
    S = (np.abs(qq) @ np.abs(k).transpose(0, 1, 3, 2)).max(-1, keepdims=True)
    M = s.max(-1, keepdims=True)
    p = np.exp2(s - M)
    return p / p.sum(-1, keepdims=True), S, M


def denominator_depth(T):
    """f32 additions on the longest path of the kernel's denominator: ceil(T / 256) sequential ones in a slot, then the 8 levels of the tree."""
    return (T + SLOTS - 1) // SLOTS + 8


def error_bound(P, S, M, T):
    """Per-element bound on |kernel - reference(stored q, k)|, from the kernel's own arithmetic (csrc/attn_rows.hip, header), none of it
    measured:

      * scores: the 64 products are exact in f32; 63 additions (7 in a slice, 3 tree levels -- counted as 64) plus the subtraction of the
        maximum and the rounding of the maximum's own score, each a rounding of a magnitude <= S + |M|:
            |ds| <= (64 + 2) 2^-24 (S + |M|)
      * each p = exp2f(s - m): relative eps_p = ds ln 2 + 2^-22 (exp2f within an ulp, with slack)
      * the denominator: every term carries eps_p, and the sum of T positive f32 terms adds a relative depth * 2^-24, depth =
        denominator_depth(T) = ceil(T / 256) + 8 (a slot's sequential part, then the 8-level tree -- what the kernel does, not T 2^-24)
      * reciprocal and product: 2^-22 together (two roundings, with slack)
      * results below the f32 normal range may be flushed: 2^-125 absolute

    so a relative eps = (1 + eps_p)(1 + 2^-22) / ((1 - eps_p)(1 - depth 2^-24)) - 1 on P, plus 2^-125."""
    ds = 66 * 2.0 ** -24 * (S + np.abs(M))
    eps_p = ds * ac.LN2 + 2.0 ** -22
    eps = (1 + eps_p) * (1 + 2.0 ** -22) / ((1 - eps_p) * (1 - denominator_depth(T) * 2.0 ** -24)) - 1
    return P * eps + 2.0 ** -125


def check_against_reference(out, P, bound, what=""):
    """(ok, message): every element finite and within its bound; none exempted."""
    out = np.asarray(out, np.float64)
    if out.shape != P.shape:
        return False, "%s: shape %s, expected %s" % (what, out.shape, P.shape)
    if not np.isfinite(out).all():
        return False, "%s: %d non-finite entries" % (what, int((~np.isfinite(out)).sum()))
    ratio = np.abs(out - P) / bound
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    msg = "%s worst at %s: |err| %.3e bound %.3e (ratio %.3f)" % (what, tuple(int(v) for v in i), abs(out[i] - P[i]), bound[i], ratio[i])
    return bool(ratio[i] <= 1.0), msg


def check_rows_sum_to_one(full_rows, T, what=""):
    """Rows over all T columns: |sum - 1| <= T 2^-23 (each of the T entries carries the shared relative error of 1 / l and its own two
    roundings; the float64 sum adds nothing)."""
    d = np.abs(np.asarray(full_rows, np.float64).sum(-1) - 1.0)
    return bool(d.max() <= T * 2.0 ** -23), "%s: max |row sum - 1| %.3e (allowed %.3e)" % (what, d.max(), T * 2.0 ** -23)
