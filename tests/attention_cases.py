"""Attention test helpers: a float64 reference, the error bound derived from the kernels' numerics, exact probes and a numpy
emulation of the kernels' arithmetic.  Imported by tests/test_gpu_attention.py (the HIP kernels) and tests/test_attention_probes.py
(the emulation and its mutants, no GPU).  Plain module, no fixtures.

Layout (as the forward): qkv is token-major [B*T, 3H] f32 holding values of the compute type T (f16 or bf16), row = [q | k | v],
head h at columns h*64 .. h*64+63 of each third; the output is [B*T, H].  q is already scaled: by 1/8 for the natural-exp
instances, by log2(e)/8 for the log2 ones the forward launches (csrc/model.cpp, QKV epilogue), so a "score" below is q.k in the
kernel's own units and the softmax weight is 2^s (log2) or e^s (natural).
"""
import numpy as np

F16, BF16 = 0, 1
DT_NAME = {F16: "f16", BF16: "bf16"}
U = {F16: 2.0 ** -11, BF16: 2.0 ** -8}  # unit roundoff of T (half an ulp, relative)
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
KT = 64  # keys per tile

# Variants of launch_attention (csrc/attention.hip): (attn_v, attn_nwv).  0 = the dispatcher's own pick.
#   v1: attention_kernel<T, LOG2, 4>        -- the batch-32 kernel (128-query blocks)
#   v2: attention2_kernel<T, LOG2, 1, nw>   -- the small-batch kernel, 32 * nw queries per block (64 / 96 / 128)
#   v3: attention_kernel<T, LOG2, 2, 2>     -- 64 queries per wave
#   v4: attention2_kernel<T, LOG2, 2, 2>    -- pipelined, 64 queries per wave
VARIANTS = {"auto": (0, 0), "v1": (1, 0), "v2nw2": (2, 2), "v2nw3": (2, 3), "v2nw4": (2, 4), "v3": (3, 0), "v4": (4, 0)}
# query-block sizes of the variants (the ragged-block mutant is planted at each)
QBLOCK = {"v1": 128, "v2nw2": 64, "v2nw3": 96, "v2nw4": 128, "v3": 128, "v4": 128}

# (B, T, nh).  T covers 1 .. 6 key tiles of attention2_kernel's tail branches (exact multiples of 64 and multiples + 1), ragged last
# query blocks of 64, 96 and 128 queries, and the model's own token counts (2, 6: tiny crops; 257 / 261: 224 px without / with 4
# registers; 1370 / 1374: 518 px; 4101: 896 px with registers).  nh in {1, 6, 16, 24}, B in {1, 3}.
SHAPES = [
    (1, 1, 1), (3, 2, 6), (1, 6, 16), (1, 63, 1), (3, 64, 6), (1, 65, 24), (1, 100, 1), (3, 128, 1), (1, 129, 6),
    (1, 161, 1), (1, 192, 1), (3, 193, 6), (1, 200, 16), (1, 256, 1), (3, 257, 6), (1, 261, 16), (1, 320, 24),
    (3, 321, 1), (1, 384, 6), (1, 1370, 6), (1, 1374, 16), (3, 1374, 6), (1, 4101, 16),
]
REF_COST_MAX = 2.0e9  # the float64 reference runs where B * nh * T^2 * 64 stays below this; larger shapes rely on the probes


def shape_id(s):
    return "B%d-T%d-nh%d" % s


def ref_affordable(B, T, nh):
    return B * nh * T * T * 64 <= REF_COST_MAX


# ------------------------------------------------------------------------------------------------------------- rounding
def round_t(a, dt):
    """Round to the compute type (nearest even) and return as f32."""
    a = np.asarray(a, np.float32)
    if dt == F16:
        return a.astype(np.float16).astype(np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32).reshape(a.shape)


def t_bits(a, dt):
    """The 16-bit pattern of T values held as f32, as int32 in a monotone order (for ulp distances)."""
    a = np.asarray(a, np.float32)
    if dt == F16:
        b = a.astype(np.float16).view(np.uint16).astype(np.int32)
    else:
        b = (a.view(np.uint32) >> 16).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b)


# ------------------------------------------------------------------------------------------------------------- reference
def split_heads(qkv, B, T, nh):
    """q, k, v as float64 [B, nh, T, 64]."""
    x = np.asarray(qkv, np.float64).reshape(B, T, 3, nh, 64)
    return tuple(x[:, :, i].transpose(0, 2, 1, 3) for i in range(3))


def merge_heads(o):
    B, nh, T, _ = o.shape
    return o.transpose(0, 2, 1, 3).reshape(B * T, nh * 64)


def _head_chunks(B, nh, T):
    step = max(1, int(4_000_000 // max(1, T * T)))
    for b in range(B):
        for h0 in range(0, nh, step):
            yield b, slice(h0, min(nh, h0 + step))


def reference(qkv, B, T, nh, log2, want_stats=True):
    """float64 attention of the stored q, k, v.  log2: p ~ 2^s, else e^s.
    Returns (o, A, S, M): o [B*T, H]; A [B*T, H] = sum_j p_j |v_jd| / sum_j p_j; per query (as [B*T, nh]) S = max_j sum_d |q_d k_jd|
    and M = max_j s_j, in the kernel's score units (the score-rounding terms of the bound)."""
    q, k, v = split_heads(qkv, B, T, nh)
    o = np.empty((B, nh, T, 64))
    A = np.empty_like(o)
    S = np.empty((B, nh, T))
    M = np.empty_like(S)
    for b, hs in _head_chunks(B, nh, T):
        s = q[b, hs] @ k[b, hs].transpose(0, 2, 1)
        M[b, hs] = s.max(-1)
        if want_stats:
            S[b, hs] = (np.abs(q[b, hs]) @ np.abs(k[b, hs]).transpose(0, 2, 1)).max(-1)
        p = np.exp((s - M[b, hs][..., None]) * (LN2 if log2 else 1.0))
        l = p.sum(-1, keepdims=True)
        o[b, hs] = (p @ v[b, hs]) / l
        A[b, hs] = (p @ np.abs(v[b, hs])) / l
    nt = lambda x: x.transpose(0, 2, 1).reshape(B * T, nh)
    return merge_heads(o), merge_heads(A), nt(S), nt(M)


def error_bound(o, A, S, M, qkv, B, T, nh, dt, log2):
    """Per-element bound on |kernel - reference(stored q, k, v)|, from the kernels' numerics (csrc/attention.hip, header):

        q, k, v and the un-normalised probabilities P are MFMA inputs in T; scores, the running max / sum and the output accumulator
        are f32; p = exp2(s - m) (log2 instances) or e^(s - m) (natural ones, v_exp_f32 of a log2(e) multiple); the running maximum m
        is deferred (moves by more than THR only), so 1 <= max_j p_j <= 2^8 and l = sum p >= 1 (the true maximum has p >= 1).

      * P is rounded to T before PV, the denominator l sums the f32 p:    |sum p_j eta_j v_jd| / l <= u A_d         (|eta| <= u)
      * f16 P below 2^-14 is subnormal, absolute error <= 2^-25 each:      n_keys 2^-25 max_j |v_jd| / l, l >= 1
        (bf16 P and f32 p: only the flush below 2^-126:                   n_keys 2^-126 max_j |v_jd|)
      * f32 scores: 4 chained 16-deep MFMAs from C = -m plus the rescale subtraction, <= 68 + 4 roundings of magnitude <= S + |M|:
            |ds| <= 72 2^-24 (S + |M|)  ->  p relative error eps_p = ds (ln 2 for log2 units) + 2^-22 (v_exp_f32, 1 ulp + slack);
        a relative error eps_p on every p moves the normalised output by at most 2 eps_p A_d
      * f32 PV accumulation, the l sum, 1/l and the rescales (alpha scales O and l alike): eps_acc A_d, eps_acc = (4 n_tiles + 64) 2^-24
      * one final rounding to T: u |o| (f16: + 2^-25 for a subnormal result)
    """
    vmax = np.abs(split_heads(qkv, B, T, nh)[2]).max(2)  # [B, nh, 64]
    vmax = np.repeat(vmax.reshape(B, 1, nh * 64), T, 1).reshape(B * T, nh * 64)
    return _bound(o, A, S, M, vmax, T, dt, log2)


def _bound(o, A, S, M, vmax, T, dt, log2):
    """error_bound's formula: o, A, vmax [rows, 64 * heads]; S, M [rows, heads]; T keys."""
    u = U[dt]
    ntiles = (T + KT - 1) // KT
    ds = 72 * 2.0 ** -24 * (S + np.abs(M))
    eps_p = np.repeat(ds * (LN2 if log2 else 1.0) + 2.0 ** -22, 64, axis=1)
    eps_acc = (4 * ntiles + 64) * 2.0 ** -24
    sub = T * (2.0 ** -25 if dt == F16 else 2.0 ** -126) * vmax
    inner = u * A + sub + 2 * eps_p * A + eps_acc * A
    return inner + u * (np.abs(o) + inner) + (2.0 ** -25 if dt == F16 else 0.0)


def reference_rows(q, k, v, log2, chunk=64):
    """reference() for SOME queries of ONE (image, head): q [nq, 64], k, v [T, 64] -> o, A [nq, 64], S, M [nq].  The same float64 arithmetic, a
    chunk of queries at a time, for sequences whose full score matrix no host holds (tests/far_cases.py)."""
    q, k, v = (np.asarray(x, np.float64) for x in (q, k, v))
    nq = len(q)
    o, A, S, M = np.empty((nq, 64)), np.empty((nq, 64)), np.empty(nq), np.empty(nq)
    ka, va = np.abs(k), np.abs(v)
    for i in range(0, nq, chunk):
        j = slice(i, min(nq, i + chunk))
        s = q[j] @ k.T
        M[j] = s.max(-1)
        S[j] = (np.abs(q[j]) @ ka.T).max(-1)
        p = np.exp((s - M[j][:, None]) * (LN2 if log2 else 1.0))
        l = p.sum(-1, keepdims=True)
        o[j] = (p @ v) / l
        A[j] = (p @ va) / l
    return o, A, S, M


def error_bound_rows(o, A, S, M, v, dt, log2):
    """error_bound for the rows of reference_rows: the same formula, with the head's own max_j |v_jd| and key count."""
    v = np.asarray(v, np.float64)
    vmax = np.repeat(np.abs(v).max(0)[None, :], len(o), 0)
    return _bound(o, A, S[:, None], M[:, None], vmax, len(v), dt, log2)


def check_against_reference(out, ref, bound):
    """(ok, message): every element finite and within its bound."""
    out = np.asarray(out, np.float64)
    if not np.isfinite(out).all():
        bad = np.argwhere(~np.isfinite(out))
        return False, "%d non-finite outputs, first at row %d col %d" % (len(bad), bad[0][0], bad[0][1])
    err = np.abs(out - ref)
    ratio = err / bound
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    msg = "worst row %d col %d: |err| %.3e bound %.3e (ratio %.3f)" % (i[0], i[1], err[i], bound[i], ratio[i])
    return bool(ratio[i] <= 1.0), msg


# ------------------------------------------------------------------------------------------------------------- regimes
def regime_input(regime, B, T, nh, dt, log2, seed):
    """Random qkv for the reference comparison.  Scores are drawn in natural units and scaled by log2(e) for the log2 instances
    (as the QKV epilogue does).
      random:  N(0,1) q k v with q * 0.5 (score sd ~ 4: a peaky softmax), V columns offset (the suite's long-standing draw)
      diffuse: score sd 0.3 -- every key carries weight, a dropped or leaked key moves the output by ~1/T of |v|
      peaky:   trained-like: |score| up to 150, one sink key (index 1, a register slot) aligned with a shared query direction"""
    rng = np.random.default_rng(seed)
    H = nh * 64
    qkv = rng.standard_normal((B * T, 3 * H))
    qkv[:, 2 * H:] += np.linspace(-1, 1, H)
    if regime == "random":
        qkv[:, :H] *= 0.5
    elif regime == "diffuse":
        qkv[:, :H] *= 0.3 / 8.0
    elif regime == "peaky":
        x = qkv.reshape(B, T, 3, nh, 64)
        udir = rng.standard_normal((nh, 64))
        udir /= np.linalg.norm(udir, axis=1, keepdims=True)
        x[:, :, 0] = 10.0 * udir + 2.0 * x[:, :, 0]
        x[:, :, 1] *= 1.2
        x[:, min(1, T - 1), 1] = 12.0 * udir
        q, k, _ = split_heads(qkv, B, T, nh)
        smax = max(np.abs(q[b] @ k[b].transpose(0, 2, 1)).max() for b in range(B))
        qkv[:, :H] *= 150.0 / smax
    else:
        raise ValueError(regime)
    if log2:
        qkv[:, :H] *= LOG2E
    return round_t(qkv, dt)


REGIMES = ("random", "diffuse", "peaky")


# ------------------------------------------------------------------------------------------------------------- exact probes
_POOLS = {}


def code_pool(n, seed=1234, min_dist=12):
    """n random +-1 codes of length 64 with pairwise Hamming distance >= min_dist (checked and asserted)."""
    key = (n, seed, min_dist)
    if key in _POOLS:
        return _POOLS[key]
    rng = np.random.default_rng(seed)
    c = rng.choice(np.array([-1.0, 1.0], np.float32), size=(n, 64))
    for _ in range(100):
        g = c @ c.T  # = 64 - 2 * Hamming distance, exact in f32
        np.fill_diagonal(g, -64)
        bad = np.argwhere(g > 64 - 2 * min_dist)
        if len(bad) == 0:
            break
        redo = np.unique(np.maximum(bad[:, 0], bad[:, 1]))
        c[redo] = rng.choice(np.array([-1.0, 1.0], np.float32), size=(len(redo), 64))
    g = c @ c.T
    np.fill_diagonal(g, -64)
    assert (64 - g.max()) / 2 >= min_dist, "code pool: minimum Hamming distance not reached"
    _POOLS[key] = c
    return c


def _head_codes(rng, pool, n):
    """A random isometric image of the pool (row order, column order and per-column sign: Hamming distances are preserved)."""
    c = pool[rng.permutation(len(pool))[:n]]
    return c[:, rng.permutation(64)] * rng.choice(np.array([-1.0, 1.0], np.float32), 64)


def _v_grid(rng, shape):
    """Multiples of 1/8 with 1/4 <= |v| <= 63/8: exact in f16 and bf16, as are half-sums of two of them."""
    return rng.integers(2, 64, size=shape) / 8.0 * rng.choice([-1.0, 1.0], size=shape)


def pair_keys(T, rng):
    """Key pairs that share a code, each pair in different tiles: (0, T-1), (63, 64) and, for long sequences, two more."""
    pairs = []
    if T >= 2:
        pairs.append((0, T - 1))
    if T >= 66:
        pairs.append((63, 64))
    if T >= 200:
        used = {j for p in pairs for j in p}
        while len(pairs) < 4:
            a, b = sorted(rng.choice(T, 2, replace=False).tolist())
            if a // KT != b // KT and a not in used and b not in used:
                pairs.append((a, b))
                used |= {a, b}
    return pairs


def probe_permutation(B, T, nh, seed):
    """Keys 2 c_j, query i = c_pi(i) (pi a random permutation), V on an exact grid: the winner scores 128, every other key <= 80
    (Hamming distance >= 12), so the exact output of query i is v[pi(i)] -- bit for bit, in both score domains.  Every key is the
    target of exactly one query.  Returns (qkv f32, expected [B*T, H])."""
    rng = np.random.default_rng(seed)
    H = nh * 64
    pool = code_pool(T)
    x = np.zeros((B, T, 3, nh, 64))
    exp = np.zeros((B, T, nh, 64))
    for b in range(B):
        for h in range(nh):
            c = _head_codes(rng, pool, T)
            pi = rng.permutation(T)
            x[b, :, 1, h] = 2.0 * c
            x[b, :, 0, h] = c[pi]
            x[b, :, 2, h] = _v_grid(rng, (T, 64))
            exp[b, :, h] = x[b, pi, 2, h]
    return x.reshape(B * T, 3 * H).astype(np.float32), exp.reshape(B * T, H).astype(np.float32)


def probe_pairs(B, T, nh, seed):
    """As probe_permutation, but the keys of each pair_keys() pair share one code: the queries aimed at a pair get (v_a + v_b) / 2
    exactly (both weights are exactly 1, l = 2; the grid keeps the half-sum exact and |v_a + v_b| >= 1/2)."""
    rng = np.random.default_rng(seed)
    H = nh * 64
    pairs = pair_keys(T, rng)
    pool = code_pool(T)
    x = np.zeros((B, T, 3, nh, 64))
    exp = np.zeros((B, T, nh, 64))
    for b in range(B):
        for h in range(nh):
            c = _head_codes(rng, pool, T)
            v = _v_grid(rng, (T, 64))
            partner = np.arange(T)
            for a, bb in pairs:
                c[bb] = c[a]
                partner[a], partner[bb] = bb, a
                while True:  # |v_a + v_b| >= 1/2 in every column
                    small = np.abs(v[a] + v[bb]) < 0.5
                    if not small.any():
                        break
                    v[bb, small] = _v_grid(rng, int(small.sum()))
            pi = rng.permutation(T)
            x[b, :, 1, h] = 2.0 * c
            x[b, :, 0, h] = c[pi]
            x[b, :, 2, h] = v
            exp[b, :, h] = (v[pi] + v[partner[pi]]) / 2.0
    return x.reshape(B * T, 3 * H).astype(np.float32), exp.reshape(B * T, H).astype(np.float32)


def onehot_columns(T, rng):
    """Key j_d of each of the 64 value columns: 0, 63, 64, 65, T-2, T-1 (those that exist) and random others, shuffled."""
    must = sorted({j for j in (0, 63, 64, 65, T - 2, T - 1) if 0 <= j < T})
    js = np.concatenate([must, rng.integers(0, T, 64 - len(must))])
    return rng.permutation(js)


def probe_onehot(B, T, nh, dt, seed):
    """q = 0 (every score exactly 0, every weight exactly 1, l = T) and V[:, d] one-hot at key j_d: every output is T(1/T) within
    one ulp.  A dropped key j_d gives 0 in column d; L leaked copies of the clamped tail key give (1 + L) / (T + L) in the column
    of key T-1 and 1 / (T + L) elsewhere.  K is random (the scores must not depend on it).  Returns (qkv, expected)."""
    rng = np.random.default_rng(seed)
    H = nh * 64
    x = np.zeros((B, T, 3, nh, 64))
    x[:, :, 1] = rng.standard_normal((B, T, nh, 64))
    for b in range(B):
        for h in range(nh):
            js = onehot_columns(T, rng)
            x[b, js, 2, h, np.arange(64)] = 1.0
    exp = np.full((B * T, H), 1.0 / T)
    return round_t(x.reshape(B * T, 3 * H), dt), round_t(exp, dt)


def check_probe(kind, out, exp, dt):
    """(ok, message).  permutation / pairs: bit for bit; onehot: within one ulp of T."""
    out = np.asarray(out, np.float32)
    if not np.isfinite(out).all():
        bad = np.argwhere(~np.isfinite(out))
        return False, "%s probe: %d non-finite outputs (unwritten rows?), first at row %d col %d" % (kind, len(bad), bad[0][0], bad[0][1])
    if kind == "onehot":
        d = np.abs(t_bits(out, dt) - t_bits(exp, dt))
        ok = d.max() <= 1
    else:
        d = (out != exp).astype(np.int32)
        ok = not d.any()
    if ok:
        return True, "%s probe: exact" % kind
    i = np.unravel_index(np.argmax(d), d.shape)
    return False, "%s probe: %d mismatches, first at row %d col %d: got %r expected %r" % (
        kind, int((d > (1 if kind == "onehot" else 0)).sum()), i[0], i[1], float(out[i]), float(exp[i]))


PROBES = ("permutation", "pairs", "onehot")


def build_probe(kind, B, T, nh, dt, seed):
    if kind == "permutation":
        return probe_permutation(B, T, nh, seed)
    if kind == "pairs":
        return probe_pairs(B, T, nh, seed)
    return probe_onehot(B, T, nh, dt, seed)


# ------------------------------------------------------------------------------------------------------------- emulation
MUTANTS = ("drop_last_key", "drop_key_64", "leak_tail", "exp_swapped", "q_scaled_twice", "heads_swapped", "ragged_rows_shifted")
# Planted bugs that finite data cannot show (every check above passes them): only a NaN tracer does (tests/tracer_cases.py).
#   mask_by_multiply: the key tail is staged from the rows that FOLLOW the image (the next image's first keys; the last image's tail from
#                     its own last key) and its weights are forced to 0 by a product, p * 0, instead of the select to -inf
TRACER_MUTANTS = ("mask_by_multiply",)


def emulate(qkv, B, T, nh, dt, log2, mutant=None, qblock=128):
    """numpy restatement of the kernels' documented arithmetic (csrc/attention.hip): q, k, v in T; per 64-key tile (keys past the
    end staged as copies of key T-1, then masked) f32 scores, a deferred running maximum (THR 8 in log2 units, 5.5 natural), f32
    weights from exp2 / exp, P rounded to T for PV, f32 l and O, one final rounding to T.  `mutant` plants one bug of MUTANTS."""
    f = np.float32
    x = np.asarray(qkv, f).reshape(B, T, 3, nh, 64)
    q, k, v = (np.ascontiguousarray(x[:, :, i].transpose(0, 2, 1, 3)) for i in range(3))
    if mutant == "q_scaled_twice":
        q = round_t(q * f(0.125 * LOG2E if log2 else 0.125), dt)
    use2 = log2 != (mutant == "exp_swapped")
    ex = (lambda z: np.exp2(z, dtype=f)) if use2 else (lambda z: np.exp(z, dtype=f))
    thr = f(8.0 if log2 else 5.5)
    ntiles = (T + KT - 1) // KT
    o = np.zeros((B, nh, T, 64), f)
    l = np.zeros((B, nh, T), f)
    m = np.zeros((B, nh, T), f)
    for jt in range(ntiles):
        idx = np.minimum(np.arange(jt * KT, jt * KT + KT), T - 1)  # the staging clamps the tail to key T-1
        kt, vt = k[:, :, idx], v[:, :, idx]
        if mutant == "mask_by_multiply" and jt == ntiles - 1 and B > 1:
            over = np.minimum(np.arange(jt * KT, jt * KT + KT) - T, T - 1)  # >= 0: position of a tail key among the next image's rows
            kt, vt = kt.copy(), vt.copy()
            kt[:-1, :, over >= 0] = k[1:, :, over[over >= 0]]
            vt[:-1, :, over >= 0] = v[1:, :, over[over >= 0]]
        s = np.matmul(q, kt.transpose(0, 1, 3, 2)) - m[..., None]
        keys = np.arange(jt * KT, jt * KT + KT)
        dead = keys >= T
        if mutant == "leak_tail":
            dead = np.zeros_like(dead)
        if mutant == "drop_last_key":
            dead = dead | (keys == T - 1)
        if mutant == "drop_key_64":
            dead = dead | (keys == 64)
        s[..., dead] = -np.inf
        mx = s.max(-1)
        need = (mx > thr) | (jt == 0)
        d = np.where(need, mx, f(0))
        alpha = np.where(jt == 0, f(0), ex(-d)).astype(f)
        m = m + d
        l = l * alpha
        o = o * alpha[..., None]
        s = s - d[..., None]
        p = ex(s)
        if mutant == "mask_by_multiply":  # the scores were masked for the maximum only: p = 2^(q.k - m) * 0 for the tail
            with np.errstate(invalid="ignore", over="ignore"):
                p = np.where(dead, ex(np.matmul(q, kt.transpose(0, 1, 3, 2)) - m[..., None]) * f(0), p)
        l = l + p.sum(-1, dtype=f)
        o = o + np.matmul(round_t(p, dt), vt)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = round_t(o * (f(1) / l)[..., None], dt)
    if mutant == "heads_swapped" and nh > 1:
        out[:, [0, 1]] = out[:, [1, 0]]
    if mutant == "ragged_rows_shifted":
        start = ((T - 1) // qblock) * qblock  # the last (ragged) query block: its rows land one row too far (the first written twice)
        out[:, :, start + 1:] = out[:, :, start:T - 1].copy()
    return merge_heads(out.astype(np.float64)).astype(np.float32)
