"""Cases for dinov2_hip_match_tokens / dinov2_hip_op_match (csrc/match.hip), shared by tests/test_match_probes.py (CPU: the numpy restatement
of the contract passes them, planted bugs do not) and tests/test_gpu_match.py (the kernels).

Contract under test (include/dinov2_hip.h): rows to unit length in f16 (f32 sum of squares, correctly rounded 1 / sqrt), f32 accumulation of
exact products, argmax over the real rows / columns with ties to the lowest index, both directions from the same products.

Three kinds of case:
  shapes   Gaussian tokens with two x50 outlier channels against the float64 cosine similarity of the un-rounded inputs.  Bound per
           similarity: tol = 2^-10 + H 2^-24 -- each operand carries <= 2^-11 relative rounding and sum |a^_k b^_k| <= 1 (Cauchy-Schwarz on
           unit rows), f32 accumulation adds <= H 2^-24.  A result is accepted when |sim - S[i, idx]| <= tol and S[i, idx] >= max_j S[i, j]
           - 2 tol: a near-tie passes with either index, a row with a clear gap must have exactly the reference index.
  probes   rows whose non-zeros are +-1 in exactly 1, 4, 16 or 64 positions: the norm is a power of two, x^ = +-2^-k exactly, every
           similarity is a short dyadic sum that is exact in f32 in any order -- so values AND indices are compared bit for bit, tie rule included.
  planted  b Gaussian, a = b[perm] + 0.1 noise: every row has one clear partner (gap asserted on the reference), so idx_ab == perm, all mutual.
"""
import numpy as np

TM = TN = 128            # match_kernel's tile (csrc/kernels.h MATCH_TM / MATCH_TN)
PASS = 128 * TM          # rows / columns of one pass (MATCH_PASS tiles): one more than this takes the multi-pass path
EMPTY = np.iinfo(np.int32).max

# (na, nb, H): tile edges and K padding at the smallest sizes; the last two cross a pass boundary in either direction (thin, so still quick)
SHAPES = [(1, 1, 8), (1, TN + 1, 8), (TM - 1, TN, 64), (TM, TN + 1, 72), (TM + 1, 2 * TN + 1, 384), (257, 300, 1536), (3, 1374, 1024),
          (PASS + 1, 3, 8), (3, PASS + 1, 8)]
PROBES = [("pm1", 64), ("pm1", 72), ("duplicates", 72), ("zero_row", 64), ("negated", 72)]
MUTANTS = ["pad_col_counted", "pad_row_counted", "tie_highest", "last_col_tile_dropped", "k_pad_not_zeroed", "directions_swapped",
           "resident_offset_wrong"]
KEYS = ("idx_ab", "sim_ab", "idx_ba", "sim_ba")


def shape_id(s):
    return "x".join(str(v) for v in s)


def tol(H):
    return 2.0 ** -10 + H * 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------------- inputs
def gaussian_tokens(n, H, seed, outliers=True):
    """Unit Gaussian rows; with `outliers`, two channels carry x50 (the massive-activation channels of trained ViT tokens)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, H))
    if outliers:
        x[:, [1, H - 2]] *= 50.0
    return x.astype(np.float32)


def shape_inputs(shape):
    na, nb, H = shape
    return gaussian_tokens(na, H, 100 + na + H), gaussian_tokens(nb, H, 200 + nb + H)


def reference(a, b):
    """float64 cosine similarity [na, nb] of the un-rounded inputs (an all-zero row: 0)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na_, nb_ = np.sqrt((a * a).sum(1)), np.sqrt((b * b).sum(1))
    an = a / np.where(na_ > 0, na_, 1.0)[:, None]
    bn = b / np.where(nb_ > 0, nb_, 1.0)[:, None]
    return an @ bn.T


def _pm1_rows(rng, n, H, positive=False):
    """Rows with +-1 (all +1, position 0 among them, with `positive`) in exactly 1, 4, 16 or 64 positions."""
    x = np.zeros((n, H), np.float32)
    for i in range(n):
        k = (1, 4, 16, 64)[int(rng.integers(4))]
        if positive:
            pos = np.concatenate([[0], 1 + rng.choice(H - 1, k - 1, replace=False)])
            x[i, pos] = 1.0
        else:
            pos = rng.choice(H, k, replace=False)
            x[i, pos] = rng.choice([-1.0, 1.0], k)
    return x


def _exact_expectation(a, b):
    """Probe rows normalise to +-2^-k exactly, so float64 gives every similarity exactly; np.argmax returns the FIRST maximum (-0 == +0)."""
    S = reference(a, b)
    S32 = S.astype(np.float32)
    assert np.array_equal(S32.astype(np.float64), S), "probe similarities are not exact in f32"
    S32 = S32 + np.float32(0.0)
    ia, ib = S.argmax(1).astype(np.int32), S.argmax(0).astype(np.int32)
    return {"idx_ab": ia, "sim_ab": S32[np.arange(len(a)), ia], "idx_ba": ib, "sim_ba": S32[ib, np.arange(len(b))]}


def build_probe(kind, H, seed=5):
    """(a, b, expected) of an exact probe; `expected` holds the four arrays bit for bit."""
    rng = np.random.default_rng(seed + H)
    na, nb = TM + 3, 2 * TN + 5  # two row tiles, three column tiles, the last ones partial
    if kind == "pm1":
        a, b = _pm1_rows(rng, na, H), _pm1_rows(rng, nb, H)
    elif kind == "duplicates":
        # 16 non-zeros everywhere: a row equals another only where planted.  Duplicates in b on each side of a column-tile boundary and in
        # the last, partial tile; in a on each side of the row-tile boundary.  The partner of a duplicated row is a copy of it: similarity 1.
        def rows16(n):
            x = np.zeros((n, H), np.float32)
            for i in range(n):
                x[i, rng.choice(H, 16, replace=False)] = rng.choice([-1.0, 1.0], 16)
            return x
        a, b = rows16(na), rows16(nb)
        b[TN + 1] = b[TN - 1]
        b[nb - 1] = b[5]
        a[0], a[1] = b[TN - 1], b[5]
        a[TM - 1] = a[TM + 1] = b[7]
        S = reference(a, b)
        assert sorted(np.flatnonzero(S[0] == 1.0)) == [TN - 1, TN + 1] and sorted(np.flatnonzero(S[1] == 1.0)) == [5, nb - 1]
        assert sorted(np.flatnonzero(S[:, 7] == 1.0)) == [TM - 1, TM + 1]
    elif kind == "zero_row":
        a, b = _pm1_rows(rng, na, H), _pm1_rows(rng, nb, H)
        a[TM + 1] = 0.0
        b[0] = 0.0
        b[TN + 2] = 0.0
    elif kind == "negated":
        # all-positive rows that share position 0: every similarity of a = -b[perm] with b is negative, so a zero padding row or column
        # that is counted wins.  Neither count is a tile multiple.
        na = nb = TN + 5
        b = _pm1_rows(rng, nb, H, positive=True)
        a = -b[rng.permutation(nb)]
        assert reference(a, b).max() < 0
    else:
        raise ValueError(kind)
    exp = _exact_expectation(a, b)
    if kind == "duplicates":
        assert exp["idx_ab"][0] == TN - 1 and exp["idx_ab"][1] == 5 and exp["idx_ba"][7] == TM - 1
    if kind == "zero_row":
        assert exp["idx_ab"][TM + 1] == 0 and exp["sim_ab"][TM + 1] == 0 and exp["idx_ba"][TN + 2] == 0
    return a, b, exp


def planted(n=300, H=384, seed=9):
    """(a, b, perm): b Gaussian without outlier channels, a = b[perm] + 0.1 noise.  The best-versus-second gap of every row and column of
    the float64 reference is asserted to be >= 4 tol before the case is used (a CPU check gave a minimum of 0.019 at H = 384)."""
    rng = np.random.default_rng(seed)
    b = gaussian_tokens(n, H, seed + 1, outliers=False)
    perm = rng.permutation(n).astype(np.int32)
    a = (b[perm] + 0.1 * rng.standard_normal((n, H))).astype(np.float32)
    S = reference(a, b)
    for M in (S, S.T):
        top = np.sort(M, axis=1)[:, -2:]
        assert (top[:, 1] - top[:, 0]).min() >= 4 * tol(H)
    assert np.array_equal(S.argmax(1), perm)
    return a, b, perm


def resident_stream(B=2, P=20, R=4, H=32, seed=13):
    """A synthetic final-LayerNorm token stream [B, T = 1 + R + P, H] for the resident view (CPU probes)."""
    return gaussian_tokens(B * (1 + R + P), H, seed).reshape(B, 1 + R + P, H), R


def resident_rows(fin, R, image, mutant=None):
    """The rows a NULL side stands for: the patch rows 1 + R .. T - 1 of `image` -- never the registers, classify or not."""
    P = fin.shape[1] - 1 - R
    first = 1 if mutant == "resident_offset_wrong" else 1 + R
    return fin[image, first:first + P]


# ------------------------------------------------------------------------------------------------------------------- restatement
def normalise_f16(x):
    x = np.asarray(x, np.float32)
    ss = (x * x).sum(1, dtype=np.float32)
    with np.errstate(divide="ignore"):
        r = np.where(ss > 0, np.float32(1.0) / np.sqrt(ss, dtype=np.float32), np.float32(0.0)).astype(np.float32)
    return (x * r[:, None]).astype(np.float16)


def emulate(a, b, mutant=None):
    """numpy restatement of the contract with the kernel's padding made explicit: operands padded to whole tiles and H to a multiple of 64,
    the argmax masked to the real rows / columns.  `mutant`: one of MUTANTS, planted."""
    na, nb, H = len(a), len(b), a.shape[1]
    na_pad, nb_pad, hpad = -(-na // TM) * TM, -(-nb // TN) * TN, -(-H // 64) * 64
    fill = 1.0 if mutant == "k_pad_not_zeroed" else 0.0
    A = np.full((na_pad, hpad), fill, np.float32)
    Bm = np.full((nb_pad, hpad), fill, np.float32)
    A[:, :H] = 0.0
    Bm[:, :H] = 0.0
    A[:na, :H] = normalise_f16(a).astype(np.float32)
    Bm[:nb, :H] = normalise_f16(b).astype(np.float32)
    S = (A @ Bm.T).astype(np.float32) + np.float32(0.0)
    rows = na_pad if mutant == "pad_row_counted" else na
    cols = nb_pad if mutant == "pad_col_counted" else nb
    if mutant == "last_col_tile_dropped" and nb_pad > TN:
        cols = nb_pad - TN

    def argbest(M):  # per row of M: (first | last) maximum
        if M.shape[1] == 0:
            return np.full(M.shape[0], EMPTY, np.int32), np.full(M.shape[0], -np.inf, np.float32)
        if mutant == "tie_highest":
            idx = M.shape[1] - 1 - M[:, ::-1].argmax(1)
        else:
            idx = M.argmax(1)
        return idx.astype(np.int32), M[np.arange(M.shape[0]), idx]

    ia, sa = argbest(S[:na, :cols])
    ib, sb = argbest(S[:rows, :nb].T)
    if mutant == "last_col_tile_dropped" and nb_pad > TN:  # the columns of the dropped tile never get a result
        ib, sb = ib.copy(), sb.copy()
        ib[cols:], sb[cols:] = EMPTY, -np.inf
    out = {"idx_ab": ia, "sim_ab": sa, "idx_ba": ib, "sim_ba": sb}
    if mutant == "directions_swapped":
        out = {"idx_ab": ib, "sim_ab": sb, "idx_ba": ia, "sim_ba": sa}
    return out


# ------------------------------------------------------------------------------------------------------------------- checks
def _well_formed(res, na, nb, what):
    for k, n in zip(KEYS, (na, na, nb, nb)):
        if np.asarray(res[k]).shape != (n,):
            return False, f"{what}: {k} has shape {np.asarray(res[k]).shape}, expected ({n},)"
    for k, n in (("idx_ab", nb), ("idx_ba", na)):
        v = np.asarray(res[k])
        if v.min() < 0 or v.max() >= n:
            return False, f"{what}: {k} outside [0, {n}): min {v.min()} max {v.max()}"
    for k in ("sim_ab", "sim_ba"):
        if not np.isfinite(res[k]).all():
            return False, f"{what}: {k} is not finite"
    return True, ""


def check_against_reference(res, S, H, what, report=None):
    """The tolerance rule of the module docstring in both directions.  `report`: a list that receives the measured figures."""
    na, nb = S.shape
    ok, msg = _well_formed(res, na, nb, what)
    if not ok:
        return ok, msg
    t = tol(H)
    for d, M, idx, sim in (("ab", S, res["idx_ab"], res["sim_ab"]), ("ba", S.T, res["idx_ba"], res["sim_ba"])):
        at = M[np.arange(M.shape[0]), idx]
        err = np.abs(sim.astype(np.float64) - at)
        short = M.max(1) - at
        if report is not None:
            report.append(f"{what} {d}: max |sim - S| {err.max():.3e} (tol {t:.3e}), max shortfall {short.max():.3e} (2 tol {2 * t:.3e}), "
                          f"{int((idx != M.argmax(1)).sum())} of {len(idx)} indices differ from the reference argmax")
        if err.max() > t:
            i = int(err.argmax())
            return False, f"{what} {d}: row {i}: sim {sim[i]!r} vs reference {at[i]!r} at index {idx[i]}: error {err[i]:.3e} > tol {t:.3e}"
        if short.max() > 2 * t:
            i = int(short.argmax())
            return False, (f"{what} {d}: row {i}: index {idx[i]} has reference similarity {at[i]!r}, the maximum is {M[i].max()!r} at "
                           f"{int(M[i].argmax())}: short by {short[i]:.3e} > 2 tol {2 * t:.3e}")
    return True, ""


def check_exact(res, exp, what):
    """All four arrays bit for bit (similarities compared as their 32-bit patterns: -0 is not +0 here)."""
    for k in KEYS:
        g, e = np.asarray(res[k]), np.asarray(exp[k])
        if g.shape != e.shape:
            return False, f"{what}: {k} has shape {g.shape}, expected {e.shape}"
        gb, eb = (g.astype(np.float32).view(np.uint32), e.astype(np.float32).view(np.uint32)) if k.startswith("sim") else (g, e)
        if not np.array_equal(gb, eb):
            i = int(np.flatnonzero(gb != eb)[0])
            return False, f"{what}: {k}[{i}] = {g[i]!r}, expected {e[i]!r} ({int((gb != eb).sum())} of {g.size} differ)"
    return True, ""


def check_planted(res, perm, what):
    if np.asarray(res["idx_ab"]).shape != perm.shape or not np.array_equal(res["idx_ab"], perm):
        return False, f"{what}: idx_ab is not the planted permutation"
    if np.asarray(res["idx_ba"]).shape != perm.shape:
        return False, f"{what}: idx_ba has the wrong length"
    mutual = res["idx_ba"][res["idx_ab"]] == np.arange(len(perm))
    if not mutual.all():
        return False, f"{what}: {int((~mutual).sum())} planted pairs are not mutual"
    return True, ""


def all_failures(match_fn, resident_fn):
    """Every case through match_fn(a, b) -> result dict and resident_fn(fin, R, image_a, image_b) -> result dict; the failure messages."""
    failures = []

    def note(ok_msg):
        if not ok_msg[0]:
            failures.append(ok_msg[1])

    for shape in SHAPES:
        a, b = shape_inputs(shape)
        note(check_against_reference(match_fn(a, b), reference(a, b), shape[2], "shape " + shape_id(shape)))
    for kind, H in PROBES:
        a, b, exp = build_probe(kind, H)
        note(check_exact(match_fn(a, b), exp, f"probe {kind} H={H}"))
    a, b, perm = planted()
    note(check_planted(match_fn(a, b), perm, "planted"))
    fin, R = resident_stream()
    note(check_exact(resident_fn(fin, R, 0, 1), emulate(resident_rows(fin, R, 0), resident_rows(fin, R, 1)), "resident view"))
    return failures
