"""Cases for the device half of dinov2_hip_pca3 (csrc/kernels_misc.hip: pca_mean_kernel, pca_center_transpose_kernel, pca_power_kernel,
pca_project_kernel; the covariance GEMM with A == W aliased; csrc/pca.cpp: the driver), shared by tests/test_pca_probes.py (CPU: the numpy
emulations pass every check, planted bugs do not), tests/test_gpu_pca_kernels.py (each kernel alone through dinov2_hip_op_pca_*) and
tests/test_gpu_parity.py (the whole call).  Plain module, no fixtures.

Every emulation takes `mutant`: the name of one planted bug (MUTANTS) or None.

Tolerances -- each is zero, or derived here from operation counts and format widths, or 16 x the emulation's own error (end to end):

  mean        bit for bit.  The kernel adds 16 strided partial sums (row t goes to group t % 16, rows in ascending order) in double, adds the groups
              in ascending order, divides by P in double and rounds to f32; mean_emulate does the same additions in the same order.  On dyadic
              inputs every sum is exact, so the expected mean is f32(float64 mean) whatever the order.
  xt          bit for bit: f16(f32(tok[p][h]) - mean[h]) (one f32 subtraction, one round-to-nearest-even conversion, subnormals kept), from the
              mean the kernel itself returned; every column p >= P exactly +0.
  covariance  |got - ref| <= Ppad 2^-24 sum_p |xt[i][p] xt[j][p]| against the float64 product of the returned xt: a product of two f16 values is
              exact in f32, so only the Ppad - 1 f32 additions round, in an order we do not need to know (Higham, Accuracy and Stability, 3.1:
              any order, (n - 1) u).  Small integers: every partial sum is an integer below 2^24, so the result is exact in any order.
  power       the kernel forms t = cov Y_prev (per entry H fused multiply-adds in double, spread over 64 lanes and folded by 6 shuffle adds: H
              terms in some order, error <= H u sum |cov_ij y_jc|, u = 2^-53), then q_b = sum_a t_a rinv_ab (8 more fused multiply-adds: 8 u).
              To first order |q - q_exact| <= (H + 8) u (|cov| |Y| |rinv|)_ib = c H u (...) with c = 1 + 8 / H; POWER_SLACK = 1.01 covers the
              second-order terms.  |Y| |rinv| stands where |Q| = |Y rinv| would if R^-1 were applied first: the kernel applies it last.
              Conditioning of R^-1: the kernel's copy of pca_chol_rinv is compiled with contraction to fma, the port here is not, so the two
              factors differ by rounding.  Cholesky is backward stable with |dG| <= gamma_9 |R^T| |R| (Higham 10.3), ||dG||_F <= 72 u ||G||_2;
              the factor moves by ||dR||_F <= kappa(G) (72 u) ||R||_2 / sqrt 2 (Higham 10.8), its inverse by kappa(R) times that relative
              change, and the back substitution adds 8 u kappa(R): phi = u (51 kappa^1.5 + 8 kappa^0.5), kappa = cond_2 of the live part of G.
              Two evaluations differ by at most 2 phi ||rinv||_2, which multiplies ||t_i||_2.  Nothing here is fitted.
  gram parts  part k = the Gram matrix of rows 16 k .. 16 k + 15 of the returned Y_next (16 fused multiply-adds in row order: 16 u sum |y_ra y_rb|),
              rows >= H contributing exactly 0; the parts sum to Y_next^T Y_next within (16 + parts) u sum |y_ra y_rb|.
  projection  |got - ref64| <= 2^-24 |ref64| + H 2^-52 sum_j |d_j c_j|: double accumulation (H terms, any order, plus the subtraction's rounding),
              one rounding to f32.
  end to end  1 - |cos| (or 1 - sigma_min for a tied pair) of each component against the float64 SVD, and the projection error relative to the
              largest projection, may be 16 x what pca3_emulate itself shows on the same input, floored at 1e-7 (E2E_MARGIN, E2E_FLOOR): the
              emulation shares the device's f16 rounding of the centred tokens, which dominates; the margin is for the f32 accumulation order of
              the matrix cores, which the emulation does not reproduce.

Measured with pca3_emulate on the CPU (tests/test_pca_probes.py prints the table; profiles/pca_tests.md keeps it beside the device's figures):

  input          size        max 1 - |cos|   projection error   steps
  structured     256 x 384   3.9e-09         2.4e-06            16
  scaled_1e-4    256 x 384   3.4e-09         4.7e-06            16
  scaled_1e3     256 x 384   3.4e-09         2.6e-06            16
  flat           256 x 384   1.4e-06         1.6e-03            112
  flat           300 x 40    4.7e-07         7.8e-04            64
  tie12          300 x 128   3.8e-09         1.5e-05            16
  neartie34      300 x 128   6.4e-10         8.2e-06            16
  eleven         700 x 100   9.5e-09         3.0e-05            16
  mean1000       300 x 128   4.2e-09         1.2e-05            16
  minimal        4 x 8       8.4e-08         3.6e-04            16
  minimal        4 x 64      2.7e-08         6.2e-05            16
  minimal        5 x 200     8.2e-08         3.5e-04            16

(The figures move a little with the BLAS that numpy uses; the tests compute them where they run.)
"""
import numpy as np

NB, ROWS = 8, 16         # block width and rows per workgroup of pca_power_kernel (csrc/kernels.h PCA_NB / PCA_ROWS)
U24, U53 = 2.0 ** -24, 2.0 ** -53
POWER_SLACK = 1.01
E2E_MARGIN, E2E_FLOOR = 16.0, 1e-7

# (P, H) of the kernel tests: P and H below, at and past the 32 x 32 transpose tile; H below, at and past the mean kernel's 64 columns per
# workgroup and the 64-lane j loops; H that is no multiple of 16 or 4 (partial workgroup / wave of the power kernel); P just past a multiple of
# 128 (zero padding); P < 16 (groups of the mean kernel without a row).
P_VALUES = (4, 31, 33, 128, 129, 300)
H_VALUES = (8, 12, 33, 63, 65, 100, 384)
SHAPES = [(4, 8), (31, 12), (33, 33), (128, 63), (129, 65), (300, 100), (4, 384), (300, 384), (129, 12), (31, 65)]
# pca_project_kernel runs 4 rows per workgroup: P % 4 = 1, 2, 3 and 0 (6 is the one P outside P_VALUES: none of those leaves 2 rows)
PROJECT_SHAPES = [(33, 33), (6, 65), (31, 12), (300, 100), (129, 384), (4, 8)]
# covariance: every shape above runs a small-tile plan (api.gemm_plan(F16, 5, H, H, Ppad): "small<64x128,w4x2,st3,ks1>" at Ppad = 128,
# "small<32x64,w1x4,st3,ks2>" at 256 and 384), and so does H = 1024 ("small<64x64,w2x4,st3,ks2>", the workload's).  The large-tile kernels of
# csrc/gemm2.hip take the aliased operands from H = 2048: these two shapes reach them.  tests/test_pca_probes.py pins the names.
COV_PLANS = {(4, 8): "small<64x128,w4x2,st3,ks1>", (129, 65): "small<32x64,w1x4,st3,ks2>", (300, 384): "small<32x64,w1x4,st3,ks2>",
             (129, 2048): "gemm2<128>", (129, 4096): "gemm2<256>"}
COV_LARGE_SHAPES = [(129, 2048), (129, 4096)]

MUTANTS = ("gram_last_group_missing", "dead_row_reads_last_row", "pad_column_not_zeroed", "mean_divided_by_ppad", "f16_before_subtract",
           "rinv_transposed", "project_skips_tail_row", "project_keeps_mean")


def shape_id(s):
    return "x".join(str(v) for v in s)


def ppad(P):
    return (P + 127) // 128 * 128


def blocks(H):
    return (H + ROWS - 1) // ROWS


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_exact(got, exp, what):
    """(ok, message): equal bit patterns (so -0 is not +0, and a NaN equals only the same NaN), with the number of differing elements."""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape or got.dtype != exp.dtype:
        return False, f"{what}: got {got.dtype}{got.shape}, expected {exp.dtype}{exp.shape}"
    bad = _bits(got) != _bits(exp)
    if not bad.any():
        return True, ""
    i = np.unravel_index(int(np.flatnonzero(bad.ravel())[0]), got.shape)
    return False, f"{what}: {int(bad.sum())} of {got.size} elements differ (first at {i}: got {got[i]!r}, expected {exp[i]!r})"


def check_bound(got, ref, bound, what, report=None):
    """(ok, message): |got - ref| <= bound per entry, everything finite.  `report` receives the worst ratio error / bound."""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    if got.shape != ref.shape:
        return False, f"{what}: got shape {got.shape}, expected {ref.shape}"
    if not np.isfinite(got).all():
        return False, f"{what}: {int((~np.isfinite(got)).sum())} of {got.size} elements are not finite"
    err = np.abs(got - ref)
    over = err > bound
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    if report is not None:
        report.append(f"{what}: max error {err.max():.3e}, worst error / bound {ratio.max():.3g}")
    if over.any():
        i = np.unravel_index(int(ratio.argmax()), got.shape)
        return False, f"{what}: {int(over.sum())} of {got.size} outside the bound (worst at {i}: got {got[i]!r}, reference {ref[i]!r}, bound {bound[i]:.3e})"
    return True, ""


# ------------------------------------------------------------------------------------------------------------------- kernel inputs
def tokens_generic(P, H, seed=0):
    """Unit Gaussian tokens on a per-column offset (patch tokens are not centred)."""
    rng = np.random.default_rng(1000 + 7 * P + H + seed)
    return (rng.standard_normal((P, H)) + 4.0 * rng.standard_normal(H)).astype(np.float32)


def tokens_dyadic(P, H):
    """Multiples of 1/8 below 64: every partial sum of a column is exact in double in any order."""
    rng = np.random.default_rng(2000 + 7 * P + H)
    return (rng.integers(-511, 512, (P, H)) / 8.0).astype(np.float32)


def _paired(a, P):
    """Rows a, -a (and a zero row for odd P): every column sums to exactly 0 in any order."""
    rows = [a[:P // 2], -a[:P // 2]] + ([np.zeros((1, a.shape[1]), a.dtype)] if P % 2 else [])
    return np.concatenate(rows, 0)


def tokens_subnormal(P, H):
    """Centred values from 2^-28 to 2^-10 with either sign: below, inside and above the f16 subnormal range (2^-24 .. 2^-14).  The mean is 0."""
    rng = np.random.default_rng(3000 + 7 * P + H)
    a = np.ldexp(rng.uniform(1.0, 2.0, (P // 2, H)), rng.integers(-28, -10, (P // 2, H))) * rng.choice([-1.0, 1.0], (P // 2, H))
    return _paired(a.astype(np.float32), P)


def tokens_large(P, H):
    """|centred value| just under the f16 limit: 65504 itself, 65519 (the last f32 integer that still rounds down to it) and values down to
    60000.  The mean is 0, so nothing overflows."""
    rng = np.random.default_rng(4000 + 7 * P + H)
    a = rng.uniform(60000.0, 65519.0, (P // 2, H)).astype(np.float32) * rng.choice([-1.0, 1.0], (P // 2, H)).astype(np.float32)
    a[0, 0], a[0, 1 % H] = 65504.0, 65519.0
    return _paired(a, P)


def tokens_integer(P, H):
    """Integer offset per column + integers in [-8, 8] in +- pairs: the mean is the offset exactly, the centred tokens are small integers, and
    every partial sum of the covariance is an integer below 2^24 (P 64 < 2^24)."""
    rng = np.random.default_rng(5000 + 7 * P + H)
    a = rng.integers(-8, 9, (P // 2, H)).astype(np.float32)
    return _paired(a, P) + rng.integers(-20, 21, H).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------- mean / centre
def mean_emulate(tok, mutant=None):
    tok = np.asarray(tok, np.float32)
    P, H = tok.shape
    x = tok.astype(np.float64)
    tot = np.zeros(H, np.float64)
    for g in range(16):
        s = np.zeros(H, np.float64)
        for t in range(g, P, 16):
            s = s + x[t]
        tot = tot + s
    return (tot / (ppad(P) if mutant == "mean_divided_by_ppad" else P)).astype(np.float32)


def center_emulate(tok, mean, mutant=None):
    """xt [H, Ppad] as f32 values of the f16 matrix; the buffer starts as NaN, as the testing entry point's does."""
    tok, mean = np.asarray(tok, np.float32), np.asarray(mean, np.float32)
    P, H = tok.shape
    xt = np.full((H, ppad(P)), np.nan, np.float32)
    xt[:, P:] = 0.0
    src = tok.astype(np.float16).astype(np.float32) if mutant == "f16_before_subtract" else tok
    with np.errstate(over="ignore"):
        xt[:, :P] = (src - mean[None, :]).astype(np.float32).astype(np.float16).astype(np.float32).T
    if mutant == "pad_column_not_zeroed":
        xt[H // 2, ppad(P) - 1] = np.nan
    return xt


def prepare_emulate(tok, mutant=None):
    mean = mean_emulate(tok, mutant)
    return mean, center_emulate(tok, mean, mutant)


def check_prepare(prepare, tok, what, exact_mean=False, finite=True):
    """prepare(tok) -> (mean [H] f32, xt [H, Ppad] f32): failure messages."""
    tok = np.asarray(tok, np.float32)
    P, H = tok.shape
    mean, xt = prepare(tok)
    fails = []
    exp_mean = mean_emulate(tok)
    if exact_mean:  # every sum exact: the float64 mean itself
        m64 = tok.astype(np.float64).mean(0).astype(np.float32)
        assert np.array_equal(_bits(exp_mean), _bits(m64)), "the input's sums are not exact"
    ok, msg = check_exact(np.asarray(mean), exp_mean, what + " mean")
    if not ok:
        fails.append(msg)
    mean = np.asarray(mean, np.float32)
    if mean.shape != (H,) or np.asarray(xt).shape != (H, ppad(P)):
        return fails + [f"{what}: shapes {mean.shape} {np.asarray(xt).shape}"]
    exp = center_emulate(tok, mean)  # from the mean the kernel returned
    if finite:
        assert np.isfinite(exp).all(), "the input overflows f16"
    ok, msg = check_exact(np.asarray(xt)[:, :P], exp[:, :P], what + " xt")
    if not ok:
        fails.append(msg)
    ok, msg = check_exact(np.asarray(xt)[:, P:], exp[:, P:], what + " xt padding (must be +0)")
    if not ok:
        fails.append(msg)
    return fails


# ------------------------------------------------------------------------------------------------------------------- covariance
def cov_emulate(xt):
    """f32 accumulation in BLAS's order (some order: the bound holds for all of them)."""
    xt = np.asarray(xt, np.float32)
    return xt @ xt.T


def cov_reference(xt):
    x = np.asarray(xt, np.float64)
    return x @ x.T, x.shape[1] * U24 * (np.abs(x) @ np.abs(x).T)


def check_cov(cov, xt, what, exact=False, report=None):
    """cov [H, H] f32 against the float64 product of the xt that prepare returned."""
    xt = np.asarray(xt, np.float32)
    if not np.isfinite(xt).all():
        return [f"{what}: xt is not finite"]
    ref, bound = cov_reference(xt)
    if exact:
        assert xt.shape[1] * 64 * 64 < 2 ** 24
        if not (np.abs(xt).max() <= 64 and np.array_equal(xt, np.round(xt))):
            return [f"{what}: xt is not the matrix of small integers this input centres to"]
        ok, msg = check_exact(np.asarray(cov) + np.float32(0.0), ref.astype(np.float32) + np.float32(0.0), what + " covariance (exact)")
    else:
        ok, msg = check_bound(cov, ref, bound, what + " covariance", report)
    return [] if ok else [msg]


# ------------------------------------------------------------------------------------------------------------------- power step
def chol_rinv(g):
    """Port of pca_chol_rinv (csrc/kernels.h): g [8, 8] (upper triangle read) -> rinv [8, 8] upper triangular with Y rinv orthonormal.  A pivot
    that is not above 1e-24 of the largest diagonal entry is dead: its row of R and its column of rinv are zero."""
    g = np.asarray(g, np.float64).reshape(NB, NB)
    R = np.zeros((NB, NB))
    dead = [False] * NB
    big = 0.0
    for a in range(NB):
        big = g[a, a] if g[a, a] > big else big
    for a in range(NB):
        d = g[a, a]
        for k in range(a):
            d -= R[k, a] * R[k, a]
        dead[a] = not (d > 1e-24 * big)
        if dead[a]:
            continue
        inv = 1.0 / np.sqrt(d)
        R[a, a] = d * inv
        for b in range(a + 1, NB):
            v = g[a, b]
            for k in range(a):
                v -= R[k, a] * R[k, b]
            R[a, b] = v * inv
    rinv = np.zeros((NB, NB))
    for a in range(NB):
        if dead[a]:
            continue
        rinv[a, a] = 1.0 / R[a, a]
        for b in range(a + 1, NB):
            if dead[b]:
                continue
            v = 0.0
            for k in range(a, b):
                v += rinv[a, k] * R[k, b]
            rinv[a, b] = -v / R[b, b]
    return rinv


def gram_sum(parts):
    """The parts added in ascending order, as the kernel and pca_ritz add them."""
    parts = np.asarray(parts, np.float64).reshape(-1, NB * NB)
    s = np.zeros(NB * NB)
    for p in parts:
        s = s + p
    return s.reshape(NB, NB)


def gram_exact(y):
    """Y^T Y with every entry summed in row order (equal columns give equal bits)."""
    g = np.zeros((NB, NB))
    for row in np.asarray(y, np.float64):
        g = g + np.outer(row, row)
    return g


def gram_parts_in_first(g, H):
    """All of G in part 0, as the driver hands the start block over."""
    parts = np.zeros((blocks(H), NB * NB))
    parts[0] = np.asarray(g).ravel()
    return parts


def gram_parts_spread(g, H):
    """Entry t of G in part t % parts: another split with exactly the same sum."""
    nb = blocks(H)
    parts = np.zeros((nb, NB * NB))
    t = np.arange(NB * NB)
    parts[t % nb, t] = np.asarray(g).ravel()
    return parts


def start_block(H):
    """The driver's start block (csrc/pca.cpp): y0[j][c] = sin(0.37 (j + 1) (c + 1)) + (c == j % 8 ? 0.5 : 0)."""
    j, c = np.arange(H)[:, None], np.arange(NB)[None, :]
    return np.sin(0.37 * (j + 1) * (c + 1)) + np.where(c == j % NB, 0.5, 0.0)


def power_emulate(cov, yprev, gparts, mutant=None):
    """(ynext [H, 8], gnext parts [blocks, 64]) in float64."""
    cov, yprev = np.asarray(cov, np.float32).astype(np.float64), np.asarray(yprev, np.float64)
    H = cov.shape[0]
    nb = blocks(H)
    rinv = chol_rinv(gram_sum(gparts))
    if mutant == "rinv_transposed":
        rinv = rinv.T.copy()
    ynext = (cov @ yprev) @ rinv
    ys = np.zeros((nb * ROWS, NB))
    ys[:H] = ynext
    if mutant == "dead_row_reads_last_row":
        ys[H:] = ynext[H - 1]
    parts = np.einsum("kra,krb->kab", ys.reshape(nb, ROWS, NB), ys.reshape(nb, ROWS, NB)).reshape(nb, NB * NB)
    if mutant == "gram_last_group_missing" and H % ROWS:
        parts[-1] = 0.0
    return ynext, parts


def power_reference(cov, yprev, gparts):
    """(reference ynext in long double, per-entry bound) -- the module docstring derives the bound."""
    ld = np.longdouble
    cov64, y = np.asarray(cov, np.float32).astype(np.float64), np.asarray(yprev, np.float64)
    H = cov64.shape[0]
    g = gram_sum(gparts)
    rinv = chol_rinv(g)
    live = np.diag(rinv) != 0
    ref = (cov64.astype(ld) @ (y.astype(ld) @ rinv.astype(ld))).astype(np.float64)
    t_abs, t = np.abs(cov64) @ np.abs(y), cov64 @ y
    op = POWER_SLACK * (H + NB) * U53 * (t_abs @ np.abs(rinv))
    gl = np.triu(g)
    gl = (gl + gl.T - np.diag(np.diag(g)))[np.ix_(live, live)]
    kappa = np.linalg.cond(gl) if live.any() else 1.0
    phi = U53 * (51.0 * kappa ** 1.5 + 8.0 * kappa ** 0.5)
    cond = 2.0 * phi * np.linalg.norm(rinv, 2) * np.linalg.norm(t[:, live], axis=1)[:, None] * live[None, :]
    return ref, op + cond


def check_power(power, cov, yprev, gparts, what, dead=(), report=None):
    """power(cov, yprev, gparts) -> (ynext, gnext parts): failure messages.  `dead`: columns that must come back exactly 0."""
    H = np.asarray(cov).shape[0]
    nb = blocks(H)
    ynext, gnext = power(cov, yprev, gparts)
    ynext, gnext = np.asarray(ynext, np.float64), np.asarray(gnext, np.float64)
    if ynext.shape != (H, NB) or gnext.shape != (nb, NB * NB):
        return [f"{what}: shapes {ynext.shape} {gnext.shape}"]
    if not (np.isfinite(ynext).all() and np.isfinite(gnext).all()):
        return [f"{what}: non-finite output"]
    fails = []
    ref, bound = power_reference(cov, yprev, gparts)
    ok, msg = check_bound(ynext, ref, bound, what + " ynext", report)
    if not ok:
        fails.append(msg)
    for c in dead:
        if not (np.array_equal(ynext[:, c], np.zeros(H)) and np.array_equal(ref[:, c], np.zeros(H))):
            fails.append(f"{what}: dropped column {c} of ynext is not exactly 0")
    # each part = the Gram matrix of its own 16 rows of the ynext that came back; rows >= H contribute exactly 0
    ld = np.longdouble
    ys = np.zeros((nb * ROWS, NB))
    ys[:H] = ynext
    ys = ys.reshape(nb, ROWS, NB)
    own = np.einsum("kra,krb->kab", ys.astype(ld), ys.astype(ld)).astype(np.float64).reshape(nb, NB * NB)
    mag = np.einsum("kra,krb->kab", np.abs(ys), np.abs(ys)).reshape(nb, NB * NB)
    ok, msg = check_bound(gnext, own, POWER_SLACK * ROWS * U53 * mag, what + " gram parts", report)
    if not ok:
        fails.append(msg)
    ok, msg = check_bound(gram_sum(gnext), own.sum(0).reshape(NB, NB), POWER_SLACK * (ROWS + nb) * U53 * mag.sum(0).reshape(NB, NB),
                          what + " gram total", report)
    if not ok:
        fails.append(msg)
    return fails


def check_gram_split(power, cov, yprev, g, what):
    """G all in part 0 (as the driver starts) and spread over all parts: the same sum, so the same ynext and parts, bit for bit."""
    H = np.asarray(cov).shape[0]
    a, b = power(cov, yprev, gram_parts_in_first(g, H)), power(cov, yprev, gram_parts_spread(g, H))
    fails = []
    for x, y, name in zip(a, b, ("ynext", "gram parts")):
        ok, msg = check_exact(np.asarray(x, np.float64), np.asarray(y, np.float64), f"{what} {name}, G in part 0 vs spread")
        if not ok:
            fails.append(msg)
    return fails


def power_case(kind, H):
    """(cov f32 [H, H], yprev [H, 8], G [8, 8], dead columns).  cov is a Gram matrix of Gaussian rows (symmetric, as the real one)."""
    rng = np.random.default_rng(6000 + H + sum(map(ord, kind)))
    x = rng.standard_normal((H, H + 3))
    cov = (x @ x.T).astype(np.float32)
    dead = ()
    if kind == "generic":
        y = rng.standard_normal((H, NB))
    elif kind == "start":
        y = start_block(H)
    elif kind == "rank_deficient":
        # Column 0 is +-1 in exactly 16 rows, so G00 = 16, R00 = 4 and everything column 0 touches is scaled by powers of two: with column 5 a copy
        # of column 0 the pivot of column 5 is exactly 0 with and without fma contraction -- the dead-pivot rule fires on every build.
        y = rng.standard_normal((H, NB))
        y[:, 0] = 0.0
        idx = rng.choice(H, 16, replace=False) if H >= 16 else None
        assert idx is not None, "needs H >= 16"
        y[idx, 0] = rng.choice([-1.0, 1.0], 16)
        y[:, 5] = y[:, 0]
        dead = (5,)
    else:
        raise ValueError(kind)
    return cov, y, gram_exact(y), dead


# ------------------------------------------------------------------------------------------------------------------- projection
def project_emulate(tok, mean, comp, mutant=None):
    tok, mean, comp = (np.asarray(a, np.float32).astype(np.float64) for a in (tok, mean, comp))
    d = tok if mutant == "project_keeps_mean" else tok - mean[None, :]
    proj = (d @ comp.T).astype(np.float32)
    P = tok.shape[0]
    if mutant == "project_skips_tail_row" and P % 4:
        proj[P - 1] = np.nan  # never written: the output starts as NaN
    return proj


def project_case(P, H):
    tok = tokens_generic(P, H, seed=3)
    mean = mean_emulate(tok)
    rng = np.random.default_rng(7000 + 7 * P + H)
    comp = np.linalg.qr(rng.standard_normal((H, 3)))[0].T.astype(np.float32)
    return tok, mean, comp


def check_project(project, tok, mean, comp, what, report=None):
    ld = np.longdouble
    t, m, c = (np.asarray(a, np.float32).astype(ld) for a in (tok, mean, comp))
    d = t - m[None, :]
    ref = (d @ c.T).astype(np.float64)
    H = t.shape[1]
    bound = U24 * np.abs(ref) + H * 2.0 ** -52 * (np.abs(d) @ np.abs(c).T).astype(np.float64)
    ok, msg = check_bound(project(tok, mean, comp), ref, bound, what + " projection", report)
    return [] if ok else [msg]


# ------------------------------------------------------------------------------------------------------------------- every kernel case
def all_failures(ops, report=None):
    """Every kernel case of tests/test_gpu_pca_kernels.py (the H = 256 k covariances left out) through ops = dict(prepare, cov, power, project);
    the failure messages."""
    fails = []
    for P, H in SHAPES:
        sid = shape_id((P, H))
        fails += check_prepare(ops["prepare"], tokens_generic(P, H), f"generic {sid}")
        fails += check_prepare(ops["prepare"], tokens_dyadic(P, H), f"dyadic {sid}", exact_mean=True)
        tok = tokens_generic(P, H)
        fails += check_cov(ops["cov"](tok), ops["prepare"](tok)[1], f"generic {sid}", report=report)
        tok = tokens_integer(P, H)
        fails += check_cov(ops["cov"](tok), ops["prepare"](tok)[1], f"integer {sid}", exact=True)
    for P, H in [(33, 33), (300, 100)]:
        fails += check_prepare(ops["prepare"], tokens_subnormal(P, H), f"subnormal {shape_id((P, H))}")
        fails += check_prepare(ops["prepare"], tokens_large(P, H), f"large {shape_id((P, H))}")
    for H in H_VALUES:
        for kind in ("generic", "start", "rank_deficient"):
            cov, y, g, dead = power_case(kind, H + 16 if kind == "rank_deficient" and H < 16 else H)
            H_ = cov.shape[0]
            fails += check_power(ops["power"], cov, y, gram_parts_in_first(g, H_), f"{kind} H={H_}", dead, report)
        cov, y, g, _ = power_case("generic", H)
        fails += check_gram_split(ops["power"], cov, y, g, f"generic H={H}")
    for P, H in PROJECT_SHAPES:
        fails += check_project(ops["project"], *project_case(P, H), f"{shape_id((P, H))}", report)
    return fails


def emulated_ops(mutant=None):
    def cov(tok):
        return cov_emulate(prepare_emulate(tok, mutant)[1])
    return {"prepare": lambda tok: prepare_emulate(tok, mutant), "cov": cov,
            "power": lambda c, y, g: power_emulate(c, y, g, mutant), "project": lambda t, m, c: project_emulate(t, m, c, mutant)}


# ------------------------------------------------------------------------------------------------------------------- the whole call
def ritz(yprev, ynext, g, vectors=True):
    """The Rayleigh-Ritz step of csrc/pca.cpp pca_ritz in numpy (eigh in place of its Jacobi sweeps): (3 largest Ritz values, comp [3, H])."""
    rinv = chol_rinv(g)
    q = yprev @ rinv
    b = q.T @ ynext
    b = 0.5 * (b + b.T)
    w, v = np.linalg.eigh(b)
    order = np.argsort(-w, kind="stable")[:3]
    if not vectors:
        return w[order], None
    comp = (q @ v[:, order]).T
    for c in comp:
        n = np.sqrt((c * c).sum())
        c *= (0.0 if n == 0 else (-1.0 if c[np.abs(c).argmax()] < 0 else 1.0) / n)
    return w[order], comp


def pca3_emulate(x):
    """dinov2_hip_pca3 in numpy: the kernel's mean, f16-rounded centred tokens, f32-rounded covariance (accumulated in float64), the driver's
    start block, CholeskyQR power steps in double, its check cadence (8 steps four times, then 16) and stopping rule, projection in double
    rounded to f32.  Returns (comp [3, H] f32, mean [H] f32, proj [P, 3] f32, steps)."""
    x = np.asarray(x, np.float32)
    P, H = x.shape
    mean, xt = prepare_emulate(x)
    cov = cov_reference(xt)[0].astype(np.float32).astype(np.float64)
    y, g = start_block(H), None
    g = gram_exact(y)
    prev, steps = np.zeros(3), 0
    with np.errstate(all="ignore"):
        for chk in range(28):
            check = 8 if chk < 4 else 16
            for _ in range(check):
                yp, gp = y, g
                y = (cov @ yp) @ chol_rinv(gp)
                g = y.T @ y
            steps += check
            ev, _ = ritz(yp, y, gp, vectors=False)
            done = chk > 0 and bool(np.all(np.abs(ev - prev) <= 1e-8 * abs(ev[0])))
            prev = ev
            if done or not ev[0] > 0.0:
                break
    comp = ritz(yp, y, gp)[1].astype(np.float32)
    return comp, mean, project_emulate(x, mean, comp), steps


def _structured(P, H, strengths, noise, seed, offset=4.0, ortho=False):
    rng = np.random.default_rng(seed)
    k = len(strengths)
    basis = np.linalg.qr(rng.standard_normal((H, k)))[0].T
    coef = rng.standard_normal((P, k))
    if ortho:  # exactly orthogonal, centred, equal-length coefficient columns: equal strengths are an exact tie in the signal
        coef = np.linalg.qr(coef - coef.mean(0))[0] * np.sqrt(P)
    return (coef * np.asarray(strengths)) @ basis + noise * rng.standard_normal((P, H)) + offset


def _e2e_structured():
    return _structured(256, 384, (9.0, 5.0, 2.5), 0.3, 256 * 7 + 384)


# name -> (builder of the float64 tokens, tied pair or None).  The structured input is the one test_pca3_matches_svd has always used.
E2E_INPUTS = {
    "structured_256x384": (_e2e_structured, None),
    "scaled_1e-4_256x384": (lambda: 1e-4 * _e2e_structured(), None),
    "scaled_1e3_256x384": (lambda: 1e3 * _e2e_structured(), None),
    "flat_256x384": (lambda: np.random.default_rng(11).standard_normal((256, 384)), None),
    "flat_300x40": (lambda: np.random.default_rng(12).standard_normal((300, 40)), None),
    "tie12_300x128": (lambda: _structured(300, 128, (6.0, 6.0, 3.0), 0.02, 13, ortho=True), (0, 1)),
    "neartie34_300x128": (lambda: _structured(300, 128, (9.0, 5.0, 2.5, 2.4), 0.05, 14, ortho=True), None),
    "eleven_700x100": (lambda: _structured(700, 100, 9.0 * 0.9 ** np.arange(11), 0.1, 15), None),
    "mean1000_300x128": (lambda: _structured(300, 128, (3.0, 2.0, 1.5), 0.3, 16, offset=1000.0), None),
    "minimal_4x8": (lambda: np.random.default_rng(17).standard_normal((4, 8)), None),
    "minimal_4x64": (lambda: np.random.default_rng(18).standard_normal((4, 64)), None),
    "minimal_5x200": (lambda: np.random.default_rng(19).standard_normal((5, 200)), None),
}
_E2E_CACHE = {}


def e2e_errors(x, comp, proj, tied=None):
    """(max over the components of 1 - |cos| against the float64 SVD of the centred f32 tokens -- for a tied pair 1 - the smallest singular
    value of comp[pair] ref[pair]^T --, projection error relative to the largest projection).  Projections are compared through the row
    norms over the components (and over a tied pair), which do not depend on signs or on the basis chosen inside a tie."""
    x = np.asarray(x, np.float32).astype(np.float64)
    xc = x - x.mean(0)
    ref = np.linalg.svd(xc, full_matrices=False)[2][:3]
    c = np.asarray(comp, np.float64)
    groups = [[0], [1], [2]] if tied is None else [list(tied)] + [[k] for k in range(3) if k not in tied]
    cos_err, proj_err = 0.0, 0.0
    want = xc @ ref.T
    for g in groups:
        s = np.linalg.svd(c[g] @ ref[g].T, compute_uv=False)
        cos_err = max(cos_err, 1.0 - float(s.min()))
        a, b = np.linalg.norm(np.asarray(proj, np.float64)[:, g], axis=1), np.linalg.norm(want[:, g], axis=1)
        proj_err = max(proj_err, float(np.abs(a - b).max()))
    return cos_err, proj_err / float(np.abs(want).max())


def e2e_case(name):
    """(tokens f32, tied pair, emulation's (cos error, projection error), emulation's steps); computed once and shared (never modified)."""
    if name not in _E2E_CACHE:
        build, tied = E2E_INPUTS[name]
        x = build().astype(np.float32)
        comp, _, proj, steps = pca3_emulate(x)
        _E2E_CACHE[name] = (x, tied, e2e_errors(x, comp, proj, tied), steps)
    return _E2E_CACHE[name]


def e2e_tolerance(emulated):
    return max(E2E_MARGIN * emulated, E2E_FLOOR)


def e2e_failures(x, comp, mean, proj, tied=None, emulated=None, what=""):
    """The acceptance rule of tests/test_gpu_parity.py::test_pca3_within_16x_of_its_emulation for one result of the whole call on tokens x:
    the kernel's mean bit for bit, unit components with a positive largest entry, the projection inside the projection kernel's bound on the
    returned components, and both errors against the float64 SVD within e2e_tolerance of what the emulation shows on the same input
    (`emulated` = its (cos error, projection error); computed here when absent).  Returns (failure messages, the figures as a string)."""
    x = np.asarray(x, np.float32)
    if emulated is None:
        ecomp, _, eproj, _ = pca3_emulate(x)
        emulated = e2e_errors(x, ecomp, eproj, tied)
    emu_cos, emu_proj = emulated
    fails = []
    if not (np.isfinite(comp).all() and np.isfinite(proj).all()):
        return [what + ": non-finite result"], ""
    cos_err, proj_err = e2e_errors(x, comp, proj, tied)
    figures = (f"{what}: 1 - |cos| {cos_err:.2e} (emulation {emu_cos:.2e}, allowed {e2e_tolerance(emu_cos):.2e}); projection {proj_err:.2e} "
               f"(emulation {emu_proj:.2e}, allowed {e2e_tolerance(emu_proj):.2e})")
    ok, msg = check_exact(mean, mean_emulate(x), what + " mean")
    if not ok:
        fails.append(msg)
    if np.abs(np.linalg.norm(np.asarray(comp, np.float64), axis=1) - 1.0).max() > 2.0 ** -23:  # unit in double, each entry rounded once to f32
        fails.append(what + ": components are not unit length")
    if not all(comp[k][np.abs(comp[k]).argmax()] > 0 for k in range(3)):
        fails.append(what + ": a component's largest entry is not positive")
    fails += check_project(lambda *_: proj, x, mean, comp, what)
    if cos_err > e2e_tolerance(emu_cos):
        fails.append(f"{what}: 1 - |cos| {cos_err:.3e} > {e2e_tolerance(emu_cos):.3e}")
    if proj_err > e2e_tolerance(emu_proj):
        fails.append(f"{what}: projection error {proj_err:.3e} > {e2e_tolerance(emu_proj):.3e}")
    return fails, figures
