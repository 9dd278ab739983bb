"""Cases, the numpy restatement and the bounds of dinov2_hip_ncut (include/dinov2_hip.h; csrc/ncut.hip, csrc/ncut.cpp), shared by the CPU
probes (tests/test_ncut_probes.py) and the GPU tests (tests/test_gpu_ncut.py).

An implementation is anything with the three methods of `Emulated`:
    apply(rows, affinity, tau, floor, scale, q, nchunk)            -> dict(t [n, 8] f64, degree [n] f64, xhat [n, H] f32)
    step(rows, affinity, tau, floor, yprev, gprev_parts, nchunk)   -> dict(ynext [n, 8], gnext_parts, ritz_parts [row tiles, 64])
    run(rows, n_eig, affinity, tau, floor, max_iter, tol)          -> dict(values, vectors, degree, residual, iterations, converged)
`Emulated` restates the contract in numpy with the kernels' padding and chunking made explicit; `Emulated(mutant)` plants one of MUTANTS.
Every check returns a list of failure texts (empty: passed); CASES names them, MUTANT_CASE says which case rejects which mutant.

The references never come from an implementation under test: the exact probes are dyadic, so plain float64 on the un-padded rows gives
every sum exactly; the Gaussian shapes, the step and the driver are held to float64 formulas on the f16 rows the implementation itself
returns (`xhat`, itself held to match_cases.normalise_f16 within 2^-10), under bounds derived below from the number formats.
"""
import numpy as np

import match_cases as mc

TILE, NB = 128, 8
TARGET_WGS, PARTIAL_MAX = 256, 32 << 20
SHAPES = [(16, 8), (127, 8), (128, 64), (129, 72), (257, 384), (300, 1536), (1369, 1024)]
AFFINITIES = ("threshold", "relu", "exp")
EXP_TAU = 0.25      # the EXP cases' temperature
PROBE_FLOOR = 2.0 ** -10
PROBES = ["pm1_threshold", "pm1_relu", "at_tau", "zero_row", "negated"]
MUTANTS = ["pad_cols_counted", "pad_rows_in_gram", "last_chunk_dropped", "chunk_local_column_index", "threshold_ge", "relu_abs", "scale_one_side",
           "shift_missing", "zero_degree_nan", "diag_zeroed", "values_descending", "sign_not_fixed"]
GAP_MIN = 0.1       # reference eigenvalues closer together than this form one group; every group's gap to the rest is asserted >= this
F32_EPS, F64_SLACK = 2.0 ** -24, 2.0 ** -40


def shape_id(s):
    return "x".join(str(v) for v in s)


# --------------------------------------------------------------------------------------------------------------------- planner
def plan(n, H, nchunk=0):
    """ncut_plan (csrc/kernels.h), restated."""
    npad, hpad = (n + TILE - 1) // TILE * TILE, (H + 63) // 64 * 64
    ntiles = npad // TILE
    per_chunk = npad * NB * 8
    if nchunk <= 0:
        nchunk = (TARGET_WGS + ntiles - 1) // ntiles
    nchunk = min(nchunk, PARTIAL_MAX // per_chunk, ntiles)
    chunk_tiles = (ntiles + nchunk - 1) // nchunk
    nchunks = (ntiles + chunk_tiles - 1) // chunk_tiles
    return {"npad": npad, "hpad": hpad, "ntiles": ntiles, "chunk_tiles": chunk_tiles, "nchunks": nchunks, "part_bytes": per_chunk * nchunks}


def chunk_ranges(p):
    """[(first column tile, one past the last)] of every chunk."""
    return [(c * p["chunk_tiles"], min((c + 1) * p["chunk_tiles"], p["ntiles"])) for c in range(p["nchunks"])]


def chunkings(n, H):
    """The chunk requests of the exact probes: 1, 2, the planner's own (0) and as many as there are column tiles."""
    return [1, 2, 0, plan(n, H)["ntiles"]]


def check_interval(steps_done):
    return 8 if steps_done < 32 else 16


# --------------------------------------------------------------------------------------------------------------------- contract pieces
def weights32(S32, affinity, tau, floor, mutant=None):
    """Contract 3 in f32 on an f32 similarity matrix."""
    s = np.asarray(S32, np.float32) + np.float32(0.0)
    tau, floor = np.float32(tau), np.float32(floor)
    if affinity == "threshold":
        hit = s >= tau if mutant == "threshold_ge" else s > tau
        return np.where(hit, np.float32(1.0), floor).astype(np.float32)
    if affinity == "relu":
        return (np.abs(s) if mutant == "relu_abs" else np.maximum(s, np.float32(0.0))).astype(np.float32)
    return np.exp(((s - np.float32(1.0)) / tau).astype(np.float32)).astype(np.float32)


def weights64(S, affinity, tau, floor):
    """The same map in float64 on a float64 similarity: the references' affinity (tau and floor are the f32 values the device holds)."""
    tau, floor = float(np.float32(tau)), float(np.float32(floor))
    if affinity == "threshold":
        return np.where(S > tau, 1.0, floor)
    if affinity == "relu":
        return np.maximum(S, 0.0)
    return np.exp((S - 1.0) / tau)


def delta_w(Wref, H, affinity, tau):
    """|w_device - w_reference| per pair, given |s_device - s_reference| <= H 2^-24 (f32 accumulation of a product of unit rows):
    RELU is 1-Lipschitz; THRESHOLD is exact where no pair lies within H 2^-24 of tau (the cases assert it); EXP is relative: the argument
    (s - 1) / tau is off by at most (H 2^-24 + 2^-23 + 2^-23) / tau -- the similarity, the rounded difference (|s - 1| <= 2), the
    correctly rounded quotient (|arg| <= 2 / tau) --, exp turns that into a relative error of expm1 of it, and expf (the device library's,
    documented at 1 ulp) with the rounding of its f32 result adds 2^-22."""
    if affinity == "threshold":
        return np.zeros_like(Wref)
    if affinity == "relu":
        return np.full_like(Wref, H * F32_EPS)
    return Wref * (np.expm1((H * F32_EPS + 2.0 ** -22) / float(np.float32(tau))) + 2.0 ** -22)


def chol_rinv(G):
    """pca_chol_rinv for a full-rank Gram matrix: upper triangular R^-1 with G = R^T R."""
    return np.linalg.inv(np.linalg.cholesky(G).T)


def start_block(deg):
    """Contract 5's start block [n, 8]."""
    n = len(deg)
    i = np.arange(n)[:, None]
    c = np.arange(NB)[None, :]
    y = np.sin(0.37 * (i + 1) * (c + 1)) + np.where(c == i % NB, 0.5, 0.0)
    y[:, 0] = np.sqrt(np.maximum(deg, 0.0))
    y[~(deg > 0)] = 0.0
    return y


def gram_parts(Y, ntiles=None):
    """Per-128-row partials [row tiles, 64] of Y^T Y."""
    n = len(Y)
    nt = (n + TILE - 1) // TILE if ntiles is None else ntiles
    g = np.zeros((nt, 64))
    for t in range((n + TILE - 1) // TILE):
        blk = Y[t * TILE:(t + 1) * TILE]
        g[t] = (blk.T @ blk).ravel()
    return g


def fix_vectors(U, cs, mutant=None):
    """Contract 6: z_k = C u_k to unit length, the entry of largest magnitude positive (the lowest index at a tie).  U [n, m] -> [m, n]."""
    Z = (cs[:, None] * U).T.copy()
    for z in Z:
        nrm = np.sqrt((z * z).sum())
        big = int(np.argmax(np.abs(z)))  # the first maximum
        sgn = -1.0 if z[big] < 0 else 1.0
        if mutant == "sign_not_fixed":
            sgn = 1.0  # whatever sign the iteration left
        z *= (sgn / nrm) if nrm > 0 else 0.0
    return Z


# --------------------------------------------------------------------------------------------------------------------- restatement
class Emulated:
    """numpy restatement of the contract with the device's layout explicit: rows padded to whole tiles with zero rows, the columns walked
    in the planner's chunks of column tiles, padding columns weighing 0 and padding rows kept out of every sum."""

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mutant = mutant

    def _w(self, rows, affinity, tau, floor, p):
        xh = mc.normalise_f16(rows)
        n = len(xh)
        xp = np.zeros((p["npad"], xh.shape[1]), np.float64)
        xp[:n] = xh.astype(np.float64)
        W = weights32((xp @ xp.T).astype(np.float32), affinity, tau, floor, self.mutant).astype(np.float64)
        if self.mutant != "pad_cols_counted":
            W[:, n:] = 0.0
        if self.mutant == "diag_zeroed":
            W[np.arange(n), np.arange(n)] = 0.0
        return xh, W

    def _sums(self, W, v, p):
        """sum_j W_ij v_j over the chunks in ascending order; v [npad, m]."""
        t = np.zeros((W.shape[0], v.shape[1]))
        ranges = chunk_ranges(p)
        for k, (t0, t1) in enumerate(ranges):
            if self.mutant == "last_chunk_dropped" and len(ranges) > 1 and k == len(ranges) - 1:
                continue
            c0, c1 = t0 * TILE, t1 * TILE
            vv = v[0:c1 - c0] if self.mutant == "chunk_local_column_index" else v[c0:c1]
            t += W[:, c0:c1] @ vv
        return t

    def _degree(self, W, n, p):
        ones = np.zeros((p["npad"], 1))
        ones[:n if self.mutant != "pad_cols_counted" else p["npad"]] = 1.0
        d = self._sums(W, ones, p)[:, 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            cs = 1.0 / np.sqrt(d) if self.mutant == "zero_degree_nan" else np.where(d > 0, 1.0 / np.sqrt(np.where(d > 0, d, 1.0)), 0.0)
        if self.mutant != "pad_rows_in_gram":
            d[n:], cs[n:] = 0.0, 0.0
        return d, cs

    def apply(self, rows, affinity, tau, floor, scale, q, nchunk=0):
        n, H = rows.shape
        p = plan(n, H, nchunk)
        xh, W = self._w(rows, affinity, tau, floor, p)
        out = {"xhat": xh.astype(np.float32), "degree": self._degree(W, n, p)[0][:n]}
        if q is not None:
            v = np.zeros((p["npad"], NB))
            v[:n] = np.asarray(q, np.float64) * (1.0 if scale is None else np.asarray(scale, np.float64)[:, None])
            out["t"] = self._sums(W, v, p)[:n]
        return out

    def _step(self, W, cs, n, p, yprev_pad, G):
        rinv = chol_rinv(G)
        inner = yprev_pad if self.mutant == "scale_one_side" else cs[:, None] * yprev_pad
        with np.errstate(invalid="ignore"):
            t = self._sums(W, inner, p)
            z = cs[:, None] * t if self.mutant == "shift_missing" else 0.5 * (yprev_pad + cs[:, None] * t)
        if self.mutant == "pad_rows_in_gram":  # the padding rows' own sums: a zero row against every real column, f(0) each
            xtra = 0.5 * cs[n:, None] * t[n:]
            z = np.concatenate([z[:n], xtra])
        else:
            z[n:] = 0.0
        ynext = z @ rinv
        qm = yprev_pad @ rinv
        qm[n:] = 0.0
        nt = p["ntiles"]
        gn = np.stack([(ynext[k * TILE:(k + 1) * TILE].T @ ynext[k * TILE:(k + 1) * TILE]).ravel() for k in range(nt)])
        rz = np.stack([(qm[k * TILE:(k + 1) * TILE].T @ ynext[k * TILE:(k + 1) * TILE]).ravel() for k in range(nt)])
        return ynext, gn, rz

    def step(self, rows, affinity, tau, floor, yprev, gprev_parts, nchunk=0):
        n, H = rows.shape
        p = plan(n, H, nchunk)
        _, W = self._w(rows, affinity, tau, floor, p)
        _, cs = self._degree(W, n, p)
        yp = np.zeros((p["npad"], NB))
        yp[:n] = yprev
        ynext, gn, rz = self._step(W, cs, n, p, yp, np.asarray(gprev_parts).reshape(-1, 64).sum(0).reshape(NB, NB))
        return {"ynext": ynext[:n], "gnext_parts": gn, "ritz_parts": rz}

    def run(self, rows, n_eig, affinity, tau, floor, max_iter, tol):
        n, H = rows.shape
        p = plan(n, H, 0)
        _, W = self._w(rows, affinity, tau, floor, p)
        d, cs = self._degree(W, n, p)
        y = np.zeros((p["npad"], NB))
        y[:n] = start_block(d[:n])
        G = y.T @ y
        steps, conv = 0, False
        while steps < max_iter:
            for _ in range(check_interval(steps)):
                y, gn, rz = self._step(W, cs, n, p, y, G)
                G = gn.sum(0).reshape(NB, NB)
                steps += 1
            B = rz.sum(0).reshape(NB, NB)
            theta, V = np.linalg.eigh(0.5 * (B + B.T))
            theta, V = theta[::-1], V[:, ::-1]
            r2 = np.einsum("ak,ab,bk->k", V, G, V) - theta ** 2
            resid = np.sqrt(np.maximum(r2, 0.0))
            if (resid[:n_eig] <= np.float32(tol)).all():
                conv = True
                break
        values = 2.0 * (1.0 - theta[:n_eig])
        if self.mutant == "values_descending":
            values = values[::-1]
        vec = fix_vectors(y[:n] @ V[:, :n_eig], cs[:n], self.mutant)
        return {"values": values.astype(np.float32), "vectors": vec.astype(np.float32), "degree": d[:n].astype(np.float32),
                "residual": resid[:n_eig].astype(np.float32), "iterations": steps, "converged": conv}


# --------------------------------------------------------------------------------------------------------------------- exact probes
def _ints(rng, n):
    return rng.integers(-2, 3, (n, NB)).astype(np.float64)


def build_probe(kind, seed=7):
    """(rows, affinity, tau, floor, q) of an exact probe.  Rows are match_cases._pm1_rows (entries +-2^-k after the normalisation), so every
    similarity, every weight (floor = 2^-10, or the similarity itself) and, with integer q in [-2, 2], every sum is a short dyadic number:
    float64 gives t and the degrees exactly in ANY order.  n = 2 * 128 + 5: three column tiles, the last partial."""
    rng = np.random.default_rng(seed)
    n, H = 2 * TILE + 5, 72
    x = mc._pm1_rows(rng, n, H)
    affinity, tau = "threshold", 0.2
    if kind == "pm1_threshold":
        pass
    elif kind == "pm1_relu":
        affinity = "relu"
    elif kind == "at_tau":
        # pairs exactly AT tau = 0.25: rows of four +-1 that share one position with one sign, on either side of a tile boundary
        tau = 0.25
        for i, j in ((3, 9), (TILE - 1, TILE + 1), (5, n - 1)):
            x[i], x[j] = 0.0, 0.0
            x[i, [0, 1, 2, 3]] = 1.0
            x[j, [0, 4, 5, 6]] = 1.0
        S = mc.reference(x, x)
        assert (S == 0.25).sum() >= 6
    elif kind == "zero_row":
        affinity = "relu"
        x[3], x[TILE + 2], x[n - 1] = 0.0, 0.0, 0.0
    elif kind == "negated":
        # A diagonal similarity is 1, so no probe has ALL similarities negative; the nearest thing: rows that all share position 0, the
        # second half negated, so every pair ACROSS the halves is negative, and tau < 0: a zero padding column (s = 0 > tau) then weighs 1,
        # more than any of those pairs (floor) -- a counted padding column wins visibly.
        tau = -2.0 ** -7  # (two rows of 64 entries that share position 0 alone: 1 / 64)
        x = mc._pm1_rows(rng, n, H, positive=True)
        x[n // 2:] *= -1.0
        S = mc.reference(x, x)
        assert S[:n // 2, n // 2:].max() < tau
    else:
        raise ValueError(kind)
    return x, affinity, tau, PROBE_FLOOR, _ints(rng, n)


def exact_apply(rows, affinity, tau, floor, q):
    """t and the degrees of an exact probe by plain float64 on the un-padded rows (no chunks, no padding: nothing shared with Emulated)."""
    S = mc.reference(rows, rows)
    S32 = S.astype(np.float32)
    assert np.array_equal(S32.astype(np.float64), S), "probe similarities are not exact in f32"
    W = weights32(S32, affinity, tau, floor).astype(np.float64)
    return W @ q, W.sum(1)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def check_probe(impl, kind, nchunk):
    rows, affinity, tau, floor, q = build_probe(kind)
    t, d = exact_apply(rows, affinity, tau, floor, q)
    res = impl.apply(rows, affinity, tau, floor, None, q, nchunk)
    bad = []
    for name, got, want in (("t", res["t"], t), ("degree", res["degree"], d)):
        got = np.asarray(got, np.float64)
        if got.shape != want.shape or not np.array_equal(bits(got + 0.0), bits(want + 0.0)):
            k = int(np.flatnonzero((got != want).ravel())[0]) if got.shape == want.shape and (got != want).any() else -1
            bad.append(f"probe {kind} nchunk {nchunk}: {name} differs from the exact value (first at flat index {k})")
    return bad


# --------------------------------------------------------------------------------------------------------------------- Gaussian shapes
def shape_rows(shape):
    n, H = shape
    return mc.gaussian_tokens(n, H, 300 + n + H, outliers=False)


def sim64(xhat):
    x = np.asarray(xhat, np.float64)
    return x @ x.T


def threshold_tau(S, H):
    """tau in the middle of the widest gap of the similarities in [0.1, 0.3] (the window's ends count as values), so that THRESHOLD is
    exact: asserts that no pair lies within 2 H 2^-24 of it."""
    v = np.unique(S[(S >= 0.1) & (S <= 0.3)])
    v = np.concatenate([[0.1], v, [0.3]])
    k = int(np.argmax(np.diff(v)))
    tau = float(np.float32(0.5 * (v[k] + v[k + 1])))
    assert np.abs(S - tau).min() > 2 * H * F32_EPS, "no gap wide enough for an exact THRESHOLD"
    return tau


def shape_case(shape, affinity):
    """(rows, tau, floor, scale, q) of a Gaussian shape."""
    n, H = shape
    rows = shape_rows(shape)
    rng = np.random.default_rng(n * 7 + H)
    tau = {"threshold": lambda: threshold_tau(sim64(mc.normalise_f16(rows)), H), "relu": lambda: 0.0, "exp": lambda: EXP_TAU}[affinity]()
    return rows, tau, 1e-5, rng.uniform(0.5, 1.5, n), rng.standard_normal((n, NB))


def check_xhat(xhat, rows, what):
    want = mc.normalise_f16(rows).astype(np.float32)
    if xhat.shape != want.shape or not np.isfinite(xhat).all() or np.abs(xhat - want).max() > 2.0 ** -10:
        return [f"{what}: xhat is not normalise_f16(rows) within 2^-10"]
    return []


def check_shape(impl, shape, affinity, report=None):
    """apply against the float64 sums over the implementation's own f16 rows.  Per element |t - t_ref| <= sum_j |dw_ij| |scale_j q_jc|
    (delta_w), plus 2^-40 sum_j w_ij |scale_j q_jc| for the f64 accumulation of at most 2^17 terms in an unspecified order."""
    n, H = shape
    rows, tau, floor, scale, q = shape_case(shape, affinity)
    what = f"shape {shape_id(shape)} {affinity}"
    res = impl.apply(rows, affinity, tau, floor, scale, q, 0)
    bad = check_xhat(res["xhat"], rows, what)
    if bad:
        return bad
    S = sim64(res["xhat"])
    if affinity == "threshold" and not np.abs(S - float(np.float32(tau))).min() > H * F32_EPS:
        return [f"{what}: a pair of the returned rows lies within H 2^-24 of tau"]
    W = weights64(S, affinity, tau, floor)
    dW = delta_w(W, H, affinity, tau)
    v = np.abs(scale[:, None] * q)
    for name, got, want, bound in (("t", res["t"], W @ (scale[:, None] * q), dW @ v + F64_SLACK * (W @ v)),
                                   ("degree", res["degree"][:, None], W.sum(1)[:, None], dW.sum(1)[:, None] + F64_SLACK * W.sum(1)[:, None])):
        err = np.abs(np.asarray(got, np.float64) - want)
        worst = float((err / np.maximum(bound, 1e-300)).max()) if np.isfinite(err).all() else np.inf
        if report is not None:
            report(f"{what}: {name} max error {np.nanmax(err):.3e}, worst error / bound {worst:.3f}")
        if not worst <= 1.0:
            bad.append(f"{what}: {name} misses its bound (error / bound = {worst:.3f})")
    return bad


# --------------------------------------------------------------------------------------------------------------------- the step
STEP_CASES = {"step_129x72_exp": ((129, 72), "exp"), "step_257x384_relu": ((257, 384), "relu"), "step_300x1536_threshold": ((300, 1536), "threshold"),
              "step_zero_row": (None, "relu")}


def step_inputs(name):
    shape, affinity = STEP_CASES[name]
    if shape is None:
        rows, affinity, tau, floor, _ = build_probe("zero_row")
    else:
        rows, tau, floor, _, _ = shape_case(shape, affinity)
    n = len(rows)
    yprev = np.random.default_rng(n + 11).standard_normal((n, NB))
    yprev[:, 0] = np.abs(yprev[:, 0]) + 0.5
    return rows, affinity, tau, floor, yprev, gram_parts(yprev)


def check_step(impl, name, report=None):
    """One step against the float64 formula on the implementation's own f16 rows.  With e_d = sum_j dw_ij the degree's error, c = d^-1/2 is off
    by dc_i <= c_i e_d_i / (2 d_i) (1 + e_d_i / d_i) (first order plus its own square); t = W (c y) by
    dt <= dW (c |y|) + W (dc |y|) + dW (dc |y|); Z = (y + c t) / 2 by dZ <= (c dt + dc |t| + dc dt) / 2; Y_next = Z R^-1 row by row, so
    dY <= dZ |R^-1| with R^-1 from the reference (the Gram matrix is the same float64 sum on both sides).  The 8 x 8 partials are sums of
    products of rows of Y_next (and of Q = Y_prev R^-1, exact): dG <= |Y|^T dY + dY^T |Y| + dY^T dY, dB <= |Q|^T dY.  Everything f64 gets a
    relative 2^-40 on top."""
    rows, affinity, tau, floor, yprev, gparts = step_inputs(name)
    n, H = rows.shape
    res = impl.step(rows, affinity, tau, floor, yprev, gparts, 0)
    xh = impl.apply(rows, affinity, tau, floor, None, None, 0)["xhat"]  # (the same normaliser launch as the step's)
    bad = check_xhat(xh, rows, name)
    if bad:
        return bad
    S = sim64(xh)
    if affinity == "threshold" and not np.abs(S - float(np.float32(tau))).min() > H * F32_EPS:
        return [f"{name}: a pair of the returned rows lies within H 2^-24 of tau"]
    W = weights64(S, affinity, tau, floor)
    dW = delta_w(W, H, affinity, tau)
    d = W.sum(1)
    pos = d > 0
    cs = np.where(pos, 1.0 / np.sqrt(np.where(pos, d, 1.0)), 0.0)
    ed = dW.sum(1)
    rel = np.where(pos, ed / np.where(pos, d, 1.0), 0.0)
    dc = 0.5 * cs * rel * (1.0 + rel)
    ay = np.abs(yprev)
    t = W @ (cs[:, None] * yprev)
    dt = dW @ (cs[:, None] * ay) + W @ (dc[:, None] * ay) + dW @ (dc[:, None] * ay)
    Z = 0.5 * (yprev + cs[:, None] * t)
    dZ = 0.5 * (cs[:, None] * dt + dc[:, None] * np.abs(t) + dc[:, None] * dt)
    rinv = chol_rinv(gparts.sum(0).reshape(NB, NB))
    Y = Z @ rinv
    dY = dZ @ np.abs(rinv) + F64_SLACK * (np.abs(Z) @ np.abs(rinv))
    Q = yprev @ rinv
    aY, aQ = np.abs(Y), np.abs(Q)
    dG = aY.T @ dY + dY.T @ aY + dY.T @ dY + F64_SLACK * (aY.T @ aY)
    dB = aQ.T @ dY + F64_SLACK * (aQ.T @ aY)
    what = f"{name}"
    nt = (n + TILE - 1) // TILE
    if np.asarray(res["gnext_parts"]).shape != (nt, 64) or np.asarray(res["ritz_parts"]).shape != (nt, 64):
        return [f"{what}: the partials are not [row tiles, 64]"]
    for nm, got, want, bound in (("ynext", res["ynext"], Y, dY), ("gnext", res["gnext_parts"].sum(0).reshape(NB, NB), Y.T @ Y, dG),
                                 ("ritz", res["ritz_parts"].sum(0).reshape(NB, NB), Q.T @ Y, dB)):
        err = np.abs(np.asarray(got, np.float64) - want)
        worst = float((err / np.maximum(bound, 1e-300)).max()) if np.isfinite(err).all() else np.inf
        if report is not None:
            report(f"{what}: {nm} max error {np.nanmax(err):.3e}, worst error / bound {worst:.3f}")
        if not worst <= 1.0:
            bad.append(f"{what}: {nm} misses its bound (error / bound = {worst:.3f})")
    # the partials themselves: every workgroup's own rows (against the returned ynext, exactly representable inputs aside: 1e-9 relative)
    yn = np.asarray(res["ynext"], np.float64)
    if np.isfinite(yn).all() and not np.allclose(res["gnext_parts"], gram_parts(yn, nt), rtol=1e-9, atol=1e-9 * max(1.0, np.abs(yn).max() ** 2)):
        bad.append(f"{what}: a Gram partial is not its own 128 rows' (rows >= n must contribute nothing)")
    return bad


# --------------------------------------------------------------------------------------------------------------------- the driver
DRIVER_CASES = {"planted3": (300, 64, (150, 100, 50)), "planted2": (129, 72, (86, 43))}
DRIVER_TOL, DRIVER_MAX_ITER = 1e-5, 400


def planted(name):
    """(rows, labels): clusters of unequal sizes round k orthogonal directions plus Gaussian noise of norm about 0.5, rows shuffled."""
    n, H, sizes = DRIVER_CASES[name]
    rng = np.random.default_rng(n + H)
    labels = np.repeat(np.arange(len(sizes)), sizes)
    rng.shuffle(labels)
    dirs = np.linalg.qr(rng.standard_normal((H, len(sizes))))[0].T
    rows = dirs[labels] + 0.5 * rng.standard_normal((n, H)) / np.sqrt(H)
    return rows.astype(np.float32), labels


def driver_params(affinity):
    return {"threshold": (0.2, 1e-5), "relu": (0.0, 0.0), "exp": (EXP_TAU, 0.0)}[affinity]


def driver_reference(xhat, H, affinity, tau, floor, n_eig):
    """eigh of the float64 A from the f16 rows: theta descending, U, d, the perturbation bound ||dA||_inf of the device's operator (the
    largest row sum of |dA_ij| <= (c_i c_j dw_ij + w_ij (dc_i c_j + c_i dc_j + dc_i dc_j)) / 2, dc as in check_step), and the degrees' error
    bound, and the groups [(first, one past last, gap)] of the leading n_eig eigenvalues."""
    W = weights64(sim64(xhat), affinity, tau, floor)
    dW = delta_w(W, H, affinity, tau)
    d = W.sum(1)
    assert (d > 0).all()
    cs = 1.0 / np.sqrt(d)
    rel = dW.sum(1) / d
    dc = 0.5 * cs * rel * (1.0 + rel)
    A = 0.5 * (np.eye(len(d)) + cs[:, None] * W * cs[None, :])
    dA = 0.5 * (cs[:, None] * dW * cs[None, :] + W * (dc[:, None] * cs[None, :] + cs[:, None] * dc[None, :] + dc[:, None] * dc[None, :]))
    pert = float(dA.sum(1).max()) + F64_SLACK
    theta, U = np.linalg.eigh(A)
    theta, U = theta[::-1], U[:, ::-1]
    groups, a = [], 0
    for k in range(1, n_eig + 1):
        if k == n_eig or theta[k - 1] - theta[k] >= GAP_MIN:
            gap = min(theta[a - 1] - theta[a] if a > 0 else np.inf, theta[k - 1] - theta[k])
            groups.append((a, k, float(gap)))
            a = k
    return theta, U, d, dW.sum(1), pert, groups


def check_driver(impl, name, affinity, report=None):
    """The driver on a planted case.  With r_k the reported residual of u_k = Q v_k against the device's operator A^ = A + dA, theta_k its
    Ritz value and gap the distance of the reference group to the rest of the spectrum (asserted >= GAP_MIN):
    - values: a Ritz value of a block that holds the whole group is within r^2 / gap of the group's eigenvalue of A^ (the block form of
      Kato-Temple; r = the root of the group's summed squared residuals), and eigenvalues move by at most ||dA||: |lambda - lambda_ref|
      <= 2 (r^2 / gap' + pert) + 2^-21 for the f32 result, gap' = gap - 2 pert.
    - vectors: the returned z_k is C (Y_next v_k) = C A^ u_k.  Its residual r'_k = ||A^ u' - rho u'|| with u' = A^ u_k / ||A^ u_k|| is at
      most r_k / ||A^ u_k|| <= r_k / theta_k (A^ commutes with A^ - theta, ||A^|| <= 1, ||A^ u|| >= u^T A^ u).  The test re-computes r'_k with
      the reference A from the returned vector and holds it to r_k / theta_k + pert + 2^-20 (f32 vectors), and Davis-Kahan gives
      sin(u', reference group) <= (r_k / theta_k + pert + 2^-20) / gap'.
    - the entry of largest magnitude of every vector is positive and the first such; the vectors have unit length; zero-degree: none here."""
    rows, labels = planted(name)
    n, H = rows.shape
    tau, floor = driver_params(affinity)
    n_eig = len(DRIVER_CASES[name][2])
    what = f"driver {name} {affinity}"
    res = impl.run(rows, n_eig, affinity, tau, floor, DRIVER_MAX_ITER, DRIVER_TOL)
    xh = impl.apply(rows, affinity, tau, floor, None, None, 0)["xhat"]
    bad = check_xhat(xh, rows, what)
    if bad:
        return bad
    theta, U, d, ed, pert, groups = driver_reference(xh, H, affinity, tau, floor, n_eig)
    assert all(g[2] >= GAP_MIN for g in groups), (what, groups)
    if not res["converged"] or res["iterations"] > DRIVER_MAX_ITER or res["iterations"] % 8:
        return [f"{what}: converged {res['converged']} after {res['iterations']} steps"]
    val, vec, r = (np.asarray(res[k], np.float64) for k in ("values", "vectors", "residual"))
    if vec.shape != (n_eig, n) or not (np.isfinite(vec).all() and np.isfinite(val).all() and (r <= DRIVER_TOL * (1 + 1e-6)).all()):
        return [f"{what}: malformed outputs or residuals above tol: {r}"]
    if not (np.abs(np.asarray(res["degree"], np.float64) - d) <= ed + 2.0 ** -23 * d).all():  # (delta_w summed; the f32 result)
        bad.append(f"{what}: degree")
    A = None
    for a, b, gap in groups:
        gp = gap - 2 * pert
        rg = np.sqrt((r[a:b] ** 2).sum())
        vb = 2 * (rg * rg / gp + pert) + 2.0 ** -21
        verr = np.abs(val[a:b] - 2 * (1 - theta[a:b])).max()
        if report is not None:
            report(f"{what}: group {a}:{b} gap {gap:.3f} pert {pert:.2e}: value error {verr:.3e} (bound {vb:.3e})")
        if not verr <= vb:
            bad.append(f"{what}: values {val[a:b]} against {2 * (1 - theta[a:b])} (bound {vb:.3e})")
        for k in range(a, b):
            u = vec[k] * np.sqrt(d)
            u /= np.sqrt((u * u).sum())
            sin = np.sqrt(max(1.0 - ((U[:, a:b].T @ u) ** 2).sum(), 0.0))
            rb = r[k] / theta[k] + pert + 2.0 ** -20
            if A is None:
                W = weights64(sim64(xh), affinity, tau, floor)
                A = 0.5 * (np.eye(n) + W / np.sqrt(d)[:, None] / np.sqrt(d)[None, :])
            Au = A @ u
            r2 = np.sqrt(((Au - (u @ Au) * u) ** 2).sum())
            if report is not None:
                report(f"{what}: vector {k}: sin {sin:.3e} (bound {rb / gp:.3e}), residual re-computed {r2:.3e} (bound {rb:.3e})")
            if not sin <= rb / gp:
                bad.append(f"{what}: vector {k} is {sin:.3e} off its reference group (bound {rb / gp:.3e})")
            if not r2 <= rb:
                bad.append(f"{what}: vector {k}'s re-computed residual {r2:.3e} is above {rb:.3e}")
    if not (np.diff(val) >= -2.0 ** -21).all():
        bad.append(f"{what}: values do not ascend: {val}")
    for k in range(n_eig):
        big = int(np.argmax(np.abs(vec[k])))
        if not vec[k, big] > 0 or abs((vec[k] ** 2).sum() - 1.0) > 1e-5:
            bad.append(f"{what}: vector {k} is not unit length with its largest entry (index {big}) positive")
    return bad


def tokencut_expectation(name="planted2"):
    """The planted foreground of the two-cluster case: the SMALLER cluster -- the second vector's entries are about +-1 / size, so the
    entry of largest magnitude lies there."""
    rows, labels = planted(name)
    sizes = DRIVER_CASES[name][2]
    return rows, labels == int(np.argmin(sizes))


FLAT = (165, 32)  # Gaussian rows with a flat spectrum: 8 steps are nowhere near 1e-4


def flat_rows():
    return mc.gaussian_tokens(FLAT[0], FLAT[1], 77, outliers=False)


def check_exits(impl):
    rows = flat_rows()
    a = impl.run(rows, 4, "relu", 0.0, 0.0, 8, 1e-4)
    b = impl.run(rows, 4, "relu", 0.0, 0.0, 8, 1e-4)
    bad = []
    if a["converged"] or a["iterations"] != 8:
        bad.append(f"exits: max_iter = 8 gave converged {a['converged']}, iterations {a['iterations']}")
    for k in ("values", "vectors", "degree", "residual"):
        if not np.array_equal(bits(np.asarray(a[k])), bits(np.asarray(b[k]))):
            bad.append(f"exits: two runs differ in {k}")
    return bad


# --------------------------------------------------------------------------------------------------------------------- the table
def _probe_case(kind, nchunk):
    return lambda impl, report=None: check_probe(impl, kind, nchunk)


CASES = {}
for _k in PROBES:
    for _c in (1, 2, 0, 3):
        CASES[f"probe_{_k}_c{_c}"] = _probe_case(_k, _c)
for _s in SHAPES:
    for _a in AFFINITIES:
        CASES[f"shape_{shape_id(_s)}_{_a}"] = (lambda s, a: lambda impl, report=None: check_shape(impl, s, a, report))(_s, _a)
for _n in STEP_CASES:
    CASES[_n] = (lambda nm: lambda impl, report=None: check_step(impl, nm, report))(_n)
for _n in DRIVER_CASES:
    for _a in AFFINITIES:
        CASES[f"driver_{_n}_{_a}"] = (lambda nm, a: lambda impl, report=None: check_driver(impl, nm, a, report))(_n, _a)
CASES["exits"] = lambda impl, report=None: check_exits(impl)

# which case rejects which mutant
MUTANT_CASE = {"pad_cols_counted": "probe_negated_c0", "pad_rows_in_gram": "step_129x72_exp", "last_chunk_dropped": "probe_pm1_relu_c2",
               "chunk_local_column_index": "probe_pm1_threshold_c3", "threshold_ge": "probe_at_tau_c0", "relu_abs": "probe_pm1_relu_c0",
               "scale_one_side": "step_257x384_relu", "shift_missing": "step_300x1536_threshold", "zero_degree_nan": "step_zero_row",
               "diag_zeroed": "probe_pm1_threshold_c1", "values_descending": "driver_planted3_relu", "sign_not_fixed": "driver_planted3_threshold"}
