"""Cases for dinov2_hip_kmeans_tokens / dinov2_hip_op_kmeans* (csrc/kmeans.hip), shared by tests/test_kmeans_probes.py (CPU: the numpy
restatement of the contract passes them, planted bugs do not) and tests/test_gpu_kmeans.py (the kernels).

Contract under test (include/dinov2_hip.h, dinov2_hip_kmeans): rows and centre vectors to unit length in f16 by match's normaliser; label =
argmax over the K real centres of match's similarity, ties to the lowest centre; S_c = the f32 sum of the members' f16 rows in an order the
planner fixes (ascending rows within a chunk, chunks ascending); an empty cluster keeps its vector; the loop of contract 5.

Bounds.
  assign   match_cases.tol(H) = 2^-10 + H 2^-24 per similarity, with match's acceptance rule (a near-tie passes with either centre).
  update   |S_c[h] - float64 sum of the device's own x^| <= (count_c + nsplit) 2^-24 sum_{i in c} |x^_ih|.  The products x^ * 1 are exact; a
           chunk's sum of m terms in f32 errs by at most (m - 1) u sum|x^| to first order (u = 2^-24, any order), the fold of the nsplit
           partials adds at most (nsplit - 1) u sum|x^|: together below (count_c + nsplit) u sum|x^|.  The form of pca_cases' covariance bound.
  driver   under the margin condition -- in the float64 Lloyd run every row's gap between its best and second-best similarity is >= 4 tol(H)
           at every iteration -- an f16 / f32 assignment (each similarity within tol of float64) cannot pick another centre, PROVIDED its
           centres are the float64 ones up to rounding; the sums of equal member sets differ from float64 by far less than tol after
           normalisation (the bound above against |S_c| ~ count_c).  So labels, counts, iterations and converged equal the float64 run's.
  probes   rows with exactly 4, 16 or 64 non-zeros of +-1: x^ = +-2^-1, +-2^-2, +-2^-3 exactly, every similarity and every cluster sum is a
           short dyadic sum, exact in f32 in any order -- compared bit for bit, whatever nsplit.
"""
import numpy as np

import match_cases as mc

TILE = 128
K_MAX, ITER_MAX, N_MAX, TARGET_WGS, PARTIAL_MAX = 1024, 1000, 1 << 20, 256, 32 << 20

# (n, K, H): tile edges in n (1, 127, 128, 129, 257), in K (1, 2, 128, 129, 300: one, two, three centre tiles), in H (8, 72, 384, 1536); two
# whose n is a multiple of the planner's chunk + 1 / - 1; one realistic slice
SHAPES = [(1, 1, 8), (127, 2, 8), (128, 128, 72), (129, 129, 384), (257, 300, 1536), (769, 300, 1536), (767, 2, 8), (1374, 8, 1024)]
CHUNK_EDGE = {(769, 300, 1536): (128, 1), (767, 2, 8): (64, 63)}  # shape -> (the planner's chunk, n mod chunk)
PROBES = ["duplicates", "zero_row", "equidistant", "one_cluster", "last_chunk"]
MUTANTS = ["tie_highest", "empty_zeroed", "pad_rows_counted", "xt_pad_not_zeroed", "last_chunk_dropped", "onehot_local_index",
           "update_from_prev_labels", "final_assign_skipped", "first_changed_not_forced", "counts_from_prev"]
NSPLIT_MAX = 1 << 14  # asks for "as many chunks as there are K-tiles": the planner lowers it


def shape_id(s):
    return "x".join(str(v) for v in s)


# ------------------------------------------------------------------------------------------------------------------- the planner
def plan(n, K, H, nsplit=0):
    """kmeans_plan (csrc/kernels.h) restated: dict of npad, kpad, hpad, hpad128, chunk, nsplit, partial_bytes."""
    npad, kpad = -(-n // 128) * 128, -(-K // 128) * 128
    hpad, hpad128 = -(-H // 64) * 64, -(-H // 128) * 128
    nt = npad // 64
    tiles = (hpad128 // 128) * (kpad // 128)
    per_split = kpad * hpad128 * 4
    if nsplit <= 0:
        nsplit = -(-TARGET_WGS // tiles)
    nsplit = min(nsplit, PARTIAL_MAX // per_split, nt)
    chunk_tiles = -(-nt // nsplit)
    nsplit = -(-nt // chunk_tiles)
    return {"npad": npad, "kpad": kpad, "hpad": hpad, "hpad128": hpad128, "chunk": 64 * chunk_tiles, "nsplit": nsplit,
            "partial_bytes": per_split * nsplit}


def chunks(p):
    """[(first row, end row)] of the update's chunks."""
    return [(i * p["chunk"], min((i + 1) * p["chunk"], p["npad"])) for i in range(p["nsplit"])]


# ------------------------------------------------------------------------------------------------------------------- inputs
def shape_inputs(shape):
    """(rows, centre vectors): Gaussian tokens with match's two outlier channels; the centres are perturbed rows, so clusters have members."""
    n, K, H = shape
    x = mc.gaussian_tokens(n, H, 300 + n + H)
    rng = np.random.default_rng(400 + K + H)
    c = (x[rng.integers(n, size=K)] + 0.5 * rng.standard_normal((K, H))).astype(np.float32)
    return x, c


def update_labelings(shape, nsplit_used):
    """{name: labels [n]} for the update cases: random, all the same, clusters that straddle the chunk edges."""
    n, K, H = shape
    rng = np.random.default_rng(500 + n + K)
    p = plan(n, K, H, nsplit_used)
    straddle = ((np.arange(n) + p["chunk"] // 2) // p["chunk"]) % K  # cluster j = the rows around the j-th chunk edge
    return {"random": rng.integers(K, size=n).astype(np.int32), "same": np.full(n, K - 1, np.int32), "straddle": straddle.astype(np.int32)}


def pm_rows(rng, n, H, nnz=(4, 16, 64)):
    """Rows with +-1 in exactly 4, 16 or 64 positions (those that fit H)."""
    nnz = [k for k in nnz if k <= H]
    x = np.zeros((n, H), np.float32)
    for i in range(n):
        k = nnz[int(rng.integers(len(nnz)))]
        x[i, rng.choice(H, k, replace=False)] = rng.choice([-1.0, 1.0], k)
    return x


def build_probe(kind, H=72, seed=11):
    """dict of an exact probe: rows x [n, H], centre vectors c [K, H], and what is planted (see each kind)."""
    rng = np.random.default_rng(seed + H)
    n = TILE + 3
    if kind == "duplicates":  # centre 129 repeats centre 3 (another centre tile), centre 7 repeats centre 5: the higher index never wins
        K = TILE + 2
        x, c = pm_rows(rng, n, H), pm_rows(rng, K, H)
        c[TILE + 1], c[7] = c[3], c[5]
        x[0], x[TILE + 1], x[2] = c[3], c[3], c[5]
        return {"x": x, "c": c, "never": [TILE + 1, 7], "labels_at": {0: 3, TILE + 1: 3, 2: 5}}
    if kind == "zero_row":  # every similarity of a zero row is 0: centre 0 by the tie rule, sim +0
        K = 5
        x, c = pm_rows(rng, n, H), pm_rows(rng, K, H)
        x[1] = 0.0
        x[TILE] = 0.0
        return {"x": x, "c": c, "labels_at": {1: 0, TILE: 0}, "sim_at": {1: 0.0, TILE: 0.0}}
    if kind == "equidistant":  # row 4 has 16 non-zeros; centres 2 and 6 are four of them each: both similarities are exactly 1/2
        K = 9
        x = pm_rows(rng, n, H, nnz=(16,))
        c = pm_rows(rng, K, H, nnz=(64,))  # (the other centres reach at most 16 * (1/4) (1/8) = 1/2 only with all signs right: asserted below)
        pos = np.flatnonzero(x[4])
        c[2], c[6] = 0.0, 0.0
        c[2, pos[:4]], c[6, pos[4:8]] = x[4, pos[:4]], x[4, pos[4:8]]
        S = mc.reference(x[4:5], c)[0]
        assert S[2] == 0.5 and S[6] == 0.5 and np.delete(S, [2, 6]).max() < 0.5
        return {"x": x, "c": c, "labels_at": {4: 2}, "sim_at": {4: 0.5}}
    if kind == "one_cluster":  # all-positive rows that share positions 0 .. 3 = centre 0; centres 1 and 2 are its negation: everything in 0
        K = 3
        x = np.zeros((n, H), np.float32)
        for i in range(n):
            x[i, :4] = 1.0
            x[i, 4 + rng.choice(H - 4, 12, replace=False)] = 1.0
        c = np.zeros((K, H), np.float32)
        c[0, :4], c[1, :4], c[2, :4] = 1.0, -1.0, -1.0
        return {"x": x, "c": c, "all": 0}
    if kind == "last_chunk":  # update only: the members of cluster 1 sit alone in the last chunk that holds rows, a partial one (rows 128 .. 130; chunks of 64)
        K = 2
        x = pm_rows(rng, n, H)
        lab = np.zeros(n, np.int32)
        lab[TILE:] = 1
        return {"x": x, "c": pm_rows(rng, K, H), "labels": lab}
    raise ValueError(kind)


def driver_case(which):
    """dict of a planted-cluster case with a deliberately bad init: x, K, init (row indices), max_iter.  K planted clusters of two tight
    sub-groups each (cluster direction + 0.5 sub-group offset + 0.05 noise per row).  The init rows are one row of EACH sub-group of cluster
    0, one row of clusters 1 .. K - 2, none of cluster K - 1: Lloyd has to merge the two centres of cluster 0 and move one over to the
    orphaned cluster, whole sub-groups at a time -- so the gaps are those between sub-groups, not between neighbouring rows.  The seeds are
    ones for which the float64 run takes 3 updates under the margin condition (tests/test_kmeans_probes.py asserts both)."""
    n, K, H, seed = {"small": (96, 4, 64, 53), "tiles": (200, 5, 72, 26)}[which]
    rng = np.random.default_rng(seed)
    G = 2 * K
    cdir = rng.standard_normal((K, H))
    dirs = cdir[np.arange(G) // 2] + 0.5 * rng.standard_normal((G, H))
    group = np.arange(n) % G
    x = (dirs[group] + 0.05 * rng.standard_normal((n, H))).astype(np.float32)
    first = [int(np.flatnonzero(group == g)[0]) for g in range(G)]
    init = [first[0], first[1]] + [first[2 * q] for q in range(1, K - 1)]
    return {"x": x, "K": K, "init": np.asarray(init, np.int32), "max_iter": 20, "cluster": group // 2}


DRIVER_CASES = ["small", "tiles"]


# ------------------------------------------------------------------------------------------------------------------- float64 reference
def unit64(v):
    v = np.asarray(v, np.float64)
    nrm = np.sqrt((v * v).sum(1))
    return v / np.where(nrm > 0, nrm, 1.0)[:, None]


def reference_run(x, K, max_iter, init_vectors):
    """Contract 5 in float64 on the un-rounded rows.  dict of labels, counts, iterations, converged, centers, and history: per assignment
    (labels, the smallest best-minus-second gap over the rows, changed)."""
    xn = unit64(x)
    vec = np.asarray(init_vectors, np.float64).copy()
    labels, it, conv, hist = None, 0, False, []
    while True:
        S = xn @ unit64(vec).T
        new = S.argmax(1)
        top = np.sort(S, axis=1)[:, -2:] if K > 1 else None
        gap = float((top[:, 1] - top[:, 0]).min()) if K > 1 else np.inf
        changed = len(x) if labels is None else int((new != labels).sum())
        labels = new
        hist.append((labels.copy(), gap, changed))
        if changed == 0:
            conv = True
            break
        if it == max_iter:
            break
        for c in range(K):
            if (labels == c).any():
                vec[c] = xn[labels == c].sum(0)
        it += 1
    return {"labels": labels.astype(np.int32), "counts": np.bincount(labels, minlength=K).astype(np.int32), "iterations": it, "converged": conv,
            "centers": vec, "history": hist}


def margin_ok(ref, H):
    """The margin condition of the module docstring, and no `changed` of 0 before the last assignment."""
    hist = ref["history"]
    return all(g >= 4 * mc.tol(H) for _, g, _ in hist) and all(ch > 0 for _, _, ch in hist[:-1])


# ------------------------------------------------------------------------------------------------------------------- restatement
def emulate_assign(x, vec, mutant=None):
    """Contract 2: match's restatement, row direction."""
    r = mc.emulate(x, vec, "tie_highest" if mutant == "tie_highest" else None)
    return {"labels": r["idx_ab"], "sim": r["sim_ab"]}


def emulate_update(xhat, labels, K, prev, nsplit=0, mutant=None):
    """Contract 3 / 4 with the kernel's padding made explicit.  xhat [n, H]: the f32 values of the f16 rows; labels [n] in [0, K)."""
    n, H = xhat.shape
    p = plan(n, K, H, nsplit)
    npad, kpad, hpad128 = p["npad"], p["kpad"], p["hpad128"]
    XT = np.zeros((hpad128, npad), np.float32)
    if mutant == "xt_pad_not_zeroed":
        XT[:] = np.nan  # what the 0xff bytes of an unwritten buffer read as
    XT[:H, :n] = np.asarray(xhat, np.float32).T
    lab = np.full(npad, 0 if mutant == "pad_rows_counted" else -1, np.int64)
    lab[:n] = labels
    cols = np.arange(kpad)
    if mutant == "onehot_local_index":
        cols = cols % TILE
    S = np.zeros((kpad, hpad128), np.float32)
    cnt = np.zeros(kpad, np.int64)
    spans = chunks(p)
    if mutant == "last_chunk_dropped" and len(spans) > 1:
        spans = spans[:-1]
    with np.errstate(invalid="ignore"):
        for a, b in spans:  # chunks ascending; within a chunk numpy's order (any order is inside the bound, and exact on the probes)
            onehot = (lab[a:b, None] == cols[None, :]).astype(np.float32)
            S = S + (onehot.T @ XT[:, a:b].T).astype(np.float32)
            cnt += onehot.sum(0).astype(np.int64)
    out = np.asarray(prev, np.float32).copy()
    for c in range(K):
        if cnt[c] > 0:
            out[c] = S[c, :H]
        elif mutant == "empty_zeroed":
            out[c] = 0.0
    return {"centers": out, "counts": cnt[:K].astype(np.int32), "nsplit": p["nsplit"]}


def emulate_run(x, K, max_iter, init_vectors, mutant=None):
    """Contract 5 on the restated kernels; the dict of Session.kmeans."""
    x = np.asarray(x, np.float32)
    n = len(x)
    xhat = mc.normalise_f16(x).astype(np.float32)
    vec = np.asarray(init_vectors, np.float32).copy()
    labels = np.zeros(n, np.int32)  # (what an unforced first comparison would see: a cleared buffer)
    counts = np.zeros(K, np.int32)
    it, conv, first = 0, False, True
    while True:
        prev = labels
        a = emulate_assign(x, vec, mutant)
        labels, sim = a["labels"], a["sim"]
        changed = n if first and mutant != "first_changed_not_forced" else int((labels != prev).sum())
        if changed == 0:
            conv = True
            break
        if it == max_iter:
            if mutant != "counts_from_prev":
                counts = np.bincount(labels, minlength=K).astype(np.int32)
            break
        u = emulate_update(xhat, prev if mutant == "update_from_prev_labels" and not first else labels, K, vec, 0, mutant)
        vec, counts = u["centers"], u["counts"]
        first = False
        it += 1
        if mutant == "final_assign_skipped" and it == max_iter:
            break
    return {"labels": labels, "sim": sim, "centers": vec, "counts": counts, "iterations": it, "converged": conv}


# ------------------------------------------------------------------------------------------------------------------- checks
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_assign(res, x, vec, what):
    """match's tolerance rule on (labels, sim) against the float64 cosine of the un-rounded inputs."""
    S = mc.reference(x, vec)
    n, K = S.shape
    lab, sim = np.asarray(res["labels"]), np.asarray(res["sim"])
    if lab.shape != (n,) or sim.shape != (n,) or lab.min() < 0 or lab.max() >= K or not np.isfinite(sim).all():
        return False, f"{what}: malformed labels / sim"
    t = mc.tol(x.shape[1])
    at = S[np.arange(n), lab]
    err, short = np.abs(sim.astype(np.float64) - at), S.max(1) - at
    if err.max() > t:
        return False, f"{what}: sim off by {err.max():.3e} > tol {t:.3e}"
    if short.max() > 2 * t:
        return False, f"{what}: a label is short of the best centre by {short.max():.3e} > 2 tol {2 * t:.3e}"
    return True, ""


def check_update(res, xhat, labels, K, prev, nsplit, what, report=None):
    """counts exact; S_c within the bound of the module docstring of the float64 sum of xhat; empty clusters keep prev bit for bit."""
    xhat64 = np.asarray(xhat, np.float64)
    want = np.bincount(labels, minlength=K)
    if not np.array_equal(res["counts"], want):
        return False, f"{what}: counts differ from the labels' ({int((np.asarray(res['counts']) != want).sum())} clusters)"
    worst = 0.0
    for c in range(K):
        got = np.asarray(res["centers"][c])
        if want[c] == 0:
            if not np.array_equal(bits(got), bits(prev[c])):
                return False, f"{what}: empty cluster {c} did not keep its vector"
            continue
        m = labels == c
        ref, mag = xhat64[m].sum(0), np.abs(xhat64[m]).sum(0)
        bound = (want[c] + nsplit) * 2.0 ** -24 * mag
        err = np.abs(got.astype(np.float64) - ref)
        if not np.isfinite(got).all() or (err > bound).any():
            h = int(np.argmax(err - bound)) if np.isfinite(got).all() else -1
            return False, f"{what}: cluster {c} column {h}: error {err[h]:.3e} > bound {bound[h]:.3e} (count {want[c]}, nsplit {nsplit})"
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
    if report is not None:
        report.append(f"{what}: worst error / bound {worst:.3f}")
    return True, ""


def check_probe_assign(assign_fn, kind, what):
    """The planted facts of a probe and the exact expectation (labels and sim bit for bit)."""
    pr = build_probe(kind)
    x, c = pr["x"], pr["c"]
    got = assign_fn(x, c)
    S = mc.reference(x, c)
    S32 = S.astype(np.float32)
    assert np.array_equal(S32.astype(np.float64), S), "probe similarities are not exact in f32"
    exp_l = S.argmax(1).astype(np.int32)
    exp_s = (S32 + np.float32(0.0))[np.arange(len(x)), exp_l]
    if not np.array_equal(got["labels"], exp_l):
        i = int(np.flatnonzero(np.asarray(got["labels"]) != exp_l)[0])
        return False, f"{what} {kind}: label[{i}] = {got['labels'][i]}, expected {exp_l[i]}"
    if not np.array_equal(bits(got["sim"]), bits(exp_s)):
        return False, f"{what} {kind}: sim differs in bits"
    for i, l in pr.get("labels_at", {}).items():
        assert exp_l[i] == l, (kind, i)
    for i, v in pr.get("sim_at", {}).items():
        assert exp_s[i] == v and not np.signbit(exp_s[i]), (kind, i)
    for j in pr.get("never", []):
        assert not (exp_l == j).any()
    if "all" in pr:
        assert (exp_l == pr["all"]).all()
    return True, ""


def exact_update_expectation(xhat, labels, K, prev):
    """Probe rows: every cluster sum is exact in f32, so float64 gives the bits."""
    out = np.asarray(prev, np.float32).copy()
    for c in range(K):
        if (labels == c).any():
            s = np.asarray(xhat, np.float64)[labels == c].sum(0)
            assert np.array_equal(s.astype(np.float32).astype(np.float64), s)
            out[c] = s.astype(np.float32)
    return out, np.bincount(labels, minlength=K).astype(np.int32)


def check_probe_update(update_fn, kind, nsplit, what):
    """update_fn(x, labels, K, prev, nsplit) -> dict(centers, counts[, xhat]) on a probe: bit for bit whatever nsplit."""
    pr = build_probe(kind)
    x, c = pr["x"], pr["c"]
    K = len(c)
    labels = pr["labels"] if "labels" in pr else mc.reference(x, c).argmax(1).astype(np.int32)
    got = update_fn(x, labels, K, c, nsplit)
    xhat = mc.normalise_f16(x).astype(np.float32)
    exp_c, exp_n = exact_update_expectation(xhat, labels, K, c)
    if not np.array_equal(got["counts"], exp_n):
        return False, f"{what} {kind} nsplit={nsplit}: counts {list(got['counts'])[:8]} expected {list(exp_n)[:8]}"
    if not np.array_equal(bits(got["centers"]), bits(exp_c)):
        bad = np.flatnonzero((bits(got["centers"]) != bits(exp_c)).any(1))
        return False, f"{what} {kind} nsplit={nsplit}: centres of clusters {list(bad[:6])} differ in bits"
    return True, ""


def run_failures(run_fn):
    """Driver cases and loop probes through run_fn(x, K, max_iter, init_vectors) -> dict of Session.kmeans; the failure messages."""
    failures = []
    for which in DRIVER_CASES:
        d = driver_case(which)
        x, K = d["x"], d["K"]
        full = reference_run(x, K, d["max_iter"], x[d["init"]])
        for m in sorted({0, 1, 2, full["iterations"], full["iterations"] + 1}):  # the labels of every iteration, through max_iter
            ref = reference_run(x, K, m, x[d["init"]])
            got = run_fn(x, K, m, x[d["init"]])
            for k in ("labels", "counts"):
                if not np.array_equal(got[k], ref[k]):
                    failures.append(f"driver {which} max_iter={m}: {k} differ from the float64 run")
            if (int(got["iterations"]), bool(got["converged"])) != (ref["iterations"], ref["converged"]):
                failures.append(f"driver {which} max_iter={m}: iterations / converged {got['iterations']} / {got['converged']}, float64 run "
                                f"{ref['iterations']} / {ref['converged']}")
            if m == 0 and not np.array_equal(bits(got["centers"]), bits(x[d["init"]])):
                failures.append(f"driver {which}: max_iter = 0 did not return the init vectors verbatim")
    # one_cluster: converged after one update; the two negated centres stay empty and keep their vectors; the sum is exact
    pr = build_probe("one_cluster")
    got = run_fn(pr["x"], 3, 5, pr["c"])
    exp_c, exp_n = exact_update_expectation(mc.normalise_f16(pr["x"]).astype(np.float32), np.zeros(len(pr["x"]), np.int32), 3, pr["c"])
    if (int(got["iterations"]), bool(got["converged"])) != (1, True) or not np.array_equal(got["counts"], exp_n) or (np.asarray(got["labels"]) != 0).any():
        failures.append(f"one_cluster: iterations {got['iterations']} converged {got['converged']} counts {list(got['counts'])}")
    if not np.array_equal(bits(got["centers"]), bits(exp_c)):
        failures.append("one_cluster: centres differ in bits (an empty cluster must keep its vector, the sum is exact)")
    # duplicates: the higher copy gets no member in the first assignment, so the one update leaves its vector alone
    pr = build_probe("duplicates")
    got = run_fn(pr["x"], len(pr["c"]), 1, pr["c"])
    for j in pr["never"]:
        if int(got["iterations"]) != 1 or not np.array_equal(bits(got["centers"][j]), bits(pr["c"][j])):
            failures.append(f"duplicates: centre {j} lost its vector in an update in which it had no member")
    return failures


def kernel_failures(assign_fn, update_fn):
    """Every shape and probe through assign_fn(x, c) and update_fn(x, labels, K, prev, nsplit) (which returns xhat too); the messages."""
    failures = []

    def note(ok_msg):
        if not ok_msg[0]:
            failures.append(ok_msg[1])

    for shape in SHAPES:
        n, K, H = shape
        x, c = shape_inputs(shape)
        note(check_assign(assign_fn(x, c), x, c, "assign " + shape_id(shape)))
        for name, lab in update_labelings(shape, 0).items():
            got = update_fn(x, lab, K, c, 0)
            note(check_update(got, got["xhat"], lab, K, c, plan(n, K, H)["nsplit"], f"update {shape_id(shape)} {name}"))
    for kind in PROBES:
        if kind != "last_chunk":
            note(check_probe_assign(assign_fn, kind, "probe"))
        for ns in (1, 2, 0, NSPLIT_MAX):
            note(check_probe_update(update_fn, kind, ns, "probe"))
    return failures
