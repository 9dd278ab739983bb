"""Cases for dinov2_hip_coreset_tokens / dinov2_hip_op_coreset* (csrc/coreset.hip), shared by tests/test_coreset_probes.py (CPU: the numpy
restatement of the contract passes them, planted bugs do not) and tests/test_gpu_coreset.py (the kernels).

Contract under test (include/dinov2_hip.h, dinov2_hip_coreset): rows to unit length in f16 by match's normaliser; sim = match's similarity;
pick 0 = first; s(i) = the largest similarity of row i to a pick, nearest(i) the lowest pick position among equal values, -0 read as +0;
the next pick is the unselected row with the smallest s, among equal values the lowest row; cover[t] = that s; selection stops before pick
t >= 1 once the smallest s is >= stop_sim.

The greedy rule is restated over a COLUMN ORACLE -- column(p) = the similarities of all rows to row p -- so that one function serves the
probes (columns of the exact similarity matrix), the device replay of tests/test_gpu_coreset.py (columns = the device's own similarities to
the rows it picked: a pick the rule would not have made asks for a column nobody has) and the far case (columns gathered per dictionary entry).

  probes   kmeans_cases.pm_rows: rows of +-1 in exactly 4, 16 or 64 places, so x^ = +-2^-1, +-2^-2 or +-2^-3 exactly and every similarity is a
           short dyadic sum, exact in f32 in any order: idx, cover, selected, nearest and near_sim are compared bit for bit.  n = 131 puts rows
           128 .. 130 in a second 128-row tile.
  shapes   Gaussian tokens (match_cases.gaussian_tokens); on the device the choice is replayed exactly over the device's own similarity bits,
           and each similarity is held to match_cases.tol(H) of float64.
"""
import numpy as np

import kmeans_cases as kc
import match_cases as mc

TILE = 128
N_MAX, PARTS_MAX, WG_BYTES = 1 << 20, 1024, 64 << 10

# (n, H, m): n in 1, 2, 127, 128, 129, 257, 1374 (tile edges; 11 tiles), H in 8, 72, 384, 1536 (K padding; 2 .. 48 k-steps, the 8-step and the
# 2-step form of the chain), m in 1, 2, 64 and n itself
SHAPES = [(1, 8, 1), (2, 8, 2), (127, 72, 64), (128, 384, 2), (129, 1536, 64), (257, 72, 64), (1374, 384, 64), (129, 8, 129), (1374, 1536, 1)]
PROBES = ["duplicates", "zero_rows", "equal_smallest", "neg_zero", "m_equals_n", "stop_equal", "stop_ulp_above"]
# every planted bug and the probe that must reject it
MUTANTS = {"tie_highest_row": "equal_smallest", "nearest_tie_latest": "duplicates", "no_selected_mark": "zero_rows",
           "pad_rows_take_part": "m_equals_n", "pick_from_prev_partials": "m_equals_n", "last_sweep_skipped": "equal_smallest",
           "stop_gt": "stop_equal", "cover_after_update": "duplicates", "neg_zero_below": "neg_zero"}
KEYS = ("idx", "cover", "selected", "nearest", "near_sim")


def shape_id(s):
    return "x".join(str(v) for v in s)


# ------------------------------------------------------------------------------------------------------------------- the planner
def plan(n, H, rows_per_wg=0):
    """coreset_plan (csrc/kernels.h) restated: dict of npad, hpad, rows_per_wg, nparts."""
    npad, hpad = -(-n // TILE) * TILE, -(-H // 64) * 64
    tiles = npad // TILE
    if rows_per_wg <= 0:
        tpw = min(-(-WG_BYTES // (TILE * hpad * 2)), tiles // 512)
    else:
        tpw = -(-rows_per_wg // TILE)
    tpw = min(max(tpw, -(-tiles // PARTS_MAX), 1), tiles)
    return {"npad": npad, "hpad": hpad, "rows_per_wg": tpw * TILE, "nparts": -(-tiles // tpw)}


# ------------------------------------------------------------------------------------------------------------------- the greedy rule
def _key(v, mutant):
    """What values are ordered by: the f32 value with -0 read as +0 (float64 holds it exactly); the planted bug puts -0 below +0."""
    v = np.asarray(v, np.float32)
    k = (v + np.float32(0.0)).astype(np.float64)
    if mutant == "neg_zero_below":
        k[(v == 0) & np.signbit(v)] = -1e-300
    return k


def greedy(column, N, n, m, first, stop_sim=np.inf, mutant=None):
    """Contracts 3 - 4.  column(p) -> f32 [N]: the similarity of every row to row p; rows n .. N - 1 are padding.  Returns the dict of
    Session.coreset.  `mutant`: one of MUTANTS, planted."""
    live = N if mutant == "pad_rows_take_part" else n
    s_key = np.full(N, -np.inf)
    s_val = np.full(N, -np.inf, np.float32)
    nearest = np.full(N, -1, np.int32)
    marked = np.zeros(N, bool)
    idx, cover, selected = np.full(m, -1, np.int32), np.full(m, np.inf, np.float32), m
    before = None  # s as it was before the latest sweep
    for t in range(m):
        if t == 0:
            p, c = int(first), np.float32(-np.inf)
        else:
            src = before if mutant == "pick_from_prev_partials" and t >= 2 else s_key
            k = src[:live].copy()
            if mutant != "no_selected_mark":
                k[marked[:live]] = np.inf
            best = k.min()
            rows = np.flatnonzero(k == best)
            p = int(rows[-1] if mutant == "tie_highest_row" else rows[0])
            if (best > stop_sim) if mutant == "stop_gt" else (best >= stop_sim):
                selected = t
                break
            c = s_val[p]
        idx[t], marked[p] = p, True
        before = s_key.copy()
        if not (mutant == "last_sweep_skipped" and t == m - 1):
            col = np.asarray(column(p), np.float32)
            kcol = _key(col, mutant)
            upd = (kcol >= s_key) if mutant == "nearest_tie_latest" else (kcol > s_key)
            s_key[upd], nearest[upd] = kcol[upd], t
            s_val[upd] = (col if mutant == "neg_zero_below" else col + np.float32(0.0))[upd]
        cover[t] = s_val[p] if mutant == "cover_after_update" and t > 0 else c
    return {"idx": idx, "cover": cover, "selected": int(selected), "nearest": nearest[:n].copy(), "near_sim": s_val[:n].copy()}


def padded_sims(x, exact=False):
    """[npad, npad] f32: the similarities of the f16 unit rows, the operand's zero padding rows included (f32 sums of exact products in
    numpy's order: inside match's tolerance for any rows, and with `exact` asserted to be the exact values)."""
    x = np.asarray(x, np.float32)
    n = len(x)
    npad = -(-n // TILE) * TILE
    xh = np.zeros((npad, x.shape[1]), np.float64)
    xh[:n] = mc.normalise_f16(x).astype(np.float64)
    S = xh @ xh.T
    S32 = S.astype(np.float32)
    if exact:
        assert np.array_equal(S32.astype(np.float64), S), "probe similarities are not exact in f32"
    return S32


def emulate(x, m, first=0, stop_sim=np.inf, mutant=None, patch=(), exact=False):
    """The contract on rows x through numpy similarities; patch: (i, j, value) entries planted into the similarity matrix (a -0)."""
    S = padded_sims(x, exact)
    for i, j, v in patch:
        assert S[i, j] == v  # (only the sign of a zero changes)
        S[i, j] = v
    return greedy(lambda p: S[:, p], len(S), len(x), m, first, stop_sim, mutant)


# ------------------------------------------------------------------------------------------------------------------- inputs
def shape_inputs(shape):
    n, H, _ = shape
    return mc.gaussian_tokens(n, H, 700 + n + H)


def build_probe(kind, H=72, seed=19):
    """dict of an exact probe: rows x [131, H], m, first, stop_sim, patch (see emulate) and what is planted (see each kind)."""
    rng = np.random.default_rng(seed + H)
    n = TILE + 3
    x = kc.pm_rows(rng, n, H)
    pr = {"m": 24, "first": 3, "stop_sim": np.inf, "patch": ()}
    if kind == "duplicates":  # row 130 repeats the first pick (s = 1: picked after everything else), rows 64 and 128 repeat each other
        x[TILE + 2], x[TILE] = x[3], x[64]
        pr.update(m=n, last=TILE + 2, twins=(64, TILE))
    elif kind == "zero_rows":  # a zero row in either tile: s = 0 whatever is picked, itself included; each is picked once
        x[10], x[TILE + 1] = 0.0, 0.0
        pr.update(m=n, zeros=(10, TILE + 1))
    elif kind == "equal_smallest":  # rows 20 and 100 are the negated first pick: both at exactly -1, the smallest there is
        x[20], x[100] = -x[3], -x[3]
        pr.update(m=3, pick1=20)
    elif kind == "neg_zero":  # a zero row whose similarity to the first pick is handed over as -0: read as +0, it stays with pick 0
        x[TILE + 1] = 0.0
        pr.update(m=4, patch=((TILE + 1, 3, np.float32(-0.0)),), stays=TILE + 1)
    elif kind == "m_equals_n":
        pr.update(m=n)
    elif kind in ("stop_equal", "stop_ulp_above"):  # stop_sim = an attained cover value: stops there; one ulp above: goes one pick further
        full = emulate(x, 24, 3, exact=True)
        t = 2 + int(np.flatnonzero(np.diff(full["cover"][1:]) > 0)[-1])  # the last pick at which cover rises: the first to attain its value
        v = full["cover"][t]
        assert full["cover"][t - 1] < v
        pr.update(at=t, stop_sim=float(v if kind == "stop_equal" else np.nextafter(v, np.float32(np.inf))))
    else:
        raise ValueError(kind)
    pr["x"] = x
    return pr


def expected(pr):
    return emulate(pr["x"], pr["m"], pr["first"], pr["stop_sim"], None, pr["patch"], exact=True)


# ------------------------------------------------------------------------------------------------------------------- checks
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def non_decreasing(cover):
    """cover[1 ..] never falls (the +inf tail after a stop included)."""
    c = np.asarray(cover)[1:]
    return bool((c[1:] >= c[:-1]).all())


def same(got, exp, what):
    """Every key of the result bit for bit (similarities as their 32-bit patterns: -0 is not +0 here)."""
    for k in KEYS:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        if g.shape != e.shape:
            return False, f"{what}: {k} has shape {g.shape}, expected {e.shape}"
        gb, eb = (bits(g), bits(e)) if k in ("cover", "near_sim") else (g, e)
        if not np.array_equal(gb, eb):
            i = int(np.flatnonzero(np.atleast_1d(gb != eb))[0])
            return False, f"{what}: {k}[{i}] = {np.atleast_1d(g)[i]!r}, expected {np.atleast_1d(e)[i]!r}"
    return True, ""


def check_probe(run_fn, kind, what="probe"):
    """run_fn(x, m, first, stop_sim, patch) -> the dict of Session.coreset, on a probe: the planted facts and the exact expectation."""
    pr = build_probe(kind)
    exp = expected(pr)
    n, m = len(pr["x"]), pr["m"]
    assert non_decreasing(exp["cover"])
    if kind == "duplicates":
        a, b = pr["twins"]
        assert exp["selected"] == n and exp["idx"][-1] == pr["last"] and sorted(exp["idx"]) == list(range(n))
        pos = {int(r): u for u, r in enumerate(exp["idx"])}
        assert exp["cover"][pos[max(a, b, key=pos.get)]] == 1.0  # the later twin waits until only similarity-1 rows are left
        assert exp["nearest"][b] == exp["nearest"][a] == min(pos[a], pos[b])
    if kind == "zero_rows":
        assert sorted(exp["idx"]) == list(range(n)) and all(exp["near_sim"][z] == 0 and not np.signbit(exp["near_sim"][z]) for z in pr["zeros"])
    if kind == "equal_smallest":
        assert exp["idx"][1] == pr["pick1"] and exp["cover"][1] == -1.0 and exp["nearest"][100] == 1 and exp["near_sim"][100] == 1.0
    if kind == "neg_zero":
        z = pr["stays"]
        assert exp["nearest"][z] == 0 and bits(exp["near_sim"][z:z + 1])[0] == 0
    if kind == "stop_equal":
        assert exp["selected"] == pr["at"] < m and (exp["idx"][pr["at"]:] == -1).all() and np.isinf(exp["cover"][pr["at"]:]).all()
        assert exp["nearest"].max() == pr["at"] - 1
    if kind == "stop_ulp_above":
        assert pr["at"] < exp["selected"] <= m
    return same(run_fn(pr["x"], m, pr["first"], pr["stop_sim"], pr["patch"]), exp, f"{what} {kind}")
