"""Cases for dinov2_hip_bank_topk / dinov2_hip_op_bank_topk (csrc/bank.hip), shared by tests/test_bank_probes.py (CPU: the numpy restatement
of the contract passes them, planted bugs do not) and tests/test_gpu_bank.py (the kernels and the session calls).

Contract under test (include/dinov2_hip.h): rows to unit length in f16 exactly as dinov2_hip_match does, f32 accumulation of exact products,
and per query row the first k of the bank's `count` rows in ONE strict total order -- larger f32 value first (-0 read as +0), among equal
values the lowest index -- whatever the chunking of the bank, the merge order and the calls the rows were added in; slots past a short
bank's count hold (-1, -inf).

  shapes    Gaussian tokens (match_cases.gaussian_tokens) against the float64 cosine S of the un-rounded inputs, tol = match_cases.tol(H),
            per row: (1) indices distinct and in [0, nb); (2) |sim_j - S[i, idx_j]| <= tol; (3) the returned f32 list is sorted by the total
            order, exactly; (4) every column not returned has S[i, c] <= S[i, idx_{k-1}] + 2 tol -- (2) applied to the excluded column and
            to the k-th returned one: the kernel saw the excluded one no better than the k-th, and each seen value is within tol of S.
  probes    the +-1 rows of match_cases (every similarity exact in f32 in any order, full of ties) at k in {1, 3, 64}: indices and the
            32-bit patterns of the similarities against a stable sort of -S.
  scenario  a bank filled in calls of 1, 130 and 169 rows against one filled in one call; after clear() and a shorter refill the stale
            rows -- copies of the queries, similarity 1 -- never appear.
  resident  LAST_CLS / LAST_PATCHES views of a synthetic token stream (CPU restatement only; the GPU test uses a real forward).
"""
import numpy as np

import match_cases as mc

TM = TN = 128                 # bank_topk_kernel's tile (match_kernel's)
PASS_TILES = 32               # csrc/kernels.h BANK_PASS_TILES
PASS = PASS_TILES * TM        # queries of one pass: one more takes the second pass
TARGET_WGS = 256              # BANK_TARGET_WGS
PARTIAL_MAX = 32 << 20        # BANK_PARTIAL_MAX
K_MAX = 64
EMPTY = np.iinfo(np.int32).max

# (nq, nb, H, k): tile edges, K padding, k at its ends, k > nb, and a second pass of queries (thin, so still quick)
SHAPES = [(1, 1, 8, 1), (1, 129, 8, 5), (127, 128, 64, 1), (128, 129, 72, 8), (129, 257, 384, 64), (5, 1000, 1024, 20), (257, 300, 1536, 33),
          (3, 5, 8, 8), (PASS + 1, 3, 8, 2)]
PROBES = list(mc.PROBES)
PROBE_KS = (1, 3, 64)
CHUNKINGS = (0, 1, 2, 1 << 20)  # the planner's choice, one tile a chunk, two, all tiles in one chunk
MUTANTS = ["tie_highest", "pad_col_counted", "stale_rows_counted", "last_chunk_dropped", "chunk_merge_duplicates_index", "list_not_sorted",
           "kth_slot_lost", "second_add_offset_wrong", "resident_cls_stride_wrong", "short_bank_tail_garbage"]


def shape_id(s):
    return "x".join(str(v) for v in s)


def shape_inputs(shape):
    nq, nb, H, _ = shape
    return mc.gaussian_tokens(nq, H, 300 + nq + H), mc.gaussian_tokens(nb, H, 400 + nb + H)


# ------------------------------------------------------------------------------------------------------------------- the planner, restated
def plan(nq, count, k, chunk_tiles=0):
    """bank_topk_plan of csrc/kernels.h: (chunk_tiles, nchunks, pass_tiles, ntiles)."""
    nq_pad = -(-nq // TM) * TM
    ntiles = -(-count // TN)
    rt = min(nq_pad // TM, PASS_TILES)
    want = -(-TARGET_WGS // rt)
    if chunk_tiles <= 0:
        chunk_tiles = -(-ntiles // want)
    per = TM * k * 8
    max_chunks = PARTIAL_MAX // per
    chunk_tiles = min(max(chunk_tiles, -(-ntiles // max_chunks)), ntiles)
    nchunks = -(-ntiles // chunk_tiles)
    return chunk_tiles, nchunks, min(rt, PARTIAL_MAX // (per * nchunks)), ntiles


# ------------------------------------------------------------------------------------------------------------------- restatement
def _first_k(v, i, k, mutant=None):
    """The first k of the pairs (v, i) in the total order, padded with (-inf, EMPTY)."""
    order = np.lexsort((-i if mutant == "tie_highest" else i, -v))
    take = k + 1 if mutant == "kth_slot_lost" else k
    order = order[:take]
    if mutant == "kth_slot_lost" and len(order) > k:
        order = np.delete(order, k - 1)  # the k-th entry is dropped, the next one moves up
    order = order[:k]
    ov = np.full(k, -np.inf, np.float32)
    oi = np.full(k, EMPTY, np.int32)
    ov[:len(order)], oi[:len(order)] = v[order], i[order]
    return ov, oi


class BankModel:
    """numpy restatement of the bank and its search with the padding, the chunking and the merge made explicit."""

    def __init__(self, H, capacity, mutant=None):
        self.H, self.capacity, self.mutant = H, capacity, mutant
        self.hpad = -(-H // 64) * 64
        self.mem = np.zeros((-(-capacity // TN) * TN, self.hpad), np.float32)  # the f16 rows, held as f32; zeroed at create
        self.count = 0
        self.high_water = 0

    def add(self, rows):
        rows = np.asarray(rows, np.float32)
        n = len(rows)
        if n > self.capacity - self.count:
            raise ValueError("bank full")
        first = self.count
        at = first - 1 if self.mutant == "second_add_offset_wrong" and first > 0 else first
        self.mem[at:at + n, :self.H] = mc.normalise_f16(rows).astype(np.float32)
        self.count += n
        self.high_water = max(self.high_water, self.count)
        return first

    def clear(self):
        self.count = 0  # the memory stays

    def topk(self, q, k, chunk_tiles=0):
        m = self.mutant
        q = np.asarray(q, np.float32)
        nq = len(q)
        count = self.high_water if m == "stale_rows_counted" else self.count
        chunk_tiles, nchunks, pass_tiles, ntiles = plan(nq, count, k, chunk_tiles)
        Q = np.zeros((-(-nq // TM) * TM, self.hpad), np.float32)
        Q[:nq, :self.H] = mc.normalise_f16(q).astype(np.float32)
        idx = np.empty((nq, k), np.int32)
        sim = np.empty((nq, k), np.float32)
        for r0 in range(0, len(Q), pass_tiles * TM):  # the passes over the queries
            r1 = min(r0 + pass_tiles * TM, nq)
            S = (Q[r0:r1] @ self.mem[:ntiles * TN].T).astype(np.float32) + np.float32(0.0)
            for r in range(r1 - r0):
                pv, pi = [], []
                for c in range(nchunks):  # one sorted list per chunk: the columns < count only
                    c0, c1 = c * chunk_tiles * TN, min((c + 1) * chunk_tiles, ntiles) * TN
                    if m != "pad_col_counted":
                        c1 = min(c1, count)
                    cols = np.arange(c0, c1, dtype=np.int32)
                    v, i = _first_k(S[r, c0:c1], cols, k, m)
                    pv.append(v)
                    pi.append(i)
                if m == "last_chunk_dropped" and nchunks > 1:
                    pv, pi = pv[:-1], pi[:-1]
                if m == "chunk_merge_duplicates_index" and nchunks > 1:
                    pv.append(pv[0][:1])
                    pi.append(pi[0][:1])
                v, i = _first_k(np.concatenate(pv), np.concatenate(pi), k, "tie_highest" if m == "tie_highest" else None)  # the merge
                if m == "list_not_sorted" and k > 1 and i[1] != EMPTY:
                    v[[0, 1]], i[[0, 1]] = v[[1, 0]], i[[1, 0]]
                empty = i == EMPTY
                if m == "short_bank_tail_garbage":
                    i[empty], v[empty] = 0, 0.0
                else:
                    i[empty], v[empty] = -1, -np.inf
                idx[r0 + r], sim[r0 + r] = i, v
        return {"idx": idx, "sim": sim}


def emulate(q, b, k, chunk_tiles=0, mutant=None):
    bank = BankModel(q.shape[1], len(b), mutant)
    bank.add(b)
    return bank.topk(q, k, chunk_tiles)


def expected_topk(S32, k):
    """Stable sort of -S (ties to the lowest index), the first k, the (-1, -inf) tail."""
    nq, nb = S32.shape
    order = np.argsort(-S32, axis=1, kind="stable")[:, :k].astype(np.int32)
    idx = np.full((nq, k), -1, np.int32)
    sim = np.full((nq, k), -np.inf, np.float32)
    idx[:, :order.shape[1]] = order
    sim[:, :order.shape[1]] = np.take_along_axis(S32, order, 1)
    return {"idx": idx, "sim": sim}


def probe_case(kind, H, k):
    """(q, b, expected) of an exact probe at k; `expected` bit for bit."""
    a, b, _ = mc.build_probe(kind, H)
    S = mc.reference(a, b)
    S32 = S.astype(np.float32)
    assert np.array_equal(S32.astype(np.float64), S), "probe similarities are not exact in f32"
    return a, b, expected_topk(S32 + np.float32(0.0), k)


# ------------------------------------------------------------------------------------------------------------------- checks
def check_against_reference(res, S, H, k, what, report=None):
    """The four per-row checks of the module docstring.  `report`: a list that receives the measured figures."""
    nq, nb = S.shape
    idx, sim = np.asarray(res["idx"]), np.asarray(res["sim"])
    if idx.shape != (nq, k) or sim.shape != (nq, k):
        return False, f"{what}: shapes {idx.shape} {sim.shape}, expected {(nq, k)}"
    real = min(k, nb)
    if not ((idx[:, real:] == -1).all() and np.isneginf(sim[:, real:]).all()):
        return False, f"{what}: slots {real} .. {k - 1} of a bank of {nb} rows must hold (-1, -inf)"
    idx, sim = idx[:, :real], sim[:, :real]
    if idx.min() < 0 or idx.max() >= nb:
        return False, f"{what}: idx outside [0, {nb}): min {idx.min()} max {idx.max()}"
    srt = np.sort(idx, 1)
    if real > 1 and (srt[:, 1:] == srt[:, :-1]).any():
        return False, f"{what}: row {int(np.flatnonzero((srt[:, 1:] == srt[:, :-1]).any(1))[0])} returns an index twice"
    if not np.isfinite(sim).all():
        return False, f"{what}: sim is not finite"
    t = mc.tol(H)
    at = np.take_along_axis(S, idx.astype(np.int64), 1)
    err = np.abs(sim.astype(np.float64) - at)
    ordered = (sim[:, :-1] > sim[:, 1:]) | ((sim[:, :-1] == sim[:, 1:]) & (idx[:, :-1] < idx[:, 1:]))
    out = np.ones(S.shape, bool)
    np.put_along_axis(out, idx.astype(np.int64), False, 1)
    excl = np.where(out, S, -np.inf).max(1)  # the best column NOT returned
    over = excl - at[:, -1]
    if report is not None:
        ref = np.argsort(-S, axis=1, kind="stable")[:, :real]
        differ = int((np.sort(ref, 1) != srt).any(1).sum())
        report.append(f"{what}: max |sim - S| {err.max():.3e} (tol {t:.3e}), best excluded over the k-th {over.max():.3e} (2 tol {2 * t:.3e}), "
                      f"{differ} of {nq} index sets differ from the reference's top-{real}")
    if err.max() > t:
        i, j = np.unravel_index(int(err.argmax()), err.shape)
        return False, f"{what}: row {i} slot {j}: sim {sim[i, j]!r} vs reference {at[i, j]!r} at index {idx[i, j]}: error {err[i, j]:.3e} > tol {t:.3e}"
    if not ordered.all():
        i, j = np.argwhere(~ordered)[0]
        return False, f"{what}: row {i}: slots {j}, {j + 1} = ({sim[i, j]!r}, {idx[i, j]}), ({sim[i, j + 1]!r}, {idx[i, j + 1]}) are out of order"
    if over.max() > 2 * t:
        i = int(over.argmax())
        return False, f"{what}: row {i}: a column left out has reference similarity {excl[i]!r}, the k-th returned {at[i, -1]!r}: over by {over[i]:.3e} > 2 tol"
    return True, ""


def check_exact(res, exp, what):
    """Both arrays bit for bit (similarities as their 32-bit patterns)."""
    for key in ("idx", "sim"):
        g, e = np.asarray(res[key]), np.asarray(exp[key])
        if g.shape != e.shape:
            return False, f"{what}: {key} has shape {g.shape}, expected {e.shape}"
        gb, eb = (g.astype(np.float32).view(np.uint32), e.astype(np.float32).view(np.uint32)) if key == "sim" else (g, e)
        if not np.array_equal(gb, eb):
            i = tuple(int(v) for v in np.argwhere(gb != eb)[0])
            return False, f"{what}: {key}{list(i)} = {g[i]!r}, expected {e[i]!r} ({int((gb != eb).sum())} of {g.size} differ)"
    return True, ""


# ------------------------------------------------------------------------------------------------------------------- scenario
def scenario_rows(H=72):
    """(queries a, rows b, first fill): the `negated` probe -- every similarity of a with b is negative -- and a first fill of 300 copies of
    the QUERIES: similarity 1 with them, so a stale row that is counted after the refill wins."""
    a, b, _ = mc.build_probe("negated", H)
    fill = np.concatenate([a, a, a])[:300]
    assert len(a) == len(b) == 133 and len(fill) == 300
    return a, b, fill


def scenario_failures(make_bank, k=5):
    """make_bank(H, capacity) -> object with add(rows) -> first, clear(), topk(q, k) -> dict, count.  The failure messages."""
    failures = []

    def note(ok_msg):
        if not ok_msg[0]:
            failures.append(ok_msg[1])

    a, b, fill = scenario_rows()
    H = a.shape[1]
    one, inc = make_bank(H, 300), make_bank(H, 300)
    if one.add(fill) != 0 or one.count != 300:
        failures.append("scenario: one add of 300 rows: first / count wrong")
    firsts = [inc.add(fill[:1]), inc.add(fill[1:131]), inc.add(fill[131:])]
    if firsts != [0, 1, 131] or inc.count != 300:
        failures.append(f"scenario: adds of 1, 130, 169 rows reported first = {firsts}, count = {inc.count}")
    S = mc.reference(a, fill).astype(np.float32) + np.float32(0.0)
    exp = expected_topk(S, k)
    note(check_exact(one.topk(a, k), exp, "scenario: one add"))
    note(check_exact(inc.topk(a, k), exp, "scenario: three adds"))
    try:
        inc.add(fill[:1])
        failures.append("scenario: a full bank accepted a row")
    except Exception:  # noqa: BLE001 (the model raises ValueError, the binding DinoError)
        pass
    if inc.count != 300:
        failures.append("scenario: a refused add changed the count")
    inc.clear()
    if inc.count != 0:
        failures.append("scenario: clear left a count")
    if inc.add(b) != 0 or inc.count != len(b):
        failures.append("scenario: refill after clear: first / count wrong")
    S = mc.reference(a, b).astype(np.float32) + np.float32(0.0)
    for kk in (k, K_MAX):
        note(check_exact(inc.topk(a, kk), expected_topk(S, kk), f"scenario: refill of {len(b)} rows after clear, k = {kk}"))
    return failures


# ------------------------------------------------------------------------------------------------------------------- resident views
def resident_view(fin, R, source, image=0, mutant=None):
    B, T, H = fin.shape
    if source == "last_cls":
        if mutant == "resident_cls_stride_wrong":
            return fin.reshape(B * T, H)[:B]  # row stride H where it is T H
        return fin[:, 0]
    return mc.resident_rows(fin, R, image)


def resident_failures(mutant=None, k=5):
    fin, R = mc.resident_stream()
    B, T, H = fin.shape
    P = T - 1 - R
    bank = BankModel(H, B + P, mutant)
    firsts = [bank.add(resident_view(fin, R, "last_cls", mutant=mutant)), bank.add(resident_view(fin, R, "last_patches", 0, mutant))]
    rows = np.concatenate([fin[:, 0], fin[0, 1 + R:]])
    failures = [] if firsts == [0, B] and bank.count == B + P else [f"resident: first = {firsts}, count = {bank.count}"]
    for src, img in (("last_patches", 1), ("last_cls", 0)):
        q_true = resident_view(fin, R, src, img)
        exp = emulate(q_true, rows, k)
        ok, msg = check_exact(bank.topk(resident_view(fin, R, src, img, mutant), k), exp, f"resident: {src} queries")
        if not ok:
            failures.append(msg)
    return failures


# ------------------------------------------------------------------------------------------------------------------- everything
def kernel_failures(topk_fn):
    """Every shape, probe and chunking case through topk_fn(q, b, k, chunk_tiles) -> {"idx", "sim"}; the failure messages."""
    failures = []

    def note(ok_msg):
        if not ok_msg[0]:
            failures.append(ok_msg[1])

    for shape in SHAPES:
        q, b = shape_inputs(shape)
        note(check_against_reference(topk_fn(q, b, shape[3], 0), mc.reference(q, b), shape[2], shape[3], "shape " + shape_id(shape)))
    for kind, H in PROBES:
        for k in PROBE_KS:
            q, b, exp = probe_case(kind, H, k)
            note(check_exact(topk_fn(q, b, k, 0), exp, f"probe {kind} H={H} k={k}"))
    q, b, exp = probe_case("duplicates", 72, 64)
    for ct in CHUNKINGS[1:]:
        note(check_exact(topk_fn(q, b, 64, ct), exp, f"probe duplicates H=72 k=64 chunk_tiles={ct}"))
    return failures
