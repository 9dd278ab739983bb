"""Cases for dinov2_hip_bank_topk_probe / dinov2_hip_op_bank_probe (csrc/probe.hip), shared by tests/test_probe_probes.py (CPU: the planner,
the refusals) and tests/test_gpu_probe.py (the kernels and the session call).

Contract under test (include/dinov2_hip.h): per query the first k rows of the union of its probed segments in bank_topk's strict total
order, under their bank rows, with the (-1, -inf) tail; the bits of bank_topk; independent of the queries that travel along, of the slot
order and of every cut the planner makes."""
import functools

import numpy as np

import match_cases as mc

NB = 389
SEGMENTS = [(0, 1), (1, 127), (128, 128), (256, 129), (385, 4)]  # lengths 1, 127, 128, 129, 4: at, below and across the tile edges
HS, KS, FORMS = (8, 40, 64, 136), (1, 5, 64), ("wide", "narrow", "auto")
PARTIAL_MAX = 32 << 20


@functools.lru_cache(maxsize=None)
def rows(kind, H, nq):
    """(q, b).  "gauss": Gaussian tokens.  "pm1": +-1 in 1, 4, 16 or 64 positions (those that fit H), which normalise to +-2^-j exactly, so
    every similarity is exact in f32 in any order and full of ties; copies of q[0] in four segments, a negated copy and a zero row."""
    if kind == "gauss":
        return mc.gaussian_tokens(nq, H, 700 + nq + H), mc.gaussian_tokens(NB, H, 800 + H)
    rng = np.random.default_rng(1000 * H + nq)
    counts = [c for c in (1, 4, 16, 64) if c <= H]
    q, b = np.zeros((nq, H), np.float32), np.zeros((NB, H), np.float32)
    for x in (q, b):
        for row in x:
            c = counts[int(rng.integers(len(counts)))]
            row[rng.choice(H, c, replace=False)] = rng.choice([-1.0, 1.0], c)
    b[[0, 5, 127, 128, 260, 386]] = q[0]
    b[300] = -q[0]
    b[9] = 0.0
    return q, b


def all_probes(nq, seed=0):
    """Every query probes all five segments, each in a slot order of its own."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(len(SEGMENTS)) for _ in range(nq)]).astype(np.int32)


def subset_probes(nq, n_probe=3, seed=1):
    """0 .. n_probe distinct segments per query at random slots, the rest -1; query 0 probes nothing."""
    rng = np.random.default_rng(seed)
    p = np.full((nq, n_probe), -1, np.int32)
    for i in range(1, nq):
        m = int(rng.integers(n_probe + 1))
        p[i, rng.choice(n_probe, m, replace=False)] = rng.choice(len(SEGMENTS), m, replace=False)
    return p


def brute(q, b, segments, probes, k):
    """float64: the cosine matrix, per query a stable sort of the columns of its probed segments (ties to the lowest bank row)."""
    S = mc.reference(q, b) + 0.0
    idx, sim = np.full((len(q), k), -1, np.int32), np.full((len(q), k), -np.inf, np.float32)
    for i, pr in enumerate(np.asarray(probes)):
        cols = np.sort(np.concatenate([np.arange(segments[s][0], sum(segments[s])) for s in pr if s >= 0] + [np.zeros(0, np.int64)])).astype(np.int64)
        best = cols[np.argsort(-S[i, cols], kind="stable")[:k]]
        idx[i, :len(best)], sim[i, :len(best)] = best, S[i, best]
        assert np.array_equal(sim[i, :len(best)].astype(np.float64), S[i, best]), "the expectation is not exact in f32"
    return {"idx": idx, "sim": sim}


def same_bits(got, exp):
    return np.array_equal(got["idx"], exp["idx"]) and np.array_equal(got["sim"].view(np.uint32), exp["sim"].view(np.uint32))


def plan_failures(plan, nq, segments, probes, k, pass_bytes, force_form):
    """The work table against a brute-force inversion of the probe table: every (query, probed segment) pair is covered by exactly one item
    per piece and the pieces tile the segment; the destinations of a pass are distinct lists of the right query; the passes are runs of
    queries within the bound (or a single query); the forms keep their widths."""
    fails = []
    passes, items, table = plan["passes"], plan["items"], plan["rows"]
    piece = plan["piece_tiles"] * 128
    if not (np.array_equal(passes[:, 0], np.cumsum(passes[:, 1]) - passes[:, 1]) and passes[:, 1].sum() == nq and (passes[:, 1] >= 1).all()):
        fails.append("the passes are not consecutive runs of all queries")
    bound = min(pass_bytes or PARTIAL_MAX, PARTIAL_MAX)
    lists = passes[:, 1].astype(np.int64) * passes[:, 2]
    if not ((lists * k * 8 <= bound) | (passes[:, 1] == 1)).all() or lists.max() * k * 8 != plan["partial_bytes"]:
        fails.append("a pass of several queries is over the bound, or partial_bytes is not the largest pass")
    seg_of = {first: s for s, (first, _) in enumerate(segments)}
    covered, taken = {}, [[] for _ in passes]
    for ps, row0, nrows, n_q, form, t0 in items:
        s = max(f for f in seg_of if f <= row0)
        first, ln = segments[seg_of[s]]
        if (row0 - first) % piece or nrows != min(piece, first + ln - row0):
            fails.append(f"item at row {row0}: not a piece of segment {seg_of[s]}")
        if not 1 <= n_q <= (16 if form == 2 else 128) or form != {"auto": form, "wide": 1, "narrow": 2}[force_form]:
            fails.append(f"item at row {row0}: {n_q} queries in form {form}")
        q0, pn, slots = passes[ps]
        for qq, dst in table[t0:t0 + n_q]:
            covered.setdefault((int(qq), seg_of[s]), []).append(int(row0))
            taken[ps].append(int(dst))
            if not (q0 <= qq < q0 + pn and dst % pn == qq - q0 and dst // pn < slots):
                fails.append(f"query {qq}: list {dst} is not one of its slots in pass {ps}")
    if any(len(set(t)) != len(t) for t in taken) or sum(len(t) for t in taken) != len(table):
        fails.append("two item rows of a pass share a list, or the row table holds rows of no item")
    want = {(i, int(s)): list(range(segments[s][0], sum(segments[s]), piece)) for i, pr in enumerate(probes) for s in pr if s >= 0}
    if {key: sorted(v) for key, v in covered.items()} != want:
        fails.append("the items do not cover every (query, probed segment) pair exactly once per piece")
    return fails
