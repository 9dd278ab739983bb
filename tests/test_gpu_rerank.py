"""dinov2_hip_bank_rerank on the GPU (csrc/rerank.hip; contract in include/dinov2_hip.h): row ranges of a bank scored against one query set.
Exact probes against a float64 brute force, Gaussian rows against the match path, the independence of a segment from its neighbours, its
place in the list and the cut into passes, and the session call on the tiny golden model with its refusals."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import match_cases as mc

pytestmark = pytest.mark.gpu

KEYS = ("score_q", "score_b", "mutual", "mutual_sim")
NB = 128 * 3 + 5
# tile edges of an unaligned range: one row; one tile at and off a tile boundary; one row into a second tile; three tiles off a boundary;
# the range that ends at the bank's last row off a boundary (its last tile reaches past the allocation) and that row alone; one range
# twice; two that overlap
SEGMENTS = [(0, 1), (0, 128), (1, 128), (127, 129), (3, 2 * 128 + 5), (130, NB - 130), (NB - 1, 1), (127, 129), (100, 150), (200, 100)]


def _bits(x):
    x = np.asarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


@functools.lru_cache(maxsize=None)
def probe(H, nq):
    """(q, b): rows of +-1 in 1, 4, 16 or 64 positions (at H = 8: 1 or 4), which normalise to +-2^-k exactly, so every similarity is a
    multiple of 2^-6 and every sum of a few hundred of them is exact in f32 in any order.  Planted: copies of q[0] in every column tile of
    the bank (ties go to the lowest column), a negated copy, a zero bank row; copies of b[7] on both sides of the query tile boundary (ties
    go to the lowest row) and a zero query row, where nq has room."""
    rng = np.random.default_rng(1000 * H + nq)
    if H >= 64:
        q, b = mc._pm1_rows(rng, nq, H), mc._pm1_rows(rng, NB, H)
    else:
        q, b = np.zeros((nq, H), np.float32), np.zeros((NB, H), np.float32)
        for x in (q, b):
            for row in x:
                k = (1, 4)[int(rng.integers(2))]
                row[rng.choice(H, k, replace=False)] = rng.choice([-1.0, 1.0], k)
    b[[5, 127, 128, 200, 260, 386]] = q[0]
    b[300] = -q[0]
    b[[9, NB - 1]] = 0.0
    if nq > 4:
        q[1] = 0.0
        q[[2, nq - 2]] = b[7]
    return q, b


def brute(q, b, segments, min_sim):
    """The contract in float64: cosine matrix, first maximum per row and column within the range, the four definitions."""
    S = mc.reference(q, b) + 0.0
    out = {k: [] for k in KEYS}
    for first, ln in segments:
        M = S[:, first:first + ln]
        iq, ib = M.argmax(1), M.argmax(0)
        sq, sb = M[np.arange(len(q)), iq], M[ib, np.arange(ln)]
        mutual = (ib[iq] == np.arange(len(q))) & (sq >= min_sim)
        for k, v in zip(KEYS, (sq.sum(), sb.sum(), int(mutual.sum()), sq[mutual].sum())):
            out[k].append(v)
    return out


@pytest.mark.parametrize("min_sim", [-np.inf, 0.5], ids=["all", "min0.5"])
@pytest.mark.parametrize("nq", [1, 128, 131])
@pytest.mark.parametrize("H", [8, 72, 384])
def test_exact_probes_bit_for_bit(api, H, nq, min_sim):
    q, b = probe(H, nq)
    exp = brute(q, b, SEGMENTS, min_sim)
    if min_sim > -np.inf:  # the threshold splits the mutual pairs
        assert exp["mutual"] != brute(q, b, SEGMENTS, -np.inf)["mutual"]
    got = api.op_bank_rerank(q, b, SEGMENTS, min_sim)
    for k in KEYS:
        e = np.asarray(exp[k], np.float64)
        assert np.array_equal(e.astype(got[k].dtype).astype(np.float64), e), k  # the expectation is exact in the output's type
        assert np.array_equal(_bits(got[k]), _bits(e.astype(got[k].dtype))), (k, got[k], e)


def test_gaussian_rows_against_match(api):
    """Per segment, op_match(q, the segment's rows) gives the four arrays: `mutual` is the count derived from them, exactly; the three sums
    lie within m 2^-24 sum|terms| of the float64 sum of match's f32 values (m terms: the bound of sequential f32 summation, so any fixed
    order passes) and within m tol(H) of the float64 cosine reference of the un-rounded inputs.  (Whether a pair is mutual is a
    discontinuous question: the seed is one at which match_cases.emulate, the numpy restatement of the f16 path, and the float64 reference
    name the same pairs in all five segments -- at seeds 31 and 41 a near tie flips one pair of one segment.)"""
    nq, H = 300, 384
    q, b = mc.gaussian_tokens(nq, H, 51), mc.gaussian_tokens(1500, H, 52)
    segments = [(0, 300), (290, 137), (427, 512), (939, 1), (1100, 400)]
    got = api.op_bank_rerank(q, b, segments)
    ref = brute(q, b, segments, -np.inf)
    for s, (first, ln) in enumerate(segments):
        m = api.op_match(q, b[first:first + ln])
        mutual = m["idx_ba"][m["idx_ab"]] == np.arange(nq)
        assert got["mutual"][s] == mutual.sum(), s
        for k, terms in (("score_q", m["sim_ab"]), ("score_b", m["sim_ba"]), ("mutual_sim", m["sim_ab"][mutual])):
            t = terms.astype(np.float64)
            print(s, k, got[k][s], abs(got[k][s] - t.sum()), len(t) * 2.0 ** -24 * np.abs(t).sum(), abs(got[k][s] - ref[k][s]), len(t) * mc.tol(H))
            assert abs(got[k][s] - t.sum()) <= len(t) * 2.0 ** -24 * np.abs(t).sum(), (s, k)
            assert abs(got[k][s] - ref[k][s]) <= len(t) * mc.tol(H), (s, k)


def test_a_segment_does_not_depend_on_its_place_its_neighbours_or_the_passes(api):
    q, b = probe(72, 131)
    base = api.op_bank_rerank(q, b, SEGMENTS, 0.5)
    perm = np.random.default_rng(3).permutation(len(SEGMENTS))
    assert api.op_rerank_plan(131, 72, [s[1] for s in SEGMENTS], pass_bytes=1)["npass"] == len(SEGMENTS)
    runs = {"permuted": (api.op_bank_rerank(q, b, [SEGMENTS[i] for i in perm], 0.5), perm),
            "one pass each": (api.op_bank_rerank(q, b, SEGMENTS, 0.5, pass_bytes=1), np.arange(len(SEGMENTS)))}
    for i, seg in enumerate(SEGMENTS):
        runs["alone %d" % i] = (api.op_bank_rerank(q, b, [seg], 0.5), np.array([i]))
    for name, (got, order) in runs.items():
        for k in KEYS:
            assert np.array_equal(_bits(got[k]), _bits(base[k][order])), (name, k)


# ------------------------------------------------------------------------------------------------------------------- the session call
@pytest.fixture(scope="module")
def golden(api, golden_dir):
    model = api.Model(os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), classify=True)
    img = np.random.default_rng(17).standard_normal((2, 3, 84, 112)).astype(np.float32)
    return model, img


def test_resident_rows_equal_the_fetched_tokens(api, golden):
    model, img = golden
    sess = api.Session(model)
    tok = sess.predict(img, classify=False, want=("patch_tokens",))["patch_tokens"]
    P, H = tok.shape[1:]
    bank = api.Bank(model, H, 2 * P)
    segments = [(bank.add(sess, source="last_patches", image=i), P) for i in (0, 1)]
    assert segments == [(0, P), (P, P)]
    got = bank.rerank(sess, source="last_patches", image=0, segments=segments)
    exp = api.op_bank_rerank(tok[0], tok.reshape(2 * P, H), segments)
    for k in KEYS:
        assert np.array_equal(_bits(got[k]), _bits(exp[k])), (k, got[k], exp[k])
    assert got["mutual"][0] == P  # every token of image 0 is its own mutual nearest neighbour
    host = bank.rerank(sess, tok[0], segments)
    for k in KEYS:
        assert np.array_equal(_bits(host[k]), _bits(got[k])), k
    bank.free()


REFUSALS = {
    "null session": dict(null_session=True), "null bank": dict(null_bank=True), "null request": dict(null_request=True),
    "empty bank": dict(empty=True), "n = 0": dict(n=0), "n = 16 385": dict(n=16385), "H is not the bank's": dict(H=16),
    "GIVEN without data": dict(no_data=True), "unknown source": dict(source=3), "resident source, no forward yet": dict(source=2),
    "n_seg = 0": dict(n_seg=0), "n_seg = 65 537": dict(n_seg=65537), "len = 0": dict(len=[0, 2]), "len = 16 385": dict(len=[16385, 2]),
    "first < 0": dict(first=[-1, 0]), "range past count": dict(first=[0, 3], len=[4, 2]), "null first": dict(null_first=True),
    "null len": dict(null_len=True), "NaN min_sim": dict(min_sim=np.nan), "no outputs": dict(no_outputs=True),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusals_return_invalid_and_touch_nothing(api, golden, name):
    kw = REFUSALS[name]
    model, _ = golden
    sess, bank = api.Session(model), api.Bank(model, 8, 6)
    x = np.ones((4, 8), np.float32)
    if not kw.get("empty"):
        assert bank.add(sess, x) == 0
    first, ln = np.array(kw.get("first", [0, 2]), np.int32), np.array(kw.get("len", [4, 2]), np.int32)
    outs = [np.full(2, -7, dt) for dt in (np.float32, np.float32, np.int32, np.float32)]
    rows = api.Rows(kw.get("source", 0), None if kw.get("no_data") else x.ctypes.data, kw.get("n", 4), kw.get("H", 8), 0, 0)
    r = api.Rerank(rows, kw.get("n_seg", 2), None if kw.get("null_first") else first.ctypes.data, None if kw.get("null_len") else ln.ctypes.data,
                   kw.get("min_sim", -np.inf), *[None if kw.get("no_outputs") else o.ctypes.data for o in outs])
    err = C.create_string_buffer(256)
    rc = api.lib().dinov2_hip_bank_rerank(None if kw.get("null_session") else sess._h, None if kw.get("null_bank") else bank._h,
                                          None if kw.get("null_request") else C.byref(r), err, len(err))
    assert rc == 4 and all((o == -7).all() for o in outs), (name, rc, err.value.decode())
    bank.free()
