"""dinov2_hip_match_tokens, dinov2_hip_bank_add / _topk and dinov2_hip_kmeans_tokens at the far end of their row offsets (cases and exact
expectations: tests/rows_far_cases.py; CPU probes: tests/test_rows_far_probes.py).

The entry points take up to 2^20 rows a side (match, k-means, the queries of a search) and 2^24 bank rows at H <= 4096: f32 sources of 16 GiB,
f16 operands of 8 GiB, row offsets past 2^31, 2^32 and 2^33 bytes.  Here they RUN there, through the public calls on a session of the tiny
golden model, on device-resident rows that dinov2_hip_op_rows_fill writes from a small dictionary (nothing far is built on, or copied from,
the host), and EVERY output is compared bit for bit: each far row's match / label / sim / top-k list, each list of the other side, counts and
centres.  Afterwards a sample of the far source rows is read back and compared with the dictionary and with a second rows_fill (the calls
must not write to their inputs), and a small call on the same session must give a fresh session's bits (the grown scratch must not leak).

Each test prints "rows_far: <case> ..." with the times of the fill and of each call, the wall time and the peak device bytes
(profiles/rows_far.md holds the figures of a run) and skips only when the device has less memory free than the case needs plus 2 GiB."""
import os
import time

import numpy as np
import pytest

import bank_cases as bc
import kmeans_cases as kc
import match_cases as mc
import rows_far_cases as rc

pytestmark = pytest.mark.gpu

GIB = float(1 << 30)


@pytest.fixture(scope="module")
def model(api, golden_dir):
    return api.Model(os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), classify=True)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _need(api, c):
    free, _ = api.device_memory()
    need = c.device_bytes() + (2 << 30)
    if free < need:
        pytest.skip("%s needs %.1f GiB of device memory (the case's %.1f GiB plus 2 GiB), %.1f GiB are free"
                    % (c.name, need / GIB, c.device_bytes() / GIB, free / GIB))
    return free


class _Clock:
    """The times of a case's steps, printed in one line."""

    def __init__(self, api, c, free0):
        self.api, self.c, self.free0, self.t0, self.steps, self.low = api, c, free0, time.perf_counter(), [], free0

    def step(self, name, fn):
        t = time.perf_counter()
        out = fn()
        self.steps.append("%s %.3f s" % (name, time.perf_counter() - t))
        self.low = min(self.low, self.api.device_memory()[0])
        return out

    def report(self):
        print("rows_far: %s wall %.2f s peak %.2f GiB; %s"
              % (self.c.name, time.perf_counter() - self.t0, (self.free0 - self.low) / GIB, "; ".join(self.steps)))


def _view(api, d, n):
    """The first n rows of DeviceArray d as a DeviceArray that owns nothing."""
    class View(api.DeviceArray):
        def __init__(self):
            pass

        def free(self):
            self.ptr = 0

    v = View()
    v.shape, v.nbytes, v.device, v.ptr = (int(n), d.shape[1]), 4 * int(n) * d.shape[1], d.device, d.ptr
    return v


def _fill(api, c, dic, dst, row0, n):
    api.op_rows_fill(dst, row0, n, dic, rc.D_COMMON, rc.SEED, c.plant_list)


def _source_unchanged(api, c, dic, ent, buf, segments):
    """segments: [(first row of buf, the operand row it holds, rows)] that buf is known to hold.  Blocks of up to 128 rows at the start and the
    end of every segment and around every planted row inside it are copied out of the far buffer and compared, bit for bit, with the
    dictionary rows of their entries and with what a second rows_fill writes into a small buffer."""
    H = c.H
    small, again = api.DeviceArray((128, H), fill_nan=True), api.DeviceArray((128, H), fill_nan=True)
    st = api.Stream()
    checked = 0
    for b0, g0, cnt in segments:
        starts = {0, max(cnt - 128, 0)} | {max(min(r - g0 - 64, cnt - 128), 0) for r in c.plant_rows if g0 <= r < g0 + cnt}
        for s in sorted(starts):
            m = min(128, cnt - s)
            st.copy(small.ptr, buf.ptr + (b0 + s) * H * 4, m * H * 4)
            st.synchronize()
            _fill(api, c, dic, again, g0 + s, m)
            got, re = small.to_host()[:m], again.to_host()[:m]
            exp = dic[ent[g0 + s:g0 + s + m]]
            assert np.array_equal(_bits(got), _bits(exp)), (c.name, "far source rows changed", g0 + s)
            assert np.array_equal(_bits(re), _bits(exp)), (c.name, "rows_fill is not repeatable", g0 + s)
            checked += m
    st.destroy()
    small.free()
    again.free()
    assert checked >= 128 or c.n < 128


def _same(got, exp, keys, what):
    for k in keys:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        assert g.shape == e.shape, (what, k, g.shape, e.shape)
        same = (_bits(g) == _bits(e)) if e.dtype == np.float32 else (g == e)
        if not same.all():
            bad = np.argwhere(~same)
            i = tuple(int(x) for x in bad[0])
            raise AssertionError("%s: %s differs at %d places, first at %s: got %r, expected %r" % (what, k, len(bad), i, g[i], e[i]))


# ------------------------------------------------------------------------------------------------------------- match
@pytest.mark.parametrize("name", ["M0", "M1", "M2"])
def test_match_at_the_far_end(api, model, name):
    """M0: both sides one row longer than a pass (the first-flags of both reduces in launch_match's double loop), host arrays.  M1: the f16 A
    just past 2^32 bytes and its f32 source past 2^33.  M2: the B side at the interface limit with H % 4 != 0 (the scalar-load normaliser) and
    the column-direction reduce over 64 passes.  All four result arrays, every element, bit for bit."""
    c = rc.BY_NAME[name]
    dic, ent = c.dictionary(), c.entries()
    other = rc.small_rows(c, dic)
    e = rc.expected_match(rc.exact_sims(dic, other), ent)
    exp = dict(zip(rc.match_result_keys(c.far), (e["idx_far"], e["sim_far"], e["idx_other"], e["sim_other"])))
    planted = np.array(c.plant_rows)
    assert (e["sim_far"][planted] == 1.0).all() and set(planted) <= set(e["idx_other"].tolist())  # the planted rows are found, at exactly 1
    if c.host:
        got = api.op_match(dic[ent], other)
        _same(got, exp, mc.KEYS, name)
        return
    clock = _Clock(api, c, _need(api, c))
    sess = api.Session(model)
    far = api.DeviceArray((c.n, c.H))
    small = api.DeviceArray.from_host(other)
    try:
        clock.step("fill", lambda: _fill(api, c, dic, far, 0, c.n))
        a, b = (far, small) if c.far == "a" else (small, far)
        got = clock.step("match", lambda: sess.match(a, b))
        _same(got, exp, mc.KEYS, name)
        _source_unchanged(api, c, dic, ent, far, [(0, 0, c.n)])
        with pytest.raises(api.DinoError):  # one more row than the interface takes (refused before anything is read)
            big = _view(api, far, rc.MATCH_N_MAX + 1)
            sess.match(big, small) if c.far == "a" else sess.match(small, big)
        # a small call on the grown scratch gives a fresh session's bits
        xa, xb = mc.shape_inputs((mc.TM + 1, 2 * mc.TN + 1, 384))
        _same(sess.match(xa, xb), api.Session(model).match(xa, xb), mc.KEYS, name + " small call afterwards")
        clock.report()
    finally:
        far.free()
        small.free()
        sess.close()


# ------------------------------------------------------------------------------------------------------------- bank
def _small_bank_call(api, model, sess, what):
    """A small bank and search on `sess` against the same on a fresh session: bit for bit."""
    q, b = bc.shape_inputs((129, 257, 384, 64))
    out = []
    for s in (sess, api.Session(model)):
        bank = api.Bank(model, 384, 300)
        assert bank.add(s, b) == 0
        out.append(bank.topk(s, q, 64))
        bank.close()
    _same(out[0], out[1], ("idx", "sim"), what + " small call afterwards")


@pytest.mark.parametrize("name", ["B1", "B2"])
def test_bank_far_rows(api, model, name):
    """B1: capacity = count = 2^24, the row index at the interface limit, the f16 bank past 2^32 bytes, filled by adds of 2^23, 2^23 - 1 and 1
    rows from one reused source buffer (bank_add's destination rows + count * hpad at a far count), searched with k = 1 and 64: indices beyond
    2^23 are in the lists.  B2: wide rows past 2^32 bytes, two query tiles.  Every list bit for bit: the planted far rows first (similarity
    exactly 1), then the lowest rows of the best common entries -- thousands of equal values decided by index across tiles, chunks and merges."""
    c = rc.BY_NAME[name]
    dic, ent = c.dictionary(), c.entries()
    queries = rc.small_rows(c, dic)
    S = rc.exact_sims(dic, queries)
    clock = _Clock(api, c, _need(api, c))
    sess = api.Session(model)
    bank = api.Bank(model, c.H, c.n)
    src = api.DeviceArray((max(c.adds), c.H))
    q = api.DeviceArray.from_host(queries)
    try:
        at, held = 0, []
        for i, a in enumerate(c.adds):
            clock.step("fill %d" % i, lambda: _fill(api, c, dic, src, at, a))
            first = clock.step("add %d" % i, lambda: bank.add(sess, _view(api, src, a)))
            assert first == at and bank.count == at + a
            held = [(0, at, a)] + [(b0 + a, g0 + a, n - a) for b0, g0, n in held if n > a][:1]
            at += a
        assert bank.count == c.n == bank.capacity
        with pytest.raises(api.DinoError):
            bank.add(sess, _view(api, src, 1))  # full
        for k in c.ks:
            exp = rc.expected_topk_far_bank(S, ent, k)
            got = clock.step("topk k=%d" % k, lambda: bank.topk(sess, q, k))
            _same(got, exp, ("idx", "sim"), "%s k=%d" % (name, k))
            if k == 64:  # every planted row is in the list of its rare entry; B1: indices beyond 2^23, the last row of the bank among them
                assert name != "B1" or (exp["idx"].max() == c.n - 1 and (exp["idx"] > 1 << 23).sum() >= 8)
                assert set(c.plant_rows) <= set(exp["idx"][:c.n_rare].ravel().tolist())
        _source_unchanged(api, c, dic, ent, src, held)
        with pytest.raises(api.DinoError):
            api.Bank(model, c.H, rc.BANK_CAP_MAX + 1)
        _small_bank_call(api, model, sess, name)
        clock.report()
    finally:
        src.free()
        q.free()
        bank.close()
        sess.close()


def test_bank_far_queries(api, model):
    """B3: 2^20 queries, the interface limit, against 300 bank rows: the f16 query operand of 8 GiB and the per-pass output offsets idx + r0 * k
    over 256 passes.  A query's list depends on its entry alone; all 2^20 lists bit for bit."""
    c = rc.BY_NAME["B3"]
    dic, ent = c.dictionary(), c.entries()
    rows = rc.small_rows(c, dic)
    k = c.ks[0]
    exp = rc.expected_topk_far_queries(rc.exact_sims(dic, rows), ent, k)
    clock = _Clock(api, c, _need(api, c))
    sess = api.Session(model)
    bank = api.Bank(model, c.H, c.small)
    far = api.DeviceArray((c.n, c.H))
    try:
        assert bank.add(sess, rows) == 0
        clock.step("fill", lambda: _fill(api, c, dic, far, 0, c.n))
        got = clock.step("topk k=%d" % k, lambda: bank.topk(sess, far, k))
        _same(got, exp, ("idx", "sim"), "B3")
        planted = np.array(c.plant_rows)
        assert (got["sim"][planted, 0] == 1.0).all() and len(set(got["idx"][planted, 0].tolist())) == len(planted)
        _source_unchanged(api, c, dic, ent, far, [(0, 0, c.n)])
        with pytest.raises(api.DinoError):
            bank.topk(sess, _view(api, far, rc.BANK_NQ_MAX + 1), k)
        _small_bank_call(api, model, sess, "B3")
        clock.report()
    finally:
        far.free()
        bank.close()
        sess.close()


# ------------------------------------------------------------------------------------------------------------- k-means
@pytest.mark.parametrize("name", ["K1", "K2"])
def test_kmeans_at_the_far_end(api, model, name):
    """K1: x16 and XT just past 2^32 bytes, two centre tiles.  K2: n at the interface limit, H % 4 != 0.  Given init centres that are
    dictionary entries (the last repeats the first: an empty cluster), max_iter = 0, 1 and 2 on the same rows:
    max_iter = 0 is the first assignment -- labels and sim of every row against the exact similarities; max_iter = 1 returns the first
    update's centres -- counts and sums bit for bit whatever nsplit the planner picked, the empty cluster's vector kept -- and the second
    assignment, whose centres are no longer dyadic: its expectation is the assignment kernel on the DICTIONARY alone, gathered through the
    rows' entries (a pair's bits depend on hpad alone: sim_tile.h); max_iter = 2 goes one update further.  iterations, converged and the
    final counts follow contract 5."""
    c = rc.BY_NAME[name]
    dic, ent = c.dictionary(), c.entries()
    init = rc.small_rows(c, dic)
    K = c.small
    clock = _Clock(api, c, _need(api, c))
    sess = api.Session(model)
    far = api.DeviceArray((c.n, c.H))
    keys = ("labels", "sim", "centers", "counts")
    try:
        clock.step("fill", lambda: _fill(api, c, dic, far, 0, c.n))
        for mi in (0, 1, 2):
            exp = rc.expected_kmeans(dic, ent, init, mi, api.op_kmeans_assign)
            got = clock.step("kmeans max_iter=%d" % mi, lambda: sess.kmeans(far, K=K, max_iter=mi, init=init))
            _same(got, exp, keys, "%s max_iter=%d" % (name, mi))
            assert (int(got["iterations"]), bool(got["converged"])) == (exp["iterations"], exp["converged"]), (name, mi)
            if mi == 0:  # the first assignment against the exact similarities, not against another run of the kernel
                ex = rc.exact_assign(dic, init)
                _same(got, {"labels": ex["labels"][ent], "sim": ex["sim"][ent], "centers": init}, keys[:3], name + " first assignment")
            else:
                assert exp["iterations"] == mi and got["counts"].sum() == c.n
                assert np.bincount(exp["first"]["labels"], minlength=K)[-1] == 0
            if mi == 1:
                assert np.array_equal(_bits(got["centers"][-1]), _bits(init[-1]))  # the empty cluster kept its vector
        _source_unchanged(api, c, dic, ent, far, [(0, 0, c.n)])
        with pytest.raises(api.DinoError):
            sess.kmeans(_view(api, far, rc.KMEANS_N_MAX + 1), K=K, max_iter=0, init=init)
        x, cen = kc.shape_inputs((257, 300, 1536))
        small = [s.kmeans(x, K=300, max_iter=2, init=cen) for s in (sess, api.Session(model))]
        _same(small[0], small[1], keys, name + " small call afterwards")
        clock.report()
    finally:
        far.free()
        sess.close()
