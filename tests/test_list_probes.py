"""CPU probes of dinov2_hip_predict_list: the plan op against its numpy restatement, the structure of every plan (items cover each
(image, head, query block) once and in order, runs partition the images, row ranges partition [0, M)), the list emulation and its planted
mutants, and the argument errors that need no device.  No GPU.  (dinov2_hip_list_rows needs a loaded model, which needs a device: it is held
to the plan in tests/test_gpu_predict_list.py.  That the header declares what the library exports is test_library_exports_every_declared_symbol's.)
"""
import ctypes as C

import numpy as np
import pytest

import attention_cases as ac
import list_cases as lc


def _random_cases():
    rng = np.random.default_rng(20260119)
    for _ in range(200):
        n = int(rng.integers(1, 13))
        yield lc.random_sizes(rng, n), int(rng.choice([1, 7, 14, 16])), int(rng.integers(0, 5)), int(rng.choice([1, 2, 6, 16])), int(rng.integers(0, 2))


def _named_cases():
    for sizes in lc.LISTS.values():
        for R in (0, 4):
            for order in (0, 1):
                yield sizes, lc.PATCH, R, 2, order


def _same(got, want):
    for k in ("images", "runs", "items"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    for k in ("M", "P", "pixels", "units"):
        assert got[k] == want[k], k


def test_plan_op_equals_restatement(api):
    cases = list(_named_cases()) + list(_random_cases())
    assert len(cases) >= 220
    for sizes, patch, R, nh, order in cases:
        _same(api.list_plan(sizes, patch, R, nh, order), lc.plan(sizes, patch, R, nh, order))


def test_token_counts_of_the_named_sizes():
    sizes = [lc.S14, lc.S14x70, lc.S70, lc.S112x126, lc.S154, lc.S154x168, lc.S224]
    assert [lc.tokens(s, 4) for s in sizes] == [6, 10, 30, 77, 126, 137, 261]
    assert [lc.tokens(s, 0) for s in sizes] == [2, 6, 26, 73, 122, 133, 257]


def test_plan_structure(api):
    for sizes, patch, R, nh, order in list(_named_cases()) + list(_random_cases()):
        p = api.list_plan(sizes, patch, R, nh, order)
        im, runs, items = p["images"], p["runs"], p["items"]
        n = len(sizes)
        # row ranges partition [0, M)
        assert im[0, 0] == 0 and np.array_equal(im[1:, 0], (im[:, 0] + im[:, 1])[:-1]) and im[-1, 0] + im[-1, 1] == p["M"]
        assert np.array_equal(im[:, 1], 1 + R + im[:, 2]) and np.array_equal(im[:, 2], im[:, 3] * im[:, 4])
        # runs partition the images, each run one size, neighbouring runs different sizes
        assert runs[0, 0] == 0 and np.array_equal(runs[1:, 0], (runs[:, 0] + runs[:, 1])[:-1]) and runs[-1, 0] + runs[-1, 1] == n
        for k, (f, c) in enumerate(runs):
            assert c >= 1 and all(tuple(sizes[i]) == tuple(sizes[f]) for i in range(f, f + c))
            assert k == 0 or tuple(sizes[f]) != tuple(sizes[f - 1])
        # the items cover every (image, head, query block) exactly once, image-major, then head, then query block
        walk = sorted(range(n), key=lambda i: -im[i, 1]) if order == 1 else range(n)
        want = [(im[i, 0], im[i, 1], h, qb) for i in walk for h in range(nh) for qb in range(-(-int(im[i, 1]) // lc.QB))]
        assert p["units"] == len(want) == len(items) and items.tolist() == [list(map(int, w)) for w in want]
        assert len({tuple(r) for r in items.tolist()}) == len(items)


def test_plan_orders_hold_the_same_items(api):
    for sizes in lc.LISTS.values():
        a, b = (api.list_plan(sizes, lc.PATCH, 4, 2, o)["items"] for o in (0, 1))
        assert sorted(map(tuple, a.tolist())) == sorted(map(tuple, b.tolist()))
    assert np.all(np.diff(api.list_plan(lc.MIXED, lc.PATCH, 4, 2, 1)["items"][:, 1]) <= 0)


def test_plan_op_refuses_bad_arguments(api):
    L = api.lib()
    h, w, tot = (C.c_int32 * 2)(14, 28), (C.c_int32 * 2)(14, 14), (C.c_int64 * 5)()
    i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    ok = lambda *a: L.dinov2_hip_op_list_plan(*a)  # noqa: E731
    assert ok(2, h, w, 14, 4, 2, 0, None, None, None, 0, tot) == 0 and list(tot) == [13, 3, 14 * 14 + 28 * 14, 4, 2]
    assert ok(0, h, w, 14, 4, 2, 0, None, None, None, 0, tot) != 0          # n <= 0
    assert ok(2, None, w, 14, 4, 2, 0, None, None, None, 0, tot) != 0       # NULL sizes
    assert ok(2, h, w, 0, 4, 2, 0, None, None, None, 0, tot) != 0           # patch
    assert ok(2, h, w, 14, -1, 2, 0, None, None, None, 0, tot) != 0         # R
    assert ok(2, h, w, 14, 4, 0, 0, None, None, None, 0, tot) != 0          # heads
    assert ok(2, h, w, 14, 4, 2, 2, None, None, None, 0, tot) != 0          # order
    assert ok(2, h, w, 14, 4, 2, 0, None, None, None, 0, None) != 0         # NULL totals
    items = (C.c_int32 * 4)()
    assert ok(2, h, w, 14, 4, 2, 0, C.cast(None, i64p), C.cast(None, i32p), items, 1, tot) != 0  # a table of 1 < 4 entries
    big_h, big_w = (C.c_int32 * 2)(14 * 40000, 14 * 40000), (C.c_int32 * 2)(14 * 40000, 14 * 40000)
    assert ok(2, big_h, big_w, 14, 0, 1, 0, None, None, None, 0, tot) != 0  # M >= 2^31: row0 would not fit the table


def test_list_rows_and_predict_list_refuse_without_a_device(api):
    """The checks that come before anything touches a device: a NULL model / session / list."""
    L = api.lib()
    err = C.create_string_buffer(256)
    il, keep = api._image_list([0], [(14, 14)], api.RGB_CHW, 0)
    off = (C.c_int64 * 2)()
    assert L.dinov2_hip_list_rows(None, C.byref(il), 0, off, err, len(err)) == 4 and b"null" in err.value
    assert L.dinov2_hip_predict_list(None, C.byref(il), None, 0, err, len(err)) == 4 and b"null" in err.value
    assert L.dinov2_hip_predict_list(None, None, None, 0, err, len(err)) == 4
    assert L.dinov2_hip_abi_version() == 1


@pytest.mark.parametrize("dt", [ac.F16, ac.BF16])
def test_emulation_passes_its_check_and_mutants_fail(dt):
    T, nh = [6, 77, 137, 30, 10], 2  # neighbouring lengths all different, none a multiple of 64, one of two query blocks
    for log2 in (True, False):
        qkv = lc.segment_input(T, nh, dt, log2, seed=5 + dt)
        ok, msg = lc.check_segments(lc.emulate_list(qkv, T, nh, dt, log2), qkv, T, nh, dt, log2)
        assert ok, msg
        for mutant in lc.ATTN_MUTANTS:
            ok, msg = lc.check_segments(lc.emulate_list(qkv, T, nh, dt, log2, mutant), qkv, T, nh, dt, log2)
            assert not ok, "mutant %s passes the per-segment check" % mutant


def test_heads_swapped_mutant_on_a_two_image_list():
    T, nh = [30, 26], 2
    qkv = lc.segment_input(T, nh, ac.F16, True, seed=11)
    assert lc.check_segments(lc.emulate_list(qkv, T, nh, ac.F16, True), qkv, T, nh, ac.F16, True)[0]
    ok, msg = lc.check_segments(lc.emulate_list(qkv, T, nh, ac.F16, True, "heads_swapped"), qkv, T, nh, ac.F16, True)
    assert not ok and "segment 1" in msg


def test_bookkeeping_passes_its_check_and_mutants_fail():
    for name, sizes in lc.LISTS.items():
        for R, first in ((4, 1), (4, 5), (0, 1)):
            ok, msg = lc.check_bookkeeping(lc.host_bookkeeping(sizes, lc.PATCH, R, first), sizes, lc.PATCH, R, first)
            assert ok, (name, msg)
    for mutant in lc.HOST_MUTANTS:
        for name in ("mixed", "reversed", "repeat_apart"):
            sizes = lc.LISTS[name]
            ok, _ = lc.check_bookkeeping(lc.host_bookkeeping(sizes, lc.PATCH, 4, 1, mutant), sizes, lc.PATCH, 4, 1)
            assert not ok, "mutant %s passes on %s" % (mutant, name)
