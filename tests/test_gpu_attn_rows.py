"""attn_rows_kernel alone (dinov2_hip_op_attn_rows, csrc/attn_rows.hip), f16 and bf16, over the shapes, query sets and key views of
tests/attn_row_cases.py: exact probes (one-hot permutations, pairs at 0.5 / 0.5, power-of-two ladders, uniform rows), a float64 reference
under the bound derived in attn_row_cases.error_bound, rows that sum to 1, views that are slices bit for bit, rows that do not depend on
the other queries, the batch, the instantiation or the run, and guard bands that stay untouched (api.op_attn_rows raises if one changed).
The same probes reject every planted bug of the numpy restatement on the CPU (tests/test_attn_row_probes.py)."""
import numpy as np
import pytest

import attention_cases as ac
import attn_row_cases as rc

pytestmark = pytest.mark.gpu

DTYPES = [ac.F16, ac.BF16]


def _views(api, dt, qkv, B, T, nh, qs, **kw):
    """{(key0, nkeys): rows} for every key view; the sliced views must be columns of the full one, bit for bit."""
    out = {}
    for key0, nkeys in rc.key_views(T):
        out[key0, nkeys] = api.op_attn_rows(dt, qkv, B, T, nh, qs, key0, nkeys, **kw)
    full = out[0, T]
    assert full.shape == (B, nh, len(qs), T)
    for (key0, nkeys), rows in out.items():
        ok, msg = rc.check_exact(rows, full[..., key0:key0 + nkeys], "view (%d, %d) vs columns of the full view" % (key0, nkeys))
        assert ok, msg
    return out


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", rc.SHAPES, ids=rc.shape_id)
def test_exact_probes(api, shape, dt):
    B, T, nh = shape
    for kind in rc.PROBES:
        qkv, exp = rc.build_probe(kind, B, T, nh, seed=100 + T)
        for qs in rc.query_sets(T):
            for (key0, nkeys), rows in _views(api, dt, qkv, B, T, nh, qs).items():
                ok, msg = rc.check_probe(kind, rows, rc.expected_view(exp, qs, key0, nkeys),
                                         "%s nq=%d view=(%d, %d)" % (rc.shape_id(shape), len(qs), key0, nkeys))
                assert ok, msg


@pytest.mark.parametrize("regime", ac.REGIMES)
@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", rc.SHAPES, ids=rc.shape_id)
def test_against_float64_reference(api, shape, dt, regime):
    """Every element within attn_row_cases.error_bound of the float64 softmax of the stored operands; rows sum to 1 within T 2^-23."""
    B, T, nh = shape
    qkv = ac.regime_input(regime, B, T, nh, dt, True, seed=7 + T)
    for qs in rc.query_sets(T):
        P, S, M = rc.reference(qkv, B, T, nh, qs)
        bound = rc.error_bound(P, S, M, T)
        for (key0, nkeys), rows in _views(api, dt, qkv, B, T, nh, qs).items():
            what = "%s %s nq=%d view=(%d, %d)" % (rc.shape_id(shape), regime, len(qs), key0, nkeys)
            ok, msg = rc.check_against_reference(rows, P[..., key0:key0 + nkeys], bound[..., key0:key0 + nkeys], what)
            print(msg)
            assert ok, msg
            if nkeys == T:
                ok, msg = rc.check_rows_sum_to_one(rows, T, what)
                assert ok, msg


@pytest.mark.parametrize("dt", DTYPES, ids=["f16", "bf16"])
@pytest.mark.parametrize("shape", rc.SHAPES, ids=rc.shape_id)
def test_rows_do_not_depend_on_the_request(api, shape, dt):
    """A row asked alone equals the same row of the all-queries (or largest) call -- the 1-query and the 8-query instantiations agree; image b
    alone equals its rows inside the batch; the two-pass form (no scores kept: an LDS budget of 1 byte) gives the same bits; four repeated
    runs are identical."""
    B, T, nh = shape
    qkv = ac.regime_input("random", B, T, nh, dt, True, seed=3 + T)
    sets = rc.query_sets(T)
    # (long sequences: 40-odd rows through the 8-query kernel, those of the small sets among them)
    big = sets[-1] if T <= 261 else sorted(set(range(0, T, T // 40)) | {v for s in sets for v in s})
    full = api.op_attn_rows(dt, qkv, B, T, nh, big)
    for q in sorted({v for s in sets[:3] for v in s} & set(big)):
        one = api.op_attn_rows(dt, qkv, B, T, nh, [q])
        ok, msg = rc.check_exact(one[:, :, 0], full[:, :, big.index(q)], "query %d alone vs in the large request" % q)
        assert ok, msg
    for qs in sets[:3]:
        few = api.op_attn_rows(dt, qkv, B, T, nh, qs)
        ok, msg = rc.check_exact(few, full[:, :, [big.index(q) for q in qs]], "queries %s vs the large request" % qs)
        assert ok, msg
    H = 64 * nh
    for b in range(B) if B > 1 else ():
        alone = api.op_attn_rows(dt, qkv[b * T:(b + 1) * T], 1, T, nh, big)
        ok, msg = rc.check_exact(alone[0], full[b], "image %d alone vs inside the batch" % b)
        assert ok, msg
    assert qkv.shape[1] == 3 * H
    for key0, nkeys in rc.key_views(T):
        two_pass = api.op_attn_rows(dt, qkv, B, T, nh, big, key0, nkeys, lds_budget=1)
        ok, msg = rc.check_exact(two_pass, full[..., key0:key0 + nkeys], "two-pass form, view (%d, %d)" % (key0, nkeys))
        assert ok, msg
    for run in range(3):
        ok, msg = rc.check_exact(api.op_attn_rows(dt, qkv, B, T, nh, big), full, "run %d" % (run + 2))
        assert ok, msg


def test_two_pass_form_passes_the_probes(api):
    """The path of sequences whose scores do not fit the LDS, reached at a small size through the op's LDS budget."""
    B, T, nh = 3, 261, 2
    for kind in rc.PROBES:
        qkv, exp = rc.build_probe(kind, B, T, nh, seed=5)
        for qs in rc.query_sets(T):
            for key0, nkeys in rc.key_views(T):
                rows = api.op_attn_rows(ac.F16, qkv, B, T, nh, qs, key0, nkeys, lds_budget=1)
                ok, msg = rc.check_probe(kind, rows, rc.expected_view(exp, qs, key0, nkeys), "two-pass nq=%d" % len(qs))
                assert ok, msg


def test_bad_arguments_are_refused(api):
    qkv = np.zeros((4, 192), np.float32)
    for qs, key0, nkeys in (([4], 0, 4), ([1, 1], 0, 4), ([2, 1], 0, 4), ([0], 2, 3), ([0], 0, 0)):
        with pytest.raises(RuntimeError):
            api.op_attn_rows(ac.F16, qkv, 1, 4, 1, qs, key0, nkeys)
