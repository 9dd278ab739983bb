"""GPU tests of launch_attention_list (csrc/attention.hip), the variable-length form of the two attention kernels, through
dinov2_hip_op_attention_list: segments of different lengths packed one after the other.  Contract: every segment is, BIT FOR BIT, the output of
dinov2_hip_op_attention_ex on that segment alone (B = 1, same forced kernel version); the two versions agree bit for bit; nothing outside
rows [0, sum T) is written (guard bands) and every row inside is (NaN fill).  Cases and helpers: tests/list_cases.py, tests/attention_cases.py.
"""
import numpy as np
import pytest

import attention_cases as ac
import list_cases as lc

pytestmark = pytest.mark.gpu


def _forced(api, attn_v, fn, list_order=None):
    try:
        api.set_tuning("attn_v", attn_v)
        api.set_tuning("attn_nwv", 0)
        if list_order is not None:
            api.set_tuning("list_order", list_order)
        return fn()
    finally:
        api.reset_tuning("attn_v")
        api.reset_tuning("attn_nwv")
        api.reset_tuning("list_order")


def _alone(api, dt, qkv, T, nh, log2):
    out = np.zeros((T, 64 * nh), np.float32)
    rc = api.lib().dinov2_hip_op_attention_ex(dt, api._ptr(np.ascontiguousarray(qkv, np.float32)), api._ptr(out), 1, T, 64 * nh, nh, int(log2))
    assert rc == 0, "dinov2_hip_op_attention_ex failed (%d)" % rc
    return out


def _assert_segments(api, out, qkv, T, nh, dt, log2, attn_v):
    assert np.isfinite(out).all(), "rows of the list output were left unwritten (NaN fill)"
    r0 = 0
    for i, t in enumerate(T):
        exp = _forced(api, attn_v, lambda: _alone(api, dt, qkv[r0:r0 + t], t, nh, log2))
        got = out[r0:r0 + t]
        assert np.array_equal(got, exp), "attn_v=%d segment %d (T=%d, rows %d..): %d elements differ from the segment alone" % (
            attn_v, i, t, r0, int((got != exp).sum()))
        r0 += t


@pytest.mark.parametrize("log2", [True, False], ids=["log2", "nat"])
@pytest.mark.parametrize("dt", [ac.F16, ac.BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("nh", [1, 6])
@pytest.mark.parametrize("case", sorted(lc.SEGMENTS))
def test_every_segment_is_its_own_attention_bit_for_bit(api, case, nh, dt, log2):
    T = lc.SEGMENTS[case]
    qkv = lc.segment_input(T, nh, dt, log2, seed=31 + nh)
    outs = {}
    for attn_v in (1, 2):
        outs[attn_v] = _forced(api, attn_v, lambda: api.op_attention_list(dt, qkv, T, nh, log2))  # (raises on a changed guard band)
        _assert_segments(api, outs[attn_v], qkv, T, nh, dt, log2, attn_v)
    assert np.array_equal(outs[1], outs[2]), "the list forms of attention_kernel and attention2_kernel disagree"


@pytest.mark.parametrize("dt", [ac.F16, ac.BF16], ids=["f16", "bf16"])
def test_table_order_and_kernel_choice_change_no_bit(api, dt):
    T, nh = lc.SEGMENTS["edges"], 6
    qkv = lc.segment_input(T, nh, dt, True, seed=77)
    base = _forced(api, 1, lambda: api.op_attention_list(dt, qkv, T, nh, True), list_order=0)
    for attn_v, order in ((1, 1), (2, 1), (0, 0), (0, 1)):  # (0: the launcher's own choice by the table's length)
        assert np.array_equal(_forced(api, attn_v, lambda: api.op_attention_list(dt, qkv, T, nh, True), list_order=order), base), (attn_v, order)


@pytest.mark.parametrize("dt", [ac.F16, ac.BF16], ids=["f16", "bf16"])
def test_segments_within_the_float64_bound(api, dt):
    """One regime input per dtype against attention_cases.reference within attention_cases.error_bound, segment by segment: catches an error
    the list and the uniform kernels would share."""
    T, nh, log2 = lc.SEGMENTS["edges"], 6, True
    regimes = [ac.REGIMES[i % len(ac.REGIMES)] for i in range(len(T))]
    qkv = np.concatenate([ac.regime_input(r, 1, t, nh, dt, log2, 900 + i) for i, (r, t) in enumerate(zip(regimes, T))])
    out = api.op_attention_list(dt, qkv, T, nh, log2)
    r0 = 0
    for i, t in enumerate(T):
        seg = qkv[r0:r0 + t]
        o, A, S, M = ac.reference(seg, 1, t, nh, log2)
        ok, msg = ac.check_against_reference(out[r0:r0 + t], o, ac.error_bound(o, A, S, M, seg, 1, t, nh, dt, log2))
        assert ok, "segment %d (%s, T=%d): %s" % (i, regimes[i], t, msg)
        r0 += t


def test_versions_without_a_list_form_are_refused(api):
    T, nh = [6, 30], 1
    qkv = lc.segment_input(T, nh, ac.F16, True, seed=3)
    for attn_v in (3, 4):
        with pytest.raises(RuntimeError):
            _forced(api, attn_v, lambda: api.op_attention_list(ac.F16, qkv, T, nh, True))


@pytest.mark.parametrize("kind", ["permutation", "pairs"])
def test_exact_probes_per_segment(api, kind):
    """attention_cases' exact probes, one per segment: query i of a segment must return the value row(s) of ITS segment's target key(s), bit
    for bit -- a key or a row taken from a neighbouring segment cannot."""
    T, nh, dt = [6, 77, 137, 30, 10, 261], 2, ac.F16
    parts = [ac.build_probe(kind, 1, t, nh, dt, 40 + i) for i, t in enumerate(T)]
    qkv, exp = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    for log2 in (True, False):
        ok, msg = ac.check_probe(kind, api.op_attention_list(dt, qkv, T, nh, log2), exp, dt)
        assert ok, msg
