"""The checks of tests/test_gpu_attention.py, on the CPU: a numpy emulation of the attention kernels' documented numerics
(tests/attention_cases.py: emulate) must pass every probe and stay inside the derived bound over the GPU file's shapes -- the bound
is not too tight -- and the same checks must reject each planted bug of MUTANTS -- the tests would notice a subtly wrong kernel.
"""
import numpy as np
import pytest

import attention_cases as ac

EMU_COST_MAX = 3.0e8  # CPU budget per emulated case: heads (then images) are trimmed until B * nh * T^2 * 64 fits; T is kept


def _trim(B, T, nh):
    while nh > 1 and B * nh * T * T * 64 > EMU_COST_MAX:
        nh = max(1, nh // 2)
    while B > 1 and B * nh * T * T * 64 > EMU_COST_MAX:
        B -= 1
    return B, T, nh


def _checks(B, T, nh, dt, log2, mutant=None, qblock=128, seed=0):
    """Run every probe and (where affordable) every reference regime through the emulation: a list of failure messages."""
    fails = []
    for kind in ac.PROBES:
        qkv, exp = ac.build_probe(kind, B, T, nh, dt, seed)
        with np.errstate(all="ignore"):
            out = ac.emulate(qkv, B, T, nh, dt, log2, mutant, qblock)
        ok, msg = ac.check_probe(kind, out, exp, dt)
        if not ok:
            fails.append(msg)
    if ac.ref_affordable(B, T, nh):
        for i, rg in enumerate(ac.REGIMES):
            qkv = ac.regime_input(rg, B, T, nh, dt, log2, seed + 7 * i + 1)
            o, A, S, M = ac.reference(qkv, B, T, nh, log2)
            bound = ac.error_bound(o, A, S, M, qkv, B, T, nh, dt, log2)
            with np.errstate(all="ignore"):
                out = ac.emulate(qkv, B, T, nh, dt, log2, mutant, qblock)
            ok, msg = ac.check_against_reference(out, o, bound)
            if not ok:
                fails.append("%s regime: %s" % (rg, msg))
    return fails


_PARAMS = [pytest.param(s, dt, log2, id="%s-%s-%s" % (ac.DT_NAME[dt], "log2" if log2 else "exp", ac.shape_id(s)))
           for s in ac.SHAPES for dt in (ac.F16, ac.BF16) for log2 in (True, False)]


@pytest.mark.parametrize("shape,dt,log2", _PARAMS)
def test_emulated_kernel_passes(shape, dt, log2):
    B, T, nh = _trim(*shape)
    fails = _checks(B, T, nh, dt, log2, seed=B * 100003 + T * 101 + nh)
    assert not fails, "; ".join(fails)


# each mutant against shapes where it is observable: T >= 66 (key 64 exists and is not the last), a key tail (T % 64 != 0),
# several heads, a ragged last query block
_MUTANT_SHAPES = [(3, 193, 6), (1, 261, 2)]


@pytest.mark.parametrize("shape", _MUTANT_SHAPES, ids=[ac.shape_id(s) for s in _MUTANT_SHAPES])
@pytest.mark.parametrize("mutant", ac.MUTANTS)
def test_mutant_rejected(mutant, shape):
    """Every combination of dtype and score domain rejects the planted bug (the message names the check that did)."""
    B, T, nh = shape
    qblocks = [128]
    if mutant == "ragged_rows_shifted":  # every block size whose last block holds two or more queries at this T
        qblocks = [qb for qb in sorted(set(ac.QBLOCK.values())) if (T - 1) % qb >= 1]
    for dt in (ac.F16, ac.BF16):
        for log2 in (True, False):
            for qb in qblocks:
                fails = _checks(B, T, nh, dt, log2, mutant, qb, seed=T + nh)
                assert fails, "mutant %s survived every check (%s, %s, %d-query blocks)" % (
                    mutant, ac.DT_NAME[dt], "log2" if log2 else "exp", qb)


def test_code_pool_distance():
    """The permutation probe's codes: pairwise Hamming distance >= 12, so the winner's score (128) leads every other (<= 80)."""
    c = ac.code_pool(4101)
    g = c @ c.T
    np.fill_diagonal(g, -64)
    assert g.max() <= 64 - 24
    rng = np.random.default_rng(0)
    h = ac._head_codes(rng, c, 4101)
    g = h @ h.T
    np.fill_diagonal(g, -64)
    assert g.max() <= 64 - 24


def test_probe_answers_are_exact():
    """The expected answers are values of T, and the pair probe covers (0, T-1) and (63, 64) in different tiles."""
    rng = np.random.default_rng(3)
    pairs = ac.pair_keys(1374, rng)
    assert (0, 1373) in pairs and (63, 64) in pairs
    assert all(a // ac.KT != b // ac.KT for a, b in pairs)
    for dt in (ac.F16, ac.BF16):
        for kind in ("permutation", "pairs"):
            _, exp = ac.build_probe(kind, 2, 261, 3, dt, 5)
            assert np.array_equal(ac.round_t(exp, dt), exp)
            assert np.abs(exp).min() >= 0.25
    js = ac.onehot_columns(300, rng)
    assert {0, 63, 64, 65, 298, 299} <= set(js.tolist())
