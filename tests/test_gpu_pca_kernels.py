"""The device stages of dinov2_hip_pca3 one at a time (dinov2_hip_op_pca_prepare / _cov / _power / _project: the driver's own launch functions on
host data, outputs framed by guard bands and NaN-filled) against the cases, float64 references and derived bounds of tests/pca_cases.py:
pca_mean_kernel and pca_center_transpose_kernel bit for bit, the aliased covariance GEMM, pca_power_kernel and pca_project_kernel inside
bounds derived from operation counts.  tests/test_pca_probes.py shows on the CPU that these checks reject the planted bugs.  A changed guard
band raises inside the api wrappers."""
import numpy as np
import pytest

import pca_cases as pc

pytestmark = pytest.mark.gpu


def _ok(failures, report=()):
    print("\n".join(report))
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------------------------- mean + centre / transpose
@pytest.mark.parametrize("shape", pc.SHAPES, ids=pc.shape_id)
def test_mean_and_centred_transpose_bit_for_bit(api, shape):
    P, H = shape
    _ok(pc.check_prepare(api.op_pca_prepare, pc.tokens_generic(P, H), "generic")
        + pc.check_prepare(api.op_pca_prepare, pc.tokens_dyadic(P, H), "dyadic", exact_mean=True))


@pytest.mark.parametrize("shape", [(33, 33), (300, 100)], ids=pc.shape_id)
def test_centred_values_at_the_edges_of_f16(api, shape):
    """Centred values below, inside and above the f16 subnormal range, and just under 65504 (65519 still rounds down to it)."""
    P, H = shape
    _ok(pc.check_prepare(api.op_pca_prepare, pc.tokens_subnormal(P, H), "subnormal")
        + pc.check_prepare(api.op_pca_prepare, pc.tokens_large(P, H), "large"))


# ------------------------------------------------------------------------------------------------------------------- covariance
@pytest.mark.parametrize("shape", pc.SHAPES + pc.COV_LARGE_SHAPES, ids=pc.shape_id)
def test_covariance_of_the_aliased_gemm(api, shape):
    """cov = Xt Xt^T through launch_pca_cov (A == W, one buffer, prepared into an xt that started as NaN) against the float64 product of the xt
    that prepare returns; small integers: exact, whatever the order of accumulation."""
    P, H = shape
    report, fails = [], []
    tok = pc.tokens_generic(P, H)
    fails += pc.check_cov(api.op_pca_cov(tok), api.op_pca_prepare(tok)[1], "generic", report=report)
    tok = pc.tokens_integer(P, H)
    fails += pc.check_cov(api.op_pca_cov(tok), api.op_pca_prepare(tok)[1], "integer", exact=True)
    _ok(fails, report)


# ------------------------------------------------------------------------------------------------------------------- power step
@pytest.mark.parametrize("H", pc.H_VALUES)
@pytest.mark.parametrize("kind", ["generic", "start", "rank_deficient"])
def test_power_step(api, kind, H):
    """One launch: ynext against long double cov (yprev R^-1) inside the derived bound; every Gram part = the Gram matrix of its own 16 rows
    (rows past H contributing exactly 0); the parts sum to ynext^T ynext.  rank_deficient: the dropped column is exactly 0, all finite."""
    if kind == "rank_deficient" and H < 16:
        H = 16 + H  # (the case needs 16 rows for its +-1 column: 24 and 28 in place of 8 and 12 -- a partial workgroup each)
    cov, y, g, dead = pc.power_case(kind, H)
    report = []
    _ok(pc.check_power(api.op_pca_power, cov, y, pc.gram_parts_in_first(g, H), f"{kind} H={H}", dead, report), report)


@pytest.mark.parametrize("H", pc.H_VALUES)
def test_power_step_sees_only_the_sum_of_the_gram_parts(api, H):
    cov, y, g, _ = pc.power_case("generic", H)
    _ok(pc.check_gram_split(api.op_pca_power, cov, y, g, f"H={H}"))


# ------------------------------------------------------------------------------------------------------------------- projection
@pytest.mark.parametrize("shape", pc.PROJECT_SHAPES, ids=pc.shape_id)
def test_projection(api, shape):
    report = []
    _ok(pc.check_project(api.op_pca_project, *pc.project_case(*shape), "generic", report), report)


def test_ops_refuse_sizes_the_driver_refuses(api):
    x = np.zeros((4, 4100), np.float32)
    d = np.zeros((600, 64), np.float64)
    L = api.lib()
    for P, H in ((3, 8), (4, 7), (4, 4097)):
        assert L.dinov2_hip_op_pca_prepare(x.ctypes.data, P, H, x.ctypes.data, x.ctypes.data) == 4
        assert L.dinov2_hip_op_pca_cov(x.ctypes.data, P, H, x.ctypes.data) == 4
        assert L.dinov2_hip_op_pca_project(x.ctypes.data, x.ctypes.data, x.ctypes.data, P, H, x.ctypes.data) == 4
    for H in (7, 4097):
        assert L.dinov2_hip_op_pca_power(x.ctypes.data, d.ctypes.data, d.ctypes.data, H, d.ctypes.data, d.ctypes.data) == 4
    assert L.dinov2_hip_op_pca_prepare(None, 4, 8, x.ctypes.data, x.ctypes.data) == 4
