"""The numpy emulations of the PCA kernels (tests/pca_cases.py) through the very checks tests/test_gpu_pca_kernels.py applies to the kernels, and
the planted bugs those checks must reject; the emulation of the whole call against the float64 SVD on every end-to-end input (the figures the
GPU tolerance is 16 x of); the port of pca_chol_rinv against the library's; the declarations and exports of the new entry points.  No GPU,
nothing skips."""
import os
import re
import subprocess

import numpy as np
import pytest

import pca_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_emulations_pass_every_check_inside_every_bound():
    report = []
    assert pc.all_failures(pc.emulated_ops(None), report) == []
    worst = {}
    for line in report:
        kind = re.search(r"(ynext|gram parts|gram total|covariance|projection):", line).group(1)
        worst[kind] = max(worst.get(kind, 0.0), float(line.rsplit(" ", 1)[1]))
    print("\nworst error / bound of the emulations: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert set(worst) == {"ynext", "gram parts", "gram total", "covariance", "projection"} and max(worst.values()) <= 1.0


@pytest.mark.parametrize("mutant", pc.MUTANTS)
def test_planted_bugs_are_rejected(mutant):
    failures = pc.all_failures(pc.emulated_ops(mutant))
    print(f"\n{mutant}: rejected by {len(failures)} checks, first: {failures[0] if failures else None}")
    assert failures, f"planted bug {mutant} passed every check"


def test_emulation_of_the_whole_call_against_svd():
    """The figures the end-to-end GPU assertions are 16 x of (floored at 1e-7): printed per input; every run converges before the driver's cap
    of 28 checks (400 steps), is finite, and sits far inside what test_pca3_matches_svd allowed before (1e-3 and 1e-2)."""
    print("\n%-24s %-14s %-18s %s" % ("input", "max 1-|cos|", "projection error", "steps"))
    for name in pc.E2E_INPUTS:
        x, tied, (cos_err, proj_err), steps = pc.e2e_case(name)
        print("%-24s %-14.1e %-18.1e %d" % (name, cos_err, proj_err, steps))
        assert np.isfinite([cos_err, proj_err]).all() and steps < 400, name
        assert pc.e2e_tolerance(cos_err) < 1e-3 and pc.e2e_tolerance(proj_err) < 1e-1, name
    # the flat spectra run past the first four checks: the 16-step cadence is exercised
    assert pc.e2e_case("flat_256x384")[3] > 32 and pc.e2e_case("flat_300x40")[3] > 32
    # a tie is a tie: the pair of the tied input is separated by less than the third gap by orders of magnitude
    x = pc.e2e_case("tie12_300x128")[0].astype(np.float64)
    s = np.linalg.svd(x - x.mean(0), compute_uv=False)
    assert (s[0] - s[1]) < 1e-2 * (s[1] - s[2])
    x = pc.e2e_case("neartie34_300x128")[0].astype(np.float64)
    s = np.linalg.svd(x - x.mean(0), compute_uv=False)
    assert (s[2] - s[3]) < 0.1 * (s[1] - s[2])
    for name in ("minimal_4x8", "minimal_4x64", "minimal_5x200"):  # rank below the block width of 8: dead or noise pivots inside the iteration
        assert pc.e2e_case(name)[0].shape[0] - 1 < pc.NB


def test_cases_are_well_formed(api):
    hdr = open(os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "kernels.h")).read()
    assert "PCA_NB = 8, PCA_ROWS = 16" in hdr and (pc.NB, pc.ROWS) == (8, 16)  # the cases sit on the kernel's real block sizes
    assert all(api.pca_ppad(P) == pc.ppad(P) for P in range(1, 700)) and all(api.pca_blocks(H) == pc.blocks(H) for H in range(8, 4097))
    assert {P for P, _ in pc.SHAPES} == set(pc.P_VALUES) and {H for _, H in pc.SHAPES} == set(pc.H_VALUES)
    assert {P % 4 for P, _ in pc.PROJECT_SHAPES} == {0, 1, 2, 3}
    for P, H in [(33, 33), (300, 100)]:
        a = np.abs(pc.tokens_subnormal(P, H))
        a = a[a > 0]
        assert a.min() < 2.0 ** -24 and ((a > 2.0 ** -24) & (a < 2.0 ** -14)).any() and a.max() > 2.0 ** -14
        big = pc.tokens_large(P, H)
        mean, xt = pc.prepare_emulate(big)
        assert not mean.any() and np.isfinite(xt).all() and xt.max() == 65504.0 and (big == 65519.0).any()
        t = pc.tokens_integer(P, H)
        mean, xt = pc.prepare_emulate(t)
        assert np.array_equal(mean, np.round(mean)) and mean.any() and np.array_equal(xt, np.round(xt)) and np.abs(xt).max() <= 8
    for H in pc.H_VALUES:
        if H >= 16:
            _, y, g, dead = pc.power_case("rank_deficient", H)
            rinv = pc.chol_rinv(g)
            assert dead == (5,) and not rinv[:, 5].any() and all(rinv[k, k] > 0 for k in range(8) if k != 5)
        g = pc.gram_exact(pc.power_case("generic", H)[1])
        for parts in (pc.gram_parts_in_first(g, H), pc.gram_parts_spread(g, H)):
            assert np.array_equal(pc.gram_sum(parts), g)
        if pc.blocks(H) > 1:
            assert np.count_nonzero(pc.gram_parts_spread(g, H).any(1)) == pc.blocks(H)


def test_covariance_shapes_reach_the_named_gemm_plans(api):
    """Which kernels the aliased covariance launch runs on at the tested shapes (dtype 0 = f16, epilogue 5 = plain f32): small tiles with one
    and two K sub-tiles per stage, and from H = 2048 the large-tile kernels."""
    for (P, H), plan in pc.COV_PLANS.items():
        assert api.gemm_plan(0, 5, H, H, api.pca_ppad(P)) == plan, (P, H)
    assert all(pc.COV_PLANS[s].startswith("gemm2<") for s in pc.COV_LARGE_SHAPES)


def test_chol_rinv_port_agrees_with_the_library(api):
    """pca_chol_rinv (csrc/kernels.h, compiled for the host) against the port: the same dead columns, and the live entries within the
    difference two roundings of the same factorisation may show (pca_cases: 2 phi ||rinv||)."""
    grams = []
    for H in (8, 33, 384):
        for kind in ("generic", "start") + (("rank_deficient",) if H >= 16 else ()):
            grams.append(pc.power_case(kind, H)[2])
    g = pc.power_case("generic", 33)[2].copy()
    g[3, :] = g[:, 3] = 0.0  # a zero column
    grams += [g, np.zeros((8, 8)), np.full((8, 8), np.nan)]
    for g in grams:
        got, exp = api.pca_chol_rinv(g), pc.chol_rinv(g)
        assert np.array_equal(got == 0, exp == 0) and np.isfinite(got).all()
        assert np.array_equal(got, np.triu(got))
        live = np.diag(exp) != 0
        if live.any():
            kappa = np.linalg.cond(g[np.ix_(live, live)])
            phi = pc.U53 * (51.0 * kappa ** 1.5 + 8.0 * kappa ** 0.5)
            assert np.abs(got - exp).max() <= 2.0 * phi * np.linalg.norm(exp, 2)
            y = np.linalg.cholesky(g[np.ix_(live, live)]).T  # any block with this Gram matrix becomes orthonormal
            q = y @ got[np.ix_(live, live)]
            assert np.abs(q.T @ q - np.eye(int(live.sum()))).max() <= 64 * kappa * 2.0 ** -52


@pytest.mark.parametrize("H", [33, 384])
def test_dead_pivot_rule_seen_through_pca_ritz(api, H):
    """Where dinov2_hip_op_pca_ritz shows the factorisation: on the rank-deficient block (one column a copy of another) it stays finite and gives
    the Ritz values of the port's Q (the dropped column contributes nothing); 8 x 8 symmetric eigenvalues from two backward-stable solvers
    agree to a few u ||B||, 1e-12 of the largest here."""
    cov, y, g, dead = pc.power_case("rank_deficient", H)
    ynext, _ = pc.power_emulate(cov, y, pc.gram_parts_in_first(g, H))
    evals, comp = np.zeros(3), np.zeros((3, H))
    assert api.lib().dinov2_hip_op_pca_ritz(np.ascontiguousarray(y).ctypes.data, np.ascontiguousarray(ynext).ctypes.data,
                                            np.ascontiguousarray(g).ctypes.data, H, evals.ctypes.data, comp.ctypes.data) == 0
    exp_evals, exp_comp = pc.ritz(y, ynext, g)
    assert np.isfinite(evals).all() and np.isfinite(comp).all()
    assert np.abs(evals - exp_evals).max() <= 1e-12 * exp_evals[0]
    assert np.abs(np.abs(np.sum(comp * exp_comp, 1)) - 1.0).max() <= 1e-9


def test_new_symbols_are_declared_and_exported(api):
    ops = open(os.path.join(ROOT, "include", "dinov2_hip_ops.h")).read()
    names = {"dinov2_hip_op_pca_" + n for n in ("ppad", "blocks", "prepare", "cov", "power", "project", "chol_rinv")}
    for n in names:
        assert re.search(r"\bint %s\(" % n, ops), n
    api.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    assert names <= set(re.findall(r" T (dinov2_hip_[a-z0-9_]+)", out))
    # the driver and the testing entry points share the padding rule and the aliased launch: one definition each
    model = open(os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "pca.cpp")).read()
    testing = open(os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "ops_testing.cpp")).read()
    for src in (model, testing):
        assert "pca_ppad(P)" in src and "launch_pca_cov(" in src and "/ 128 * 128" not in src
