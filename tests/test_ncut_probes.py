"""The numpy restatement of the spectral-embedding contract (tests/ncut_cases.py) through the very cases tests/test_gpu_ncut.py applies to
the kernels, and the planted bugs those cases must reject; the planner against its restatement; the refusals that need no device; where
the tile's text lives; the struct layout of the new C-ABI.  No GPU, nothing skips."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ncut_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dinov2.cpp_amd", "csrc")


@pytest.mark.parametrize("case", sorted(nc.CASES))
def test_restatement_passes_every_case(case):
    """Probes bit for bit across the chunkings, shapes and the step under their bounds, the driver cases, the exits."""
    assert nc.CASES[case](nc.Emulated()) == []


@pytest.mark.parametrize("mutant", nc.MUTANTS)
def test_planted_bugs_are_rejected_by_their_named_case(mutant):
    assert nc.CASES[nc.MUTANT_CASE[mutant]](nc.Emulated(mutant)) != [], mutant


def test_cases_are_well_formed():
    hdr = open(os.path.join(CSRC, "kernels.h")).read()
    assert "NCUT_NB = PCA_NB, NCUT_N_MIN = 16, NCUT_N_MAX = 1 << 17, NCUT_EIG_MAX = 6, NCUT_ITER_MAX = 10000, NCUT_TARGET_WGS = 256" in hdr
    assert "NCUT_PARTIAL_MAX = (size_t)32 << 20" in hdr and "constexpr int PCA_NB = 8" in hdr
    assert nc.SHAPES == [(16, 8), (127, 8), (128, 64), (129, 72), (257, 384), (300, 1536), (1369, 1024)]
    assert sorted(nc.MUTANT_CASE) == sorted(nc.MUTANTS) and set(nc.MUTANT_CASE.values()) <= set(nc.CASES)
    n = len(nc.build_probe("pm1_relu")[0])
    assert nc.chunkings(n, 72) == [1, 2, 0, 3] and nc.plan(n, 72)["nchunks"] == 3 and nc.plan(n, 72, 2)["nchunks"] == 2
    rows, aff, tau, floor, q = nc.build_probe("at_tau")
    assert tau == 0.25 and (nc.mc.reference(rows, rows) == 0.25).any()
    rows, aff, *_ = nc.build_probe("zero_row")
    assert aff == "relu" and (np.abs(rows).sum(1) == 0).sum() == 3
    for kind in nc.PROBES:
        rows, aff, tau, floor, q = nc.build_probe(kind)
        assert floor == 2.0 ** -10 and np.array_equal(q, np.round(q)) and np.abs(q).max() <= 2
        nc.exact_apply(rows, aff, tau, floor, q)
    for shape in nc.SHAPES:  # THRESHOLD's tau sits in a gap (asserted inside) near 0.2
        assert 0.1 <= nc.shape_case(shape, "threshold")[1] <= 0.3
    rows, fg = nc.tokencut_expectation()
    assert fg.sum() == 43 and len(fg) == 129


def test_driver_cases_have_their_gaps():
    """On the CPU: every reference group of every planted case is at least GAP_MIN from the rest of the spectrum."""
    for name, (n, H, sizes) in nc.DRIVER_CASES.items():
        rows, _ = nc.planted(name)
        for aff in nc.AFFINITIES:
            tau, floor = nc.driver_params(aff)
            theta, U, d, ed, pert, groups = nc.driver_reference(nc.mc.normalise_f16(rows).astype(np.float32), H, aff, tau, floor, len(sizes))
            assert groups and all(g[2] >= nc.GAP_MIN for g in groups) and pert < 1e-3, (name, aff, groups, pert)
            assert abs(theta[0] - 1.0) < 1e-12


def test_planner_equals_its_restatement(api):
    """ncut_plan (csrc/kernels.h, through dinov2_hip_op_ncut_plan; no device) against ncut_cases.plan, and what it promises.  Fails before
    this feature: the symbol is not there."""
    rng = np.random.default_rng(31)
    cases = [(n, H, c) for n, H in nc.SHAPES for c in (0, 1, 2, 1 << 20)]
    cases += [(1 << 17, 4096, 0), (1 << 17, 8, 1 << 20), (32 * 1369, 1024, 0), (16, 8, 0), (65536, 64, 7)]
    cases += [(int(rng.integers(16, (1 << 17) + 1)), int(rng.integers(8, 4097)), int(rng.integers(0, 40))) for _ in range(200)]
    for n, H, c in cases:
        got, want = api.op_ncut_plan(n, H, c), nc.plan(n, H, c)
        assert {k: got[k] for k in want} == want, (n, H, c)
        ranges = nc.chunk_ranges(want)
        assert ranges[0][0] == 0 and ranges[-1][1] == want["ntiles"] and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))  # covered once
        assert all(t1 > t0 for t0, t1 in ranges)
        assert got["part_bytes"] <= 32 << 20 and got["bytes"] >= got["part_bytes"]
    one = api.op_ncut_plan(1369, 1024)
    assert one["ntiles"] == 11 and one["nchunks"] == 11 and one["ntiles"] * one["nchunks"] >= 100  # a single image fills the chip
    for bad in ((15, 8, 0), ((1 << 17) + 1, 8, 0), (16, 7, 0), (16, 4097, 0), (16, 8, -1)):
        with pytest.raises(ValueError):
            api.op_ncut_plan(*bad)


def _request(api, x, out, **kw):
    f = dict(source=0, n=x.shape[0], H=x.shape[1], all_images=0, affinity=0, tau=0.2, floor=1e-5, n_eig=2, max_iter=8, tol=1e-4)
    f.update(kw)
    rows = api.Rows(f["source"], x.ctypes.data, f["n"], f["H"], 0, 0)
    return api.NCut(rows, f["all_images"], f["affinity"], f["tau"], f["floor"], f["n_eig"], f["max_iter"], f["tol"],
                    *(None if o is None else o.ctypes.data for o in out))


# every argument error that can be told from the request alone: (what, the fields that differ from a good request)
BAD_REQUESTS = [("n below 16", dict(n=15)), ("n above 2^17", dict(n=(1 << 17) + 1)), ("H below 8", dict(H=7)), ("H above 4096", dict(H=4097)),
                ("unknown affinity", dict(affinity=3)), ("negative affinity", dict(affinity=-1)), ("n_eig 0", dict(n_eig=0)),
                ("n_eig 7", dict(n_eig=7)), ("max_iter 0", dict(max_iter=0)), ("max_iter above 10 000", dict(max_iter=10001)),
                ("tol below 1e-6", dict(tol=1e-7)), ("tol above 1e-1", dict(tol=0.2)), ("tol NaN", dict(tol=float("nan"))),
                ("threshold tau 1", dict(tau=1.0)), ("threshold tau below -1", dict(tau=-1.5)), ("threshold tau NaN", dict(tau=float("nan"))),
                ("floor negative", dict(floor=-0.1)), ("floor above 1", dict(floor=1.5)), ("exp tau too small", dict(affinity=2, tau=2.0 ** -7)),
                ("exp tau too large", dict(affinity=2, tau=17.0)), ("all_images with GIVEN", dict(all_images=1)), ("all_images 2", dict(all_images=2))]


def test_argument_errors_need_no_device(api):
    """Every refusal returns DINOV2_HIP_ERR_INVALID (4) before any HIP call -- this machine has no GPU -- and leaves the outputs as they
    were.  The session is a block of zeros: no check before the refusal may read it.  Fails before this feature: no such symbols."""
    L = api.lib()
    x = np.ones((32, 8), np.float32)
    fake = C.create_string_buffer(1 << 16)
    err = C.create_string_buffer(256)

    def outputs():
        return [np.full(6, -7.0, np.float32), np.full((6, 32), -7.0, np.float32), np.full(32, -7.0, np.float32), np.full(6, -7.0, np.float32),
                np.full(1, -7, np.int32), np.full(1, -7, np.int32)]

    out = outputs()
    assert L.dinov2_hip_ncut_tokens(None, C.byref(_request(api, x, out)), err, len(err)) == 4 and b"null session" in err.value
    assert L.dinov2_hip_ncut_tokens(fake, None, err, len(err)) == 4
    for what, kw in BAD_REQUESTS:
        assert L.dinov2_hip_ncut_tokens(fake, C.byref(_request(api, x, out, **kw)), err, len(err)) == 4, what
        assert err.value.startswith(b"ncut: "), what
    assert L.dinov2_hip_ncut_tokens(fake, C.byref(_request(api, x, [None] * 6)), err, len(err)) == 4 and b"no output" in err.value
    rq = _request(api, x, out)
    rq.rows.data = None
    assert L.dinov2_hip_ncut_tokens(fake, C.byref(rq), err, len(err)) == 4 and b"data == NULL" in err.value
    rq = _request(api, x, out)
    rq.rows.data, rq.rows.on_device = x.ctypes.data | 8, 1
    assert L.dinov2_hip_ncut_tokens(fake, C.byref(rq), err, len(err)) == 4 and b"16-byte aligned" in err.value
    rq = _request(api, x, out, source=7)
    assert L.dinov2_hip_ncut_tokens(fake, C.byref(rq), err, len(err)) == 4 and b"unknown rows source" in err.value
    for src in (1, 2):  # a resident source of a session that has run no forward (the zeros say so)
        assert L.dinov2_hip_ncut_tokens(fake, C.byref(_request(api, x, out, source=src)), err, len(err)) == 4 and b"there is none" in err.value
    assert L.dinov2_hip_ncut_tokens(fake, C.byref(_request(api, x, out, source=2, all_images=1)), err, len(err)) == 4
    for a, b in zip(out, outputs()):
        assert np.array_equal(a, b)
    # the ops
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    xp = x.ctypes.data_as(fp)
    d8 = np.zeros((32, 8)).ctypes.data_as(dp)
    plan = (C.c_int64 * 8)()
    assert L.dinov2_hip_op_ncut_plan(32, 8, 0, None) == 4 and L.dinov2_hip_op_ncut_plan(15, 8, 0, plan) == 4
    for n, H, aff, tau, floor, chunk in ((15, 8, 1, 0, 0, 0), (32, 7, 1, 0, 0, 0), (32, 8, 3, 0, 0, 0), (32, 8, 0, 1.0, 0, 0), (32, 8, 2, 0.001, 0, 0),
                                         (32, 8, 1, 0, 0, -1), (32, 8, 0, 0.2, 2.0, 0)):
        assert L.dinov2_hip_op_ncut_apply(xp, n, H, aff, tau, floor, None, d8, chunk, d8, d8, None) == 4
        assert L.dinov2_hip_op_ncut_step(xp, n, H, aff, tau, floor, chunk, d8, d8, d8, d8, d8) == 4
    assert L.dinov2_hip_op_ncut_apply(None, 32, 8, 1, 0, 0, None, d8, 0, d8, d8, None) == 4
    assert L.dinov2_hip_op_ncut_apply(xp, 32, 8, 1, 0, 0, None, None, 0, d8, d8, None) == 4   # t_out without q
    assert L.dinov2_hip_op_ncut_apply(xp, 32, 8, 1, 0, 0, None, d8, 0, None, None, None) == 4  # no output
    assert L.dinov2_hip_op_ncut_step(xp, 32, 8, 1, 0, 0, 0, None, d8, d8, d8, d8) == 4
    for n_eig, it, tol in ((0, 8, 1e-4), (7, 8, 1e-4), (2, 0, 1e-4), (2, 8, 1.0)):
        assert L.dinov2_hip_op_ncut(xp, 32, 8, 1, 0, 0, n_eig, it, tol, None, None, None, None, None, None) == 4
    assert L.dinov2_hip_op_ncut(None, 32, 8, 1, 0, 0, 2, 8, 1e-4, None, None, None, None, None, None) == 4
    ms, st = (C.c_float * 3)(), (C.c_int32 * 1)()
    assert L.dinov2_hip_op_ncut_bench(None, 32, 8, 1, 0, 0, 0, 2, 8, 1e-4, 0, 1, ms, st) == 4
    assert L.dinov2_hip_op_ncut_bench(0x1000, 32, 8, 1, 0, 0, 0, 2, 8, 1e-4, 0, 0, ms, st) == 4  # iters = 0


def test_the_tile_has_one_source_and_the_exponential_is_named():
    """csrc/ncut.hip takes the similarity tile from sim_tile.h and restates none of its fingerprints (the needle list of
    test_similarity_tile_and_its_order_have_a_single_source); the exponential is expf, which the header's contract names."""
    text = open(os.path.join(CSRC, "ncut.hip")).read()
    assert re.search(r'^#include "sim_tile\.h"', text, re.M)
    for needle in ("(row >> 1) & 7)) << 4", "^ sw) << 4", "^ p.sw) << 4", "mfma16(", "struct Best", "bool better(", "bool before("):
        assert needle not in text, needle
    assert "sim_tile(p, sA, sB" in text and "SimRows" in text and "const SimPlace p;" in text
    assert "__expf(" not in text and "expf(" in text and "atomic" not in text.replace("No atomics", "")
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read()
    assert "expf((s - 1) / tau)" in hdr and "int dinov2_hip_ncut_tokens(" in hdr
    mk = open(os.path.join(ROOT, "dinov2.cpp_amd", "Makefile")).read()
    assert "csrc/ncut.hip" in mk and "csrc/ncut.cpp" in mk


def test_ctypes_struct_matches_the_header(api, tmp_path):
    src = tmp_path / "sz.cpp"
    fields = ["all_images", "affinity", "tau", "floor", "n_eig", "max_iter", "tol", "values", "vectors", "degree", "residual", "iterations",
              "converged", "reserved"]
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "dinov2_hip.h"\nint main() { std::printf("%zu", sizeof(dinov2_hip_ncut));\n'
                   + "".join(f'std::printf(" %zu", offsetof(dinov2_hip_ncut, {f}));\n' for f in fields) + "}\n")
    exe = tmp_path / "sz"
    subprocess.run(["g++", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(api.NCut)] + [getattr(api.NCut, f).offset for f in fields]
    assert (api.NCUT_THRESHOLD, api.NCUT_RELU, api.NCUT_EXP, api.NCUT_NB) == (0, 1, 2, 8)


def test_tokencut_rule(api):
    """Session.tokencut's mask (api.tokencut_mask): v > mean(v), flipped so that the entry of largest magnitude is foreground -- on the
    restatement's second vector of the planted two-cluster case it is the planted foreground, whatever the vector's sign."""
    rows, fg = nc.tokencut_expectation()
    v = nc.Emulated().run(rows, 2, "threshold", 0.2, 1e-5, nc.DRIVER_MAX_ITER, nc.DRIVER_TOL)["vectors"][1]
    assert np.array_equal(api.tokencut_mask(v), fg) and np.array_equal(api.tokencut_mask(-v), fg)
