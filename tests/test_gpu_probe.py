"""dinov2_hip_bank_topk_probe on the GPU (csrc/probe.hip; contract in include/dinov2_hip.h): the top-k over each query's own subset of row
ranges of a bank.  Every check is equality of bits: against dinov2_hip_op_bank_topk where every segment is probed, against a float64 top-k
restricted to the union on exact rows, between the cuts of the planner, and between the session call and the kernels alone."""
import functools
import os

import numpy as np
import pytest

import probe_cases as pc

pytestmark = pytest.mark.gpu
cases = pytest.mark.parametrize("H, k, form", [(H, k, f) for H in pc.HS for k in pc.KS for f in pc.FORMS])


@functools.lru_cache(maxsize=None)
def sweep(api, kind, H, nq, k):
    return api.op_bank_topk(*pc.rows(kind, H, nq), k)


@functools.lru_cache(maxsize=None)
def subsets(api, H, k, form):
    """Case 2, shared with case 3: (q, b, probes, the result under the planner's own cuts)."""
    q, b = pc.rows("pm1", H, 200)
    probes = pc.subset_probes(200)
    return q, b, probes, api.op_bank_probe(q, b, pc.SEGMENTS, probes, k, force_form=form)


@cases
def test_probing_every_segment_is_bank_topk(api, H, k, form):
    for nq in (1, 17, 129, 200):
        for kind in ("gauss", "pm1"):
            q, b = pc.rows(kind, H, nq)
            got = api.op_bank_probe(q, b, pc.SEGMENTS, pc.all_probes(nq), k, force_form=form)
            assert pc.same_bits(got, sweep(api, kind, H, nq, k)), (nq, kind)


@cases
def test_subsets_equal_a_float64_topk_of_the_union(api, H, k, form):
    q, b, probes, got = subsets(api, H, k, form)
    exp = pc.brute(q, b, pc.SEGMENTS, probes, k)
    assert (exp["idx"][0] == -1).all() and (exp["idx"][1:, 0] >= 0).any()  # the unprobed query gets the tail alone
    assert pc.same_bits(got, exp)


@cases
def test_a_query_does_not_depend_on_the_cuts_or_its_company(api, H, k, form):
    q, b, probes, base = subsets(api, H, k, form)
    small = 4 * k * 8 * 70  # 70 queries of at most four lists each
    assert api.op_bank_probe_plan(200, pc.NB, H, pc.SEGMENTS, probes, k, 1, small, form)["npass"] >= 3
    assert pc.same_bits(api.op_bank_probe(q, b, pc.SEGMENTS, probes, k, piece_tiles=1, pass_bytes=small, force_form=form), base)
    assert pc.same_bits(api.op_bank_probe(q, b, pc.SEGMENTS, probes, k, piece_tiles=8, force_form=form), base)
    perm = np.random.default_rng(3).permutation(200)
    got = api.op_bank_probe(q[perm], b, pc.SEGMENTS, probes[perm], k, force_form=form)
    assert pc.same_bits(got, {key: base[key][perm] for key in base})
    few = api.op_bank_probe(q[5:8], b, pc.SEGMENTS, probes[5:8, ::-1], k, force_form=form)  # three of them alone, slots reversed
    assert pc.same_bits(few, {key: base[key][5:8] for key in base})


@pytest.mark.parametrize("form", pc.FORMS)
def test_long_pieces_and_a_deep_k_loop(api, form):
    """A piece of 700 rows (a wave of the narrow form walks its groups in three rounds; six column tiles in the wide form) at hpad = 320
    (two four-step rounds of the narrow K loop and a two-step rest), against bank_topk."""
    q, b = pc.mc.gaussian_tokens(19, 264, 1), pc.mc.gaussian_tokens(900, 264, 2)
    segments, probes = [(100, 700), (0, 100), (800, 100)], np.tile(np.array([[2, 0, 1]], np.int32), (19, 1))
    got = api.op_bank_probe(q, b, segments, probes, 7, piece_tiles=8, force_form=form)
    assert pc.same_bits(got, api.op_bank_topk(q, b, 7))


def test_session_call_on_resident_patches(api, golden_dir):
    model = api.Model(os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), classify=True)
    sess = api.Session(model)
    img = np.random.default_rng(17).standard_normal((2, 3, 84, 112)).astype(np.float32)
    tok = sess.predict(img, classify=False, want=("patch_tokens",))["patch_tokens"]
    P, H = tok.shape[1:]
    bank = api.Bank(model, H, 2 * P)
    assert [bank.add(sess, source="last_patches", image=i) for i in (0, 1)] == [0, P]
    segments = [(0, 7), (7, P - 7), (P, P // 2), (P + P // 2, P - P // 2)]
    rng = np.random.default_rng(5)
    probes = np.stack([rng.permutation(4)[:3] for _ in range(P)]).astype(np.int32)
    probes[rng.random(probes.shape) < 0.3] = -1
    got = bank.topk_probe(sess, source="last_patches", image=1, segments=segments, probes=probes, k=5)
    exp = api.op_bank_probe(tok[1], tok.reshape(2 * P, H), segments, probes, 5)
    assert pc.same_bits(got, exp) and (got["idx"] >= 0).any()
    assert pc.same_bits(bank.topk_probe(sess, tok[1], segments, probes, 5), got)
    with pytest.raises(api.DinoError, match="query 3 probes segment 2 twice"):
        bank.topk_probe(sess, tok[1], segments, np.where(np.arange(P)[:, None] == 3, 2, probes), 5)
    bank.free()
