"""CPU side of the patch_stride tests: the closed forms of tests/stride_cases.py against brute force, the limits of the strided im2col
restated from its conditions, the expansion identity in numpy, and the refusals of dinov2_hip_model_load that need no device."""
import os
import re

import numpy as np
import pytest

import stride_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_footprint_against_brute_force():
    """Every pixel of small images, several (patch, stride) pairs: the closed form lists exactly the col elements a brute-force gather of a
    one-hot image lights up, never more than (p / s)^2 of them, one when the pixel is a corner."""
    for p, s, h, w in [(14, 7, 28, 42), (14, 2, 16, 20), (14, 1, 16, 17), (4, 2, 8, 10), (4, 4, 8, 12), (6, 3, 6, 6),
                       (2, 1, 4, 24), (3, 1, 5, 33), (5, 1, 7, 9), (6, 2, 10, 12), (7, 1, 9, 11)]:
        Kpad = (3 * p * p + 7) // 8 * 8
        for b, c, y, x in [(b, c, y, x) for b in range(2) for c in range(3) for y in range(h) for x in range(w)][::7]:
            rgb = np.zeros((2, 3, h, w), np.float32)
            rgb[b, c, y, x] = 1.0
            lit = {(int(r), int(k)) for r, k in zip(*np.nonzero(sc.col_reference(rgb, p, s, Kpad)))}
            got = sc.footprint(b, c, y, x, h, w, p, s)
            assert len(got) == len(set(got)) and set(got) == lit, (p, s, y, x)
            assert 1 <= len(got) <= (p // s) ** 2
        assert len(sc.footprint(0, 0, 0, 0, h, w, p, s)) == 1 and len(sc.footprint(1, 2, h - 1, w - 1, h, w, p, s)) == 1
        if h >= 2 * p - s and w >= 2 * p - s:  # an interior pixel of a grid that is large enough is under the full count
            assert len(sc.footprint(0, 1, p - 1, p - 1, h, w, p, s)) == (p // s) ** 2


def test_expansion_identity():
    """The default im2col of the expanded image is the strided im2col of the image, grid included: the identity every GPU test rests on."""
    rng = np.random.default_rng(0)
    for p, s, h, w in [(14, 7, 28, 42), (14, 2, 16, 20), (14, 1, 16, 17), (16, 4, 32, 48), (8, 1, 16, 20), (14, 14, 28, 42)] + \
            sc.SMALL_KERNEL + [(p, s, h, w) for p, s, _, h, w in sc.SYNTH]:
        rgb = rng.standard_normal((2, 3, h, w)).astype(np.float32)
        E = sc.expand(rgb, p, s)
        h0, w0 = sc.grid(h, w, p, s)
        assert E.shape == (2, 3, h0 * p, w0 * p) and sc.grid(h0 * p, w0 * p, p, p) == (h0, w0)
        assert np.array_equal(sc.col_reference(E, p, p, sc.kpad(p)), sc.col_reference(rgb, p, s, sc.kpad(p)))
        hwc = np.ascontiguousarray(rgb.transpose(0, 2, 3, 1))
        assert np.array_equal(sc.expand(hwc, p, s, axes=(1, 2)), E.transpose(0, 2, 3, 1))
        if s == p:
            assert np.array_equal(E, rgb)


def test_limits_restated_from_the_kernel():
    """im2col_stride_ok as csrc/kernels.h states it: read the constants from the header, then walk the pairs.  Every divisor of every patch
    size the loader takes (1 .. 32) is inside; the strip of 3 p rows of ten patch widths stops fitting 64 KiB at patch 34 whatever the
    stride, and patch 33 is the last inside."""
    src = open(os.path.join(ROOT, "dinov2.cpp_amd", "csrc", "kernels.h")).read()
    assert int(re.search(r"constexpr int IM2COL_CHUNK = (\d+);", src).group(1)) == sc.IM2COL_CHUNK
    body = src[src.index("inline bool im2col_stride_ok"):]
    body = body[:body.index("\n}\n")]
    assert "64 * 1024" in body and "patch % stride != 0" in body and ">> 20" in body and "32768" in body
    assert "(IM2COL_CHUNK - 1) * patch / stride + 1" in src and "(((width + 1) / 2) | 1) * 2" in src
    for p in range(1, 33):
        for s in range(1, p + 1):
            assert sc.stride_ok(p, s, sc.kpad(p)) == (p % s == 0), (p, s)
            if p % s == 0:
                width = (sc.run(p, s) - 1) * s + p
                assert width <= sc.IM2COL_CHUNK * p  # the strip never outgrows the default kernel's ten patch widths
                assert (sc.pitch(p, s) // 2) % 2 == 1 and sc.pitch(p, s) >= width  # an odd number of dwords, the whole strip inside
    assert sc.stride_ok(33, 11, sc.kpad(33)) and sc.stride_ok(33, 33, sc.kpad(33))
    assert not any(sc.stride_ok(34, s, sc.kpad(34)) for s in (1, 2, 17, 34))
    assert not sc.stride_ok(14, 7, 588) and not sc.stride_ok(14, 7, 584)  # Kpad: a multiple of 8 that holds 3 p^2
    assert sc.run(14, 14) == 10 and sc.run(14, 7) == 19 and sc.run(14, 2) == 64 and sc.run(14, 1) == 127


def test_small_patch_cases_sit_where_the_comments_say():
    """Every (patch, stride) of SMALL_PS is inside the kernel's limits, with one grid row of exactly one run and one of more; the synthetic
    checkpoints' sizes are on their strides and give the grids the comment names."""
    assert sc.SMALL_PS == [(p, s) for p in range(2, 8) for s in range(1, p) if p % s == 0]  # every proper divisor of every patch 2 .. 7
    assert {p for p, _ in sc.SMALL_PS} == {2, 3, 4, 5, 6, 7} and len(sc.SMALL_KERNEL) == 2 * len(sc.SMALL_PS)
    assert [sc.run(p, s) for p, s in sc.SMALL_PS] == [19, 28, 37, 19, 46, 55, 28, 19, 64]
    for p, s, h, w in sc.SMALL_KERNEL:
        assert sc.stride_ok(p, s, sc.kpad(p)) and (h - p) % s == 0 and (w - p) % s == 0
        h0, w0 = sc.grid(h, w, p, s)
        assert h0 == 3 and w0 in (sc.run(p, s), sc.run(p, s) + 2)
    for p, s in sc.SMALL_PS:
        assert sorted(sc.grid(h, w, p, s)[1] > sc.run(p, s) for q, t, h, w in sc.SMALL_KERNEL if (q, t) == (p, s)) == [False, True]
    small = [c for c in sc.SYNTH if c[0] < 8]
    assert [(p, s) for p, s, _, _, _ in small] == [(2, 1), (3, 1), (4, 2), (6, 2), (6, 3), (7, 1)]
    assert [sc.grid(h, w, p, s) for p, s, _, h, w in small] == [(4, 7), (4, 5), (3, 5), (3, 4), (2, 4), (4, 6)]
    assert all(img == 4 * p and (h - p) % s == 0 and (w - p) % s == 0 for p, s, img, h, w in small)


def test_sizes_sit_where_the_comments_say():
    w0 = lambda s, w: sc.grid(14, w, 14, s)[1]
    assert (w0(7, 77), w0(7, 84), w0(7, 140), w0(7, 147), w0(7, 154)) == (10, 11, 19, 20, 21)
    assert (w0(2, 140), w0(2, 142), w0(1, 30), w0(1, 141)) == (64, 65, 17, 128)
    assert sc.grid(14, 14, 14, 7) == (1, 1) and sc.grid(28, 42, 14, 7) == (3, 5) and sc.grid(28, 28, 14, 1) == (15, 15)
    for s, h, w in sc.SIZES_14:
        assert (h - 14) % s == 0 and (w - 14) % s == 0
    R = 4
    assert (sc.OVER - 13) ** 2 + 1 + R == 702249 > sc.LIMIT_ROWS == 699050 > (sc.UNDER - 13) ** 2 + 1 + R == 698901


@pytest.mark.parametrize("stride", [3, 15, -1, 28])
def test_load_refuses_a_stride_that_does_not_divide_the_patch(api, golden_dir, stride):
    """Before the loader touches a device: DINOV2_HIP_ERR_UNSUPPORTED, a message that names the value and the rule."""
    with pytest.raises(api.DinoError) as e:
        api.Model(os.path.join(golden_dir, "tiny_gelu_reg4.gguf"), patch_stride=stride)
    assert e.value.status == 3 and "patch_stride %d" % stride in str(e.value) and "divide patch_size 14" in str(e.value)


def test_load_refuses_patch_33_whatever_the_stride(api, pkg, tmp_path):
    """Patch 33 at stride 11 is inside im2col_stride_ok, but the default kernel's limit (patch 32) comes first and names the patch size."""
    path = str(tmp_path / "p33.gguf")
    pkg.synth.write_synthetic_gguf(path, sc.synth_config(33, 66), registers=0, num_classes=4)
    with pytest.raises(api.DinoError) as e:
        api.Model(path, patch_stride=11)
    assert e.value.status == 3 and "patch_size 33" in str(e.value)


def test_default_opts_and_abi(api):
    """The option took reserved[0]: the struct keeps its size, the ABI version its value, the default is 0; the two new calls exist."""
    import ctypes as C
    o = api.LoadOpts()
    api.lib().dinov2_hip_default_load_opts(C.byref(o))
    assert o.patch_stride == 0 and C.sizeof(api.LoadOpts) == 16 * 4 and api.LoadOpts.patch_stride.offset == 8 * 4
    assert api.lib().dinov2_hip_abi_version() == 1
    assert api.lib().dinov2_hip_model_patch_stride(None) == 0
    h0, w0 = C.c_int32(), C.c_int32()
    err = C.create_string_buffer(256)
    assert api.lib().dinov2_hip_model_grid(None, 28, 28, C.byref(h0), C.byref(w0), err, len(err)) != 0 and err.value


def test_python_grid_is_the_one_definition(api):
    """api._grid / Model.tokens go through api._grid_dims; with a stride it is the rule of the header."""
    from types import SimpleNamespace as NS
    assert api._grid_dims(NS(patch_size=14), 56, 84) == (4, 6)
    assert api._grid_dims(NS(patch_size=14, patch_stride=0), 56, 84) == (4, 6)
    assert api._grid_dims(NS(patch_size=14, patch_stride=7), 56, 84) == (7, 11)
    assert api._grid(NS(patch_size=14, patch_stride=7), 56, 84, api.RGB_CHW, False) == (56, 84, 77)
    assert api._grid(NS(patch_size=14, patch_stride=2), 45, 61, api.U8_BGR_HWC, False)[:2] == api.preprocess_size(0, 45, 61, 14)
    src = open(os.path.join(ROOT, "dinov2.cpp_amd", "api.py")).read() + open(os.path.join(ROOT, "dinov2.cpp_amd", "inference.py")).read()
    assert not re.search(r"//\s*(hp\.|self\.hparams\.)?(patch_size|ps)\b", src), "a grid computed by dividing by the patch size"
