"""api._images and api._grid: the one place the image argument of every predict is normalised and checked, and the patch grid that follows
from it.  No GPU; no library either, except test_grid_of_raw_input."""
import types

import numpy as np
import pytest


@pytest.mark.parametrize("layout, shape, dtype", [("RGB_CHW", (3, 28, 42), np.float32), ("BGR_HWC", (28, 42, 3), np.float32),
                                                  ("U8_BGR_HWC", (28, 42, 3), np.uint8)])
def test_images_one_image_and_batches(api, layout, shape, dtype):
    lay = getattr(api, layout)
    rng = np.random.default_rng(3)
    one = (rng.random(shape) * 255).astype(dtype)
    img, B, hh, ww = api._images(one, lay)
    assert (B, hh, ww) == (1, 28, 42) and img.shape == (1,) + shape and img.dtype == dtype and img.flags.c_contiguous
    assert np.array_equal(img[0], one)
    batch = np.stack([one, one[::-1].copy() if layout == "RGB_CHW" else one[:, ::-1].copy()])
    img, B, hh, ww = api._images(batch, lay)
    assert (B, hh, ww) == (2, 28, 42) and img.dtype == dtype and np.array_equal(img, batch)
    # a non-contiguous view becomes contiguous, the values kept
    wide = np.zeros((2, 3, 56, 84) if layout == "RGB_CHW" else (2, 56, 84, 3), dtype)
    view = wide[:, :, ::2, ::2] if layout == "RGB_CHW" else wide[:, ::2, ::2, :]
    view[...] = batch
    assert not view.flags.c_contiguous
    img, B, hh, ww = api._images(view, lay)
    assert img.flags.c_contiguous and (B, hh, ww) == (2, 28, 42) and np.array_equal(img, batch)


def test_images_dtypes(api):
    x64 = np.linspace(-1, 1, 2 * 3 * 14 * 14).reshape(2, 3, 14, 14)
    img, *_ = api._images(x64, api.RGB_CHW)
    assert img.dtype == np.float32 and np.array_equal(img, x64.astype(np.float32))
    u8 = np.arange(14 * 28 * 3, dtype=np.uint8).reshape(14, 28, 3)
    img, B, hh, ww = api._images(u8, api.U8_BGR_HWC)
    assert img.dtype == np.uint8 and (B, hh, ww) == (1, 14, 28)
    # debug_hidden's call: float32 whatever the layout
    img, B, hh, ww = api._images(u8, api.U8_BGR_HWC, np.float32)
    assert img.dtype == np.float32 and (B, hh, ww) == (1, 14, 28) and np.array_equal(img[0], u8.astype(np.float32))
    img, *_ = api._images(u8.astype(np.float64), api.BGR_HWC)
    assert img.dtype == np.float32


@pytest.mark.parametrize("layout, shape", [("RGB_CHW", (2, 1, 14, 14)), ("RGB_CHW", (2, 14, 14, 3)), ("BGR_HWC", (2, 14, 14, 4)),
                                           ("BGR_HWC", (2, 3, 14, 14)), ("U8_BGR_HWC", (2, 14, 14, 4)), ("RGB_CHW", (14, 14)),
                                           ("BGR_HWC", (14, 14)), ("RGB_CHW", (1, 2, 3, 14, 14)), ("RGB_CHW", (1, 14, 14)),
                                           ("BGR_HWC", (14, 14, 1))])
def test_images_refuses_other_shapes(api, layout, shape):
    """What Group always refused, with its text; Session used to hand such an array to the library, which reads B * 3 * H * W elements."""
    with pytest.raises(ValueError) as e:
        api._images(np.zeros(shape, np.float32), getattr(api, layout))
    shown = shape if len(shape) != 3 else (1,) + shape
    assert str(e.value) == f"expected [B, 3, H, W] (RGB_CHW) or [B, H, W, 3] images, got shape {shown}"


def test_grid(api):
    hp = types.SimpleNamespace(patch_size=14)
    for classify in (False, True):
        assert api._grid(hp, 56, 84, api.RGB_CHW, classify) == (56, 84, 24)
        assert api._grid(hp, 56, 84, api.BGR_HWC, classify) == (56, 84, 24)
        assert api._grid(hp, 60, 75, api.RGB_CHW, classify) == (60, 75, 20)  # (the library refuses such a size; the grid is floor division)
    assert api._grid(types.SimpleNamespace(patch_size=16), 64, 32, api.RGB_CHW, False) == (64, 32, 8)


def test_grid_of_raw_input(api):
    """Raw 8-bit input: the size after the preprocessing.  This one needs the built library: api.preprocess_size asks its host code
    (dinov2_hip_preprocess_size); still no GPU."""
    hp = types.SimpleNamespace(patch_size=14)
    assert api._grid(hp, 90, 123, api.U8_BGR_HWC, True) == (224, 224, 256)
    nh, nw = api.preprocess_size(0, 90, 123, 14)
    assert api._grid(hp, 90, 123, api.U8_BGR_HWC, False) == (nh, nw, (nh // 14) * (nw // 14)) == (98, 126, 63)
