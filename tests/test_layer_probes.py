"""The numpy restatement of the layer taps (tests/layer_cases.py) through the very checks tests/test_gpu_layers.py applies to the library,
and the planted bugs those checks must reject; plus the declarations, exports and struct layout of the new C-ABI.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import layer_cases as lc
import misc_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, B, R, H, H0, W0 = 3, 5, 4, 64, 3, 5  # h0 != w0, B > chunk, R > 0: every planted bug has something to get wrong
LAYERS = [0, 2, 3]


def _streams():
    rng = np.random.default_rng(0)
    T = 1 + R + H0 * W0
    raw = rng.standard_normal((L + 1, B, T, H)).astype(np.float32)
    w, b = mc.ln_affine(H, 1)
    w1, b1 = mc.ln_affine(H, 2)  # "a layer's own norm1"
    normed = mc.ln_emulate(raw.reshape(-1, H), w, b, 1e-6, mc.F32).reshape(raw.shape)
    wrong = mc.ln_emulate(raw.reshape(-1, H), w1, b1, 1e-6, mc.F32).reshape(raw.shape)
    return raw, normed, wrong


@pytest.mark.parametrize("layout", [lc.TOKENS, lc.CHW])
@pytest.mark.parametrize("norm", [0, 1])
def test_restatement_passes_the_gpu_checks(norm, layout):
    raw, normed, wrong = _streams()
    stream = normed if norm else raw
    for chunk in (None, 2):
        got = lc.request(stream, LAYERS, R, H0, W0, layout, chunk=chunk)
        ok, msg = lc.check_taps(got, stream, LAYERS, R, H0, W0, layout, "restatement")
        assert ok, msg
    # CHW is a pure permutation of TOKENS
    t = lc.request(stream, LAYERS, R, H0, W0, lc.TOKENS)["patch"]
    c = lc.request(stream, LAYERS, R, H0, W0, lc.CHW)["patch"]
    assert c.shape == (len(LAYERS), B, H, H0, W0)
    ok, msg = mc.check_exact(c.reshape(len(LAYERS), B, H, H0 * W0).transpose(0, 1, 3, 2), t, "CHW vs TOKENS")
    assert ok, msg
    assert c[1, 2, 7, 1, 3] == stream[LAYERS[1], 2, 1 + R + 1 * W0 + 3, 7]  # element (c, y, x) = channel c of patch y * w0 + x


# (h0 / w0 only enter the CHW layout)
@pytest.mark.parametrize("mutant,layout", [(m, lo) for m in lc.MUTANTS for lo in (lc.TOKENS, lc.CHW) if (m, lo) != ("hw_swapped", lc.TOKENS)])
def test_planted_bugs_are_rejected(mutant, layout):
    raw, normed, wrong = _streams()
    got = lc.request(normed, LAYERS, R, H0, W0, layout, mutant=mutant, wrong_stream=wrong, chunk=2)
    ok, msg = lc.check_taps(got, normed, LAYERS, R, H0, W0, layout, mutant)
    assert not ok, f"planted bug {mutant} passed the checks"
    assert msg


def test_new_symbols_are_declared_and_exported(api):
    """Declared in the headers and exported by the built library (a library that is not there fails here, as in
    test_library_exports_every_declared_symbol, which then holds them to declared == exported)."""
    hdr = open(os.path.join(ROOT, "include", "dinov2_hip.h")).read()
    ops = open(os.path.join(ROOT, "include", "dinov2_hip_ops.h")).read()
    assert re.search(r"\bint dinov2_hip_predict_layers\(", hdr) and "typedef struct dinov2_hip_layers" in hdr
    assert re.search(r"\bint dinov2_hip_op_layer_tap\(", ops)
    api.lib()
    out = subprocess.check_output(["nm", "-D", "--defined-only", api.LIB_PATH], text=True)
    exported = set(re.findall(r" T (dinov2_hip_[a-z0-9_]+)", out))
    assert {"dinov2_hip_predict_layers", "dinov2_hip_op_layer_tap"} <= exported


def test_ctypes_struct_matches_the_header(api, tmp_path):
    cxx = "g++"  # as tests/test_gguf_and_abi.py and tests/test_layers_cpp.py: no guard, a missing compiler fails
    src = tmp_path / "sz.cpp"
    src.write_text('#include <cstdio>\n#include <cstddef>\n#include "dinov2_hip.h"\n'
                   'int main() { std::printf("%zu %zu %zu %zu\\n", sizeof(dinov2_hip_layers), offsetof(dinov2_hip_layers, patch_tokens), '
                   'offsetof(dinov2_hip_layers, on_device), offsetof(dinov2_hip_layers, reserved)); }\n')
    exe = tmp_path / "sz"
    subprocess.run([cxx, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, timeout=120)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Ly = api.Layers
    assert got == [C.sizeof(Ly), Ly.patch_tokens.offset, Ly.on_device.offset, Ly.reserved.offset]
