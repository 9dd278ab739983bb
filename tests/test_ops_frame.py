"""csrc/ops_frame.h, the host-only half of the diagnostic ops' device harness (csrc/ops_testing.cpp): no GPU, no library."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ops_frame_under_sanitizers(tmp_path):
    """tests/cpp/ops_frame_san.cpp built with AddressSanitizer + UndefinedBehaviorSanitizer.  Frames [ng | n | ng] of esz-byte elements, esz in
    {1, 2, 4, 8}, n in {0, 1, 7, 4096}, ng in {0, 3, 5, 128, 128 * 37}, payload edge bytes 0xff and not, on exactly sized heap buffers: an untouched
    frame hands back the payload; one flipped bit in the first or last byte of either band reads as changed.  Widening: all 65 536 f16 and
    bf16 patterns, from an odd address, against a decode from the definition (bit for bit; NaN by NaN-ness)."""
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.skip("ROCm clang not available")
    flags = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    # a skip only where the sanitizer runtimes themselves are missing: an empty program does not link with them
    empty = tmp_path / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    r = subprocess.run([cxx, *flags, str(empty), "-o", str(tmp_path / "empty")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    exe = str(tmp_path / "ops_frame_san")
    r = subprocess.run([cxx, *flags, os.path.join(ROOT, "tests", "cpp", "ops_frame_san.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.startswith("ops_frame: 240 frames, 2 x 65536 values OK"), r.stdout
