"""tests/cpp/attention_smoke.cpp: include/dinov2_compat.hpp's dino_get_attention from a plain g++ caller."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "attention_smoke")
    libdir = os.path.join(ROOT, "dinov2.cpp_amd")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "attention_smoke.cpp"),
                           "-o", exe, "-L" + libdir, "-ldinov2_hip", "-Wl,-rpath," + libdir, "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_attention_helper_compiles_with_plain_gxx(tmp_path):
    exe = _build(tmp_path)
    r = subprocess.run([exe, "/nonexistent.gguf"], capture_output=True, text=True)
    assert r.returncode == 1 and "failed to open" in r.stderr


@pytest.mark.gpu
def test_cpp_attention_helper_runs(tmp_path, golden_dir):
    exe = _build(tmp_path)
    r = subprocess.run([exe, os.path.join(golden_dir, "tiny_gelu_reg4.gguf")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "attention: 2 layers, heads 2, keys 35; last layer patches only: 2 queries x 30 keys, grid 5 x 6" in r.stdout, r.stdout
    assert "outside 1 .." in r.stderr
