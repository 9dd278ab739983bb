"""What intermediate-layer taps cost (dinov2_hip_predict_layers): synthetic ViT-L/14 + 4 registers, f16, 518 x 518, batch 32 and batch 1,
device-resident inputs and outputs.  Three arms, interleaved round by round so that clock and thermal drift hit all of them alike:

  (a) plain predict on a build of the PARENT commit (--parent-lib path/to/libdinov2_hip.so; runs in a child process, because the binding
      loads one library per process; skipped when not given)
  (b) plain predict on this tree
  (c) predict_layers with layers [5, 12, 18, 24], norm = 1, patch tokens + CLS, in TOKENS and in CHW layout

(b) against (a) is the no-regression reading; (c) - (b) is the price of four taps.  A profiled pass (HIP events per launch,
dinov2_hip_session_profile) then gives the tap kernel's own time next to the final LayerNorm's -- the existing kernel that moves about the
same bytes -- and the achieved bandwidth of both.  Prints one JSON line per batch size; --markdown FILE appends a table.

  python tools/layers_cost.py [--parent-lib LIB] [--rounds 7] [--iters 10] [--markdown profiles/intermediate_layers.md]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAYERS = [5, 12, 18, 24]
SIZE, H, R, P = 518, 1024, 4, 37 * 37


def setup(gguf, B):
    from importlib import import_module
    from __graft_entry__ import PKG_NAME, load_package
    pkg = load_package()
    api = import_module(PKG_NAME + ".api")
    sess = api.Session(api.Model(gguf, dtype=api.F16, classify=False))
    x = api.DeviceArray.from_host(pkg.synth.synthetic_images(B, SIZE, SIZE, seed=42))
    return api, sess, x


def timed(fn, sess, iters):
    sess.sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    sess.sync()
    return (time.perf_counter() - t0) * 1e3 / iters


def worker(gguf, B, iters, lib_path):
    """Arm (a): one line in -> `iters` plain predicts -> mean ms out.  The parent's library knows nothing of the new entry points, so it is
    driven through ctypes directly (the binding's structs, not its loader)."""
    import ctypes as C
    from importlib import import_module
    from __graft_entry__ import PKG_NAME, load_package
    pkg = load_package()
    api = import_module(PKG_NAME + ".api")
    L = C.CDLL(lib_path)
    hip = None
    for name in ("libamdhip64.so.7", "libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):  # the names api.DeviceArray tries
        try:
            hip = C.CDLL(name)
            break
        except OSError:
            continue
    assert hip is not None, "libamdhip64 not found"
    vp = C.c_void_p
    L.dinov2_hip_model_load.argtypes = [C.c_char_p, C.POINTER(api.LoadOpts), C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.dinov2_hip_session_create.argtypes = [vp, vp, C.POINTER(vp), C.c_char_p, C.c_size_t]
    L.dinov2_hip_predict.argtypes = [vp, C.POINTER(api.Input), C.POINTER(api.Output), C.c_uint32, C.c_char_p, C.c_size_t]
    L.dinov2_hip_session_sync.argtypes = [vp]
    L.dinov2_hip_default_load_opts.argtypes = [C.POINTER(api.LoadOpts)]
    hip.hipMalloc.argtypes = [C.POINTER(vp), C.c_size_t]
    hip.hipMemcpy.argtypes = [vp, vp, C.c_size_t, C.c_int]
    o = api.LoadOpts()
    L.dinov2_hip_default_load_opts(C.byref(o))
    o.compute_dtype, o.classify = api.F16, 0
    err = C.create_string_buffer(512)
    model, sess, x, out = vp(), vp(), vp(), vp()
    assert L.dinov2_hip_model_load(gguf.encode(), C.byref(o), C.byref(model), err, 512) == 0, err.value
    assert L.dinov2_hip_session_create(model, None, C.byref(sess), err, 512) == 0, err.value
    imgs = pkg.synth.synthetic_images(B, SIZE, SIZE, seed=42)
    assert hip.hipMalloc(C.byref(x), imgs.nbytes) == 0 and hip.hipMalloc(C.byref(out), 4 * B * P * H) == 0
    assert hip.hipMemcpy(x, imgs.ctypes.data, imgs.nbytes, 1) == 0
    i = api.Input(x.value, B, SIZE, SIZE, api.RGB_CHW, 1)
    oo = api.Output(None, out.value, None, None, None, None, 0, 1)

    class S:
        @staticmethod
        def sync():
            L.dinov2_hip_session_sync(sess)

    def run():
        assert L.dinov2_hip_predict(sess, C.byref(i), C.byref(oo), 0, err, 512) == 0, err.value
    timed(run, S, 3)
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() == "quit":
            break
        print(timed(run, S, iters), flush=True)


def read_line(child, what, timeout_s=300):
    """One line from the parent-library worker; a worker that died or hangs ends the tool with a message instead of a hang."""
    import select
    ready, _, _ = select.select([child.stdout], [], [], timeout_s)
    line = child.stdout.readline().strip() if ready else ""
    if not line:
        child.kill()
        raise RuntimeError(f"parent-library worker gave no {what} (exit status {child.poll()}, waited {timeout_s} s); "
                           "its messages are on stderr above")
    return line


def measure(gguf, B, rounds, iters, parent_lib):
    api, sess, x = setup(gguf, B)
    out = api.DeviceArray((B, P, H))
    taps = api.DeviceArray((len(LAYERS), B, P, H))
    tcls = api.DeviceArray((len(LAYERS), B, H))
    arms = {"b_plain": lambda: sess.predict_device(x.ptr, B, SIZE, SIZE, classify=False, patch_ptr=out.ptr)}
    for name, chw in (("c_tokens", False), ("c_chw", True)):
        arms[name] = lambda chw=chw: sess.predict_layers_device(x.ptr, B, SIZE, SIZE, LAYERS, norm=True, reshape=chw, patch_ptr=out.ptr,
                                                                layer_patch_ptr=taps.ptr, layer_cls_ptr=tcls.ptr)
    child = None
    if parent_lib:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", gguf, str(B), str(iters), os.path.abspath(parent_lib)],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        assert read_line(child, "ready line") == "ready"
    for fn in arms.values():
        timed(fn, sess, 3)
    ms = {k: [] for k in (["a_parent"] if child else []) + list(arms)}
    for _ in range(rounds):
        if child:
            child.stdin.write("go\n")
            child.stdin.flush()
            ms["a_parent"].append(float(read_line(child, "timing")))
        for k, fn in arms.items():
            ms[k].append(timed(fn, sess, iters))
    if child:
        child.stdin.write("quit\n")
        child.stdin.flush()
        child.wait(timeout=60)
    res = {"batch": B, "rounds": rounds, "iters": iters, "build": api.build_id()}
    for k, v in ms.items():
        res[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    # the kernels' own times: HIP events around every launch
    M = B * (1 + R + P)
    tap_bytes = 2 * 4 * B * (P + 1) * H  # patch + CLS rows read once, written once
    ln_bytes = 2 * 4 * M * H
    for name in ("c_tokens", "c_chw"):
        sess.profile(True)
        for _ in range(iters):
            arms[name]()
        prof = sess.profile_read()
        sess.profile(False)
        tap_us = prof["layer_tap"][0] * 1e3 / prof["layer_tap"][1]
        ln_us = prof["final_layernorm"][0] * 1e3 / prof["final_layernorm"][1]
        res[name + "_kernel"] = {"tap_us": tap_us, "tap_TBps": tap_bytes / tap_us / 1e6, "tap_launches": prof["layer_tap"][1],
                                 "final_ln_us": ln_us, "final_ln_TBps": ln_bytes / ln_us / 1e6}
    return res


def markdown(results):
    lines = ["| batch | arm | step ms (median, min - max) | tap kernel us | tap TB/s | final LN us | final LN TB/s |", "|---|---|---|---|---|---|---|"]
    for r in results:
        for k in ("a_parent", "b_plain", "c_tokens", "c_chw"):
            if k + "_ms" not in r:
                continue
            m, kern = r[k + "_ms"], r.get(k + "_kernel")
            tail = f"{kern['tap_us']:.1f} | {kern['tap_TBps']:.2f} | {kern['final_ln_us']:.1f} | {kern['final_ln_TBps']:.2f}" if kern else " | | | "
            lines.append(f"| {r['batch']} | {k} | {m['median']:.3f} ({m['min']:.3f} - {m['max']:.3f}) | {tail} |")
    return "\n".join(lines) + "\n"


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        return worker(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[32, 1])
    ap.add_argument("--markdown")
    a = ap.parse_args()
    from __graft_entry__ import load_package
    pkg = load_package()
    results = []
    with tempfile.TemporaryDirectory() as td:
        gguf = os.path.join(td, "large.gguf")
        pkg.synth.write_synthetic_gguf(gguf, "large", registers=R, num_classes=1000, seed=42)
        for B in a.batches:
            r = measure(gguf, B, a.rounds, a.iters if B > 1 else a.iters * 4, a.parent_lib)
            print(json.dumps(r), flush=True)
            results.append(r)
    if a.markdown:
        with open(a.markdown, "a") as f:
            f.write(markdown(results))


if __name__ == "__main__":
    main()
