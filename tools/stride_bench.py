#!/usr/bin/env python3
"""Times dinov2_hip_load_opts.patch_stride against the only route a user had before it: the EXPANDED image (every patch of the dense grid
laid out next to the others: 1022 x 1022 for 518 x 518 at stride 7) through the unchanged default path.  Synthetic ViT-L/14 with 4 registers,
f16, 518 x 518; stride 7 at batch 1 and 8 (42 672 token rows: as many as the default path's batch 32), stride 2 at batch 1 (64 014 token
rows in ONE image: it fills the chip alone).  Both routes compute the same bits (tests/test_gpu_stride.py); the tool checks the CLS rows.
  (a) the im2col kernel per launch, from the session profile (an event pair around the launch): the strided kernel on the image, the
      default kernel on the expanded image
  (b) images / s of the whole forward, no outputs: device-resident input for both routes, and host input (pageable numpy arrays, as
      Session.predict takes them) where the expanded route uploads (p / s)^2 times the pixels.  The host-side expansion itself is NOT
      counted (it is numpy fancy indexing here; a user's cost will differ), which favours the expanded route.
Calls of the two routes alternate; host clock around calls that end in a stream synchronise; median and minimum of `--calls` after `--warmup`.
The in-kernel clock of the box (FFN-in GEMM: shader cycles over 100 MHz ticks) over the whole run goes with the numbers.

    python tools/stride_bench.py [--calls 10] [--warmup 2] [--json out.json]
"""
import argparse, json, os, sys, tempfile, time
import ctypes as C
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--json", default=None)
ap.add_argument("--cases", default="7:1,7:8,2:1", help="stride:batch, comma separated")
args = ap.parse_args()
import torch
torch.cuda.init()  # (before the library touches the device; no GPU: this raises)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from importlib import import_module
from __graft_entry__ import PKG_NAME, load_package
pkg = load_package(); api = import_module(PKG_NAME + ".api")

SIZE, PATCH = 518, 14
path = os.path.join(tempfile.gettempdir(), "stride_bench_large_reg4.gguf")
if not os.path.exists(path):
    pkg.synth.write_synthetic_gguf(path, "large", registers=4, num_classes=0, seed=42)


def clock():
    c, t = C.c_uint64(), C.c_uint64()
    assert api.lib().dinov2_hip_op_clock_probe(C.byref(c), C.byref(t)) == 0
    return c.value, t.value


def expand(img, s):  # [B, 3, h, w] -> [B, 3, h0 p, w0 p]
    n = (img.shape[2] - PATCH) // s + 1
    idx = (np.arange(n)[:, None] * s + np.arange(PATCH)[None, :]).reshape(-1)
    return np.ascontiguousarray(img[:, :, idx][:, :, :, idx])


def stats(v, B):
    v = np.sort(np.asarray(v))
    return {"median_ms": float(np.median(v)), "min_ms": float(v[0]), "images_per_s": float(B * 1e3 / np.median(v))}


def timed(fns, sync, calls, warmup):
    ts = {k: [] for k in fns}
    for it in range(warmup + calls):
        for k, fn in fns.items():
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if it >= warmup:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    return ts


def kernel_us(sess, fn, kind, n=5):
    fn(); sess.sync()
    sess.profile(True)
    for _ in range(n):
        fn()
    prof = sess.profile_read()
    sess.profile(False)
    total = sum(ms for ms, cnt in prof.values())
    ms, cnt = prof[kind]
    assert cnt == n, (kind, prof)
    return ms * 1e3 / cnt, ms / total


results = {"build_id": api.build_id(), "device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup, "cases": []}
c0 = clock()
default = api.Model(path, classify=False)
sd = api.Session(default)
for case in args.cases.split(","):
    s, B = (int(v) for v in case.split(":"))
    calls, warmup = (args.calls, args.warmup) if s >= 7 else (max(3, args.calls // 3), 1)  # (stride 2: about a second per call)
    model = api.Model(path, classify=False, patch_stride=s)
    ss = api.Session(model)
    img = pkg.synth.synthetic_images(B, SIZE, SIZE, seed=s)
    E = expand(img, s)
    h0, w0 = model.grid(SIZE, SIZE)
    assert default.grid(*E.shape[2:]) == (h0, w0)
    dI, dE = torch.from_numpy(img).cuda(), torch.from_numpy(E).cuda()
    a = ss.predict(img, want=("cls",))["cls"]
    b = sd.predict(E, want=("cls",))["cls"]
    same = bool(np.array_equal(a, b))
    run_s = lambda: ss.predict_device(dI.data_ptr(), B, SIZE, SIZE, classify=False)
    run_e = lambda: sd.predict_device(dE.data_ptr(), B, E.shape[2], E.shape[3], classify=False)
    k_s, share_s = kernel_us(ss, run_s, "im2col_stride")
    k_e, share_e = kernel_us(sd, run_e, "im2col")
    sync = lambda: (ss.sync(), sd.sync())
    dev = timed({"strided": run_s, "expanded": run_e}, sync, calls, warmup)
    host = timed({"strided": lambda: ss.predict(img, want=()), "expanded": lambda: sd.predict(E, want=())}, sync, calls, warmup)
    r = {"stride": s, "batch": B, "grid": [h0, w0], "tokens_per_image": 5 + h0 * w0, "expanded_size": list(E.shape[2:]), "cls_bit_equal": same,
         "im2col_us_per_launch": {"strided_kernel_on_image": k_s, "default_kernel_on_expanded": k_e},
         "im2col_share_of_kernel_time": {"strided": share_s, "expanded": share_e},
         "col_bytes": int(B * h0 * w0 * 640 * 2), "image_bytes": int(img.nbytes), "expanded_bytes": int(E.nbytes),
         "forward_device_input": {k: stats(v, B) for k, v in dev.items()}, "forward_host_input": {k: stats(v, B) for k, v in host.items()}}
    results["cases"].append(r)
    print("stride %d batch %d: grid %d x %d, %d tokens / image, expanded %d x %d, cls bit-equal %s" % (s, B, h0, w0, 5 + h0 * w0, E.shape[2], E.shape[3], same))
    print("  (a) im2col per launch: strided kernel %.1f us (%.2f %% of the forward's kernel time), default kernel on the expanded image %.1f us (%.2f %%)"
          % (k_s, 100 * share_s, k_e, 100 * share_e))
    for tag, d in (("device input", r["forward_device_input"]), ("host input  ", r["forward_host_input"])):
        print("  (b) %s: strided %.2f ms (min %.2f) = %.2f img/s | expanded %.2f ms (min %.2f) = %.2f img/s | x %.3f"
              % (tag, d["strided"]["median_ms"], d["strided"]["min_ms"], d["strided"]["images_per_s"], d["expanded"]["median_ms"],
                 d["expanded"]["min_ms"], d["expanded"]["images_per_s"], d["expanded"]["median_ms"] / d["strided"]["median_ms"]))
    del ss, model, dI, dE
c1 = clock()
results["in_kernel_clock_ghz"] = (c1[0] - c0[0]) / ((c1[1] - c0[1]) * 10.0) if c1[1] > c0[1] else None
print("in-kernel clock over the run (FFN-in GEMM): %s GHz" % results["in_kernel_clock_ghz"])
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    json.dump(results, open(args.json, "w"), indent=1)
