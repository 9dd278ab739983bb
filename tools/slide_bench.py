#!/usr/bin/env python3
"""Times dinov2_hip_predict_dense_slide (csrc/slide.hip, csrc/slide.cpp) on a synthetic ViT-L/14 with 4 registers: one street-scene image of
1024 x 2048, crop 518, stride 345 (about 2/3 of the crop: 3 x 6 = 18 windows), taps 5 / 12 / 18 / 24, argmax heads of C = 19 and C = 150.
Legs, on the same device in the same run:
  slide_device   device image in, device labels out: HIP events on the session's stream around the call (median, min, p90 of --calls)
  slide_host     host image in, host labels out: host wall clock around the call
  stages         from dinov2_hip_session_profile: a profiled slide call against a profiled dinov2_hip_predict_dense of the same window batch
                 with `logits` out -- gather = the difference of the "im2col" kind, reduce = the difference of the "head" kind, forward = all
                 kinds of the predict_dense call (patch embedding, blocks, packing, the logits GEMM)
  host_route     what a caller had before this call, host wall clock: crops cut on the host (every overlap uploaded twice), ONE
                 dinov2_hip_predict_dense over the window batch with `logits` out to the host, then numpy -- every window's logits resampled
                 to the crop (bilinear, float32), accumulated into C full-resolution planes, divided by the count, argmax
and writes the table to --md (default profiles/dense_slide.md).

    python tools/slide_bench.py [--calls 10] [--warmup 2] [--host-calls 2] [--md profiles/dense_slide.md] [--json out.json]
"""
import argparse, json, os, sys, tempfile, time
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--host-calls", type=int, default=2)
ap.add_argument("--md", default=None)
ap.add_argument("--json", default=None)
args = ap.parse_args()
import torch
torch.cuda.init()  # (before the library touches the device: torch's lazy init fails when it comes second; no GPU: this raises)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from importlib import import_module
from __graft_entry__ import PKG_NAME, load_package
pkg = load_package(); api = import_module(PKG_NAME + ".api")

path = os.path.join(tempfile.gettempdir(), "dense_bench_large_reg4.gguf")
if not os.path.exists(path):
    pkg.synth.write_synthetic_gguf(path, "large", registers=4, num_classes=0, seed=42)
model = api.Model(path, classify=False)
sess = api.Session(model)
stream = torch.cuda.ExternalStream(sess.stream)
LAYERS, HID, IMG_H, IMG_W, CROP, STRIDE, G = [5, 12, 18, 24], 1024, 1024, 2048, 518, 345, 37
rng = np.random.default_rng(1)
y1, x1 = model.slide_windows(IMG_H, IMG_W, CROP, STRIDE)
NWIN, P = len(y1) * len(x1), G * G


def stats(v):
    v = np.sort(np.asarray(v, np.float64))
    return {"median_ms": float(np.median(v)), "min_ms": float(v[0]), "p90_ms": float(v[int(0.9 * (len(v) - 1))]), "n": int(len(v))}


def axis(n_in, n_out):
    src = np.maximum(np.float32(n_in) / np.float32(n_out) * (np.arange(n_out, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5), np.float32(0))
    i0 = np.minimum(src.astype(np.int32), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), src - i0.astype(np.float32)


def host_route(img, head, C_):
    """The caller's own sliding window around predict_dense: (labels [h, w], seconds spent in numpy after the call)."""
    crops = np.stack([img[:, y:y + CROP, x:x + CROP] for y in y1 for x in x1])
    lg = sess.predict_dense(crops, head, want=("logits",))["logits"]  # [windows, P, C]
    t0 = time.perf_counter()
    i0, i1, lam = axis(G, CROP)
    a, b = lam[None, :, None], lam[:, None, None]
    acc = np.zeros((IMG_H, IMG_W, C_), np.float32)
    cnt = np.zeros((IMG_H, IMG_W, 1), np.float32)
    for k in range(NWIN):
        g = lg[k].reshape(G, G, C_)
        top = (1 - a) * g[i0][:, i0] + a * g[i0][:, i1]
        bot = (1 - a) * g[i1][:, i0] + a * g[i1][:, i1]
        y, x = int(y1[k // len(x1)]), int(x1[k % len(x1)])
        acc[y:y + CROP, x:x + CROP] += (1 - b) * top + b * bot
        cnt[y:y + CROP, x:x + CROP] += 1
    labels = np.argmax(acc / cnt, axis=2).astype(np.uint8)
    return labels, time.perf_counter() - t0


def profile_of(fn, n):
    sess.profile(True)
    for _ in range(n):
        fn()
    sess.sync()
    prof = sess.profile_read()
    sess.profile(False)
    return {k: v[0] / n for k, v in prof.items()}


results = {"build_id": api.build_id(), "device": torch.cuda.get_device_name(0), "image": [IMG_H, IMG_W], "crop": CROP, "stride": STRIDE,
           "windows": [len(y1), len(x1)], "calls": args.calls, "warmup": args.warmup, "host_calls": args.host_calls, "classes": {}}
img = rng.standard_normal((1, 3, IMG_H, IMG_W)).astype(np.float32)
x = torch.from_numpy(img).cuda()
labels = torch.empty((1, IMG_H, IMG_W), dtype=torch.uint8, device="cuda")
win = torch.from_numpy(np.stack([img[0][:, y:y + CROP, x_:x_ + CROP] for y in y1 for x_ in x1])).cuda()
torch.cuda.synchronize()
for C_ in (19, 150):
    K = len(LAYERS) * HID
    head = api.DenseHead(model, LAYERS, (rng.standard_normal((C_, K)) * (4.0 / np.sqrt(K))).astype(np.float32),
                         rng.standard_normal(C_).astype(np.float32), norm=True, concat_cls=False)
    lgw = torch.empty((NWIN, P, C_), device="cuda")
    slide = lambda: sess.predict_dense_slide_device(x.data_ptr(), 1, IMG_H, IMG_W, head, CROP, STRIDE, labels_ptr=labels.data_ptr())
    batch = lambda: sess.predict_dense_device(win.data_ptr(), NWIN, CROP, CROP, head, logits_ptr=lgw.data_ptr())
    ts = []
    for it in range(args.warmup + args.calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record()
            slide()
            e1.record()
        e1.synchronize()
        if it >= args.warmup:
            ts.append(e0.elapsed_time(e1))
    dev_labels = labels.cpu().numpy()[0]
    th = []
    for it in range(1 + args.host_calls):
        t0 = time.perf_counter()
        r = sess.predict_dense_slide(img, head, CROP, STRIDE, want=("labels",))
        if it:
            th.append(1e3 * (time.perf_counter() - t0))
    assert np.array_equal(r["labels"][0], dev_labels)
    ps, pb = profile_of(slide, args.calls), profile_of(batch, args.calls)
    tr, tn = [], []
    for it in range(args.host_calls):
        t0 = time.perf_counter()
        ref_labels, numpy_s = host_route(img[0], head, C_)
        tr.append(1e3 * (time.perf_counter() - t0))
        tn.append(1e3 * numpy_s)
    agree = float((ref_labels == dev_labels).mean())
    stages = {"gather_ms": ps["im2col"] - pb["im2col"], "reduce_ms": ps["head"] - pb["head"], "forward_ms": sum(pb.values()),
              "profiled_call_ms": sum(ps.values())}
    results["classes"][str(C_)] = {"slide_device": stats(ts), "slide_host": stats(th), "stages": stages, "host_route": stats(tr),
                                   "host_route_numpy": stats(tn), "labels_agree_with_host_route": agree}
    print("C = %3d  slide_device median %.2f ms  slide_host %.2f ms  host_route %.1f ms (numpy %.1f ms)  gather %.3f  forward %.2f  reduce %.3f ms"
          "  labels agree %.5f" % (C_, stats(ts)["median_ms"], stats(th)["median_ms"], stats(tr)["median_ms"], stats(tn)["median_ms"],
                                   stages["gather_ms"], stages["forward_ms"], stages["reduce_ms"], agree))
print(json.dumps(results))
if args.json:
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
if args.md:
    L = ["# Sliding-window dense inference: times", "",
         "Written by `tools/slide_bench.py` (library build `%s`, %s).  Synthetic ViT-L/14 with 4 registers, f16; one image of %d x %d, crop %d, "
         "stride %d: %d x %d = %d windows; taps 5 / 12 / 18 / 24 (K = 4 096), argmax heads.  `slide_device`: device image in, device labels out, "
         "HIP events on the session's stream, %d calls after %d warm-up calls.  `slide_host` and `host_route`: host wall clock, %d calls after "
         "one.  Stage times: HIP events per launch (`dinov2_hip_session_profile`), mean per call over %d calls; the events themselves cost "
         "time, so the stages add up to more than an unprofiled call."
         % (results["build_id"], results["device"], IMG_H, IMG_W, CROP, STRIDE, len(y1), len(x1), NWIN, args.calls, args.warmup, args.host_calls,
            args.calls), "",
         "| C | slide_device median (min, p90) ms | slide_host median ms | host_route median ms | of it numpy ms | labels equal to host_route |",
         "|---|---|---|---|---|---|"]
    for C_, r in results["classes"].items():
        L.append("| %s | %.2f (%.2f, %.2f) | %.1f | %.1f | %.1f | %.3f %% |" % (
            C_, r["slide_device"]["median_ms"], r["slide_device"]["min_ms"], r["slide_device"]["p90_ms"], r["slide_host"]["median_ms"],
            r["host_route"]["median_ms"], r["host_route_numpy"]["median_ms"], 100 * r["labels_agree_with_host_route"]))
    L += ["", "| C | gather ms | forward + head GEMM ms | reduce ms | reduce share of the profiled call |", "|---|---|---|---|---|"]
    for C_, r in results["classes"].items():
        s = r["stages"]
        L.append("| %s | %.3f | %.2f | %.3f | %.2f %% |" % (C_, s["gather_ms"], s["forward_ms"], s["reduce_ms"], 100 * s["reduce_ms"] / s["profiled_call_ms"]))
    L += ["", "`host_route` is the route a caller had before this call: crops cut on the host, one `predict_dense` over the window batch with "
          "`logits` out, numpy float32 resampling, averaging and argmax (the upload, the forward and the download of the logits are inside "
          "`host_route`, the numpy part is listed beside it).  The forward is the same work on both routes; what the call removes is the "
          "host-side planes.", ""]
    with open(args.md, "w") as f:
        f.write("\n".join(L))
