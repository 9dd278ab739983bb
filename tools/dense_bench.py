#!/usr/bin/env python3
"""Times dinov2_hip_predict_dense (csrc/dense.hip) with device-resident input and outputs on a synthetic ViT-L/14 with 4 registers at
518 x 518, batch 32 and batch 1, taps 5 / 12 / 18 / 24: a segmentation head (C = 150, argmax at the input size, K = 4 096) and a depth head
(C = 256, bins at 4 h0 x 4 w0, patch and CLS concatenated, K = 8 192).  HIP events on the session's stream around every call; the calls of one
batch size alternate; median and spread of `--calls` calls after `--warmup`.  Next to them, on the same device in the same run:
  forward        dinov2_hip_predict with no outputs: what the dense stage is added to
  (a) layers     dinov2_hip_predict_layers of the same taps with device outputs [4, B, P, H] f32: what a caller had before this call
  (b) torch      the planes materialised: F.interpolate(bilinear, align_corners=False) of the device's own low-resolution logits to the
                 output size, then argmax over the classes (the forward not included: compare with dense minus forward)
The product never calls the yardsticks.

    python tools/dense_bench.py [--calls 20] [--warmup 3] [--batches 32,1] [--json out.json]
"""
import argparse, json, os, sys, tempfile
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--batches", default="32,1")
ap.add_argument("--json", default=None)
args = ap.parse_args()
import torch
import torch.nn.functional as F
torch.cuda.init()  # (before the library touches the device: torch's lazy init fails when it comes second; no GPU: this raises)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from importlib import import_module
from __graft_entry__ import PKG_NAME, load_package
pkg = load_package(); api = import_module(PKG_NAME + ".api")

path = os.path.join(tempfile.gettempdir(), "dense_bench_large_reg4.gguf")
if not os.path.exists(path):
    pkg.synth.write_synthetic_gguf(path, "large", registers=4, num_classes=0, seed=42)
model = api.Model(path, classify=False)
sess = api.Session(model)
stream = torch.cuda.ExternalStream(sess.stream)
LAYERS, HW, H, P, G = [5, 12, 18, 24], 518, 1024, 37 * 37, 37
rng = np.random.default_rng(1)


def head(C_, concat_cls, **kw):
    K = len(LAYERS) * H * (2 if concat_cls else 1)
    W = (rng.standard_normal((C_, K)) * (4.0 / np.sqrt(K))).astype(np.float32)
    return api.DenseHead(model, LAYERS, W, rng.standard_normal(C_).astype(np.float32), norm=True, concat_cls=concat_cls, **kw)


seg = head(150, False)
dep = head(256, True, reduce="bins", bin_centers=np.linspace(0.001, 10.0, 256).astype(np.float32), bins_eps=0.1)


def timed(fns):
    """fns: name -> callable that enqueues on the session's stream (or on torch's current stream inside `with torch.cuda.stream(stream)`)."""
    ts = {k: [] for k in fns}
    for it in range(args.warmup + args.calls):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record()
                fn()
                e1.record()
            e1.synchronize()
            if it >= args.warmup:
                ts[k].append(e0.elapsed_time(e1))
    out = {}
    for k, v in ts.items():
        v = np.sort(np.asarray(v))
        out[k] = {"median_ms": float(np.median(v)), "min_ms": float(v[0]), "p90_ms": float(v[int(0.9 * (len(v) - 1))])}
    return out


results = {"build_id": api.build_id(), "device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup, "batches": {}}
for B in [int(v) for v in args.batches.split(",")]:
    x = torch.randn((B, 3, HW, HW), device="cuda")
    labels = torch.empty((B, HW, HW), dtype=torch.uint8, device="cuda")
    depth = torch.empty((B, 4 * G, 4 * G), device="cuda")
    lg_seg = torch.empty((B, P, 150), device="cuda")
    lg_dep = torch.empty((B, P, 256), device="cuda")
    taps = torch.empty((4, B, P, H), device="cuda")
    torch.cuda.synchronize()
    sess.predict_dense_device(x.data_ptr(), B, HW, HW, seg, logits_ptr=lg_seg.data_ptr())  # the logits the torch yardstick works on
    sess.predict_dense_device(x.data_ptr(), B, HW, HW, dep, (4 * G, 4 * G), logits_ptr=lg_dep.data_ptr())
    sess.sync()

    def torch_argmax():
        planes = F.interpolate(lg_seg.view(B, G, G, 150).permute(0, 3, 1, 2), size=(HW, HW), mode="bilinear", align_corners=False)
        return planes.argmax(1)

    def torch_bins():
        planes = F.interpolate(lg_dep.view(B, G, G, 256).permute(0, 3, 1, 2), size=(4 * G, 4 * G), mode="bilinear", align_corners=False)
        r = torch.relu(planes) + 0.1
        return (r * torch.linspace(0.001, 10.0, 256, device="cuda").view(1, -1, 1, 1)).sum(1) / r.sum(1)

    r = timed({
        "forward": lambda: sess.predict_device(x.data_ptr(), B, HW, HW, classify=False),
        "layers_device": lambda: sess.predict_layers_device(x.data_ptr(), B, HW, HW, LAYERS, norm=True, layer_patch_ptr=taps.data_ptr()),
        "dense_argmax_c150_518": lambda: sess.predict_dense_device(x.data_ptr(), B, HW, HW, seg, labels_ptr=labels.data_ptr()),
        "dense_bins_c256_4x": lambda: sess.predict_dense_device(x.data_ptr(), B, HW, HW, dep, (4 * G, 4 * G), value_ptr=depth.data_ptr()),
        "torch_interpolate_argmax_c150_518": torch_argmax,
        "torch_interpolate_bins_c256_4x": torch_bins,
    })
    same = bool((torch_argmax().to(torch.uint8) == labels).float().mean().item() > 0.999)  # (F.interpolate may contract: ties near a boundary)
    results["batches"][str(B)] = {"times": r, "labels_agree_with_torch": same}
    fw = r["forward"]["median_ms"]
    for k, v in r.items():
        print("batch %2d  %-36s median %9.3f ms  min %9.3f  p90 %9.3f  (%+.2f %% of forward)"
              % (B, k, v["median_ms"], v["min_ms"], v["p90_ms"], 100.0 * (v["median_ms"] - fw) / fw if not k.startswith("torch") else
                 100.0 * v["median_ms"] / fw))
    del x, labels, depth, lg_seg, lg_dep, taps
print(json.dumps(results))
if args.json:
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
