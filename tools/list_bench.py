#!/usr/bin/env python3
"""Times dinov2_hip_predict_list (csrc/model.cpp forward() over a list's runs, csrc/attention.hip launch_attention_list) with device-resident inputs and no
outputs on a synthetic ViT-L/14 with 4 registers, f16.  HIP events on the session's stream around every call; the calls that are compared
alternate; median, minimum and p90 of `--calls` calls after `--warmup`.
  (a) 32 images, all 518 x 518: the list call against the uniform dinov2_hip_predict at batch 32 (the difference is the attention table
      lookup, and the images' gather where they are not contiguous -- here they are), with the attention kernel's time per launch from the
      session profile for both
  (b) 32 images with sides drawn (seeded) from 224 .. 644 in steps of 14: the list call against the same images as 32 sequential batch-1
      dinov2_hip_predict calls -- the comparison the call exists for
  (c) the list of (b) with the attention work table in list order and with the longest images first ("list_order"), in alternating blocks
      (a change of order uploads a new table: that call is a warm-up call)

    python tools/list_bench.py [--calls 20] [--warmup 3] [--json out.json]
"""
import argparse, json, os, sys, tempfile
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()
import torch
torch.cuda.init()  # (before the library touches the device: torch's lazy init fails when it comes second; no GPU: this raises)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from importlib import import_module
from __graft_entry__ import PKG_NAME, load_package
pkg = load_package(); api = import_module(PKG_NAME + ".api")

path = os.path.join(tempfile.gettempdir(), "list_bench_large_reg4.gguf")
if not os.path.exists(path):
    pkg.synth.write_synthetic_gguf(path, "large", registers=4, num_classes=0, seed=42)
model = api.Model(path, classify=False)
sess = api.Session(model)
stream = torch.cuda.ExternalStream(sess.stream)
N = 32


def stats(v):
    v = np.sort(np.asarray(v))
    return {"median_ms": float(np.median(v)), "min_ms": float(v[0]), "p90_ms": float(v[int(0.9 * (len(v) - 1))])}


def timed(fns, calls=args.calls, warmup=args.warmup):
    """fns: name -> callable that enqueues on the session's stream; the callables alternate call by call."""
    ts = {k: [] for k in fns}
    for it in range(warmup + calls):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(stream):
                e0.record()
                fn()
                e1.record()
            e1.synchronize()
            if it >= warmup:
                ts[k].append(e0.elapsed_time(e1))
    return {k: stats(v) for k, v in ts.items()}


def attention_ms_per_launch(fn):
    sess.profile(True)
    fn()
    ms, n = sess.profile_read()["attention"]
    sess.profile(False)
    return ms / max(n, 1)


def show(tag, r, base):
    for k, v in r.items():
        print("%s  %-28s median %9.3f ms  min %9.3f  p90 %9.3f  (x %.3f of %s)" % (tag, k, v["median_ms"], v["min_ms"], v["p90_ms"],
                                                                                   v["median_ms"] / r[base]["median_ms"], base))


results = {"build_id": api.build_id(), "device": torch.cuda.get_device_name(0), "calls": args.calls, "warmup": args.warmup}

# (a) 32 x 518 x 518, one allocation
x = torch.randn((N, 3, 518, 518), device="cuda")
torch.cuda.synchronize()
one = 3 * 518 * 518 * 4
ptrs_a, sizes_a = [x.data_ptr() + i * one for i in range(N)], [(518, 518)] * N
list_a = lambda: sess.predict_list_device(ptrs_a, sizes_a, classify=False)  # noqa: E731
uni_a = lambda: sess.predict_device(x.data_ptr(), N, 518, 518, classify=False)  # noqa: E731
ra = timed({"uniform_b32": uni_a, "list_32x518": list_a})
ra_att = {"uniform_b32": attention_ms_per_launch(uni_a), "list_32x518": attention_ms_per_launch(list_a)}
results["a"] = {"times": ra, "attention_ms_per_launch": ra_att}
show("(a)", ra, "uniform_b32")
print("(a)  attention per launch: uniform %.4f ms, list %.4f ms" % (ra_att["uniform_b32"], ra_att["list_32x518"]))
del x

# (b) 32 mixed sizes against 32 batch-1 calls
rng = np.random.default_rng(7)
sides = np.arange(224, 645, 14)
sizes_b = [(int(rng.choice(sides)), int(rng.choice(sides))) for _ in range(N)]
imgs = [torch.randn((3, h, w), device="cuda") for h, w in sizes_b]
torch.cuda.synchronize()
ptrs_b = [t.data_ptr() for t in imgs]
list_b = lambda: sess.predict_list_device(ptrs_b, sizes_b, classify=False)  # noqa: E731


def seq_b():
    for p, (h, w) in zip(ptrs_b, sizes_b):
        sess.predict_device(p, 1, h, w, classify=False)


rb = timed({"sequential_32_batch1": seq_b, "list_mixed": list_b})
T = [model.tokens(h, w) for h, w in sizes_b]
results["b"] = {"sizes": sizes_b, "tokens": T, "rows": int(sum(T)), "times": rb, "attention_ms_per_launch_list": attention_ms_per_launch(list_b)}
show("(b)", rb, "sequential_32_batch1")

# (c) table order, in alternating blocks
tc = {"list_order": [], "longest_first": []}
for rnd in range(2):
    for name, order in (("list_order", 0), ("longest_first", 1)):
        api.set_tuning("list_order", order)
        r = timed({name: list_b}, calls=max(args.calls // 2, 5), warmup=2)
        tc[name].append(r[name])
api.reset_tuning("list_order")
results["c"] = tc
for name, v in tc.items():
    print("(c)  %-14s medians per block: %s ms" % (name, ", ".join("%.3f" % b["median_ms"] for b in v)))
print(json.dumps(results))
if args.json:
    with open(args.json, "w") as f:
        json.dump(results, f, indent=1)
