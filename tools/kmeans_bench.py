#!/usr/bin/env python3
"""Times dinov2_hip_kmeans_tokens (csrc/kmeans.hip) with device-resident rows at the two sizes its users run -- the patches of one image
(n = 1 369, H = 1 024, K = 8 and 64) and of a batch of 32 (n = 43 808, K = 64 and 256) -- next to the same algorithm in PyTorch-ROCm on the
same device in the same run: F.normalize -> half -> x @ c.T -> argmax -> index_add_ of the f32 unit rows -> normalise, `--iters` iterations,
labels and centres copied to the host like the call's.  Calls alternate between the two; median and spread of `--calls` calls after
`--warmup`.  The product never calls the yardstick.  One assignment and one update on their own, without the host's 4-byte read per
iteration, come from dinov2_hip_op_kmeans_bench (HIP events); the fetch of the [n, H] f32 rows to the host that the call removes is timed too.

    python tools/kmeans_bench.py [--calls 20] [--warmup 5] [--iters 10] [--json out.json]
"""
import argparse, ctypes as C, json, os, sys, tempfile, time
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--json", default=None)
args = ap.parse_args()
import torch
import torch.nn.functional as F
torch.cuda.init()  # (before the library touches the device: torch's lazy init fails when it comes second; no GPU: this raises)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from importlib import import_module
from __graft_entry__ import PKG_NAME, load_package
pkg = load_package(); api = import_module(PKG_NAME + ".api")

path = os.path.join(tempfile.gettempdir(), "match_bench_small.gguf")  # any model gives a session
if not os.path.exists(path):
    pkg.synth.write_synthetic_gguf(path, "small", registers=4, num_classes=0, seed=42)
sess = api.Session(api.Model(path, classify=False))


def stats(ts):
    ts = np.sort(np.asarray(ts)) * 1e3
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts[0]), "p90_ms": float(ts[int(0.9 * (len(ts) - 1))])}


def torch_kmeans(x, init, iters):
    """The yardstick: a fixed number of iterations (no convergence read), then the final assignment; results to the host."""
    xn = F.normalize(x, dim=1)
    xh = xn.half()
    c = x[init].clone()
    for _ in range(iters):
        labels = (xh @ F.normalize(c, dim=1).half().T).argmax(1)
        s = torch.zeros_like(c).index_add_(0, labels, xn)
        cnt = torch.bincount(labels, minlength=c.shape[0])
        c = torch.where((cnt > 0)[:, None], s, c)
    sim, labels = (xh @ F.normalize(c, dim=1).half().T).max(1)
    return labels.cpu(), sim.float().cpu(), c.cpu()


results = []
for n, H, K in ((1369, 1024, 8), (1369, 1024, 64), (43808, 1024, 64), (43808, 1024, 256)):
    g = torch.Generator(device="cuda").manual_seed(n + K)
    dirs = torch.randn((K, H), generator=g, device="cuda")
    x = (dirs[torch.randint(K, (n,), generator=g, device="cuda")] + 1.5 * torch.randn((n, H), generator=g, device="cuda")).contiguous()
    init = np.sort(np.random.default_rng(0).choice(n, K, replace=False)).astype(np.int32)
    tinit = torch.from_numpy(init.astype(np.int64)).cuda()
    torch.cuda.synchronize()
    out = {"labels": np.empty(n, np.int32), "sim": np.empty(n, np.float32), "centers": np.empty((K, H), np.float32), "counts": np.empty(K, np.int32)}
    it, conv = C.c_int32(0), C.c_int32(0)
    req = api.KMeans(api.Rows(api.ROWS_GIVEN, x.data_ptr(), n, H, 0, 1), 0, K, args.iters, api.KMEANS_INIT_ROWS, None, init.ctypes.data,
                     out["labels"].ctypes.data, out["sim"].ctypes.data, out["centers"].ctypes.data, out["counts"].ctypes.data, C.addressof(it),
                     C.addressof(conv))
    err = C.create_string_buffer(256)
    t_hip, t_ref, t_fetch = [], [], []
    for i in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        rc = api.lib().dinov2_hip_kmeans_tokens(sess._h, C.byref(req), err, len(err))  # synchronous: returns after the copy-out
        t1 = time.perf_counter()
        ref = torch_kmeans(x, tinit, int(it.value))  # as many updates as the call performed
        t2 = time.perf_counter()
        assert rc == 0, err.value
        if i >= args.warmup:
            t_hip.append(t1 - t0)
            t_ref.append(t2 - t1)
    for i in range(args.calls):  # what a caller without the call pays first (a loop of its own: a 180 MB pageable copy disturbs what follows it)
        t2 = time.perf_counter()
        host = x.cpu()
        t_fetch.append(time.perf_counter() - t2)
    ms = (C.c_float * 3)()
    rc = api.lib().dinov2_hip_op_kmeans_bench(x.data_ptr(), n, K, H, 0, args.iters, args.warmup, args.calls, ms)
    assert rc == 0, rc
    p = api.op_kmeans_plan(n, K, H)
    flop = 2.0 * p["npad"] * p["kpad"] * p["hpad"]
    row = {"n": n, "H": H, "K": K, "max_iter": args.iters, "iterations": int(it.value), "converged": int(conv.value), "kmeans_tokens": stats(t_hip),
           "torch_yardstick": stats(t_ref), "fetch_rows_to_host": stats(t_fetch), "assign_ms": float(ms[0]), "update_ms": float(ms[1]),
           "whole_call_events_ms": float(ms[2]), "assign_tflops": flop / (ms[0] * 1e-3) / 1e12, "update_tflops": flop / (ms[1] * 1e-3) / 1e12,
           "plan": p, "same_labels": float((ref[0].numpy() == out["labels"]).mean())}  # (not a check: the yardstick sums in another order)
    results.append(row)
    print(json.dumps(row), flush=True)
    del x, dirs
    torch.cuda.empty_cache()
if args.json:
    with open(args.json, "w") as f:
        json.dump({"build_id": api.build_id(), "calls": args.calls, "results": results}, f, indent=1)
