#!/usr/bin/env python3
"""Times dinov2_hip_match_tokens (csrc/match.hip) with device-resident inputs at the sizes its users run -- 1 369 x 1 369 x 1 024 (518 px,
ViT-L), 2 170 x 2 170 x 1 024 (the realtime grid), 1 369 x 1 369 x 384 -- next to the vendor yardstick on the same device in the same run:
PyTorch-ROCm F.normalize in f32 -> f16 -> a @ b.T -> .max(1) and .max(0), the four result vectors copied to the host like the call's.
Calls alternate between the two; median and spread of `--calls` calls after `--warmup`.  The product never calls the yardstick.

    python tools/match_bench.py [--calls 30] [--warmup 5] [--no-torch] [--json out.json]

Kernel shares (normalise / match / reduce) come from a run of their own under a kernel trace:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/match_bench.py --no-torch --calls 10
"""
import argparse, json, os, sys, tempfile, time
import numpy as np
SHAPES = [(1369, 1369, 1024), (2170, 2170, 1024), (1369, 1369, 384)]
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--no-torch", action="store_true")
ap.add_argument("--json", default=None)
args = ap.parse_args()
torch = None
if not args.no_torch:
    import torch
    import torch.nn.functional as F
    torch.cuda.init()  # (before the library touches the device: torch's lazy init fails when it comes second; no GPU: this raises)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from importlib import import_module
from __graft_entry__ import PKG_NAME, load_package
pkg = load_package(); api = import_module(PKG_NAME + ".api")

# any model gives a session; with both sides given, H need not be the model's hidden size
path = os.path.join(tempfile.gettempdir(), "match_bench_small.gguf")
if not os.path.exists(path):
    pkg.synth.write_synthetic_gguf(path, "small", registers=4, num_classes=0, seed=42)
sess = api.Session(api.Model(path, classify=False))


def yardstick(ta, tb):
    s = F.normalize(ta, dim=1).half() @ F.normalize(tb, dim=1).half().T
    ab, ba = s.max(1), s.max(0)
    return [x.cpu() for x in (ab.indices, ab.values, ba.indices, ba.values)]  # (.cpu() waits for the device)


def stats(ts):
    ts = np.sort(np.asarray(ts)) * 1e3
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts[0]), "p90_ms": float(ts[int(0.9 * (len(ts) - 1))])}


results = []
for na, nb, H in SHAPES:
    rng = np.random.default_rng(na + H)
    a = rng.standard_normal((na, H)).astype(np.float32)
    b = (a[rng.permutation(na)[:nb]] + 0.5 * rng.standard_normal((nb, H))).astype(np.float32)
    da, db = api.DeviceArray.from_host(a), api.DeviceArray.from_host(b)
    if torch is not None:
        ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    t_hip, t_ref = [], []
    for i in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        got = sess.match(da, db)  # synchronous: returns after the copy-out
        t1 = time.perf_counter()
        if torch is not None:
            ref = yardstick(ta, tb)
        t2 = time.perf_counter()
        if i >= args.warmup:
            t_hip.append(t1 - t0)
            t_ref.append(t2 - t1)
    row = {"na": na, "nb": nb, "H": H, "match_tokens": stats(t_hip), "mutual": int(got["mutual"].sum()),
           "tflops": 2.0 * na * nb * H / np.median(t_hip) / 1e12}
    if torch is not None:
        row["torch_yardstick"] = stats(t_ref)
        row["same_idx_ab"] = float((ref[0].numpy() == got["idx_ab"]).mean())  # (not a check: the yardstick rounds the product to f16)
    results.append(row)
    print(json.dumps(row), flush=True)
    da.free()
    db.free()
if args.json:
    with open(args.json, "w") as f:
        json.dump({"build_id": api.build_id(), "calls": args.calls, "results": results}, f, indent=1)
