#!/usr/bin/env python3
"""Times one pick of dinov2_hip_coreset_tokens (csrc/coreset.hip: one launch = one sweep over the n x hpad f16 rows) with device-resident
rows, through dinov2_hip_op_coreset_bench (HIP events around a chain of m launches, no host read in between), at the sizes its users run:
the patches of one image (n = 1 369, H = 1 024), of a batch of 32 (43 808), a bank of 2^20 rows at H = 1 024 and at H = 128 (projected
rows).  Each next to two yardsticks: the bytes one sweep streams (the f16 rows plus 9 bytes of state per row read and, at worst, written)
divided by the measured copy rate of the part, 6.29 TB/s; and the same loop in PyTorch-ROCm on the same device in the same run -- mv of
the f16 unit rows with the picked row, maximum, masked argmin, the index kept on the device -- which the product never calls.  Writes the
table as markdown.

    python tools/coreset_bench.py [--iters 5] [--warmup 2] [--out profiles/coreset.md] [--json out.json]
"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "coreset.md"))
ap.add_argument("--json", default=None)
args = ap.parse_args()
import torch
import torch.nn.functional as F
torch.cuda.init()  # (before the library touches the device: torch's lazy init fails when it comes second; no GPU: this raises)
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from importlib import import_module
from __graft_entry__ import PKG_NAME, load_package
pkg = load_package(); api = import_module(PKG_NAME + ".api")

COPY_RATE = 6.29e12  # bytes / s: the measured copy rate of the part


def torch_coreset(xh, m, first):
    """The yardstick: m picks, nothing read by the host in between."""
    n = xh.shape[0]
    s = torch.full((n,), -float("inf"), device="cuda")
    sel = torch.zeros(n, dtype=torch.bool, device="cuda")
    inf = torch.full((n,), float("inf"), device="cuda")
    idx = torch.empty(m, dtype=torch.int64, device="cuda")
    p = torch.tensor(first, device="cuda")
    for t in range(m):
        idx[t] = p
        sel[p] = True
        s = torch.maximum(s, torch.mv(xh, xh[p]).float())
        p = torch.where(sel, inf, s).argmin()
    return idx


results = []
for n, H, m in ((1369, 1024, 256), (43808, 1024, 256), (1 << 20, 1024, 64), (1 << 20, 128, 64)):
    g = torch.Generator(device="cuda").manual_seed(n + H)
    x = torch.randn((n, H), generator=g, device="cuda")
    xh = F.normalize(x, dim=1).half()
    torch.cuda.synchronize()
    us = C.c_float(0)
    rc = api.lib().dinov2_hip_op_coreset_bench(x.data_ptr(), n, H, m, 0, args.warmup, args.iters, C.byref(us))
    assert rc == 0, rc
    ts = []
    for i in range(args.warmup + args.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch_coreset(xh, m, 0)
        torch.cuda.synchronize()
        if i >= args.warmup:
            ts.append((time.perf_counter() - t0) / m * 1e6)
    p = api.op_coreset_plan(n, H, m)
    sweep_bytes = p["npad"] * p["hpad"] * 2 + n * 9
    row = {"n": n, "H": H, "picks": m, "us_per_pick": float(us.value), "floor_us": sweep_bytes / COPY_RATE * 1e6,
           "torch_us_per_pick": float(np.median(ts)), "sweep_bytes": sweep_bytes, "tb_per_s": sweep_bytes / (us.value * 1e-6) / 1e12, "plan": p}
    results.append(row)
    print(json.dumps(row), flush=True)
    del x, xh
    torch.cuda.empty_cache()

lines = ["# Greedy k-center selection: microseconds per pick", "",
         "`tools/coreset_bench.py` on one %s, build `%s`, torch %s; %d timed chains after %d." % (
             torch.cuda.get_device_name(0), api.build_id(), torch.__version__, args.iters, args.warmup), "",
         "One pick is one launch of `coreset_sweep_kernel`: one pass over the `n x hpad` f16 rows.  `floor` is the bytes of that pass (the rows plus",
         "9 bytes of state per row) at the part's measured copy rate, 6.29 TB/s; `torch` is the same loop (`mv`, `maximum`, masked `argmin`, the",
         "index kept on the device) in PyTorch-ROCm on the same device in the same run.", "",
         "| n | H | workgroups | picks per chain | µs per pick | floor µs | × floor | TB/s | torch µs per pick | torch / ours |",
         "|---|---|---|---|---|---|---|---|---|---|"]
for r in results:
    lines.append("| %d | %d | %d | %d | %.2f | %.2f | %.2f | %.2f | %.2f | %.2f |" % (
        r["n"], r["H"], r["plan"]["nparts"], r["picks"], r["us_per_pick"], r["floor_us"], r["us_per_pick"] / r["floor_us"], r["tb_per_s"],
        r["torch_us_per_pick"], r["torch_us_per_pick"] / r["us_per_pick"]))
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
if args.json:
    with open(args.json, "w") as f:
        json.dump({"build_id": api.build_id(), "results": results}, f, indent=1)
