#!/usr/bin/env python3
"""Times dinov2_hip_propagate (csrc/propagate.hip) on device-resident rows -- the workload of record: a 37 x 37 grid (1 369 patches), H = 1 024,
8 slots, k = 5, radius 12, T = 0.1, C = 8 -- next to three yardsticks on the same box in the same run:
  (a) no window  the same call with radius = -1: what the window test and the tile skip cost or gain;
  (b) bank       dinov2_hip_bank_topk's kernels on the same rows (a bank of 8 x 1 369 rows, k = 5): the floor of the selection;
  (c) torch      the affinity-matrix procedure in PyTorch-ROCm on the device: F.normalize -> half -> feats @ q.T -> exp(S / T) -> window
                 mask -> topk -> zero the rest -> normalise -> labels x affinity, the result copied to the host like the call's.
The device work of (the two settings of) the call and of (b) comes from dinov2_hip_op_propagate_bench / dinov2_hip_op_bank_bench (HIP
events, the mean of `--iters` launches after a warm-up); the session call and (c) are wall-clock medians of `--calls` alternating calls
after `--warmup`.  The product never calls a yardstick.

    python tools/propagate_bench.py [--calls 20] [--warmup 5] [--iters 50] [--json out.json]
"""
import argparse, ctypes as C, json, os, sys, tempfile, time
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--iters", type=int, default=50)
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
model = api.Model(path, classify=False)
sess = api.Session(model)
GRID, H, FRAMES, K, RADIUS, T, CH = (37, 37), 1024, 8, 5, 12, 0.1, 8
P = GRID[0] * GRID[1]
SLOTS = (1 << FRAMES) - 1


def stats(ts):
    ts = np.sort(np.asarray(ts)) * 1e3
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts[0]), "p90_ms": float(ts[int(0.9 * (len(ts) - 1))])}


g = torch.Generator(device="cuda").manual_seed(7)
q = torch.randn((P, H), generator=g, device="cuda").contiguous()
rows = (q[None] + 0.7 * torch.randn((FRAMES, P, H), generator=g, device="cuda")).contiguous()  # frames that resemble the query frame
labels = torch.randn((FRAMES, P, CH), generator=g, device="cuda").contiguous()
yy, xx = torch.div(torch.arange(P, device="cuda"), GRID[1], rounding_mode="floor"), torch.arange(P, device="cuda") % GRID[1]
WIN = (torch.maximum((yy[:, None] - yy[None]).abs(), (xx[:, None] - xx[None]).abs()) <= RADIUS).repeat(FRAMES, 1)  # [frames P, P]
torch.cuda.synchronize()


def torch_propagate(radius):
    feats = F.normalize(rows.view(-1, H), dim=1).half()
    aff = torch.exp((feats @ F.normalize(q, dim=1).half().T).float() / T)  # [frames P, P]: column i = query i
    if radius >= 0:
        aff = aff * WIN
    val, top = torch.topk(aff, K, dim=0)
    aff = torch.zeros_like(aff).scatter_(0, top, val)
    aff = aff / aff.sum(0, keepdim=True)
    return (labels.view(-1, CH).T @ aff).T.contiguous().cpu()


mem = api.PropMemory(model, H, GRID, FRAMES, CH)
for f in range(FRAMES):
    mem.set(sess, f, rows[f].cpu().numpy(), labels[f].cpu().numpy())
out = np.empty((P, CH), np.float32)
err = C.create_string_buffer(256)
results = {}
for name, radius in (("window", RADIUS), ("no_window", -1)):
    req_out = api.PropagateReq(api.Rows(api.ROWS_GIVEN, q.data_ptr(), P, H, 0, 1), SLOTS, radius, K, T, 0, out.ctypes.data, None, None, None)
    req_keep = api.PropagateReq(api.Rows(api.ROWS_GIVEN, q.data_ptr(), P, H, 0, 1), SLOTS, radius, K, T, 1, None, None, None, None)
    t_out, t_keep, t_torch = [], [], []
    for i in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        rc1 = api.lib().dinov2_hip_propagate(sess._h, mem._h, C.byref(req_out), err, len(err))  # synchronous: returns after the copy-out
        t1 = time.perf_counter()
        rc2 = api.lib().dinov2_hip_propagate(sess._h, mem._h, C.byref(req_keep), err, len(err))  # the realtime loop: nothing crosses PCIe
        t2 = time.perf_counter()
        ref = torch_propagate(radius)
        t3 = time.perf_counter()
        assert rc1 == 0 and rc2 == 0, err.value
        if i >= args.warmup:
            t_out.append(t1 - t0)
            t_keep.append(t2 - t1)
            t_torch.append(t3 - t2)
    ms = (C.c_float * 1)()
    rc = api.lib().dinov2_hip_op_propagate_bench(q.data_ptr(), rows.data_ptr(), GRID[0], GRID[1], H, FRAMES, CH, SLOTS, radius, K, T, 0, args.warmup,
                                                 args.iters, ms)
    assert rc == 0, rc
    p = api.op_propagate_plan(GRID, H, FRAMES, radius, K, CH)
    results[name] = {"radius": radius, "call_labels_out": stats(t_out), "call_keep_only": stats(t_keep), "torch_yardstick": stats(t_torch),
                     "device_work_events_ms": float(ms[0]), "plan": {k: v for k, v in p.items() if k != "ranges"},
                     "kept_tiles_per_query_tile": [int(b - a) for a, b in p["ranges"].tolist()],
                     # (not a check: the yardstick keeps all ties and sums in another order)
                     "max_abs_diff_torch": float(np.abs(ref.numpy() - out).max())}
    print(json.dumps({name: results[name]}), flush=True)
bank_ms = {}
for key, floor_only in (("topk", 0), ("sweep_floor", 1)):
    ms = (C.c_float * 1)()
    rc = api.lib().dinov2_hip_op_bank_bench(q.data_ptr(), P, rows.data_ptr(), FRAMES * P, H, K, 0, args.warmup, args.iters, floor_only, ms)
    assert rc == 0, rc
    bank_ms[key] = float(ms[0])
results["bank_topk_same_rows"] = {"device_work_events_ms": bank_ms, "plan": api.bank_plan(P, FRAMES * P, H, K)}
print(json.dumps({"bank_topk_same_rows": results["bank_topk_same_rows"]}), flush=True)
mem.free()
if args.json:
    with open(args.json, "w") as f:
        json.dump({"build_id": api.build_id(), "calls": args.calls, "iters": args.iters,
                   "workload": {"grid": GRID, "H": H, "slots": FRAMES, "k": K, "radius": RADIUS, "T": T, "C": CH}, "results": results}, f, indent=1)
