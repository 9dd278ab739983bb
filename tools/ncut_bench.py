#!/usr/bin/env python3
"""Times dinov2_hip_ncut_tokens (csrc/ncut.hip, csrc/ncut.cpp) with device-resident rows at the two sizes its users run -- the patches of
one image (n = 1 369, H = 1 024) and of a batch of 32 (n = 43 808) -- next to the same computation in PyTorch-ROCm on the same device in the
same run: F.normalize -> half -> x @ x.T -> the affinity map -> D^-1/2 W D^-1/2 materialised, then torch.linalg.eigh (the small size only)
and torch.lobpcg for the `--eig` leading pairs; vectors copied to the host like the call's.  Calls alternate between the two; median and
spread of `--calls` calls after `--warmup`.  The product never calls the yardstick.  One ncut_apply_kernel launch and one
ncut_finish_kernel launch on their own, and the whole call without the session, come from dinov2_hip_op_ncut_bench (HIP events).

    python tools/ncut_bench.py [--calls 5] [--warmup 2] [--eig 4] [--tol 1e-4] [--sizes 1369,43808] [--json out.json]
"""
import argparse, ctypes as C, json, os, sys, tempfile, time
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--eig", type=int, default=4)
ap.add_argument("--tol", type=float, default=1e-4)
ap.add_argument("--sizes", default="1369,43808")
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
AFFINITIES = {"threshold": (api.NCUT_THRESHOLD, 0.2, 1e-5), "relu": (api.NCUT_RELU, 0.0, 0.0), "exp": (api.NCUT_EXP, 0.25, 0.0)}


def stats(ts):
    ts = np.sort(np.asarray(ts)) * 1e3
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts[0]), "p90_ms": float(ts[int(0.9 * (len(ts) - 1))])}


def torch_operator(x, aff, tau, floor):
    """The yardstick's first half: D^-1/2 W D^-1/2, materialised in f32."""
    xh = F.normalize(x, dim=1).half()
    s = (xh @ xh.T).float()
    w = torch.where(s > tau, 1.0, floor) if aff == "threshold" else s.clamp_min(0.0) if aff == "relu" else torch.exp((s - 1.0) / tau)
    c = w.sum(1).rsqrt()
    return w * c[:, None] * c[None, :], c


def torch_eigh(x, aff, tau, floor, k):
    a, c = torch_operator(x, aff, tau, floor)
    val, vec = torch.linalg.eigh(a)
    return (1.0 - val[-k:]).flip(0).cpu(), (vec[:, -k:] * c[:, None]).T.flip(0).cpu()


def torch_lobpcg(x, aff, tau, floor, k, tol):
    a, c = torch_operator(x, aff, tau, floor)
    val, vec = torch.lobpcg(a, k=k, largest=True, tol=tol)
    return (1.0 - val).cpu(), (vec * c[:, None]).T.cpu()


results = []
for n in (int(v) for v in args.sizes.split(",")):
    H, k = 1024, args.eig
    g = torch.Generator(device="cuda").manual_seed(n)
    dirs = torch.randn((6, H), generator=g, device="cuda")
    x = (dirs[torch.randint(6, (n,), generator=g, device="cuda")] + 1.5 * torch.randn((n, H), generator=g, device="cuda")).contiguous()
    torch.cuda.synchronize()
    for aff, (aid, tau, floor) in AFFINITIES.items():
        out = {"values": np.empty(k, np.float32), "vectors": np.empty((k, n), np.float32), "degree": np.empty(n, np.float32),
               "residual": np.empty(k, np.float32)}
        it, conv = C.c_int32(0), C.c_int32(0)
        req = api.NCut(api.Rows(api.ROWS_GIVEN, x.data_ptr(), n, H, 0, 1), 0, aid, tau, floor, k, 1000, args.tol, out["values"].ctypes.data,
                       out["vectors"].ctypes.data, out["degree"].ctypes.data, out["residual"].ctypes.data, C.addressof(it), C.addressof(conv))
        err = C.create_string_buffer(256)
        t_hip, t_lob, t_eigh = [], [], []
        for i in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            rc = api.lib().dinov2_hip_ncut_tokens(sess._h, C.byref(req), err, len(err))  # synchronous: returns after the copy-out
            t1 = time.perf_counter()
            ref = torch_lobpcg(x, aff, tau, floor, k, args.tol)
            t2 = time.perf_counter()
            if n <= 4096:
                ref = torch_eigh(x, aff, tau, floor, k)
            t3 = time.perf_counter()
            assert rc == 0, err.value
            if i >= args.warmup:
                t_hip.append(t1 - t0)
                t_lob.append(t2 - t1)
                t_eigh.append(t3 - t2)
        ms, steps = (C.c_float * 3)(), (C.c_int32 * 1)()
        rc = api.lib().dinov2_hip_op_ncut_bench(x.data_ptr(), n, H, aid, tau, floor, 0, k, 1000, args.tol, args.warmup, args.calls, ms, steps)
        assert rc == 0, rc
        p = api.op_ncut_plan(n, H)
        flop = 2.0 * p["npad"] * p["npad"] * p["hpad"]
        row = {"n": n, "H": H, "affinity": aff, "n_eig": k, "tol": args.tol, "iterations": int(it.value), "converged": int(conv.value),
               "ncut_tokens": stats(t_hip), "torch_lobpcg": stats(t_lob), "torch_eigh": stats(t_eigh) if n <= 4096 else None,
               "apply_ms": float(ms[0]), "finish_ms": float(ms[1]), "step_ms": float(ms[0] + ms[1]), "whole_call_events_ms": float(ms[2]),
               "apply_tflops_f16": flop / (ms[0] * 1e-3) / 1e12, "plan": p,
               "values": out["values"].tolist(), "torch_values": ref[0].tolist()}  # (not a check; lambda = 1 - mu, mu an eigenvalue of D^-1/2 W D^-1/2)
        results.append(row)
        print(json.dumps(row), flush=True)
    del x, dirs
    torch.cuda.empty_cache()
if args.json:
    with open(args.json, "w") as f:
        json.dump({"build_id": api.build_id(), "calls": args.calls, "results": results}, f, indent=1)
