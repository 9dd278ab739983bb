#!/usr/bin/env python3
"""Times dinov2_hip_vlad_tokens (csrc/vlad.hip) on device-resident rows -- the patches of one image (1 369 rows) and of a batch of 32
(32 segments of 1 369 rows), H = 1 024, K = 32 and 64, intra and L2 norms on -- next to two yardsticks on the same box in the same run:
  fetch route   what a caller had before the call: the [n, H] f32 tokens fetched to the host, the labels from
                dinov2_hip_kmeans_tokens(max_iter = 0) on the device rows, the aggregation in numpy;
  torch         the same arithmetic in PyTorch-ROCm on the device: F.normalize -> half -> x @ c.T -> argmax -> index_add_ of the unit rows per
                (segment, centre) -> residual -> the two norms, descriptors copied to the host like the call's.
Calls alternate between the three; median and spread of `--calls` calls after `--warmup`.  The product never calls a yardstick.  The
assignment and the sums on their own come from dinov2_hip_op_vlad_bench (HIP events).

    python tools/vlad_bench.py [--calls 20] [--warmup 5] [--json out.json]
"""
import argparse, ctypes as C, json, os, sys, tempfile, time
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
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
FLAGS = api.VLAD_INTRA_NORM | api.VLAD_L2_NORM


def stats(ts):
    ts = np.sort(np.asarray(ts)) * 1e3
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts[0]), "p90_ms": float(ts[int(0.9 * (len(ts) - 1))])}


def unit(v, axis):
    nrm = np.sqrt((v * v).sum(axis, keepdims=True))
    return v / np.where(nrm > 0, nrm, 1.0)


def fetch_route(x, cen, n_seg, P, K):
    """Tokens to the host, labels from the library's k-means assignment on the device rows, numpy for the rest."""
    host = x.cpu().numpy()
    labels = np.empty(len(host), np.int32)
    km = api.KMeans(api.Rows(api.ROWS_GIVEN, x.data_ptr(), len(host), host.shape[1], 0, 1), 0, K, 0, api.KMEANS_INIT_GIVEN, cen.ctypes.data, None,
                    labels.ctypes.data, None, None, None, None, None)
    e = C.create_string_buffer(256)
    assert api.lib().dinov2_hip_kmeans_tokens(sess._h, C.byref(km), e, len(e)) == 0, e.value
    xn, cn = unit(host, 1), unit(cen, 1)
    out = np.empty((n_seg, K, host.shape[1]), np.float32)
    for s in range(n_seg):
        onehot = (labels[s * P:(s + 1) * P, None] == np.arange(K)[None, :]).astype(np.float32)
        out[s] = onehot.T @ xn[s * P:(s + 1) * P] - onehot.sum(0)[:, None] * cn
    return unit(unit(out, 2), (1, 2))


def torch_vlad(x, cen_t, n_seg, P, K):
    xn = F.normalize(x, dim=1)
    cn = F.normalize(cen_t, dim=1)
    labels = (xn.half() @ cn.half().T).argmax(1)
    slot = labels + K * torch.arange(n_seg, device=x.device).repeat_interleave(P)
    S = torch.zeros((n_seg * K, x.shape[1]), device=x.device).index_add_(0, slot, xn)
    cnt = torch.bincount(slot, minlength=n_seg * K).float()
    R = (S - cnt[:, None] * cn.repeat(n_seg, 1)).view(n_seg, K, -1)
    R = F.normalize(R, dim=2)
    return F.normalize(R.reshape(n_seg, -1), dim=1).view(n_seg, K, -1).cpu()


results = []
P, H = 1369, 1024
for n_seg, K in ((1, 32), (1, 64), (32, 32), (32, 64)):
    n = n_seg * P
    g = torch.Generator(device="cuda").manual_seed(n + K)
    dirs = torch.randn((K, H), generator=g, device="cuda")
    x = (dirs[torch.randint(K, (n,), generator=g, device="cuda")] + 1.5 * torch.randn((n, H), generator=g, device="cuda")).contiguous()
    cen_t = (dirs + 0.1 * torch.randn((K, H), generator=g, device="cuda")).contiguous()
    cen = cen_t.cpu().numpy()
    off = (np.arange(n_seg + 1) * P).astype(np.int32)
    torch.cuda.synchronize()
    out = np.empty((n_seg, K, H), np.float32)
    req = api.Vlad(api.Rows(api.ROWS_GIVEN, x.data_ptr(), n, H, 0, 1), 0, off.ctypes.data, n_seg, K, cen.ctypes.data, FLAGS, out.ctypes.data, None,
                   None, None)
    err = C.create_string_buffer(256)
    t_hip, t_fetch, t_torch = [], [], []
    for i in range(args.warmup + args.calls):
        t0 = time.perf_counter()
        rc = api.lib().dinov2_hip_vlad_tokens(sess._h, C.byref(req), err, len(err))  # synchronous: returns after the copy-out
        t1 = time.perf_counter()
        ref_fetch = fetch_route(x, cen, n_seg, P, K)
        t2 = time.perf_counter()
        ref_torch = torch_vlad(x, cen_t, n_seg, P, K)
        t3 = time.perf_counter()
        assert rc == 0, err.value
        if i >= args.warmup:
            t_hip.append(t1 - t0)
            t_fetch.append(t2 - t1)
            t_torch.append(t3 - t2)
    t_copy = []
    for i in range(args.calls):  # the fetch alone
        t0 = time.perf_counter()
        host = x.cpu()
        t_copy.append(time.perf_counter() - t0)
    ms = (C.c_float * 3)()
    rc = api.lib().dinov2_hip_op_vlad_bench(x.data_ptr(), off.ctypes.data_as(C.POINTER(C.c_int32)), n_seg, cen_t.data_ptr(), K, H, FLAGS, args.warmup,
                                            args.calls, ms)
    assert rc == 0, rc
    p = api.op_vlad_plan(off, K, H)
    row = {"n_seg": n_seg, "rows": n, "H": H, "K": K, "vlad_tokens": stats(t_hip), "fetch_route": stats(t_fetch), "torch_yardstick": stats(t_torch),
           "fetch_rows_to_host": stats(t_copy), "assign_ms": float(ms[0]), "sums_ms": float(ms[1]), "device_work_events_ms": float(ms[2]),
           "plan": {k: v for k, v in p.items() if k not in ("segs", "chunks")},
           # (not checks: the yardsticks sum in other orders and assign near-ties differently)
           "max_abs_diff_fetch_route": float(np.abs(ref_fetch - out).max()), "max_abs_diff_torch": float(np.abs(ref_torch.numpy() - out).max())}
    results.append(row)
    print(json.dumps(row), flush=True)
    del x, dirs, cen_t
    torch.cuda.empty_cache()
if args.json:
    with open(args.json, "w") as f:
        json.dump({"build_id": api.build_id(), "calls": args.calls, "results": results}, f, indent=1)
