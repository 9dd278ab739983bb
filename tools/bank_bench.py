#!/usr/bin/env python3
"""Times dinov2_hip_bank_topk (csrc/bank.hip) with device-resident inputs at the two sizes its users run -- 32 CLS queries against a
1 M x 1 024 bank (k-NN / retrieval) and 1 369 x 1 369 x 1 024 (dense correspondence with k > 1) -- at k = 1, 20, 64, next to the vendor
yardstick on the same device in the same run: PyTorch-ROCm F.normalize -> f16 -> q @ bank.T -> topk, its results copied to the host like the
call's (the bank side normalised once, outside the timing, like ours).  Calls alternate between the two; median and spread of `--calls`
calls after `--warmup`.  The second size also times dinov2_hip_match_tokens on the same rows.  The product never calls the yardstick.
The kernel's own floor -- the sweep with its selection epilogue compiled out -- and the kernel times without the copy-out come from
dinov2_hip_op_bank_bench (HIP events).

    python tools/bank_bench.py [--calls 30] [--warmup 5] [--bank-rows 1048576] [--json out.json]

Kernel shares (normalise / sweep / merge) come from a run of their own under a kernel trace:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bank_bench.py --calls 10
"""
import argparse, ctypes as C, json, os, sys, tempfile, time
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--bank-rows", type=int, default=1 << 20)
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


def stats(ts):
    ts = np.sort(np.asarray(ts)) * 1e3
    return {"median_ms": float(np.median(ts)), "min_ms": float(ts[0]), "p90_ms": float(ts[int(0.9 * (len(ts) - 1))])}


def kernel_ms(tq, tb, k, floor_only):
    ms = C.c_float(0)
    rc = api.lib().dinov2_hip_op_bank_bench(tq.data_ptr(), tq.shape[0], tb.data_ptr(), tb.shape[0], tq.shape[1], k, 0, args.warmup, args.calls,
                                            int(floor_only), C.byref(ms))
    assert rc == 0, rc
    return float(ms.value)


results = []
for nq, nb, H, with_match in ((32, args.bank_rows, 1024, False), (1369, 1369, 1024, True)):
    g = torch.Generator(device="cuda").manual_seed(nq + H)
    tb = torch.randn((nb, H), generator=g, device="cuda")
    tq = (tb[torch.randperm(nb, device="cuda")[:nq]] + 0.5 * torch.randn((nq, H), generator=g, device="cuda")).contiguous()
    tbn = F.normalize(tb, dim=1).half()  # the yardstick's resident bank
    torch.cuda.synchronize()
    bank = api.Bank(model, H, nb)
    slab = 1 << 16
    for r0 in range(0, nb, slab):
        rows = tb[r0:r0 + slab]
        r = api.Rows(api.ROWS_GIVEN, rows.data_ptr(), rows.shape[0], H, 0, 1)
        err = C.create_string_buffer(256)
        assert api.lib().dinov2_hip_bank_add(sess._h, bank._h, C.byref(r), None, err, len(err)) == 0, err.value
    assert bank.count == nb
    for k in (1, 20, 64):
        idx, sim = np.empty((nq, k), np.int32), np.empty((nq, k), np.float32)
        req = api.TopK(api.Rows(api.ROWS_GIVEN, tq.data_ptr(), nq, H, 0, 1), k, idx.ctypes.data, sim.ctypes.data)
        err = C.create_string_buffer(256)
        t_hip, t_ref, t_match = [], [], []
        for i in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            rc = api.lib().dinov2_hip_bank_topk(sess._h, bank._h, C.byref(req), err, len(err))  # synchronous: returns after the copy-out
            t1 = time.perf_counter()
            top = (F.normalize(tq, dim=1).half() @ tbn.T).topk(k, dim=1)
            ref = [top.indices.cpu(), top.values.cpu()]  # (.cpu() waits for the device)
            t2 = time.perf_counter()
            assert rc == 0, err.value
            if with_match and k == 1:
                m = api.Match(tq.data_ptr(), tb.data_ptr(), nq, nb, H, 0, 0, 1, idx.ctypes.data, sim.ctypes.data, None, None)
                t3 = time.perf_counter()
                assert api.lib().dinov2_hip_match_tokens(sess._h, C.byref(m), err, len(err)) == 0, err.value
                t_match.append(time.perf_counter() - t3)
            if i >= args.warmup:
                t_hip.append(t1 - t0)
                t_ref.append(t2 - t1)
        full, floor = kernel_ms(tq, tb, k, False), kernel_ms(tq, tb, k, True)
        row = {"nq": nq, "nb": nb, "H": H, "k": k, "bank_topk": stats(t_hip), "torch_yardstick": stats(t_ref), "kernels_ms": full, "floor_ms": floor,
               "bank_TBps": nb * H * 2 / (full * 1e-3) / 1e12, "floor_TBps": nb * H * 2 / (floor * 1e-3) / 1e12,
               "tflops": 2.0 * nq * nb * H / (full * 1e-3) / 1e12, "plan": api.bank_plan(nq, nb, H, k),
               "same_top1": float((ref[0].numpy()[:, 0] == idx[:, 0]).mean())}  # (not a check: the yardstick rounds the product to f16)
        if t_match:
            row["match_tokens"] = stats(t_match[args.warmup:])
        results.append(row)
        print(json.dumps(row), flush=True)
    bank.free()
    del tb, tq, tbn
    torch.cuda.empty_cache()
if args.json:
    with open(args.json, "w") as f:
        json.dump({"build_id": api.build_id(), "calls": args.calls, "results": results}, f, indent=1)
