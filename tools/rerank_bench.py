#!/usr/bin/env python3
"""Times dinov2_hip_bank_rerank (csrc/rerank.hip) -- S candidates of `len` rows each, resident in a bank, scored against nq query rows in
one call -- next to the two ways of getting the same scores without it, in the same run on the same device, the three alternating:

  loop    the loop it replaces: S calls of dinov2_hip_match_tokens on device-resident f32 operands (each normalises both sides, runs five
          launches, copies four arrays to the host and waits), the host reduction of the arrays not counted
  torch   PyTorch-ROCm, which the product never calls: bmm of the f16 unit queries with the gathered segments, amax in both directions and
          the sums, in chunks of at most 100 segments, one synchronise at the end

All three are host wall clock around calls that end in a device synchronise, per repeat the mean of `--inner` calls; `--repeats` repeats after
`--warmup`.  `device` is the call's device work alone by HIP events (dinov2_hip_op_rerank_bench: normalise, table uploads, both kernels, the
copies out), from which the achieved rate 2 nq sum(len) hpad / time is formed.  Writes the table as markdown.

    python tools/rerank_bench.py [--repeats 5] [--warmup 2] [--out profiles/bank_rerank.md] [--json out.json]
"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bank_rerank.md"))
ap.add_argument("--json", default=None)
args = ap.parse_args()
import torch
import torch.nn.functional as F
torch.cuda.init()  # (before the library touches the device: torch's lazy init fails when it comes second; no GPU: this raises)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from importlib import import_module
from __graft_entry__ import PKG_NAME, load_package
pkg = load_package(); api = import_module(PKG_NAME + ".api")
L = api.lib()
model = api.Model(os.path.join(ROOT, "tests", "golden", "tiny_gelu_reg4.gguf"))  # (a session needs one; no forward runs)
sess = api.Session(model)


def wall(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e3


results = []
for nq, ln, H, S in ((1369, 1369, 1024, 20), (1369, 1369, 1024, 100), (1369, 1369, 1024, 1000), (256, 256, 384, 100)):
    g = torch.Generator(device="cuda").manual_seed(nq + H + S)
    q = torch.randn((nq, H), generator=g, device="cuda")
    rows = torch.randn((S * ln, H), generator=g, device="cuda")
    q16, rows16 = F.normalize(q, dim=1).half(), F.normalize(rows, dim=1).half().view(S, ln, H)
    torch.cuda.synchronize()
    first, lens = np.arange(S, dtype=np.int32) * ln, np.full(S, ln, np.int32)
    bank = api.Bank(model, H, S * ln)
    r = api.Rows(api.ROWS_GIVEN, rows.data_ptr(), S * ln, H, 0, 1)
    api._call(L.dinov2_hip_bank_add, sess._h, bank._h, C.byref(r), None)
    out = api._rerank_out(S)
    req = api.Rerank(api.Rows(api.ROWS_GIVEN, q.data_ptr(), nq, H, 0, 1), S, first.ctypes.data, lens.ctypes.data, -np.inf,
                     *[out[k].ctypes.data for k in ("score_q", "score_b", "mutual", "mutual_sim")])
    m_out = [np.empty(nq, np.int32), np.empty(nq, np.float32), np.empty(ln, np.int32), np.empty(ln, np.float32)]

    def ours():
        api._call(L.dinov2_hip_bank_rerank, sess._h, bank._h, C.byref(req))

    def loop():
        for s in range(S):
            m = api.Match(q.data_ptr(), rows.data_ptr() + s * ln * H * 4, nq, ln, H, 0, 0, 1, *[a.ctypes.data for a in m_out])
            api._call(L.dinov2_hip_match_tokens, sess._h, C.byref(m))

    def torch_route():
        res = []
        for s0 in range(0, S, 100):
            sim = torch.matmul(q16, rows16[s0:s0 + 100].transpose(1, 2))  # [<= 100, nq, len]
            res.append((sim.amax(2).float().sum(1), sim.amax(1).float().sum(1)))
        return [torch.cat(x).cpu() for x in zip(*res)]

    t = {"ours": [], "loop": [], "torch": []}
    for i in range(args.warmup + args.repeats):
        for name, fn, inner in (("ours", ours, args.inner), ("loop", loop, 1), ("torch", torch_route, args.inner)):
            ms = wall(fn, inner)
            if i >= args.warmup:
                t[name].append(ms)
    # the loop's last call scored the last segment: the same number
    assert abs(float(m_out[1].astype(np.float64).sum()) - float(out["score_q"][S - 1])) <= nq * 2.0 ** -24 * nq
    dev = (C.c_float * args.repeats)()
    rc = L.dinov2_hip_op_rerank_bench(q.data_ptr(), nq, rows.data_ptr(), S * ln, H, api._ptr(first), api._ptr(lens), S, args.warmup, args.repeats, dev)
    assert rc == 0, rc
    flop = 2.0 * nq * S * ln * (-(-H // 64) * 64)
    row = {"nq": nq, "len": ln, "H": H, "S": S, "plan": {k: v for k, v in api.op_rerank_plan(nq, H, lens).items() if k != "pass_of"},
           "ours_ms": t["ours"], "loop_ms": t["loop"], "torch_ms": t["torch"], "device_ms": list(dev), "flop": flop,
           "tflops": flop / (min(dev) * 1e-3) / 1e12}
    results.append(row)
    print(json.dumps(row), flush=True)
    bank.free()
    del q, rows, q16, rows16
    torch.cuda.empty_cache()


def mmm(v):
    return "%.3f (%.3f – %.3f)" % (float(np.median(v)), min(v), max(v))


lines = ["# Re-ranking a shortlist: one call against the loop of match calls", "",
         "`tools/rerank_bench.py` on one %s, build `%s`, torch %s; %d repeats after %d, the three routes alternating; the device clock was not"
         % (torch.cuda.get_device_name(0), api.build_id(), torch.__version__, args.repeats, args.warmup),
         "read.  Milliseconds per scored shortlist, median (min – max): host wall clock around calls that end in a synchronise.  `ours` is one",
         "`dinov2_hip_bank_rerank` with device-resident queries; `loop` is S calls of `dinov2_hip_match_tokens` on device-resident operands (the",
         "host's reduction of its four arrays not counted); `torch` is `matmul` + `amax` + `sum` on f16 unit rows, which gives the two scores only.",
         "`device` is the call's device work by HIP events (minimum), and TFLOP/s is 2 · nq · Σlen · hpad over it.", "",
         "| nq | len | H | S | workgroups | passes | ours ms | loop ms | loop / ours | torch ms | device ms | TFLOP/s |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|"]
for r in results:
    lines.append("| %d | %d | %d | %d | %d | %d | %s | %s | %.1f | %s | %.3f | %.1f |" % (
        r["nq"], r["len"], r["H"], r["S"], r["S"] * r["plan"]["qtiles"], r["plan"]["npass"], mmm(r["ours_ms"]), mmm(r["loop_ms"]),
        np.median(r["loop_ms"]) / np.median(r["ours_ms"]), mmm(r["torch_ms"]), min(r["device_ms"]), r["tflops"]))
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
if args.json:
    with open(args.json, "w") as f:
        json.dump({"build_id": api.build_id(), "results": results}, f, indent=1)
