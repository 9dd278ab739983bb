#!/usr/bin/env python3
"""Times dinov2_hip_bank_topk_probe (csrc/probe.hip) as the search step of an inverted file, next to dinov2_hip_bank_topk sweeping the same
bank for the same queries, in the same run, the two alternating, and reports recall@k of the probed search against that brute force.

The gallery is synthetic and clustered: `--rows` rows around 4 096 centres that lie in a 16-dimensional subspace.  Per list count the coarse quantiser is trained by
Session.kmeans on a subsample, every row is assigned by dinov2_hip_bank_topk (k = 1) on a small bank of the centres, api.ivf_order sorts
the rows by list and they are added to the bank list by list.  Per query set the probes are dinov2_hip_bank_topk (k = n_probe) on the bank
of centres (timed apart, as `coarse`).

Both routes are host wall clock around calls that end in a device synchronise (the probed call includes its host-side planner), per
window the mean of `--inner` calls; `--repeats` windows after `--warmup`.  `read` is the share of the bank's rows the items walk, counted
from the plan.  Writes the table as markdown.

    python tools/probe_bench.py [--rows 1048576] [--H 1024] [--k 10] [--repeats 5] [--warmup 2] [--out profiles/bank_probe.md] [--json out.json]
"""
import argparse, ctypes as C, json, os, sys, time
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=1 << 20)
ap.add_argument("--H", type=int, default=1024)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--inner", type=int, default=10)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "bank_probe.md"))
ap.add_argument("--json", default=None)
args = ap.parse_args()
import torch
torch.cuda.init()  # (before the library touches the device: torch's lazy init fails when it comes second; no GPU: this raises)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from importlib import import_module
from __graft_entry__ import PKG_NAME, load_package
pkg = load_package(); api = import_module(PKG_NAME + ".api")
L = api.lib()
model = api.Model(os.path.join(ROOT, "tests", "golden", "tiny_gelu_reg4.gguf"))  # (a session needs one; no forward runs)
sess = api.Session(model)
N, H, K = args.rows, args.H, args.k
CHUNK = 1 << 16


def dev_rows(t):
    return api.Rows(api.ROWS_GIVEN, t.data_ptr(), t.shape[0], t.shape[1], 0, 1)


def add(bank, t):
    api._call(L.dinov2_hip_bank_add, sess._h, bank._h, C.byref(dev_rows(t)), None)


def topk(bank, t, k):
    out = {"idx": np.empty((t.shape[0], k), np.int32), "sim": np.empty((t.shape[0], k), np.float32)}
    req = api.TopK(dev_rows(t), k, out["idx"].ctypes.data, out["sim"].ctypes.data)
    api._call(L.dinov2_hip_bank_topk, sess._h, bank._h, C.byref(req))
    return out


def wall(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner * 1e3


g = torch.Generator(device="cuda").manual_seed(N + H)
true_c = torch.randn((4096, 16), generator=g, device="cuda") @ torch.randn((16, H), generator=g, device="cuda")


def draw(n):
    """n rows: one of the 4 096 true centres -- themselves points of a 16-dimensional subspace, so that a coarse quantiser has neighbouring
    clusters to group -- plus noise of half its norm (cosine to the centre about 0.9)."""
    lab = torch.randint(0, len(true_c), (n,), generator=g, device="cuda")
    return true_c[lab] + 2.0 * torch.randn((n, H), generator=g, device="cuda")


rows = torch.cat([draw(min(CHUNK, N - i)) for i in range(0, N, CHUNK)])
sample = rows[torch.randperm(N, generator=g, device="cuda")[:min(N, 1 << 16)]].cpu().numpy()
queries = {nq: draw(nq) for nq in (1, 32, 128, 1369)}
torch.cuda.synchronize()  # (torch's stream wrote them; the session's stream reads them)
results = []
for lists in (256, 1024):
    centers = sess.kmeans(sample, K=lists, max_iter=10)["centers"]
    cbank = api.Bank(model, H, lists)
    cbank.add(sess, centers)
    labels = np.concatenate([topk(cbank, rows[i:i + CHUNK], 1)["idx"][:, 0] for i in range(0, N, CHUNK)])
    perm, first, ln = api.ivf_order(labels, lists)
    used = np.flatnonzero(ln > 0)
    seg_of = np.full(lists + 1, -1, np.int32)  # (a list id of -1 stays -1)
    seg_of[used] = np.arange(len(used), dtype=np.int32)
    first, ln = np.ascontiguousarray(first[used]), np.ascontiguousarray(ln[used])
    segments = np.stack([first, ln], 1)
    bank = api.Bank(model, H, N)
    perm_t = torch.from_numpy(perm.astype(np.int64)).cuda()
    for i in range(0, N, CHUNK):
        chunk = rows[perm_t[i:i + CHUNK]]
        torch.cuda.synchronize()  # (the gather runs on torch's stream, the add on the session's)
        add(bank, chunk)
    for nq, q in queries.items():
        brute = topk(bank, q, K)
        for n_probe in (1, 8, 32):
            coarse = lambda: topk(cbank, q, n_probe)  # noqa: E731
            probes = np.ascontiguousarray(seg_of[coarse()["idx"]])
            out = {"idx": np.empty((nq, K), np.int32), "sim": np.empty((nq, K), np.float32)}
            req = api.TopkProbe(dev_rows(q), len(ln), first.ctypes.data, ln.ctypes.data, n_probe, probes.ctypes.data, K, out["idx"].ctypes.data,
                                out["sim"].ctypes.data)
            probe = lambda: api._call(L.dinov2_hip_bank_topk_probe, sess._h, bank._h, C.byref(req))  # noqa: E731
            sweep = lambda: topk(bank, q, K)  # noqa: E731
            t = {"probe": [], "sweep": [], "coarse": []}
            for i in range(args.warmup + args.repeats):
                for name, fn in (("probe", probe), ("sweep", sweep), ("coarse", coarse)):
                    ms = wall(fn, args.inner)
                    if i >= args.warmup:
                        t[name].append(ms)
            recall = float(np.mean([len(set(a) & set(b)) / K for a, b in zip(out["idx"].tolist(), brute["idx"].tolist())]))
            plan = api.op_bank_probe_plan(nq, N, H, segments, probes, K)
            it = plan["items"]
            walked = int(it[:, 2].sum())
            row = {"rows": N, "H": H, "k": K, "lists": lists, "nq": nq, "n_probe": n_probe, "recall": recall, "probe_ms": t["probe"],
                   "sweep_ms": t["sweep"], "coarse_ms": t["coarse"], "n_wide": plan["n_wide"], "n_narrow": plan["n_narrow"],
                   "piece_tiles": plan["piece_tiles"], "npass": plan["npass"], "queries_per_item": float(it[:, 3].mean()),
                   "rows_walked": walked, "read": walked / N, "bytes_walked": walked * plan["hpad"] * 2}
            results.append(row)
            print(json.dumps(row), flush=True)
    bank.free()
    cbank.free()


def mmm(v):
    return "%.3f (%.3f – %.3f)" % (float(np.median(v)), min(v), max(v))


lines = ["# Inverted-file search: top-k over probed lists against the sweep of the whole bank", "",
         "`tools/probe_bench.py` on one %s, build `%s`, torch %s; bank of %d x %d, k = %d; %d windows of %d calls after %d, the routes"
         % (torch.cuda.get_device_name(0), api.build_id(), torch.__version__, N, H, K, args.repeats, args.inner, args.warmup),
         "alternating; the device clock was not read.  Milliseconds per call, median (min – max) over the windows: host wall clock around calls",
         "that end in a synchronise.  `probe` is one `dinov2_hip_bank_topk_probe` (its host-side planner included), `sweep` one",
         "`dinov2_hip_bank_topk` over the whole bank with the same device-resident queries, `coarse` the `dinov2_hip_bank_topk` on the bank of",
         "centres that names the lists (needed before `probe`, not included in it).  `read` = the bank rows the items walk over the bank's rows",
         "(a list probed by several items counts once per item); GB/s = those bytes over the median probe time, host overheads and all.", "",
         "| lists | nq | n_probe | recall@k | items wide + narrow | tiles a piece | queries / item | read | probe ms | sweep ms | sweep / probe | coarse ms | GB/s |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
for r in results:
    pm = float(np.median(r["probe_ms"]))
    lines.append("| %d | %d | %d | %.3f | %d + %d | %d | %.1f | %.4f | %s | %s | %.1f | %s | %.0f |" % (
        r["lists"], r["nq"], r["n_probe"], r["recall"], r["n_wide"], r["n_narrow"], r["piece_tiles"], r["queries_per_item"], r["read"],
        mmm(r["probe_ms"]), mmm(r["sweep_ms"]), np.median(r["sweep_ms"]) / pm, mmm(r["coarse_ms"]), r["bytes_walked"] / (pm * 1e-3) / 1e9))
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
if args.json:
    with open(args.json, "w") as f:
        json.dump({"build_id": api.build_id(), "results": results}, f, indent=1)
