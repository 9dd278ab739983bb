"""What attention rows cost (dinov2_hip_predict_attention): synthetic ViT-L/14 + 4 registers, f16, 518 x 518, device-resident inputs and
outputs.  Modelled on tools/layers_cost.py, whose set-up, timing loop and parent-library worker it uses.

  (a) batch 32, interleaved round by round: plain predict on a build of the PARENT commit (--parent-lib; a child process), plain predict on
      this tree, and predict_attention with the CLS rows of all 24 blocks.  Plain against parent is the no-regression reading.
  (b) the CLS rows' own time: HIP events per launch (dinov2_hip_session_profile, kind "layer_tap"), next to the final LayerNorm's, with the
      achieved bytes/s of both.  One launch reads K of one block, B T H 2 bytes, and one q row per head.
  (c) batch 1: one full T x T map (all 1 374 queries) of the last block, per-launch time.

Prints one JSON line; --markdown FILE appends a table.  Run the whole tool under a time limit of its own.

  python tools/attention_rows_cost.py [--parent-lib LIB] [--rounds 7] [--iters 10] [--markdown profiles/attention_rows.md]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layers_cost as lc  # noqa: E402

L, NH, T = 24, 16, 1 + lc.R + lc.P


def per_launch(sess, fn, iters):
    sess.profile(True)
    for _ in range(iters):
        fn()
    prof = sess.profile_read()
    sess.profile(False)
    return (prof["layer_tap"][0] * 1e3 / prof["layer_tap"][1], prof["layer_tap"][1],
            prof["final_layernorm"][0] * 1e3 / prof["final_layernorm"][1])


def measure(gguf, rounds, iters, parent_lib):
    B = 32
    api, sess, x = lc.setup(gguf, B)
    out = api.DeviceArray((B, lc.P, lc.H))
    rows = api.DeviceArray((L, B, NH, 1, T))
    layers = list(range(1, L + 1))
    arms = {"b_plain": lambda: sess.predict_device(x.ptr, B, lc.SIZE, lc.SIZE, classify=False, patch_ptr=out.ptr),
            "c_cls_rows_24": lambda: sess.predict_attention_device(x.ptr, B, lc.SIZE, lc.SIZE, layers, rows, patch_ptr=out.ptr)}
    child = None
    if parent_lib:
        child = subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", "layers_cost.py"), "--worker", gguf, str(B), str(iters),
                                  os.path.abspath(parent_lib)], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        assert lc.read_line(child, "ready line") == "ready"
    for fn in arms.values():
        lc.timed(fn, sess, 3)
    ms = {k: [] for k in (["a_parent"] if child else []) + list(arms)}
    for _ in range(rounds):
        if child:
            child.stdin.write("go\n")
            child.stdin.flush()
            ms["a_parent"].append(float(lc.read_line(child, "timing")))
        for k, fn in arms.items():
            ms[k].append(lc.timed(fn, sess, iters))
    if child:
        child.stdin.write("quit\n")
        child.stdin.flush()
        child.wait(timeout=60)
    res = {"batch": B, "rounds": rounds, "iters": iters, "build": api.build_id()}
    for k, v in ms.items():
        res[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    us, n, ln_us = per_launch(sess, arms["c_cls_rows_24"], iters)
    k_bytes = B * T * lc.H * 2
    res["cls_rows"] = {"us_per_launch": us, "launches": n, "K_bytes": k_bytes, "TBps": k_bytes / us / 1e6, "final_ln_us": ln_us,
                       "final_ln_TBps": 2 * 4 * B * T * lc.H / ln_us / 1e6}
    # (c) one full map at batch 1
    x1 = api.DeviceArray.from_host(api.DeviceArray.to_host(x)[:1])
    full = api.DeviceArray((1, 1, NH, T, T))
    qs = list(range(T))
    fn = lambda: sess.predict_attention_device(x1.ptr, 1, lc.SIZE, lc.SIZE, [L], full, qs)  # noqa: E731
    lc.timed(fn, sess, 3)
    us, n, _ = per_launch(sess, fn, iters)
    res["full_map_b1"] = {"us_per_launch": us, "launches": n, "queries": T, "out_bytes": 4 * NH * T * T,
                          "out_TBps": 4 * NH * T * T / us / 1e6}
    return res


def markdown(r):
    lines = ["| arm (batch 32) | step ms (median, min - max) |", "|---|---|"]
    for k in ("a_parent", "b_plain", "c_cls_rows_24"):
        if k + "_ms" in r:
            m = r[k + "_ms"]
            lines.append(f"| {k} | {m['median']:.3f} ({m['min']:.3f} - {m['max']:.3f}) |")
    c, f = r["cls_rows"], r["full_map_b1"]
    lines += ["", f"CLS rows, batch 32: {c['us_per_launch']:.1f} us per launch over {c['launches']} launches, {c['K_bytes'] / 1e6:.1f} MB of K: "
              f"{c['TBps']:.2f} TB/s (final LayerNorm: {c['final_ln_us']:.1f} us, {c['final_ln_TBps']:.2f} TB/s).",
              f"Full {f['queries']} x {f['queries']} map of one block, batch 1: {f['us_per_launch']:.1f} us per launch "
              f"({f['out_bytes'] / 1e6:.1f} MB written, {f['out_TBps']:.2f} TB/s of output).", f"Build: {r['build']}.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--markdown")
    a = ap.parse_args()
    from __graft_entry__ import load_package
    pkg = load_package()
    with tempfile.TemporaryDirectory() as td:
        gguf = os.path.join(td, "large.gguf")
        pkg.synth.write_synthetic_gguf(gguf, "large", registers=lc.R, num_classes=1000, seed=42)
        r = measure(gguf, a.rounds, a.iters, a.parent_lib)
    print(json.dumps(r), flush=True)
    if a.markdown:
        with open(a.markdown, "a") as f:
            f.write(markdown(r))


if __name__ == "__main__":
    main()
