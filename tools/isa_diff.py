#!/usr/bin/env python3
"""Device instruction streams of two source trees, compared function by function (no GPU needed).

    tools/isa_diff.py <tree A> <tree B> [csrc/gemm.hip csrc/gemm2.hip ...]        (default: the three GEMM files)

Each named file (relative to <tree>/dinov2.cpp_amd) is cross-compiled from both trees with the Makefile's CXXFLAGS plus
`-S --cuda-device-only`, and the assembly is normalised the way tests/test_kernel_build_checks.py::misc_instruction_streams does it:
comments and directives dropped, branch labels numbered per function.  Per file: functions and instructions on either side, and the names
of the functions whose streams differ (with the size of a unified diff of the two).  Exit status 1 if anything differs.  A refactor that is
meant to leave the kernels alone proves it with `git worktree add /tmp/parent HEAD~1 && tools/isa_diff.py /tmp/parent .`; one that moves
the similarity tile of csrc/sim_tile.h names its users: `... /tmp/parent . csrc/match.hip csrc/bank.hip csrc/kmeans.hip`."""
import argparse
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
DEFAULT_FILES = ["csrc/gemm.hip", "csrc/gemm2.hip", "csrc/gemm4.hip"]


def makefile_cxxflags(tree, arch):
    """The CXXFLAGS line of <tree>/dinov2.cpp_amd/Makefile, $(ARCH) expanded."""
    txt = open(os.path.join(tree, "dinov2.cpp_amd", "Makefile")).read()
    m = re.search(r"^CXXFLAGS\s*=\s*(.*)$", txt, re.M)
    if not m:
        sys.exit("no CXXFLAGS in %s's Makefile" % tree)
    return m.group(1).replace("$(ARCH)", arch).split()


def instruction_streams(asm_text):
    """function name -> its instructions (comments and directives dropped, branch labels numbered per function)."""
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end", asm_text, re.S | re.M):
        ins = []
        for line in m.group(2).splitlines():
            s = line.split(";")[0].strip()
            if s and not s.startswith(".") and not s.endswith(":"):
                ins.append(re.sub(r"\.LBB\d+_(\d+)", r"L\1", s))
        out[m.group(1)] = ins
    return out


def compile_asm(tree, rel, arch, extra, out):
    src = os.path.join(tree, "dinov2.cpp_amd", rel)
    cmd = [HIPCC, *makefile_cxxflags(tree, arch), *extra, "-x", "hip", "-S", "--cuda-device-only", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("%s failed:\n%s" % (" ".join(cmd), r.stderr[-4000:]))
    return instruction_streams(open(out).read())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("files", nargs="*", default=DEFAULT_FILES)
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--flags", default="", help="extra compiler flags for both sides, e.g. '-DDINO_PREC=31'")
    ap.add_argument("--jobs", type=int, default=6)
    ap.add_argument("--show", type=int, default=0, metavar="N", help="print the first N lines of each differing function's diff")
    ap.add_argument("--rename", action="append", default=[], metavar="REGEX=REPL",
                    help="rewrite function names on both sides before they are matched (repeatable): for a change that alters mangled names "
                         "but must not alter bodies, e.g. a defaulted template parameter")
    a = ap.parse_args()
    extra = a.flags.split()

    def renamed(fns):
        out = {}
        for n, ins in fns.items():
            for r in a.rename:
                pat, _, repl = r.partition("=")
                n = re.sub(pat, repl, n)
            if n in out:
                sys.exit("--rename maps two functions to %s" % n)
            out[n] = ins
        return out
    differing = 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        jobs = {(side, rel): pool.submit(compile_asm, tree, rel, a.arch, extra, os.path.join(tmp, "%s_%s.s" % (side, os.path.basename(rel))))
                for rel in a.files for side, tree in (("a", a.tree_a), ("b", a.tree_b))}
        for rel in a.files:
            fa, fb = renamed(jobs["a", rel].result()), renamed(jobs["b", rel].result())
            names = sorted(set(fa) | set(fb))
            diff = [n for n in names if fa.get(n) != fb.get(n)]
            differing += len(diff)
            print("%s: A %d functions / %d instructions, B %d functions / %d instructions, %d differ" %
                  (rel, len(fa), sum(map(len, fa.values())), len(fb), sum(map(len, fb.values())), len(diff)))
            for n in diff:
                if n not in fa or n not in fb:
                    print("  %s: only in %s" % (n, "A" if n in fa else "B"))
                    continue
                d = [l for l in difflib.unified_diff(fa[n], fb[n], lineterm="", n=0) if not l.startswith(("---", "+++", "@@"))]
                print("  %s: %d / %d instructions, %d diff lines" % (n, len(fa[n]), len(fb[n]), len(d)))
                for l in d[:a.show]:
                    print("      " + l)
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
