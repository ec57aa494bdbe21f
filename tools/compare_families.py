"""Kernel families and source files of several rocprofv3 kernel traces of the same bench command, side by side (ms per step).

    python tools/compare_families.py --steps 4 A1=a1_kernel_trace.csv A2=a2_kernel_trace.csv B=b_kernel_trace.csv ...

The first two traces are taken as the same library traced twice: their difference is the trace-to-trace repeatability that every other
column is set against.  A kernel belongs to the source file of esvit_amd/csrc that defines it (kernels defined in a header are listed
under the header: gemm_kernels.h is instantiated by gemm.hip in the training step).  tools/kernel_families.py has the grouping by name
for a single kernel_stats.csv; this one reads the traces themselves so that no two runs need --stats.
"""
import collections
import csv
import os
import re
import sys

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "esvit_amd", "csrc")


def kernel_files():
    """kernel name -> source file, from the __global__ definitions of csrc"""
    out = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            for m in re.finditer(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", open(os.path.join(CSRC, f)).read()):
                out.setdefault(m.group(1), f)
    return out


def kernel_name(n):
    """the bare kernel name of a demangled or mangled trace entry"""
    n = re.sub(r"^void ", "", n)
    n = re.sub(r"\(anonymous namespace\)::", "", n)
    m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", n)
    if m:
        k = int(m.group(1))
        return n[m.end():m.end() + k]
    m = re.match(r"([A-Za-z0-9_:]+?)\s*[<(]", n)
    return (m.group(1) if m else n)[:50]


def load(path):
    fam = collections.defaultdict(float)
    for r in csv.DictReader(open(path)):
        fam[kernel_name(r["Kernel_Name"])] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
    return fam


def main():
    args = sys.argv[1:]
    steps = 1.0
    if args and args[0] == "--steps":
        steps = float(args[1])
        args = args[2:]
    labels = [a.split("=", 1)[0] for a in args]
    traces = [load(a.split("=", 1)[1]) for a in args]
    files = kernel_files()
    names = sorted(set().union(*traces), key=lambda k: -traces[0].get(k, 0.0))
    print("# ms per step (%g traced steps); repeat = |%s - %s|" % (steps, labels[0], labels[1] if len(labels) > 1 else labels[0]))
    hdr = "%-34s %-20s" % ("kernel", "file") + "".join("%10s" % l for l in labels) + "%10s" % "repeat"
    print(hdr)
    per_file = collections.defaultdict(lambda: [0.0] * len(traces))
    for k in names:
        v = [t.get(k, 0.0) / steps for t in traces]
        f = files.get(re.sub(r".*::", "", k), "-")
        for i, x in enumerate(v):
            per_file[f][i] += x
        if max(v) >= 0.02:
            print("%-34s %-20s" % (k[:34], f) + "".join("%10.3f" % x for x in v) + "%10.3f" % (abs(v[0] - v[1]) if len(v) > 1 else 0.0))
    print()
    print("# per source file")
    print(hdr)
    for f, v in sorted(per_file.items(), key=lambda kv: -kv[1][0]):
        print("%-34s %-20s" % ("(all kernels)", f) + "".join("%10.3f" % x for x in v) + "%10.3f" % (abs(v[0] - v[1]) if len(v) > 1 else 0.0))
    tot = [sum(v[i] for v in per_file.values()) for i in range(len(traces))]
    print("%-55s" % "total" + "".join("%10.3f" % x for x in tot))


if __name__ == "__main__":
    main()
