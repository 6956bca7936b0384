#!/usr/bin/env python3
"""keep_regions_label parted into its two stages by a kernel trace.

The call launches the labelling kernels of tissue.hip (cc_*) and then rank + relabel (regions_root_count / regions_scan /
regions_root_rank / regions_relabel); device events around the call see the sum.  Run the call alone on one mask under the
profiler, once per mask, each run into a directory named after the mask:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR/tissue -- \\
        python tools/regions_bench.py --sizes 8192 --calls label --masks tissue --reps 20 --out ""

and give the directories to this tool, which reads every *kernel_stats.csv below each of them:

    python tools/regions_kernel_split.py DIR/tissue DIR/raw ... [--out profiles/regions_kernel_split.txt]

Per mask it prints the kernel time of one call in each stage (the stage's TotalDurationNs over the calls of regions_relabel_kernel,
which runs once per call; the warm-up calls count like the timed ones) and every kernel's launches per call and average.  Kernel time
leaves out the gaps between launches, so the two stages add up to less than the device-event time of the call.
"""
import argparse
import csv
import glob
import os
import sys

LINES = []
RANK = ("regions_root_count_kernel", "regions_scan_kernel", "regions_root_rank_kernel", "regions_relabel_kernel")


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def short(name):
    return name.split("(")[0].split("<")[0].split()[-1].split("::")[-1]          # no return type, namespace, template or arguments


def read(directory):
    """{kernel: (calls, total ns)} summed over the directory's kernel summaries."""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                k = short(r["Name"])
                c, t = out.get(k, (0, 0))
                out[k] = (c + int(r["Calls"]), t + int(r["TotalDurationNs"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dirs", nargs="+")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    say("tools/regions_kernel_split.py: kernel time of one keep_regions_label call, from rocprofv3 --kernel-trace --stats (one box)")
    for d in a.dirs:
        stats = read(d)
        calls = stats.get("regions_relabel_kernel", (0, 0))[0]
        if not calls:
            sys.exit(f"{d}: no regions_relabel_kernel in a *kernel_stats.csv below it")
        stage = {"labelling": 0, "rank + relabel": 0}
        for k, (c, t) in stats.items():
            if k.startswith("cc_"):
                stage["labelling"] += t
            elif k in RANK:
                stage["rank + relabel"] += t
        total = sum(stage.values())
        say(f"{os.path.basename(os.path.normpath(d))}: {calls} calls; labelling {stage['labelling'] / calls / 1e6:.3f} ms, rank + relabel "
            f"{stage['rank + relabel'] / calls / 1e6:.3f} ms per call ({100 * stage['rank + relabel'] / total:.1f} % of the call's kernel time)")
        for k, (c, t) in sorted(stats.items(), key=lambda kv: -kv[1][1]):
            if k.startswith("cc_") or k in RANK:
                say(f"    {k:28s} {c / calls:6.1f} launches per call, average {t / c / 1e3:9.1f} us, {t / calls / 1e6:8.3f} ms per call")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
