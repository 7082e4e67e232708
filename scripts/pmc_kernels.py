"""Per-launch means of rocprofv3 --pmc counters for the kernels whose names
contain one of the given words.

Usage: python scripts/pmc_kernels.py <dir of a --pmc run> <word> [<word> ...]
Reads every *counter_collection.csv under the directory; prints one JSON
object {kernel: {counter: mean per launch, "launches": n}}.
"""
import csv
import glob
import json
import os
import re
import sys


def short(name):
    name = name.replace("otm::(anonymous namespace)::", "").replace("void ", "")
    return re.sub(r"\(.*", "", name)


def main():
    d, words = sys.argv[1], sys.argv[2:]
    acc = {}
    for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            k = short(r["Kernel_Name"])
            if not any(w in k for w in words):
                continue
            acc.setdefault(k, {}).setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
    out = {}
    for k, cs in sorted(acc.items()):
        out[k] = {c: round(sum(v) / len(v), 1) for c, v in sorted(cs.items())}
        out[k]["launches"] = max(len(v) for v in cs.values())
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
