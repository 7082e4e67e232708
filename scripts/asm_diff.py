#!/usr/bin/env python3
"""Compare the device assembly of every .hip file in reporter_amd/csrc between
two git revisions, kernel by kernel.  No GPU needed.

    scripts/asm_diff.py REV_A [REV_B]      (REV_B defaults to the working tree;
                                            the word WORKTREE names it too)

Each revision's reporter_amd/csrc and include/ are unpacked under
build/asm_diff/ and every .hip file is compiled with that revision's Makefile
HIPFLAGS plus --cuda-device-only -S.  Per function symbol (kernels, and any
device function the compiler left out of line) the script prints one of
identical / differs / added / removed; what is not a function's (device
variables, the rest of the metadata) is compared as one entry "<data>" per
file.  Before comparing, the per-file __hip_cuid_<hash> symbol and the
function numbers inside local labels (.LBB<n>_<m>, .Lfunc_end<n>), which shift
when a function is added or removed above, are normalised.
"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("reporter_amd", "csrc")
WORK = os.path.join(ROOT, "build", "asm_diff")


def unpack(rev):
    """The revision's sources under build/asm_diff/<name>/; returns that directory."""
    name = "worktree" if rev == "WORKTREE" else subprocess.check_output(
        ["git", "-C", ROOT, "rev-parse", "--short", rev + "^{commit}"], text=True).strip()
    dst = os.path.join(WORK, name)
    subprocess.check_call(["rm", "-rf", dst])
    os.makedirs(dst)
    if rev == "WORKTREE":
        files = subprocess.check_output(["git", "-C", ROOT, "ls-files", "-co", "--exclude-standard", CSRC, "include"],
                                        text=True).split("\n")
        tar = subprocess.Popen(["tar", "-C", ROOT, "-cf", "-", "-T", "-"], stdin=subprocess.PIPE,
                               stdout=subprocess.PIPE)
        untar = subprocess.Popen(["tar", "-C", dst, "-xf", "-"], stdin=tar.stdout)
        tar.stdin.write("\n".join(f for f in files if f and os.path.exists(os.path.join(ROOT, f))).encode())
        tar.stdin.close()
    else:
        tar = subprocess.Popen(["git", "-C", ROOT, "archive", rev, CSRC, "include"], stdout=subprocess.PIPE)
        untar = subprocess.Popen(["tar", "-C", dst, "-xf", "-"], stdin=tar.stdout)
    if untar.wait() or tar.wait():
        sys.exit("could not unpack %s" % rev)
    return dst


def make_var(csrc, var):
    out = subprocess.check_output(["make", "-s", "-C", csrc, "--eval", "asm-diff-print: ; @echo $(%s)" % var,
                                   "asm-diff-print"], text=True)
    return out.strip().split()


def compile_all(tree):
    """{file.hip: assembly text} of the tree."""
    csrc = os.path.join(tree, CSRC)
    hipcc, flags = make_var(csrc, "HIPCC"), make_var(csrc, "HIPFLAGS")
    jobs = []
    for f in sorted(os.listdir(csrc)):
        if f.endswith(".hip"):
            out = os.path.join(csrc, f[:-4] + ".s")
            jobs.append((f, out, subprocess.Popen(hipcc + flags + ["--cuda-device-only", "-S", f, "-o", out], cwd=csrc)))
    asm = {}
    for f, out, p in jobs:
        if p.wait():
            sys.exit("compiling %s in %s failed" % (f, tree))
        with open(out) as fh:
            asm[f] = fh.read()
    return asm


def normalise(line):
    line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", line)
    line = re.sub(r"(\.L|\b)BB\d+_(\d+)", r"\1BB_\2", line)  # (.LBB<n>_<m> labels and the loop comments naming them)
    line = re.sub(r"\.L(func_begin|func_end|tmp)\d+", r".L\1", line)
    return re.sub(r"\s+;", " ;", line)  # (a comment's column follows the label's length)


def split(text):
    """{symbol: [lines]} of one assembly file.  A function's lines are its
    section from "-- Begin function" to the register summary after "-- End
    function" (body, kernel descriptor, resource comments) and its entry in
    the amdhsa.kernels metadata; every other line goes under "<data>"."""
    parts = {"<data>": []}
    data = parts["<data>"]
    cur, ended, csdata = None, False, False   # the function being read
    entry = None                              # the metadata entry being read
    for raw in text.split("\n"):
        line = normalise(raw.rstrip())
        if entry is not None:
            if line.startswith("    "):
                entry.append(line)
                continue
            m = [re.match(r"    \.name:\s+(\S+)$", x) for x in entry]
            name = [x.group(1) for x in m if x]
            parts.setdefault(name[0] if name else "<data>", []).extend(entry)
            entry = None
        if line.startswith("  - ."):
            entry = [line]
            continue
        m = re.search(r"; -- Begin function (\S+)$", line)
        if m:
            cur, ended, csdata = m.group(1), False, False
            parts[cur] = [data.pop()] if data and data[-1].startswith("\t.section") else []
        elif cur is not None and ended:
            first_csdata = line.startswith("\t.section\t.AMDGPU.csdata") and not csdata
            csdata = csdata or first_csdata
            if not (first_csdata or line.startswith(";") or line.startswith("\t.set " + cur + ".")):
                cur = None
        if cur is None:
            data.append(line)
        else:
            parts[cur].append(line)
            ended = ended or line.strip() == "; -- End function"
    return parts


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    a, b = sys.argv[1], (sys.argv[2] if len(sys.argv) > 2 else "WORKTREE")
    asm_a, asm_b = compile_all(unpack(a)), compile_all(unpack(b))
    print("# device assembly, %s -> %s" % (a, b))
    count = {}
    for f in sorted(set(asm_a) | set(asm_b)):
        pa, pb = split(asm_a.get(f, "")), split(asm_b.get(f, ""))
        for sym in sorted(set(pa) | set(pb)):
            if sym not in pb or (sym != "<data>" and f not in asm_b):
                what = "removed"
            elif sym not in pa or (sym != "<data>" and f not in asm_a):
                what = "added"
            else:
                what = "identical" if pa[sym] == pb[sym] else "differs"
            count[what] = count.get(what, 0) + 1
            print("%-14s %-9s %s" % (f, what, sym))
    print("# " + ", ".join("%d %s" % (n, w) for w, n in sorted(count.items())))


if __name__ == "__main__":
    main()
