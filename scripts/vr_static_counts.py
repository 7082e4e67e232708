"""Static instruction counts of k_viterbi_row from a gfx950 assembly listing.

  hipcc <the Makefile's HIPFLAGS> -S --cuda-device-only -o kernels.s kernels.hip
  python scripts/vr_static_counts.py kernels.s

Prints the kernel's size and register use, some opcode totals, and the
instructions by class of the parts of the chunk loop, cut at what the listing
shows: a build with the plain-step fast path lays a step out as its fast body,
closed by an s_branch over the general body to the step's end, then the
general body; a build without it has one body per step.  The chunk prologue
is what stands between the loop's header and the first step.  Counts are of
the listing's lines in those ranges (blocks the compiler moved out of line,
behind the loop, are not in them).  A record for
profiles/viterbi_plain/README.md, not a test.
"""
import re
import sys


def kernel_lines(path, name="k_viterbi_row"):
    out, inside, tail = [], False, []
    for ln in open(path):
        if not inside:
            if re.match(r"^_Z\w*\d+%s[A-Z]\w*:" % name, ln):
                inside = True
            continue
        if tail or ln.startswith(".Lfunc_end"):
            tail.append(ln.rstrip("\n"))
            if "Occupancy" in ln:
                break
            continue
        out.append(ln.rstrip("\n"))
    return out, tail


def cls(op):
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    if op.startswith("s_"):
        return "SALU"
    return "other"


def count(seg):
    c = {"VALU": 0, "SALU": 0, "LDS": 0, "VMEM": 0}
    for i in seg:
        c[cls(i.split()[0])] = c.get(cls(i.split()[0]), 0) + 1
    c["all"] = len(seg)
    for key in ("s_and_saveexec_b64", "s_cbranch_execz", "s_waitcnt", "s_nop", "v_add_f32_dpp", "v_pk_add_f32",
                "v_mov_b32_dpp", "ds_read_b32", "ds_bpermute_b32"):
        c[key] = sum(1 for i in seg if i.split()[0] == key)
    return c


def main():
    lines, tail = kernel_lines(sys.argv[1])
    ins, labels = [], {}
    for ln in lines:
        s = ln.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        if not s or s.startswith((";", ".", "/")) or s.endswith(":"):
            continue
        ins.append(s.split(";")[0].strip())
    print("whole kernel:", count(ins))
    for ln in tail:
        if re.search(r"; (codeLenInByte|NumVgprs|ScratchSize|Occupancy)", ln):
            print(" ", ln.strip("; ").strip())
    rec = [k for k, i in enumerate(ins) if i.startswith(("v_add_f32_dpp", "v_mov_b32_dpp")) and "row_newbcast:0 " in i]
    if len(rec) == 4:
        # one body per step: a step runs from recurrence to recurrence
        for k in range(1, 3):
            print("step %d (one body), first sum to the next step's: %s" % (k, count(ins[rec[k]:rec[k + 1]])))
        return
    assert len(rec) == 8, "expected four steps with one or two recurrences each, found %d" % len(rec)
    ends = []  # per step: (the fast body's closing branch, the step's end)
    for k in range(4):
        br = next(p for p in range(rec[2 * k], len(ins)) if ins[p].startswith("s_branch"))
        ends.append((br, labels[ins[br].split()[1]]))
    # the loop's header: the last 16-byte window store's block start before the first recurrence
    w128 = [p for p in range(rec[0]) if ins[p].startswith("ds_write_b128")]
    print("chunk prologue (first window store to step 0's first sum, less step 0's head): see the listing; "
          "window stores %d, to the first sum %d instructions" % (len(w128), rec[0] - w128[0] if w128 else -1))
    for k in range(1, 4):
        start = ends[k - 1][1]
        br, end = ends[k]
        print("step %d fast body    %s" % (k, count(ins[start:br + 1])))
        print("step %d general body %s" % (k, count(ins[br + 1:end])))


if __name__ == "__main__":
    main()
