#!/usr/bin/env python
"""Share of K5 row-form wave steps that are plain, from the CPU oracle alone.

A wave of k_viterbi_row holds four consecutive traces and steps them together;
a step is plain when every row is idle (past its trace's end), at an
interpolated point, or at a column with candidates that is linked to the
column before.  Counts them for a config's batch (default:
config 2, 10k traces x 100 points) from the oracle's stage arrays; no GPU.
Also counts the linked pairs whose block holds no finite cost (the steps that
leave the fast path from inside) and the chunks of four points whose blocks
exceed the 256-float window.  Prints one JSON line
(profiles/viterbi_plain/README.md).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    from oracle import pyoracle
    from reporter_amd import synth
    cfg = synth.CONFIGS[args.config]
    graph = synth.cached_graph(args.config)
    t = cfg["traces"]
    batch = synth.make_traces(graph, t["n_vehicles"], t["points_per_vehicle"], interval_s=t["interval_s"],
                              noise_sigma_m=t["noise_sigma_m"], accuracy=t["accuracy"], seed=7)
    p = pyoracle.params(**dict(cfg.get("meili", {})))
    orc = pyoracle.match_batch(pyoracle.Graph(graph), batch, p=p, keep_stages=True, nthreads=args.threads)
    off = np.asarray(batch["trace_off"], np.int64)
    T = len(off) - 1
    nc, cp, toff = orc["ncand"], orc["col_prev"], orc["trans_off"]
    is_col = np.asarray(orc["gc"]) > 0
    is_col[off[:-1][np.diff(off) > 0]] = True
    odd = is_col & ~((nc > 0) & (cp >= 0))       # a column that is not a linked one with candidates
    n = np.diff(off)
    steps = plain = 0
    for w0 in range(0, T, 4):
        rows = range(w0, min(w0 + 4, T))
        m = int(max(n[t_] for t_ in rows))
        bad = np.zeros(m, bool)
        for t_ in rows:
            bad[:n[t_]] |= odd[off[t_]:off[t_ + 1]]
        steps += m
        plain += int((~bad).sum())
    trans = orc["trans"]
    dead = 0
    for q in np.nonzero((cp >= 0) & (nc > 0))[0]:
        blk = trans[int(toff[q]):int(toff[q + 1])]
        if len(blk) and not np.isfinite(blk).any():
            dead += 1
    # chunks of four points (from a trace's first) whose blocks exceed the window
    big = chunks = 0
    for t_ in range(T):
        for c0 in range(int(off[t_]), int(off[t_ + 1]), 4):
            c1 = min(c0 + 4, int(off[t_ + 1]))
            chunks += 1
            big += int(toff[c1] - toff[c0] > 256)
    print(json.dumps({"config": args.config, "traces": T, "points": int(off[-1]), "columns": int(is_col.sum()),
                      "wave_steps": steps, "plain_wave_steps": plain, "plain_share": round(plain / steps, 5),
                      "linked_pairs": int(((cp >= 0) & (nc > 0)).sum()), "dead_linked_pairs": dead,
                      "chunks": chunks, "chunks_over_256_floats": big}))


if __name__ == "__main__":
    main()
