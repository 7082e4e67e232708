#!/usr/bin/env python
"""Config 2's batch with and without match scores (DESIGN.md §3 rule 7e).

--leg on|off runs the batch (10k vehicles x 100 points on the config-2 graph)
--batches times, one batch at a time, with the switch on or off and nothing
else: the runs of a kernel trace that give k_scores' time beside k_viterbi_row's
(profiles/scores/kernels.json).  --form 1|4 forces a form of the score pass
(OTM_SCORE_FORM); K5 runs its row form either way (the form of this batch
size), so the yardstick is the same kernel in every run.  The `on`
leg also fetches the records once and prints what they hold, and the HBM the
switch adds.  Prints one JSON line.  Not part of bench.py.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_points import config2_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("on", "off"), required=True)
    ap.add_argument("--form", type=int, choices=(0, 1, 4), default=0, help="0: by batch size")
    ap.add_argument("--batches", type=int, default=12)
    args = ap.parse_args()
    if args.form:
        os.environ["OTM_SCORE_FORM"] = str(args.form)
    from reporter_amd import Engine, _lib
    graph, batch = config2_batch()
    n = int(len(batch["lat"]))
    out = {"leg": args.leg, "form": args.form, "batches": args.batches, "points": n}
    with Engine(graph_path=graph, scores=args.leg == "on") as eng:
        ms = []
        for _ in range(args.batches):
            t = time.perf_counter()
            res = eng.match(batch)
            ms.append((time.perf_counter() - t) * 1e3)
        out["match_ms_median"] = round(float(np.median(ms)), 3)
        out["segments"] = int(len(res.segments))
        if args.leg == "on":
            t = time.perf_counter()
            rec = eng.scores()
            out["fetch_ms"] = round((time.perf_counter() - t) * 1e3, 3)
            f = rec["flags"]
            out["records"] = {k: int(((f & b) != 0).sum()) for k, b in (
                ("scored", _lib.SC_SCORED), ("chain_start", _lib.SC_CHAIN_START), ("chain_end", _lib.SC_CHAIN_END),
                ("alone", _lib.SC_ALONE), ("tie", _lib.SC_TIE))}
            m = rec["margin"][((f & _lib.SC_SCORED) != 0) & np.isfinite(rec["margin"])]
            out["margin"] = {"median": round(float(np.median(m)), 3), "p10": round(float(np.percentile(m, 10)), 3),
                             "p1": round(float(np.percentile(m, 1)), 4)}
            # what the switch adds in HBM: the records, alpha in the candidates' layout, the packed form's list
            # (computed from engine.cpp bind_scores' element counts, not read from the device)
            kmax = _lib.lib().otm_kmax()
            out["hbm_bytes_per_point"] = {"records": 32, "alpha": 4 * kmax,
                                          "list_per_trace": 4, "total": 32 + 4 * kmax}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
