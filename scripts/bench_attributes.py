#!/usr/bin/env python
"""Config 2's batch with and without trace attributes (DESIGN.md §3 rule 7g).

--leg on|off runs the batch (10k vehicles x 100 points on the config-2 graph)
--batches times, one batch at a time, with the attributes' mask (--mask, 15 by
default) or with mask 0, and nothing else.  The `on` leg makes and fetches the
bodies after every batch and times the first call's three parts on the host,
each ended by a wait for the device:
  count_ms   otm_attributes_size: the dense traversals and the shape for the
             bits that need them (a wait each), the count pass, the two scans
             and the copy of the body offsets (the call's own wait), and the
             launch of the write pass
  write_ms   a device synchronisation behind it: what is left of the write pass
  d2h_ms     otm_fetch_attributes: the copy of the blob
and `refetch_ms`, a second fetch (the copy alone).  Under
`rocprofv3 --kernel-trace --stats` the same run gives the kernels' times
(profiles/attributes/README.md).  Prints one JSON line.  Not part of bench.py.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_shape import _ms, config2_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("on", "off"), required=True)
    ap.add_argument("--mask", type=int, default=15)
    ap.add_argument("--batches", type=int, default=12)
    args = ap.parse_args()
    from reporter_amd import Engine, _lib
    graph, batch = config2_batch()
    hip = C.CDLL("libamdhip64.so")
    out = {"leg": args.leg, "mask": args.mask if args.leg == "on" else 0, "batches": args.batches,
           "points": int(len(batch["lat"]))}
    with Engine(graph_path=graph, attributes=args.mask if args.leg == "on" else 0) as eng:
        ms, parts = [], {"count_ms": [], "write_ms": [], "d2h_ms": [], "refetch_ms": []}
        for _ in range(args.batches):
            t, res = _ms(lambda: eng.match(batch))
            ms.append(t)
            if args.leg == "on":
                nt, nb = C.c_int64(), C.c_int64()
                parts["count_ms"].append(
                    _ms(lambda: _lib.lib().otm_attributes_size(eng.h, C.byref(nt), C.byref(nb)))[0])
                parts["write_ms"].append(_ms(hip.hipDeviceSynchronize)[0])
                t, got = _ms(eng.attributes)
                parts["d2h_ms"].append(t)
                parts["refetch_ms"].append(_ms(eng.attributes)[0])
        out["match_ms_median"] = round(float(np.median(ms)), 3)
        out["segments"] = int(len(res.segments))
        if args.leg == "on":
            out.update({k: round(float(np.median(v)), 3) for k, v in parts.items()})
            blob, off = got
            n = len(off) - 1
            out["attributes"] = {"traces": n, "bytes": len(blob), "bytes_per_trace": round(len(blob) / n, 1),
                                 "bytes_per_point": round(len(blob) / len(batch["lat"]), 1),
                                 "max_body": int(np.diff(off).max()), "min_body": int(np.diff(off).min())}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
