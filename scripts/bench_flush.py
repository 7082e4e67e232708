#!/usr/bin/env python
"""The datastore flush on the GPU against the Python path it replaces.

Two shapes:
  config2  the window of one config-2 bench batch (10k vehicles x 100 points)
           on the real config-2 graph: Engine.window_flush and
           Engine.flush_body_device on the matched histogram;
  metro    a metro-scale graph (--metro-km square, engine without an index) with
           a synthetic fill at 0.1 %, 10 % and 100 % of rows nonzero.
Each timed from device buffers to body bytes on the host, after warm runs,
median and range over --repeats; the replaced path (D2H of the slice,
datastore.flush_records, datastore.serialize) on the same buffers in the same
process (--no-python skips it: a profiler run).  call_span_on_stream is the
call between two events on its stream (the second is recorded after the call
returns, so it holds the host's copy of the body too); the kernels alone are
timed by a kernel trace of this script (profiles/flush/kernel_stats.txt).
Bodies are compared once per shape.
Writes one JSON file (--out) and prints it.  Not part of bench.py.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs):
    xs = sorted(xs)
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(xs[0], 4), "max_ms": round(xs[-1], 4),
            "runs": len(xs)}


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return stats(out)


def python_path(h, s, ids, nbins, bin_kph):
    from reporter_amd import datastore
    return datastore.serialize(datastore.flush_records(h.cpu().numpy(), s.cpu().numpy(), ids, 0, 1, nbins, bin_kph))


def device_leg(torch, eng, h, s, ids, nbins, bin_kph, warm, reps, py_reps):
    """flush_body_device on (h, s): wall, device span, and the Python path."""
    side = torch.cuda.Stream()
    spans = []

    def dev():
        with torch.cuda.stream(side):
            a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            body = eng.flush_body_device(h, s, 0, 1, nbins, bin_kph)
            z.record()
        z.synchronize()
        spans.append(a.elapsed_time(z))
        return body
    torch.cuda.synchronize()
    body, nrec = dev()
    wall = timed(dev, warm, reps)
    span = stats(spans[-reps:])
    pys, want = [], None
    for _ in range(py_reps):
        t = time.perf_counter()
        want = python_path(h, s, ids, nbins, bin_kph)
        pys.append((time.perf_counter() - t) * 1e3)
    rows = int(s.numel())
    read_bytes = rows * nbins * 4 + rows * 8
    return {"rows": rows, "nbins": nbins, "records": nrec, "body_bytes": len(body), "bytes_equal": body == want if pys else None,
            "slice_bytes": read_bytes, "flush_body_device": wall, "call_span_on_stream": span,
            "python_path": {"median_ms": round(statistics.median(pys), 3), "min_ms": round(min(pys), 3),
                            "max_ms": round(max(pys), 3), "runs": py_reps} if pys else None,
            "speedup_median": round(statistics.median(pys) / wall["median_ms"], 1) if pys else None,
            }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--metro-km", type=float, default=170.0, help="side of the metro graph (0: skip the metro shape)")
    ap.add_argument("--densities", default="0.001,0.1,1", help="metro fill densities, comma separated")
    ap.add_argument("--no-python", action="store_true", help="skip the replaced Python path (profiler runs)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flush", "bench_flush.json"))
    args = ap.parse_args()
    import torch

    from reporter_amd import Engine, _lib, synth
    res = {"device": torch.cuda.get_device_name(0), "hip_runtime": _lib.runtime_info(), "torch": torch.__version__,
           "library": os.path.relpath(_lib.LIB_PATH, ROOT), "library_bytes": os.path.getsize(_lib.LIB_PATH),
           "repeats": args.repeats, "warm": args.warm, "nbins": 16, "bin_kph": 10.0}
    nbins, bin_kph = 16, 10.0

    # ---- config 2: the window of one bench batch
    graph = synth.cached_graph(2)
    ids = synth.segment_ids(graph)
    t = synth.CONFIGS[2]["traces"]
    batch = synth.make_traces(graph, t["n_vehicles"], t["points_per_vehicle"], interval_s=t["interval_s"],
                              noise_sigma_m=t["noise_sigma_m"], accuracy=t["accuracy"], seed=7)
    with Engine(graph_path=graph) as eng:
        nseg = eng.graph_info()["segments"]
        h = torch.zeros(nseg * nbins, dtype=torch.int32, device="cuda:0")
        s = torch.zeros(nseg, dtype=torch.int64, device="cuda:0")
        eng.hist_bind(h, nbins, bin_kph, speed_sum=s)
        eng.match(batch)
        eng.hist_bind(None, 0, 1.0)
        torch.cuda.synchronize()
        leg = device_leg(torch, eng, h, s, ids, nbins, bin_kph, args.warm, args.repeats, 0 if args.no_python else 5)
        # the engine-owned window: filled by the batch (untimed), closed (timed)
        eng.window_begin(nbins, bin_kph)
        wf, body = [], None
        for k in range(args.warm + args.repeats):
            eng.match(batch)
            t0 = time.perf_counter()
            body, _ = eng.window_flush()
            if k >= args.warm:
                wf.append((time.perf_counter() - t0) * 1e3)
        eng.window_end()
        leg["window_flush"] = stats(wf)
        leg["window_bytes_equal"] = body == python_path(h, s, ids, nbins, bin_kph)
        leg["segments"] = nseg
        res["config2"] = leg
    print(json.dumps({"config2": res["config2"]}), flush=True)

    # ---- metro: synthetic fill at three densities
    if args.metro_km > 0:
        d = tempfile.mkdtemp(prefix="otm_flush_")
        path = os.path.join(d, "metro.otmg")
        synth.make_graph(path, width_m=args.metro_km * 1000.0, height_m=args.metro_km * 1000.0)
        ids = synth.segment_ids(path)
        res["metro"] = {"km": args.metro_km, "segments": len(ids), "densities": {}}
        with Engine(graph_path=path, index_radius_m=0) as eng:
            nseg = len(ids)
            rng = np.random.default_rng(11)
            for dens in [float(x) for x in args.densities.split(",")]:
                py_reps = 0 if args.no_python else (5 if dens < 0.01 else 3)
                rows = np.nonzero(rng.random(nseg) < dens)[0] if dens < 1.0 else np.arange(nseg)
                c = np.zeros((nseg, nbins), np.int32)
                c[rows] = rng.integers(0, 200, size=(len(rows), nbins), dtype=np.int32)
                c[rows, 0] += 1
                sm = np.zeros(nseg, np.int64)
                sm[rows] = rng.integers(1, 2 ** 36, size=len(rows))
                h = torch.from_numpy(c.reshape(-1)).to("cuda:0")
                s = torch.from_numpy(sm).to("cuda:0")
                leg = device_leg(torch, eng, h, s, ids, nbins, bin_kph, args.warm, args.repeats, py_reps)
                res["metro"]["densities"]["%g" % dens] = leg
                print(json.dumps({"metro_%g" % dens: leg}), flush=True)
        os.unlink(path)
        os.rmdir(d)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
