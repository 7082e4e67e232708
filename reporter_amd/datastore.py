"""Datastore flush of a rank's reduced speed histograms.

The reference never posts to the datastore: DATASTORE_URL is a TODO
(docker-compose.yml:17, README.md:30,56,94), and the reports it would send
are only returned in each /report response (py/reporter_service.py:160-166,
"datastore" in README.md:135-141).  Authentication is a `secret_key` query
parameter already in the URL (README.md:196-198), so the flush posts to the
URL exactly as configured.

After flush.reduce_histograms, rank r owns segment rows
[r*S_pad/W, (r+1)*S_pad/W).  This module turns that slice into one JSON body
(segments with at least one report: id, count, speed sum and per-bin counts)
and POSTs it.  The body format is this build's own (the datastore's API is
not in the reference); it carries everything the reduced buffers hold.
"""
import json
import os
import urllib.request

import numpy as np


def rank_rows(n_segments_padded, rank, world):
    """The histogram rows rank `rank` owns after the reduce-scatter."""
    per = n_segments_padded // world
    return rank * per, (rank + 1) * per


def flush_records(counts, speed_sums, segment_ids, rank, world, nbins, bin_kph):
    """Records of one rank's slice: counts int [rows * nbins] and speed sums
    int [rows] (1/1000 km/h) as reduce_histograms returned them; segment_ids
    u64 [n_segments] of the graph (synth.segment_ids)."""
    counts = np.asarray(counts, np.int64).reshape(-1, nbins)
    sums = np.asarray(speed_sums, np.int64).reshape(-1)
    r0, _ = rank_rows(counts.shape[0] * world, rank, world)
    out = []
    tot = counts.sum(axis=1)
    for k in np.nonzero(tot > 0)[0]:
        row = r0 + int(k)
        if row >= len(segment_ids):  # padding rows never count
            continue
        out.append({"id": int(segment_ids[row]), "count": int(tot[k]),
                    "speed_sum_kph": int(sums[k]) / 1000.0,
                    "bins": [int(x) for x in counts[k]]})
    return {"mode": "auto", "bin_kph": float(bin_kph), "rank": rank, "world": world, "segments": out}


PAIR_BUCKETS = 4096  # time buckets of one pair window (the key's 12 high bits)
PAIR_STATS = ("reports", "keys", "records", "suppressed_keys", "suppressed_reports", "out_of_range", "dropped")


def pair_records(reports, segment_ids, bucket_s, origin, privacy):
    """The pair window's definition: the reports aggregated per
    (time bucket, segment, next segment).  reports: the structured array
    Results.reports is (id, next_id, t0, t1, length, queue_length, flags);
    segment_ids: synth.segment_ids(graph), the row of an id its index there.
    A report is admitted by the histogram's rule (t1 not the int -1, a speed
    >= 0 in float64, an id with a row); its bucket is k = floor(t0 / bucket_s)
    - origin / bucket_s, and a k outside [0, PAIR_BUCKETS) only counts in
    out_of_range.  Keys with count < privacy stay out of the body.  Returns
    (dict, stats); every aggregate is an integer, so no sum depends on order."""
    bucket_s, origin, privacy = int(bucket_s), int(origin), int(privacy)
    if bucket_s < 1 or privacy < 1 or origin < 0 or origin % bucket_s:
        raise ValueError("bucket_s >= 1, privacy >= 1, origin >= 0 and a multiple of bucket_s")
    ids = np.asarray(segment_ids).astype(np.uint64)
    r = np.asarray(reports)
    t0, t1 = r["t0"].astype(np.float64), r["t1"].astype(np.float64)
    length = r["length"].astype(np.int64)
    # the row of an id (a next_id of -1, or with no row: none)
    order = np.argsort(ids, kind="stable")
    sid = ids[order]

    def rows(v):
        v = v.astype(np.int64).view(np.uint64)
        if not len(sid):
            return np.full(len(v), -1, np.int64)
        at = np.minimum(np.searchsorted(sid, v), len(sid) - 1)
        return np.where(sid[at] == v, order[at], -1).astype(np.int64)
    gi = rows(r["id"])
    gn = np.where(r["next_id"] == -1, -1, rows(r["next_id"]))
    with np.errstate(all="ignore"):
        speed = length / (t1 - t0) * 3.6
        k = np.floor(t0 / np.float64(bucket_s)) - np.float64(origin // bucket_s)
    partial = ((r["flags"] & 1) != 0) & (t1 == -1.0)  # OTM_REP_T1_INT: the -1 of a partial next segment
    admitted = ~partial & (speed >= 0.0) & (gi >= 0)
    inside = admitted & (k >= 0.0) & (k < PAIR_BUCKETS)
    stats = dict.fromkeys(PAIR_STATS, 0)
    stats["out_of_range"] = int((admitted & ~inside).sum())
    stats["reports"] = int(inside.sum())
    t0, t1, length, gi, gn = t0[inside], t1[inside], length[inside], gi[inside], gn[inside]
    queue = r["queue_length"][inside].astype(np.int64)
    # the key as the table holds it: one word whose integer order is the body's
    key = ((k[inside].astype(np.int64) << 52) | (gi << 26) | (gn + 1)).view(np.uint64)
    uk, first, inv = np.unique(key, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    count = np.bincount(inv, minlength=len(uk))
    dur, qsum = np.zeros(len(uk), np.int64), np.zeros(len(uk), np.int64)
    np.add.at(dur, inv, ((t1 - t0) * 1000.0 + 0.5).astype(np.int64))  # (truncates as int() does)
    np.add.at(qsum, inv, queue)
    t_min = np.full(len(uk), np.iinfo(np.int64).max)
    t_max = np.full(len(uk), np.iinfo(np.int64).min)
    np.minimum.at(t_min, inv, np.floor(t0).astype(np.int64))
    np.maximum.at(t_max, inv, np.floor(t1).astype(np.int64))
    out = []
    for j in range(len(uk)):
        if count[j] < privacy:
            stats["suppressed_keys"] += 1
            stats["suppressed_reports"] += int(count[j])
            continue
        i = first[j]
        rec = {"id": int(ids[gi[i]])}
        if gn[i] >= 0:
            rec["next_id"] = int(ids[gn[i]])
        rec.update({"bucket": origin + (int(uk[j]) >> 52) * bucket_s, "count": int(count[j]),
                    "duration_ms": int(dur[j]), "length": int(length[i]), "queue_length": int(qsum[j]),
                    "t_min": int(t_min[j]), "t_max": int(t_max[j])})
        out.append(rec)
    stats["keys"] = len(uk)
    stats["records"] = len(out)
    return {"mode": "auto", "bucket_s": bucket_s, "origin": origin, "privacy": privacy, "pairs": out}, stats


def serialize(records):
    """Compact JSON, as reporter_service.py writes its bodies (:215)."""
    return json.dumps(records, separators=(",", ":")).encode("utf-8")


def flush_body_host(counts, speed_sums, segment_ids, rank, world, nbins, bin_kph):
    """serialize(flush_records(...)) written by libotmatch's host writer
    (otm_flush_body_host): counts [rows * nbins] read as u32, speed sums [rows]
    as u64, segment_ids u64 [n_segments].  Returns (bytes, n_records)."""
    import ctypes as C

    from . import _lib
    from .engine import _check
    c = np.ascontiguousarray(np.asarray(counts).reshape(-1))
    c = c if c.dtype == np.uint32 else c.astype(np.int64).astype(np.uint32)
    s = np.ascontiguousarray(np.asarray(speed_sums).reshape(-1))
    s = s if s.dtype == np.uint64 else s.astype(np.int64).astype(np.uint64)
    ids = np.ascontiguousarray(np.asarray(segment_ids, np.uint64))
    out, n, nrec = C.c_void_p(), C.c_size_t(), C.c_int64()
    _check(_lib.lib().otm_flush_body_host(c.ctypes.data, s.ctypes.data, ids.ctypes.data, len(ids), len(s), nbins,
                                          bin_kph, rank, world, C.byref(out), C.byref(n), C.byref(nrec)))
    return _lib.take(out, n.value), nrec.value


def flush_body(engine, part, spart, rank, world, nbins, bin_kph, segment_ids=None):
    """The flush body of a rank's slice (part, spart as reduce_histograms
    returned them): written on the GPU when the tensors are there
    (Engine.flush_body_device, with the engine's own copy of the ids), by the
    host writer otherwise (a gloo run: segment_ids = synth.segment_ids(graph),
    engine unused).  Returns (bytes, n_records)."""
    if getattr(part, "is_cuda", False):
        return engine.flush_body_device(part, spart, rank, world, nbins, bin_kph)
    if segment_ids is None:
        raise ValueError("host tensors need segment_ids (synth.segment_ids of the graph)")
    to_np = lambda t: t.numpy() if hasattr(t, "numpy") else np.asarray(t)
    return flush_body_host(to_np(part), to_np(spart), segment_ids, rank, world, nbins, bin_kph)


def post(body, url=None, timeout=10.0):
    """POST a flush body to the datastore (url or env DATASTORE_URL, its
    secret_key query parameter included).  Returns the HTTP status; raises on
    transport errors.  No URL configured: nothing is sent (returns None), as
    in the reference."""
    url = url or os.environ.get("DATASTORE_URL")
    if not url:
        return None
    req = urllib.request.Request(url, data=body, method="POST",
                                 headers={"Content-type": "application/json;charset=utf-8"})
    with urllib.request.urlopen(req, timeout=timeout) as r:
        return r.status
