"""Engine: one MI355X, its HBM-resident road graph, the /report hot path.

Python face of libotmatch.so's C ABI (include/otmatch.h).  Mirrors the
reference's matcher interface (py/reporter_service.py): Engine.report(body)
answers like SegmentMatcherHandler.handle_request (:218-240) and
Engine.match_json(body) like valhalla.SegmentMatcher().Match (:112); the
binary entry points (match, match_device) are the benchmark path.
"""
import ctypes as C
import json
import os
import tempfile

import numpy as np

from . import _lib
from ._lib import lib, take


class OtmError(RuntimeError):
    pass


def _check(rc):
    if rc != _lib.OTM_OK:
        raise OtmError("libotmatch error %d: %s" % (rc, _lib.last_error()))


def write_config(path, graph_path, index_radius_m=None, grid_mult=None, trans_lanes=None, index_near_m=None,
                 queue_speed_kph=None, **meili):
    """Write an engine config: {"otm":{"graph":...,"index_radius_m":R},"meili":{"default":{...}}}.
    index_near_m: the near indexes' radii (a list; [] for none; default a
    fraction of the index radius, engine.cpp build_index).
    queue_speed_kph: the queue threshold (DESIGN.md §3 rule 7b; None or 0: off)."""
    otm = {"graph": os.path.abspath(graph_path)}
    if index_radius_m is not None:
        otm["index_radius_m"] = index_radius_m
    if index_near_m is not None:
        otm["index_near_m"] = list(index_near_m)
    if grid_mult is not None:
        otm["grid_mult"] = grid_mult
    if trans_lanes is not None:
        otm["trans_lanes"] = trans_lanes
    if queue_speed_kph is not None:
        otm["queue_speed_kph"] = queue_speed_kph
    cfg = {"otm": otm, "meili": {"default": meili}}
    with open(path, "w") as f:
        json.dump(cfg, f)
    return path


def compact_batch(batch):
    """A batch narrowed to otm_batch_compact (the Java host's Point types):
    int64 time base per trace (its first time), int32 time deltas, int16
    accuracies.  Raises ValueError when a time is not a whole number of
    seconds, a delta leaves int32 or an accuracy leaves int16 (such a batch
    goes through Engine.match)."""
    off = np.ascontiguousarray(batch["trace_off"], dtype=np.int64)
    tm = np.asarray(batch["time"], dtype=np.float64)
    acc = np.asarray(batch["accuracy"], dtype=np.float32)
    ti = tm.astype(np.int64)
    if not np.array_equal(ti.astype(np.float64), tm):
        raise ValueError("compact batches carry whole-second times")
    ia = acc.astype(np.int64)
    if not np.array_equal(ia.astype(np.float32), acc) or (len(ia) and (ia.min() < -32768 or ia.max() > 32767)):
        raise ValueError("compact batches carry int16 accuracies")
    nt = len(off) - 1
    lens = np.diff(off)
    base = np.zeros(nt, dtype=np.int64)
    nz = lens > 0
    base[nz] = ti[off[:-1][nz]]
    delta = ti - np.repeat(base, lens)
    if len(delta) and (delta.min() < -2**31 or delta.max() >= 2**31):
        raise ValueError("a trace's times span more than int32 seconds")
    return {"trace_off": off, "time_base": base,
            "lat": np.ascontiguousarray(batch["lat"], dtype=np.float32),
            "lon": np.ascontiguousarray(batch["lon"], dtype=np.float32),
            "time_delta": delta.astype(np.int32), "accuracy": ia.astype(np.int16)}


class RequestArena(object):
    """Request bodies written back to back into library-owned page-locked
    memory (otm_request_arena_alloc), as the Java host writes its
    body.getBytes(ISO_8859_1) into a MemorySegment over the arena; pass it to
    Engine.report_batch / submit_batch in place of the bodies."""

    def __init__(self, bodies):
        bs = [b.encode("utf-8") if isinstance(b, str) else b for b in bodies]
        self.n = len(bs)
        total = sum(len(b) for b in bs)
        self.base = lib().otm_request_arena_alloc(max(total, 1))
        if not self.base:
            raise OtmError("otm_request_arena_alloc: %s" % _lib.last_error())
        blob = b"".join(bs)
        C.memmove(self.base, blob, len(blob))
        offs = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum([len(b) for b in bs], out=offs[1:])
        self.ptrs = (C.c_void_p * self.n)(*[self.base + int(o) for o in offs[:-1]])
        self.ptrs = C.cast(self.ptrs, C.POINTER(C.c_char_p))
        self.lens = (C.c_size_t * self.n)(*[len(b) for b in bs])
        self.bytes = total

    def release(self):
        if self.base:
            _check(lib().otm_request_arena_release(self.base))
            self.base = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.release()


class Results(object):
    """Host copy of one batch's results (numpy structured arrays)."""

    def __init__(self, r):
        self.traces = _lib.as_array(r.traces, _lib.TRACE_DTYPE, r.n_traces)
        self.segments = _lib.as_array(r.segments, _lib.SEGMENT_DTYPE, r.n_segments)
        self.reports = _lib.as_array(r.reports, _lib.REPORT_DTYPE, r.n_reports)
        self.way_ids = _lib.as_array(r.way_ids, np.int64, r.n_way_ids)


class Engine(object):
    def __init__(self, config_path=None, graph_path=None, device=0, index_radius_m=None, grid_mult=None,
                 trans_lanes=None, devices=None, index_near_m=None, queue_speed_kph=None, matched_points=False,
                 traversals=False, scores=False, shape=False, attributes=0, **meili):
        """Either a config file (valhalla.Configure-style) or a graph path.
        devices=[d0, d1, ...] makes a multi-device engine (otm_engine_create
        with ndev > 1): traces go to member murmur2(uuid) % ndev.
        matched_points: the per-point records of DESIGN.md §3 rule 7c
        (set_points / points; off: nothing changes).
        traversals: the per-edge records of rule 7d (set_traversals /
        traversals; off: nothing changes).
        scores: the per-point match scores of rule 7e (set_scores / scores;
        off: nothing changes).
        shape: the matched route's geometry of rule 7f (set_shape / shape;
        off: nothing changes).
        attributes: the section mask of rule 7g's per-trace JSON bodies
        (_lib.ATTR_*; True: every section; 0 or False: off, nothing changes)."""
        L = lib()
        self._tmp = None
        if config_path is None:
            if graph_path is None:
                raise ValueError("config_path or graph_path required")
            fd, self._tmp = tempfile.mkstemp(suffix=".json", prefix="otm_cfg_")
            os.close(fd)
            config_path = write_config(self._tmp, graph_path, index_radius_m=index_radius_m, grid_mult=grid_mult,
                                       trans_lanes=trans_lanes, index_near_m=index_near_m,
                                       queue_speed_kph=queue_speed_kph, **meili)
        h = C.c_void_p()
        devs = list(devices) if devices is not None else [device]
        dev = (C.c_int * len(devs))(*devs)
        rc = L.otm_engine_create(config_path.encode(), dev, len(devs), C.byref(h))
        if rc != _lib.OTM_OK:
            raise OtmError("otm_engine_create failed (%d): %s" % (rc, _lib.last_error()))
        self.h = h
        self.device = devs[0]
        self.devices = devs
        if matched_points:
            self.set_points(True)
        if traversals:
            self.set_traversals(True)
        if scores:
            self.set_scores(True)
        if shape:
            self.set_shape(True)
        if attributes:
            self.set_attributes(attributes)

    def members(self):
        """Member count: ndev of a multi-device engine, else 1."""
        return lib().otm_engine_members(self.h)

    def member(self, i):
        """Member i of a multi-device engine as an Engine view (owned by self:
        do not close it; it lives as long as self)."""
        h = lib().otm_engine_member(self.h, i)
        if not h:
            raise OtmError("no member %d" % i)
        e = Engine.__new__(Engine)
        e._tmp = None
        e.h = C.c_void_p(h)
        e.device = self.devices[i] if len(self.devices) > 1 else self.device
        e.parent = self
        e._view = True
        return e

    def clone(self):
        """A second batch context on this GPU sharing the graph and index
        (otm_engine_clone): its own stream and buffers, so batches on the two
        run concurrently from different host threads.  Close it before self."""
        h = C.c_void_p()
        rc = lib().otm_engine_clone(self.h, C.byref(h))
        if rc != _lib.OTM_OK:
            raise OtmError("otm_engine_clone failed (%d): %s" % (rc, _lib.last_error()))
        e = Engine.__new__(Engine)
        e._tmp = None
        e.h = h
        e.device = self.device
        e.parent = self
        return e

    def close(self):
        if getattr(self, "_view", False):
            self.h = None  # a member view: its group owns it
        if getattr(self, "h", None):
            lib().otm_engine_destroy(self.h)
            self.h = None
        if getattr(self, "_tmp", None):
            try:
                os.unlink(self._tmp)
            except OSError:
                pass
            self._tmp = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ------------------------------------------------------------ request level
    def report(self, body):
        """-> (http_code, body_str), exactly as reporter_service.py answers /report."""
        b = body.encode("utf-8") if isinstance(body, str) else body
        out = C.c_void_p()
        n = C.c_size_t()
        code = lib().otm_report(self.h, b, len(b), C.byref(out), C.byref(n))
        return code, take(out, n.value).decode("utf-8")

    def report_batch(self, bodies):
        """otm_report_batch over request bodies (bytes / str), or over a
        RequestArena's bodies (sent to HBM straight from the arena)."""
        if isinstance(bodies, RequestArena):
            n, arr, lens = bodies.n, bodies.ptrs, bodies.lens
        else:
            bs = [b.encode("utf-8") if isinstance(b, str) else b for b in bodies]
            n = len(bs)
            arr = (C.c_char_p * n)(*bs)
            lens = (C.c_size_t * n)(*[len(b) for b in bs])
        outs = (C.c_void_p * n)()
        olens = (C.c_size_t * n)()
        codes = (C.c_int * n)()
        _check(lib().otm_report_batch(self.h, n, arr, lens, outs, olens, codes))
        return [(codes[i], take(outs[i], olens[i]).decode("utf-8")) for i in range(n)]

    def match_json(self, body):
        b = body.encode("utf-8") if isinstance(body, str) else body
        out = C.c_void_p()
        n = C.c_size_t()
        code = lib().otm_match_json(self.h, b, len(b), C.byref(out), C.byref(n))
        return code, take(out, n.value).decode("utf-8")

    def report_segments(self, body, match_output):
        return report_segments(body, match_output, self)

    def report_segments_device(self, pairs):
        """report() on the GPU (k_report) over [(request body, Match output)]
        -> [(code, body)]; code 0 where a Match output does not fit the typed
        records (otm_report_segments_device)."""
        enc = lambda x: x.encode("utf-8") if isinstance(x, str) else x  # noqa: E731
        rq = [enc(a) for a, _ in pairs]
        mo = [enc(b) for _, b in pairs]
        n = len(pairs)
        outs = (C.c_void_p * n)()
        olens = (C.c_size_t * n)()
        codes = (C.c_int * n)()
        _check(lib().otm_report_segments_device(self.h, n, (C.c_char_p * n)(*rq), (C.c_size_t * n)(*map(len, rq)),
                                                (C.c_char_p * n)(*mo), (C.c_size_t * n)(*map(len, mo)), outs, olens,
                                                codes))
        return [(codes[i], take(outs[i], olens[i]).decode("utf-8")) for i in range(n)]

    def submit(self, body, tag):
        b = body.encode("utf-8") if isinstance(body, str) else body
        _check(lib().otm_submit(self.h, b, len(b), tag))

    def submit_batch(self, bodies, tags):
        """otm_submit_batch: many requests in one call (in order); a
        RequestArena's bodies are referenced, not copied."""
        if isinstance(bodies, RequestArena):
            n, arr, lens = bodies.n, bodies.ptrs, bodies.lens
        else:
            bs = [b.encode("utf-8") if isinstance(b, str) else b for b in bodies]
            n = len(bs)
            arr = (C.c_char_p * n)(*bs)
            lens = (C.c_size_t * n)(*[len(b) for b in bs])
        tg = (C.c_uint64 * n)(*tags)
        _check(lib().otm_submit_batch(self.h, n, arr, lens, tg))

    def poll(self, max_results=1024, timeout_us=0):
        res = (_lib.Result * max_results)()
        n = lib().otm_poll(self.h, res, max_results, timeout_us)
        if n < 0:
            _check(n)
        return [(res[i].tag, res[i].code, take(res[i].body, res[i].body_len).decode("utf-8")) for i in range(n)]

    # ------------------------------------------------------------ binary level
    def match(self, batch):
        """Host batch (dict of numpy arrays) -> Results."""
        off = np.ascontiguousarray(batch["trace_off"], dtype=np.int64)
        lat = np.ascontiguousarray(batch["lat"], dtype=np.float32)
        lon = np.ascontiguousarray(batch["lon"], dtype=np.float32)
        tm = np.ascontiguousarray(batch["time"], dtype=np.float64)
        acc = np.ascontiguousarray(batch["accuracy"], dtype=np.float32)
        b = _lib.Batch(len(off) - 1, int(off[-1]), off.ctypes.data, lat.ctypes.data, lon.ctypes.data,
                       tm.ctypes.data, acc.ctypes.data)
        r = _lib.Results()
        _check(lib().otm_match_soa(self.h, C.byref(b), C.byref(r)))
        return Results(r)

    def match_compact(self, batch):
        """Host batch -> Results through otm_match_compact: the batch narrowed
        to the Java host's own integers (compact_batch), 14 B per point over
        the link, widened on the device."""
        cb = compact_batch(batch)
        b = _lib.BatchCompact(len(cb["trace_off"]) - 1, int(cb["trace_off"][-1]), cb["trace_off"].ctypes.data,
                              cb["time_base"].ctypes.data, cb["lat"].ctypes.data, cb["lon"].ctypes.data,
                              cb["time_delta"].ctypes.data, cb["accuracy"].ctypes.data)
        r = _lib.Results()
        _check(lib().otm_match_compact(self.h, C.byref(b), C.byref(r)))
        return Results(r)

    def match_device(self, trace_off, lat, lon, time, accuracy, stream=None):
        """Device batch: torch tensors already in this GPU's HBM.  Results
        stay on the device; call fetch() for a host copy."""
        n_traces = trace_off.numel() - 1
        b = _lib.Batch(n_traces, int(lat.numel()), trace_off.data_ptr(), lat.data_ptr(), lon.data_ptr(),
                       time.data_ptr(), accuracy.data_ptr())
        _check(lib().otm_match_device(self.h, C.byref(b), C.c_void_p(stream) if stream else None))

    def fetch(self):
        r = _lib.Results()
        _check(lib().otm_fetch_results(self.h, C.byref(r)))
        return Results(r)

    def hist_bind(self, tensor, nbins, bin_kph, speed_sum=None):
        """Per-segment speed histogram (u32 counts [n_segments * nbins]) and,
        optionally, the per-segment speed sums (int64 [n_segments], 1/1000
        km/h), both caller-owned device tensors (otm_hist_bind_ex)."""
        ptr = None if tensor is None else tensor.data_ptr()
        sp = None if speed_sum is None or tensor is None else speed_sum.data_ptr()
        _check(lib().otm_hist_bind_ex(self.h, ptr, nbins, bin_kph, sp))

    def window_begin(self, nbins, bin_kph):
        """Open an engine-owned histogram window (otm_window_begin): counts
        and speed sums in library-owned HBM, bound as hist_bind binds."""
        _check(lib().otm_window_begin(self.h, nbins, bin_kph))

    def window_flush(self):
        """Close the window: (the datastore flush body as bytes, its record
        count); the buffers are zeroed and the window goes on.  No match call
        may be in progress on this engine, its clones or its members."""
        out, n, nrec = C.c_void_p(), C.c_size_t(), C.c_int64()
        _check(lib().otm_window_flush(self.h, C.byref(out), C.byref(n), C.byref(nrec)))
        return _lib.take(out, n.value), nrec.value

    def window_end(self):
        _check(lib().otm_window_end(self.h))

    def pairs_begin(self, bucket_s, origin=0, privacy=1, max_keys=0):
        """Open a pair window (otm_pairs_begin): the reports aggregated per
        (time bucket, segment, next segment) in a hash table in HBM, as
        datastore.pair_records defines.  max_keys 0: max(65536, 8 x segments)."""
        cfg = _lib.PairsCfg(bucket_s, privacy, origin, max_keys)
        _check(lib().otm_pairs_begin(self.h, C.byref(cfg)))

    def pairs_add_reports(self, reports):
        """Host report records (a _lib.REPORT_DTYPE array, e.g. Results.reports
        of another matcher or a replay) into the open pair window."""
        r = np.ascontiguousarray(reports, dtype=_lib.REPORT_DTYPE)
        _check(lib().otm_pairs_add_reports(self.h, len(r), r.ctypes.data if len(r) else None))

    def pairs_flush(self):
        """(the pair window's body as bytes, its stats as a dict); the table is
        cleared and the window goes on.  No match call may be in progress on
        this engine, its clones or its members."""
        out, n, st = C.c_void_p(), C.c_size_t(), _lib.PairsStats()
        _check(lib().otm_pairs_flush(self.h, C.byref(out), C.byref(n), C.byref(st)))
        return _lib.take(out, n.value), {k: getattr(st, k) for k in _lib.PAIRS_STATS}

    def pairs_end(self):
        _check(lib().otm_pairs_end(self.h))

    def pairs_info(self):
        """The open pair window: (bucket_s, origin, privacy, max_keys resolved, slots of one table)."""
        cfg, slots = _lib.PairsCfg(), C.c_int64()
        _check(lib().otm_pairs_info(self.h, C.byref(cfg), C.byref(slots)))
        return {"bucket_s": cfg.bucket_s, "origin": cfg.origin, "privacy": cfg.privacy, "max_keys": cfg.max_keys,
                "slots": slots.value}

    def flush_body_device(self, counts, sums, rank, world, nbins, bin_kph):
        """The flush body of a histogram slice in this GPU's HBM, written on
        the GPU (otm_flush_body_device): counts int32 / uint32 tensor
        [rows * nbins], sums int64 tensor [rows] (flush.reduce_histograms'
        slices, or a whole window with world 1).  Returns (bytes, n_records)."""
        import torch
        rows = int(sums.numel())
        if counts.element_size() != 4 or sums.element_size() != 8 or not counts.is_contiguous() \
                or not sums.is_contiguous() or (nbins >= 1 and counts.numel() != rows * nbins):
            raise ValueError("counts: 4-byte [rows * nbins], sums: 8-byte [rows], both contiguous")
        # the tensors are ready on torch's current stream; the null stream has
        # no handle to pass, so wait for it here
        st = torch.cuda.current_stream(counts.device)
        if not st.cuda_stream:
            st.synchronize()
        out, n, nrec = C.c_void_p(), C.c_size_t(), C.c_int64()
        _check(lib().otm_flush_body_device(self.h, counts.data_ptr(), sums.data_ptr(), rows, nbins, bin_kph, rank, world,
                                           C.c_void_p(st.cuda_stream) if st.cuda_stream else None, C.byref(out),
                                           C.byref(n), C.byref(nrec)))
        return _lib.take(out, n.value), nrec.value

    def graph_info(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        _check(lib().otm_graph_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"nodes": a.value, "edges": b.value, "segments": c.value}

    def index_info(self):
        r, e, i, ms = C.c_float(), C.c_int64(), C.c_int32(), C.c_float()
        _check(lib().otm_index_info(self.h, C.byref(r), C.byref(e), C.byref(i), C.byref(ms)))
        return {"radius_m": r.value, "entries": e.value, "incomplete_rows": i.value, "build_ms": ms.value}

    def index_levels(self):
        """The near indexes: [{"radius_m": r, "entries": n}, ...], smallest radius first."""
        r = (C.c_float * 8)()
        e = (C.c_int64 * 8)()
        n = lib().otm_index_levels(self.h, r, e, 8)
        if n < 0:
            raise OtmError("otm_index_levels failed: %s" % _lib.last_error())
        return [{"radius_m": r[i], "entries": e[i]} for i in range(min(n, 8))]

    def index_tables(self):
        """The route index's device tables (full + near): {"slots", "bytes",
        "load_pct"} (otm_index_tables)."""
        n, b, p = C.c_int64(), C.c_int64(), C.c_int32()
        _check(lib().otm_index_tables(self.h, C.byref(n), C.byref(b), C.byref(p)))
        return {"slots": n.value, "bytes": b.value, "load_pct": p.value}

    def grid_info(self):
        cd, r, c, n, m = C.c_double(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
        _check(lib().otm_grid_info(self.h, C.byref(cd), C.byref(r), C.byref(c), C.byref(n), C.byref(m)))
        return {"cell_deg": cd.value, "rows": r.value, "cols": c.value, "entries": n.value, "mult": m.value}

    def queue_info(self):
        """The queue threshold in km/h (otm_queue_info; 0.0: off)."""
        k = C.c_float()
        _check(lib().otm_queue_info(self.h, C.byref(k)))
        return k.value

    # The optional per-batch outputs (matched points, matched route, match
    # scores, matched shape): one switch, one info call, one fetch and one device call each,
    # the same but for the C function's name and the record's dtype.
    def _set_switch(self, fn, on):
        _check(getattr(lib(), fn)(self.h, 1 if on else 0))

    def _switch_info(self, fn):
        on = C.c_int()
        _check(getattr(lib(), fn)(self.h, C.byref(on)))
        return bool(on.value)

    def _fetch_per_point(self, fn, dtype):
        fetch, n = getattr(lib(), fn), C.c_int64()
        _check(fetch(self.h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=dtype)
        _check(fetch(self.h, out.ctypes.data if n.value else None, n.value, C.byref(n)))
        return out

    def _records_device(self, fn, pointers=1):
        ptrs, n = [C.c_void_p() for _ in range(pointers)], C.c_int64()
        _check(getattr(lib(), fn)(self.h, *[C.byref(p) for p in ptrs], C.byref(n)))
        return tuple(p.value or 0 for p in ptrs) + (n.value,)

    def set_points(self, on):
        """The matched-points switch of this handle (otm_set_points; a multi-device
        engine passes it to every member, a clone inherits it when it is made)."""
        self._set_switch("otm_set_points", on)

    def points_info(self):
        """Whether matched points are on (otm_points_info)."""
        return self._switch_info("otm_points_info")

    def points(self):
        """The last binary-level batch's matched points (otm_fetch_points): one
        _lib.POINT_DTYPE record per input point, in input order."""
        return self._fetch_per_point("otm_fetch_points", _lib.POINT_DTYPE)

    def points_device(self):
        """(device pointer, count) of the last batch's records in this GPU's HBM
        (otm_points_device; a one-device engine's, valid until its next batch)."""
        return self._records_device("otm_points_device")

    def set_traversals(self, on):
        """The matched-route switch of this handle (otm_set_traversals; a multi-device
        engine passes it to every member, a clone inherits it when it is made)."""
        self._set_switch("otm_set_traversals", on)

    def traversals_info(self):
        """Whether the matched route is on (otm_traversals_info)."""
        return self._switch_info("otm_traversals_info")

    def traversals(self):
        """The matched route of the handle's last binary-level batch
        (otm_traversals_size, otm_fetch_traversals): (records, trav_off) --
        _lib.TRAVERSAL_DTYPE records, dense and in trace order, trace t's at
        [trav_off[t], trav_off[t + 1]).  Both arrays are sized by the library's
        own counts (a member view: its share of the group's batch)."""
        nt, n = C.c_int64(), C.c_int64()
        _check(lib().otm_traversals_size(self.h, C.byref(nt), C.byref(n)))
        off = np.zeros(nt.value + 1, dtype=np.int64)
        out = np.zeros(n.value, dtype=_lib.TRAVERSAL_DTYPE)
        _check(lib().otm_fetch_traversals(self.h, out.ctypes.data if n.value else None, n.value, off.ctypes.data,
                                          C.byref(n)))
        return out, off

    def traversals_device(self):
        """(records pointer, trav_off pointer, count) of the last batch's dense
        records in this GPU's HBM (otm_traversals_device; a one-device engine's,
        valid until its next batch)."""
        return self._records_device("otm_traversals_device", pointers=2)

    def set_scores(self, on):
        """The match-scores switch of this handle (otm_set_scores; a multi-device
        engine passes it to every member, a clone inherits it when it is made)."""
        self._set_switch("otm_set_scores", on)

    def scores_info(self):
        """Whether match scores are on (otm_scores_info)."""
        return self._switch_info("otm_scores_info")

    def scores(self):
        """The last binary-level batch's match scores (otm_fetch_scores): one
        _lib.SCORE_DTYPE record per input point, in input order."""
        return self._fetch_per_point("otm_fetch_scores", _lib.SCORE_DTYPE)

    def scores_device(self):
        """(device pointer, count) of the last batch's records in this GPU's HBM
        (otm_scores_device; a one-device engine's, valid until its next batch)."""
        return self._records_device("otm_scores_device")

    def set_shape(self, on):
        """The matched-shape switch of this handle (otm_set_shape; a multi-device
        engine passes it to every member, a clone inherits it when it is made)."""
        self._set_switch("otm_set_shape", on)

    def shape_info(self):
        """Whether the matched shape is on (otm_shape_info)."""
        return self._switch_info("otm_shape_info")

    def shape(self):
        """The matched shape of the handle's last binary-level batch
        (otm_shape_size, otm_fetch_shape): (vertices, vtx_off, spans, trav_off,
        polyline_bytes, poly_off) -- _lib.SHAPE_VERTEX_DTYPE vertices in
        microdegrees, trace t's at [vtx_off[t], vtx_off[t + 1]); one
        _lib.SHAPE_SPAN_DTYPE span of trace-relative vertex indices per
        traversal, in traversals()' order and offsets; the traces' polyline6
        strings in one bytes object, trace t's at [poly_off[t], poly_off[t + 1])."""
        z = _lib.ShapeSizes()
        _check(lib().otm_shape_size(self.h, C.byref(z)))
        vtx = np.zeros(z.n_vertices, dtype=_lib.SHAPE_VERTEX_DTYPE)
        spans = np.zeros(z.n_traversals, dtype=_lib.SHAPE_SPAN_DTYPE)
        poly = np.zeros(z.n_bytes, dtype=np.uint8)
        offs = [np.zeros(z.n_traces + 1, dtype=np.int64) for _ in range(3)]
        dst = _lib.ShapeOut(vtx.ctypes.data if len(vtx) else None, len(vtx), offs[0].ctypes.data,
                            spans.ctypes.data if len(spans) else None, len(spans), offs[1].ctypes.data,
                            poly.ctypes.data if len(poly) else None, len(poly), offs[2].ctypes.data)
        _check(lib().otm_fetch_shape(self.h, C.byref(dst)))
        return vtx, offs[0], spans, offs[1], poly.tobytes(), offs[2]

    def shape_device(self):
        """The last batch's matched shape in this GPU's HBM (otm_shape_device; a
        one-device engine's, valid until its next batch): (_lib.ShapeOut of
        device pointers, its caps the counts; _lib.ShapeSizes)."""
        dev, z = _lib.ShapeOut(), _lib.ShapeSizes()
        _check(lib().otm_shape_device(self.h, C.byref(dev), C.byref(z)))
        return dev, z

    def set_attributes(self, mask):
        """The trace attributes' section mask of this handle (otm_set_attributes):
        _lib.ATTR_* bits, True for every section, 0 or False for off.  A
        multi-device engine passes it to every member, a clone inherits it."""
        mask = _lib.ATTR_ALL if mask is True else int(mask or 0)
        _check(lib().otm_set_attributes(self.h, mask))

    def attributes_info(self):
        """The trace attributes' section mask (otm_attributes_info; 0: off)."""
        m = C.c_uint32()
        _check(lib().otm_attributes_info(self.h, C.byref(m)))
        return m.value

    def attributes(self):
        """The trace attributes of the handle's last binary-level batch
        (otm_attributes_size, otm_fetch_attributes): (blob, body_off) -- one
        JSON body per trace in one bytes object, trace t's at
        [body_off[t], body_off[t + 1]) (int64 array of n_traces + 1)."""
        nt, nb = C.c_int64(), C.c_int64()
        _check(lib().otm_attributes_size(self.h, C.byref(nt), C.byref(nb)))
        blob = np.zeros(nb.value, dtype=np.uint8)
        off = np.zeros(nt.value + 1, dtype=np.int64)
        _check(lib().otm_fetch_attributes(self.h, blob.ctypes.data if nb.value else None, nb.value, off.ctypes.data,
                                          C.byref(nb)))
        return blob.tobytes(), off

    def attributes_device(self):
        """The last batch's trace attributes in this GPU's HBM
        (otm_attributes_device; a one-device engine's, valid until its next
        batch): (blob pointer, body_off pointer, n_traces, n_bytes)."""
        dev, off, nt, nb = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_int64()
        _check(lib().otm_attributes_device(self.h, C.byref(dev), C.byref(off), C.byref(nt), C.byref(nb)))
        return dev.value or 0, off.value or 0, nt.value, nb.value

    def set_counting(self, on):
        _check(lib().otm_set_counting(self.h, 1 if on else 0))

    def counters(self):
        c = _lib.WorkCounters()
        _check(lib().otm_get_counters(self.h, C.byref(c)))
        return {n: getattr(c, n) for n in _lib.COUNTER_NAMES}

    def set_timing(self, on):
        _check(lib().otm_set_timing(self.h, 1 if on else 0))

    STAGES = ("columns", "candidates", "links_scan", "transitions", "viterbi", "route", "segment_bound",
              "segments_report")

    def stage_ms(self):
        ms = (C.c_float * 8)()
        _check(lib().otm_get_stage_ms(self.h, ms, 8))
        return dict(zip(self.STAGES, list(ms)))

    def kernel_ms(self):
        """Per-kernel times (ms) of the last timed match_device call, by kernel name."""
        n = 0
        while lib().otm_kernel_name(n):
            n += 1
        ms = (C.c_float * n)()
        _check(lib().otm_get_kernel_ms(self.h, ms, n))
        return {lib().otm_kernel_name(k).decode(): ms[k] for k in range(n)}

    def spill_stats(self):
        """Work units of the last batch that each fallback tier took."""
        st = _lib.SpillStats()
        _check(lib().otm_get_spill_stats(self.h, C.byref(st)))
        return {n: getattr(st, n) for n, _ in _lib.SpillStats._fields_ if n != "pad"}

    TIERS = {"cand_big": 1, "trans_online": 2, "route_online": 4, "vit_lists": 8, "seg_large": 16}

    def tiers(self):
        """Tiers on demand (otm_get_tiers): the on-demand launch groups this
        context does not launch now, by name, and the stream dispatches of its
        last batch's final attempt."""
        mask, disp = C.c_int32(), C.c_int32()
        _check(lib().otm_get_tiers(self.h, C.byref(mask), C.byref(disp)))
        return {"dormant": {n for n, b in self.TIERS.items() if mask.value & b}, "mask": mask.value,
                "dispatches": disp.value}

    _DEBUG = {"ncand": (0, np.int32), "cand_edge": (1, np.int32), "cand_off": (2, np.float32),
              "cand_emis": (3, np.float32), "trans_off": (4, np.int64), "trans": (5, np.float32),
              "state": (6, np.int32), "col_prev": (7, np.int32), "route_dist": (8, np.float32),
              "gc": (9, np.float32), "ipos": (10, np.float32),
              # the last batch's inputs as the GPU request reader decoded them
              "in_trace_off": (11, np.int64), "in_lat": (12, np.float32), "in_lon": (13, np.float32),
              "in_time": (14, np.float64), "in_acc": (15, np.float32),
              "chain_start": (16, np.uint8), "is_col": (17, np.uint8),
              # the spatial work order (after a batch of at least OTM_SMALL_POINTS points)
              "order_item": (18, np.int32), "order_tile": (19, np.uint16), "order_grp": (20, np.int32)}

    def debug(self, name):
        what, dt = self._DEBUG[name]
        need = C.c_size_t()
        _check(lib().otm_debug_fetch(self.h, what, None, 0, C.byref(need)))
        out = np.zeros(need.value // np.dtype(dt).itemsize, dtype=dt)
        _check(lib().otm_debug_fetch(self.h, what, out.ctypes.data, out.nbytes, None))
        return out


def report_segments(body, match_output, engine=None):
    """report() (py/reporter_service.py:110-215) over any matcher's output."""
    b = body.encode("utf-8") if isinstance(body, str) else body
    m = match_output.encode("utf-8") if isinstance(match_output, str) else match_output
    out = C.c_void_p()
    n = C.c_size_t()
    code = lib().otm_report_segments(engine.h if engine is not None else None, b, len(b), m, len(m), C.byref(out),
                                     C.byref(n))
    return code, take(out, n.value).decode("utf-8")


def encode_request(uuid, lat, lon, time, accuracy):
    """The Java batcher's request bytes (Batch.java:52-61, Point.java:39-45) as
    HttpClient.POST sends them (ISO-8859-1, HttpClient.java:26).  uuid: the
    record key, a str or its UTF-8 bytes."""
    lat = np.ascontiguousarray(lat, dtype=np.float32)
    lon = np.ascontiguousarray(lon, dtype=np.float32)
    tm = np.ascontiguousarray(time, dtype=np.int64)
    acc = np.ascontiguousarray(accuracy, dtype=np.int32)
    out = C.c_void_p()
    n = C.c_size_t()
    ub = uuid if isinstance(uuid, bytes) else uuid.encode("utf-8")
    _check(lib().otm_encode_request(ub, len(lat), lat.ctypes.data, lon.ctypes.data,
                                    tm.ctypes.data, acc.ctypes.data, C.byref(out), C.byref(n)))
    return take(out, n.value)


def murmur2_partition(key, n):
    """Kafka DefaultPartitioner shard of a uuid (Reporter.java:97 keys by uuid)."""
    b = key.encode("utf-8") if isinstance(key, str) else key
    return (lib().otm_murmur2(b, len(b)) & 0x7fffffff) % n
