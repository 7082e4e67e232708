"""Pair windows on the GPU (reporter_amd/csrc/pairs.hip, the upsert inside
k_report) through the C ABI (otm_pairs_*), byte for byte against the
definition, datastore.serialize(datastore.pair_records(...)), over the reports
the same calls returned."""
import json
import threading

import numpy as np
import pytest

import flush_cases as fc
from reporter_amd import Engine, _lib, datastore, encode_request, flush, synth
from reporter_amd.engine import OtmError

pytestmark = pytest.mark.gpu

ORIGIN = 1499999940  # a whole minute below the traces' first time (1500000000)


def empty_body(bucket_s, origin, privacy=1):
    return b'{"mode":"auto","bucket_s":%d,"origin":%d,"privacy":%d,"pairs":[]}' % (bucket_s, origin, privacy)


def want(reports, ids, bucket_s, origin, privacy=1):
    d, st = datastore.pair_records(reports, ids, bucket_s, origin, privacy)
    return datastore.serialize(d), st


@pytest.fixture(scope="module")
def ids(small_graph):
    return synth.segment_ids(small_graph)


@pytest.fixture(scope="module")
def eng(small_graph):
    with Engine(graph_path=small_graph) as e:
        yield e


@pytest.fixture(scope="module")
def batches(small_graph, eng):
    """The 300 x 100 batch of tests/test_gpu_flush.py and the same vehicles at
    40 s a point, each with the reports of one match (no window open)."""
    out = {}
    for name, kw in (("base", {}), ("slow", {"interval_s": 40.0})):
        b = synth.make_traces(small_graph, 300, 100, seed=23, **kw)
        out[name] = (b, eng.match(b).reports.copy())
    return out


def _sub(b, t0, t1):
    off = b["trace_off"]
    a, e = int(off[t0]), int(off[t1])
    return {"trace_off": (off[t0:t1 + 1] - off[t0]).copy(), "lat": b["lat"][a:e].copy(), "lon": b["lon"][a:e].copy(),
            "time": b["time"][a:e].copy(), "accuracy": b["accuracy"][a:e].copy()}


# ------------------------------------------------------------------ 1. matched windows
@pytest.mark.parametrize("name,bucket_s,origin", [("base", 60, ORIGIN), ("base", 300, 1499999700),
                                                  ("base", 3600, 1499997600), ("slow", 60, ORIGIN)])
def test_matched_window(eng, ids, batches, name, bucket_s, origin):
    b, reports = batches[name]
    body, st = want(reports, ids, bucket_s, origin)
    print(name, bucket_s, st)
    assert st["reports"] > 100 and st["keys"] > 100 and st["out_of_range"] == 0
    eng.pairs_begin(bucket_s, origin)
    try:
        info = eng.pairs_info()
        assert (info["bucket_s"], info["origin"], info["privacy"]) == (bucket_s, origin, 1)
        assert info["max_keys"] == max(65536, 8 * len(ids)) and info["slots"] == 2 * info["max_keys"]
        res = eng.match(b)
        assert res.reports.tobytes() == reports.tobytes()  # the reports are what they were without a window
        assert eng.pairs_flush() == (body, st)
        assert eng.pairs_flush() == (empty_body(bucket_s, origin), dict.fromkeys(st, 0))
        eng.match(b)
        assert eng.pairs_flush() == (body, st)
    finally:
        eng.pairs_end()


# ------------------------------------------------------------------ 2. privacy
@pytest.mark.parametrize("privacy", [2, 3])
def test_privacy_floor(eng, ids, batches, privacy):
    b, reports = batches["base"]
    body, st = want(reports, ids, 60, ORIGIN, privacy)
    print(privacy, st)
    assert st["records"] >= 1 and st["suppressed_keys"] >= 1  # the reference keeps some and suppresses some
    assert st["suppressed_reports"] >= st["suppressed_keys"]
    eng.pairs_begin(60, ORIGIN, privacy=privacy)
    try:
        eng.match(b)
        assert eng.pairs_flush() == (body, st)
    finally:
        eng.pairs_end()


# ------------------------------------------------------------------ 3. order-free
def test_order_free(small_graph, ids, batches):
    b, reports = batches["base"]
    body, st = want(reports, ids, 60, ORIGIN)
    cuts = [0, 37, 150, 151, 300]
    parts = [_sub(b, cuts[i], cuts[i + 1]) for i in range(4)]
    index_of = {int(v): i for i, v in enumerate(ids)}
    h, sums = flush.histograms_from_reports(reports, index_of, len(ids), 16, 10.0)
    hist_want = fc.reference(h, sums, ids, 0, 1, 16, 10.0)
    with Engine(graph_path=small_graph) as parent:
        parent.pairs_begin(60, ORIGIN)
        for order in ((0, 1, 2, 3), (3, 1, 0, 2)):
            for i in order:
                parent.match(parts[i])
            assert parent.pairs_flush() == (body, st), order
        # four host threads on four clones at once
        clones = [parent.clone() for _ in range(4)]
        err = []

        def run(i):
            try:
                clones[i].match(parts[i])
            except Exception as e:  # noqa: BLE001
                err.append(e)
        th = [threading.Thread(target=run, args=(i,)) for i in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not err, err
        assert parent.pairs_flush() == (body, st)
        for c in clones:
            c.close()
        # with a histogram window open beside it: neither knows of the other
        parent.window_begin(16, 10.0)
        parent.match(b)
        assert parent.window_flush() == hist_want
        assert parent.pairs_flush() == (body, st)
        parent.window_end()
        parent.match(b)
        assert parent.pairs_flush() == (body, st)
        parent.pairs_end()


# ------------------------------------------------------------------ 4. table pressure
def test_max_keys_exactly_the_key_count(eng, ids, batches):
    b, reports = batches["base"]
    body, st = want(reports, ids, 60, ORIGIN)
    eng.pairs_begin(60, ORIGIN, max_keys=st["keys"])
    try:
        assert eng.pairs_info()["max_keys"] == st["keys"]
        eng.match(b)
        got, gst = eng.pairs_flush()
        assert gst["dropped"] == 0
        assert (got, gst) == (body, st)
    finally:
        eng.pairs_end()


@pytest.mark.parametrize("max_keys", [1, 64])
def test_full_table_drops_and_counts(eng, ids, batches, max_keys):
    b, reports = batches["base"]
    d, st = datastore.pair_records(reports, ids, 60, ORIGIN, 1)
    assert st["keys"] > max_keys
    ref = {(p["id"], p.get("next_id"), p["bucket"]): p for p in d["pairs"]}
    eng.pairs_begin(60, ORIGIN, max_keys=max_keys)
    try:
        assert eng.pairs_info()["slots"] >= 2 * max_keys
        eng.match(b)
        got, gst = eng.pairs_flush()   # (the call returns: nothing hangs)
    finally:
        eng.pairs_end()
    print(max_keys, gst)
    assert gst["keys"] == max_keys == gst["records"]
    assert gst["dropped"] > 0
    assert gst["reports"] + gst["out_of_range"] + gst["dropped"] == st["reports"] + st["out_of_range"]
    pairs = json.loads(got)["pairs"]
    assert len(pairs) == max_keys and sum(p["count"] for p in pairs) == gst["reports"]
    keys = [(p["id"], p.get("next_id"), p["bucket"]) for p in pairs]
    assert len(set(keys)) == max_keys
    for k, p in zip(keys, pairs):
        assert k in ref and 1 <= p["count"] <= ref[k]["count"]
        assert p["length"] == ref[k]["length"] and p["duration_ms"] <= ref[k]["duration_ms"]
        assert p["t_min"] >= ref[k]["t_min"] and p["t_max"] <= ref[k]["t_max"]


def _records(n, ids, key_of):
    """n host records: record r on key key_of(r) = (k, row, next row)."""
    r = np.arange(n, dtype=np.int64)
    k, gi, gn = key_of(r)
    rec = np.zeros(n, _lib.REPORT_DTYPE)
    sid = np.asarray(ids).astype(np.uint64).view(np.int64)
    rec["id"] = sid[gi]
    rec["next_id"] = sid[gn]
    rec["t0"] = ORIGIN + k * 60 + (r % 50) + 0.25
    rec["t1"] = rec["t0"] + 1.0 + (r % 7) * 0.5
    rec["length"] = 10 + gi   # one value per id
    rec["queue_length"] = r % 5
    return rec


def test_contention_on_one_key(eng, ids):
    n = 200000
    rec = _records(n, ids, lambda r: (np.full(n, 7), np.full(n, 3), np.full(n, 5)))
    body, st = want(rec, ids, 60, ORIGIN)
    assert (st["reports"], st["keys"]) == (n, 1)
    eng.pairs_begin(60, ORIGIN)
    try:
        eng.pairs_add_reports(rec)
        got, gst = eng.pairs_flush()
    finally:
        eng.pairs_end()
    p, = json.loads(got)["pairs"]
    assert p["count"] == n and p["queue_length"] == int(rec["queue_length"].sum())
    assert p["duration_ms"] == int(((rec["t1"] - rec["t0"]) * 1000.0 + 0.5).astype(np.int64).sum())
    assert (got, gst) == (body, st)


def test_exactly_max_keys_distinct_keys_in_twice_the_slots(eng, ids):
    n, max_keys = 200000, 65536
    nrow = len(ids)
    assert nrow >= 17

    def key_of(r):
        j = (r * 40503) % max_keys   # every key of the 65,536, each about three times
        return j % 4096, j // 4096, (j // 4096 + 1 + j % 7) % nrow
    rec = _records(n, ids, key_of)
    body, st = want(rec, ids, 60, ORIGIN)
    assert st["keys"] == max_keys and st["reports"] == n
    eng.pairs_begin(60, ORIGIN, max_keys=max_keys)
    try:
        assert eng.pairs_info()["slots"] == 2 * max_keys
        half = n // 2
        eng.pairs_add_reports(rec[:half])
        eng.pairs_add_reports(rec[half:])
        got, gst = eng.pairs_flush()
        assert gst["dropped"] == 0
        assert (got, gst) == (body, st)
        # one more key than the table holds: exactly its reports drop
        extra = _records(3, ids, lambda r: (np.full(3, 4095), np.full(3, 16), np.full(3, 0)))
        eng.pairs_add_reports(rec)
        eng.pairs_add_reports(extra)
        got, gst = eng.pairs_flush()
        assert gst["dropped"] == 3 and gst["keys"] == max_keys
        assert got == body
    finally:
        eng.pairs_end()


# ------------------------------------------------------------------ 5. range
@pytest.mark.parametrize("origin", [1500000200, 1500000000 - 4000])
def test_bucket_range(eng, ids, batches, origin):
    b, reports = batches["base"]
    _, st = want(reports, ids, 1, origin)
    print(origin, st)
    assert st["out_of_range"] > 0 and st["reports"] > 0
    # two host records on the window's last second and on the first one past it
    edge = np.zeros(2, _lib.REPORT_DTYPE)
    edge[:] = reports[reports["next_id"] >= 0][0]
    edge["t0"] = [origin + 4095.5, origin + 4096.0]
    edge["t1"] = edge["t0"] + 10.0
    body, st2 = want(np.concatenate([reports, edge]), ids, 1, origin)
    assert st2["reports"] == st["reports"] + 1 and st2["out_of_range"] == st["out_of_range"] + 1
    assert b'"bucket":%d,' % (origin + 4095) in body and b'"bucket":%d,' % (origin + 4096) not in body
    eng.pairs_begin(1, origin)
    try:
        eng.match(b)
        eng.pairs_add_reports(edge)
        assert eng.pairs_flush() == (body, st2)
    finally:
        eng.pairs_end()


# ------------------------------------------------------------------ 6. queue sums
def test_queue_length_sums(small_graph, ids, batches, tmp_path_factory):
    import queue_cases as qc
    b, _ = batches["base"]
    with Engine(graph_path=small_graph, queue_speed_kph=20.0) as e:
        e.pairs_begin(60, ORIGIN)
        res = e.match(b)
        got = e.pairs_flush()
        e.pairs_end()
    assert got == want(res.reports, ids, 60, ORIGIN)
    if not any(p["queue_length"] > 0 for p in json.loads(got[0])["pairs"]):
        # the city batch queued nowhere: the hand road whose segment 16 queues 80 m
        roads = qc.graphs(tmp_path_factory.mktemp("queue_pairs"))
        rids = synth.segment_ids(roads["road"])
        hb = qc.batch([qc.hand_cases()["queue_1s"][1]])
        origin = (int(qc.T0) // 60 - 1) * 60
        with Engine(graph_path=roads["road"], queue_speed_kph=qc.KPH) as e:
            e.pairs_begin(60, origin)
            res = e.match(hb)
            got = e.pairs_flush()
            e.pairs_end()
        assert got == want(res.reports, rids, 60, origin)
    assert any(p["queue_length"] > 0 for p in json.loads(got[0])["pairs"])


# ------------------------------------------------------------------ 7. the drop-in paths
def _bodies(b, n):
    out = []
    for t in range(n):
        a, e = b["trace_off"][t], b["trace_off"][t + 1]
        out.append(encode_request("veh%d" % t, b["lat"][a:e], b["lon"][a:e], b["time"][a:e].astype(np.int64),
                                  b["accuracy"][a:e].astype(np.int32)))
    return out


def _reports_of_responses(bodies):
    """The datastore reports of /report response bodies as report records."""
    rows = []
    for body in bodies:
        d = json.loads(body)
        for r in d.get("datastore", {}).get("reports", []):
            rows.append((r["id"], r.get("next_id", -1), r["t0"], r["t1"], r["length"], r["queue_length"],
                         (1 if isinstance(r["t1"], int) else 0) | (2 if isinstance(r["t0"], int) else 0), 0))
    rec = np.zeros(len(rows), _lib.REPORT_DTYPE)
    for i, row in enumerate(rows):
        rec[i] = row
    return rec


def test_report_batch_feeds_the_window(small_graph, eng, ids):
    bodies = _bodies(synth.make_traces(small_graph, 90, 60, seed=71), 90)
    assert len(bodies) >= 32   # the GPU reader and writer run
    eng.pairs_begin(60, ORIGIN)
    try:
        out = eng.report_batch(bodies)
        got = eng.pairs_flush()
    finally:
        eng.pairs_end()
    assert all(code == 200 for code, _ in out)
    rec = _reports_of_responses([body for _, body in out])
    assert len(rec) > 20
    assert got == want(rec, ids, 60, ORIGIN)


@pytest.mark.parametrize("json_path", [False, True], ids=["binary", "json"])
def test_native_batcher_feeds_the_window(small_graph, ids, json_path):
    """The batcher forwards few of its responses (clean() and close() discard
    theirs, and the binary path writes none for them), so the responses come
    from the same stream posted through a handler that keeps every one of
    them: the batcher over the engine must leave the same window."""
    from reporter_amd.batcher import Batcher
    from test_batcher import make_stream, run_native
    recs = make_stream(small_graph, n_veh=30, n_pts=80, seed=47)
    seen = []
    with Engine(graph_path=small_graph) as e:
        e.pairs_begin(60, ORIGIN)

        def post(bodies):
            out = e.report_batch(bodies)
            seen.extend(body for code, body in out if code == 200)
            return out
        st = run_native(recs, Batcher(handler=post)).stats()
        by_handler = e.pairs_flush()
        nst = run_native(recs, Batcher(engine=e, json_path=json_path, threads=4)).stats()
        native = e.pairs_flush()
        e.pairs_end()
    assert nst["requests"] == st["requests"] > nst["forwarded"] > 10
    rec = _reports_of_responses(seen)
    ref = want(rec, ids, 60, ORIGIN)
    assert ref[1]["records"] >= 2   # (the batcher's requests are short: few of them report)
    assert by_handler == ref
    assert native == by_handler


# ------------------------------------------------------------------ 8. multi-device engines
@pytest.mark.parametrize("members", [2, 3])
def test_multi_device_engine(small_graph, eng, ids, batches, members):
    b, reports = batches["base"]
    body, st = want(reports, ids, 60, ORIGIN)
    with Engine(graph_path=small_graph, devices=[0] * members) as grp:
        with pytest.raises(OtmError, match="pair window"):
            grp.pairs_flush()
        with pytest.raises(OtmError, match="pair window"):
            grp.pairs_end()
        grp.pairs_begin(60, ORIGIN)
        with pytest.raises(OtmError, match="already open"):
            grp.pairs_begin(60, ORIGIN)
        for call in (lambda: grp.member(1).pairs_begin(60, ORIGIN), lambda: grp.member(0).pairs_flush(),
                     lambda: grp.member(1).pairs_end(), lambda: grp.member(0).pairs_info()):
            with pytest.raises(OtmError, match="multi-device"):
                call()
        grp.match(b)
        got = grp.pairs_flush()
        assert got == (body, st)
        assert grp.pairs_flush() == (empty_body(60, ORIGIN), dict.fromkeys(st, 0))
        grp.match(b)
        grp.pairs_add_reports(reports)
        got2, st2 = grp.pairs_flush()
        assert st2["reports"] == 2 * st["reports"] and st2["keys"] == st["keys"]
        grp.pairs_end()
    # one engine gives the same body
    eng.pairs_begin(60, ORIGIN)
    try:
        eng.match(b)
        assert eng.pairs_flush() == got
    finally:
        eng.pairs_end()


def test_refusals_and_lifetime(small_graph, eng, batches):
    import torch
    b, _ = batches["base"]
    for call in (eng.pairs_flush, eng.pairs_end, eng.pairs_info, lambda: eng.pairs_add_reports(batches["base"][1])):
        with pytest.raises(OtmError, match="no pair window"):
            call()
    for kw, word in ((dict(bucket_s=0), "bucket_s"), (dict(bucket_s=60, privacy=0), "privacy"),
                     (dict(bucket_s=60, origin=-60), "origin"), (dict(bucket_s=60, origin=61), "multiple"),
                     (dict(bucket_s=60, max_keys=-1), "max_keys")):
        with pytest.raises(OtmError, match=word):
            eng.pairs_begin(**kw)
    c = eng.clone()
    for call in (lambda: c.pairs_begin(60, ORIGIN), c.pairs_flush, c.pairs_end):
        with pytest.raises(OtmError, match="parent"):
            call()
    c.close()
    eng.pairs_begin(60, ORIGIN)
    with pytest.raises(OtmError, match="already open"):
        eng.pairs_begin(60, ORIGIN)
    eng.pairs_end()
    # destroying an engine with an open pair window is clean
    small = _sub(b, 0, 20)
    with Engine(graph_path=small_graph) as e2:
        e2.pairs_begin(60, ORIGIN)
        e2.match(small)
    # begin / flush / end cycles hold no device memory
    free = []
    for k in range(8):
        eng.pairs_begin(60, ORIGIN)
        eng.match(small)
        body, st = eng.pairs_flush()
        assert st["records"] > 0 and body.startswith(b'{"mode":"auto","bucket_s":60,')
        eng.pairs_end()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(0)[0])
    assert free[-1] == free[1], free


# ------------------------------------------------------------------ 9. errors contribute nothing
def test_error_traces_contribute_nothing(small_graph, ids, monkeypatch):
    """The zero-division batch of tests/test_gpu_report.py: a trace whose
    report() raises posts nothing, its earlier reports included."""
    for k in ("REPORT_LEVELS", "TRANSITION_LEVELS", "THRESHOLD_SEC"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("REPORT_LEVELS", "0,1,2")
    monkeypatch.setenv("TRANSITION_LEVELS", "0,1,2")
    b = synth.make_traces(small_graph, 40, 100, interval_s=5.0, noise_sigma_m=5.0, accuracy=5.0, seed=71)
    b["time"] = b["time"].copy()
    off = b["trace_off"]
    for t in range(0, 40, 2):  # every other trace: points 20..79 share one timestamp
        b["time"][off[t] + 20:off[t] + 80] = b["time"][off[t] + 20]
    with Engine(graph_path=small_graph) as e:
        e.pairs_begin(60, ORIGIN)
        r = e.match(b)
        got = e.pairs_flush()
        e.pairs_end()
    zd = (r.traces["code"] == 500) & (r.traces["error_kind"] == 1)
    assert zd.sum() >= 5
    assert (r.traces["rep_cnt"][zd] == 0).all()
    body, st = want(r.reports, ids, 60, ORIGIN)
    assert st["reports"] > 20
    assert got == (body, st)
