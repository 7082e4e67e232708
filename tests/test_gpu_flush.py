"""The datastore flush on the GPU (reporter_amd/csrc/flush.hip) and the
engine-owned windows behind the C ABI (otm_flush_body_device,
otm_window_begin / _flush / _end), byte for byte against
datastore.serialize(datastore.flush_records(...)) on the same numbers."""
import threading

import numpy as np
import pytest

import flush_cases as fc
from reporter_amd import Engine, datastore, encode_request, flush, synth
from reporter_amd.engine import OtmError

pytestmark = pytest.mark.gpu

EMPTY = b'{"mode":"auto","bin_kph":10.0,"rank":0,"world":1,"segments":[]}'
DEVICE_MAX_NBINS = 64  # include/otmatch.h: otm_flush_body_device


@pytest.fixture(scope="module")
def eng(small_graph):
    with Engine(graph_path=small_graph) as e:
        yield e


@pytest.fixture(scope="module")
def ids(small_graph):
    return synth.segment_ids(small_graph)


def _dev(c, s):
    import torch
    ct = torch.from_numpy(np.ascontiguousarray(c.reshape(-1).astype(np.int32))).to("cuda:0")
    st = torch.from_numpy(np.ascontiguousarray(np.asarray(s, np.uint64).view(np.int64))).to("cuda:0")
    return ct, st


def _ref_of_reports(reports, ids, nbins, bin_kph):
    index_of = {int(v): i for i, v in enumerate(ids)}
    h, sums = flush.histograms_from_reports(reports, index_of, len(ids), nbins, bin_kph)
    return fc.reference(h, sums, ids, 0, 1, nbins, bin_kph), int(h.sum())


@pytest.mark.parametrize("nbins", [1, 16, 17, 40])
def test_device_writer_on_synthetic_slices(eng, ids, nbins):
    nseg = eng.graph_info()["segments"]
    assert nseg >= 300 and nseg == len(ids)
    n = 0
    for world in (1, 2, 3, 7):
        windows = [fc.window("rows", nseg, nbins, world, rows_at=(0, 63, 64, 65, nseg - 1, nseg)),
                   fc.window("dense", nseg, nbins, world), fc.window("empty", nseg, nbins, world),
                   fc.window("row0", nseg, nbins, world), fc.window("special", nseg, nbins, world),
                   fc.window("random", nseg, nbins, world, seed=world)]
        for wi, (c, s) in enumerate(windows):
            bin_kph = (10.0, 2.5, 0.1)[(wi + world) % 3]
            for rank in range(world):
                cr, sr = fc.slice_of(c, s, rank, world)
                want, nrec = fc.reference(cr, sr, ids, rank, world, nbins, bin_kph)
                got, got_n = eng.flush_body_device(*_dev(cr, sr), rank, world, nbins, bin_kph)
                assert got == want, (world, wi, rank)
                assert got_n == nrec
                n += nrec
    assert n > nseg


def test_device_writer_declines_a_sum_past_its_float_range(eng, ids):
    nseg = len(ids)
    c, s = fc.window("rows", nseg, 16, 1, rows_at=(0, 64, nseg - 1))
    s[64] = np.uint64(fc.DECLINE_SUM)
    assert fc.DECLINE_SUM >= 2 ** 52 * 1000
    want, nrec = fc.reference(c, s, ids, 0, 1, 16, 10.0)
    assert nrec == 3
    assert eng.flush_body_device(*_dev(c, s), 0, 1, 16, 10.0) == (want, nrec)
    # the largest sum the device writes itself, and the call after a decline
    s[64] = np.uint64(2 ** 52 * 1000 - 1)
    assert eng.flush_body_device(*_dev(c, s), 0, 1, 16, 10.0) == fc.reference(c, s, ids, 0, 1, 16, 10.0)


def test_device_writer_refuses_nbins_past_its_limit(eng, ids):
    nseg = len(ids)
    c, s = fc.window("row0", nseg, DEVICE_MAX_NBINS + 1, 1)
    with pytest.raises(OtmError, match="nbins"):
        eng.flush_body_device(*_dev(c, s), 0, 1, DEVICE_MAX_NBINS + 1, 10.0)
    c, s = fc.window("dense", nseg, DEVICE_MAX_NBINS, 1)
    assert eng.flush_body_device(*_dev(c, s), 0, 1, DEVICE_MAX_NBINS, 10.0) == \
        fc.reference(c, s, ids, 0, 1, DEVICE_MAX_NBINS, 10.0)
    # datastore.flush_body picks the writer by where the tensors are
    ct, st = _dev(c, s)
    want = fc.reference(c, s, ids, 0, 1, DEVICE_MAX_NBINS, 10.0)
    assert datastore.flush_body(eng, ct, st, 0, 1, DEVICE_MAX_NBINS, 10.0) == want
    assert datastore.flush_body(None, ct.cpu(), st.cpu(), 0, 1, DEVICE_MAX_NBINS, 10.0, segment_ids=ids) == want


@pytest.fixture(scope="module")
def matched(small_graph, ids):
    """The 300 x 100 batch of test_histogram_bins_and_speed_sums, its window's
    flush body from an engine-owned window, and the reference body."""
    b = synth.make_traces(small_graph, 300, 100, seed=23)
    with Engine(graph_path=small_graph) as e:
        e.window_begin(16, 10.0)
        res = e.match(b)
        first = e.window_flush()
        second = e.window_flush()
        e.match(b)
        third = e.window_flush()
        e.window_end()
    (want, nrec), counted = _ref_of_reports(res.reports, ids, 16, 10.0)
    return dict(batch=b, first=first, second=second, third=third, want=want, nrec=nrec, counted=counted)


def test_matched_window(matched):
    assert matched["counted"] > 100
    assert matched["first"] == (matched["want"], matched["nrec"])
    assert matched["second"] == (EMPTY, 0)  # flushed: the window goes on from zero
    assert matched["third"] == matched["first"]


def _sub(b, t0, t1):
    off = b["trace_off"]
    a, e = int(off[t0]), int(off[t1])
    return {"trace_off": (off[t0:t1 + 1] - off[t0]).copy(), "lat": b["lat"][a:e].copy(), "lon": b["lon"][a:e].copy(),
            "time": b["time"][a:e].copy(), "accuracy": b["accuracy"][a:e].copy()}


def test_window_collects_clones_batches(small_graph, matched):
    b = matched["batch"]
    halves = [_sub(b, 0, 150), _sub(b, 150, 300)]
    with Engine(graph_path=small_graph) as parent:
        parent.window_begin(16, 10.0)
        clones = [parent.clone(), parent.clone()]
        err = []

        def run(i):
            try:
                clones[i].match(halves[i])
            except Exception as e:  # noqa: BLE001
                err.append(e)
        th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not err, err
        got = parent.window_flush()
        for c in clones:
            c.close()
        parent.window_end()
    assert got == matched["first"]


def _bodies(b, n):
    out = []
    for t in range(n):
        a, e = b["trace_off"][t], b["trace_off"][t + 1]
        out.append(encode_request("veh%d" % t, b["lat"][a:e], b["lon"][a:e], b["time"][a:e].astype(np.int64),
                                  b["accuracy"][a:e].astype(np.int32)))
    return out


def test_multi_device_window(small_graph, ids):
    bodies = _bodies(synth.make_traces(small_graph, 90, 60, seed=71), 90)
    b257 = synth.make_traces(small_graph, 257, 70, seed=73)
    with Engine(graph_path=small_graph, devices=[0, 0, 0]) as grp, Engine(graph_path=small_graph) as one:
        grp.window_begin(16, 10.0)
        one.window_begin(16, 10.0)
        # the public binding keeps refusing a multi-device engine
        import torch
        with pytest.raises(OtmError):
            grp.hist_bind(torch.zeros(16, dtype=torch.int32, device="cuda:0"), 16, 10.0)
        # a member's window belongs to the group's handle
        for call in (lambda: grp.member(1).window_end(), lambda: grp.member(1).window_begin(16, 10.0),
                     lambda: grp.member(0).window_flush()):
            with pytest.raises(OtmError, match="multi-device"):
                call()
        assert grp.report_batch(bodies) == one.report_batch(bodies)
        (want, nrec), counted = _ref_of_reports(grp.fetch().reports, ids, 16, 10.0)
        assert counted > 20
        got = grp.window_flush()
        assert got == one.window_flush()
        assert got == (want, nrec)
        r = grp.match(b257)
        one.match(b257)
        (want, nrec), counted = _ref_of_reports(r.reports, ids, 16, 10.0)
        assert counted > 100
        got = grp.window_flush()
        assert got == one.window_flush()
        assert got == (want, nrec)
        assert grp.window_flush() == (EMPTY, 0)
        # a caller's slice on the group handle (member 0's graph) and on a clone of a member
        c, s = fc.window("special", len(ids), 17, 2)
        cr, sr = fc.slice_of(c, s, 1, 2)
        want = fc.reference(cr, sr, ids, 1, 2, 17, 2.5)
        assert grp.flush_body_device(*_dev(cr, sr), 1, 2, 17, 2.5) == want
        cl = one.clone()
        assert cl.flush_body_device(*_dev(cr, sr), 1, 2, 17, 2.5) == want
        cl.close()
        grp.window_end()
        one.window_end()
        with pytest.raises(OtmError):
            grp.window_flush()


def test_window_errors_and_lifetime(small_graph, eng):
    import torch
    nseg = eng.graph_info()["segments"]
    h = torch.zeros(nseg * 16, dtype=torch.int32, device="cuda:0")
    sums = torch.zeros(nseg, dtype=torch.int64, device="cuda:0")
    with pytest.raises(OtmError, match="window"):
        eng.window_flush()
    with pytest.raises(OtmError, match="window"):
        eng.window_end()
    for nbins, kph in ((0, 10.0), (16, 0.0), (16, -1.0), (DEVICE_MAX_NBINS + 1, 10.0)):
        with pytest.raises(OtmError, match="nbins"):
            eng.window_begin(nbins, kph)
    c = eng.clone()
    with pytest.raises(OtmError, match="parent"):
        c.window_begin(16, 10.0)
    c.close()
    eng.hist_bind(h, 16, 10.0, speed_sum=sums)
    with pytest.raises(OtmError, match="otm_hist_bind"):
        eng.window_begin(16, 10.0)  # a caller's binding is in place
    eng.hist_bind(None, 0, 1.0)
    eng.window_begin(16, 10.0)
    with pytest.raises(OtmError, match="already open"):
        eng.window_begin(16, 10.0)
    with pytest.raises(OtmError, match="window"):
        eng.hist_bind(h, 16, 10.0)
    with pytest.raises(OtmError, match="window"):
        eng.hist_bind(h, 16, 10.0, speed_sum=sums)
    assert eng.window_flush() == (EMPTY, 0)
    eng.window_end()
    # the caller's binding works again
    b = synth.make_traces(small_graph, 20, 60, seed=23)
    eng.hist_bind(h, 16, 10.0, speed_sum=sums)
    eng.match(b)
    eng.hist_bind(None, 0, 1.0)
    torch.cuda.synchronize()
    assert int(h.sum()) > 0
    # destroying an engine with an open window is clean
    with Engine(graph_path=small_graph) as e2:
        e2.window_begin(16, 10.0)
        e2.match(b)
    # begin / flush / end cycles hold no device memory
    free = []
    for k in range(20):
        eng.window_begin(16, 10.0)
        eng.match(b)
        body, nrec = eng.window_flush()
        assert nrec > 0 and body.startswith(b'{"mode":"auto","bin_kph":10.0,')
        eng.window_end()
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(0)[0])
    assert free[-1] == free[1], free
