"""The engine's device and page-locked arrays (reporter_amd/csrc/buffers.h)
through one cycle of every call that sizes, binds or reads them: the outputs
of an engine whose batch is regrown and redone (OTM_TRANS_CAP / OTM_POOL_CAP
pinned small) equal those of a plain engine, and create / use / destroy cycles
hold no device memory."""
import json
import os

import numpy as np
import pytest

import flush_cases as fc
from reporter_amd import Engine, encode_request, synth

pytestmark = pytest.mark.gpu

ORIGIN = 1499999940  # a whole minute below the traces' first time (tests/test_gpu_pairs.py)
PINNED = {"OTM_TRANS_CAP": "64", "OTM_POOL_CAP": "8"}
REPORT_ENV = ("REPORT_LEVELS", "TRANSITION_LEVELS", "THRESHOLD_SEC")
with open(os.path.join(os.path.dirname(__file__), "golden", "report_cases.json")) as _f:
    CASE = next(c for c in json.load(_f) if c["name"] == "rand0")


@pytest.fixture(scope="module")
def inputs(small_graph):
    """20 traces of 60 points (tests/test_gpu_flush.py), 40 request bodies (the
    GPU request reader and writer start at 32), one histogram slice."""
    b = synth.make_traces(small_graph, 20, 60, seed=23)
    rq = synth.make_traces(small_graph, 40, 60, seed=71)
    off = rq["trace_off"]
    bodies = [encode_request("veh%d" % t, rq["lat"][off[t]:off[t + 1]], rq["lon"][off[t]:off[t + 1]],
                             rq["time"][off[t]:off[t + 1]].astype(np.int64),
                             rq["accuracy"][off[t]:off[t + 1]].astype(np.int32)) for t in range(40)]
    nseg = len(synth.segment_ids(small_graph))
    return b, bodies, fc.window("random", nseg, 16, 1, seed=5)


def _records(r):
    return tuple(getattr(r, k).tobytes() for k in ("traces", "segments", "reports", "way_ids"))


def _cycle(small_graph, inputs, monkeypatch, pinned, before_destroy=None):
    """One engine's life: every call whose arrays the engine owns, then the destroy."""
    import torch
    b, bodies, (counts, sums) = inputs
    for k in REPORT_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in PINNED.items():
        if pinned:
            monkeypatch.setenv(k, v)
        else:
            monkeypatch.delenv(k, raising=False)
    out = {}
    with Engine(graph_path=small_graph, matched_points=True) as e:
        e.set_counting(True)
        r = e.match(b)
        reports = r.reports.copy()
        out["match"] = _records(r)
        out["attempts"] = e.spill_stats()["attempts"]
        out["counted_points"] = e.counters()["points"]
        out["match_compact"] = _records(e.match_compact(b))
        out["report_batch"] = e.report_batch(bodies)
        e.match(b)
        out["points"] = e.points().tobytes()
        out["state"] = e.debug("state").tobytes()
        out["report_segments"] = e.report_segments_device([(CASE["request"], CASE["match_output"])])
        e.window_begin(16, 10.0)
        e.match(b)
        out["window"] = e.window_flush()
        e.window_end()
        e.pairs_begin(60, ORIGIN)
        e.pairs_add_reports(reports)
        out["pairs"] = e.pairs_flush()
        e.pairs_end()
        ct = torch.from_numpy(np.ascontiguousarray(counts.reshape(-1).astype(np.int32))).to("cuda:0")
        st = torch.from_numpy(np.ascontiguousarray(np.asarray(sums, np.uint64).view(np.int64))).to("cuda:0")
        out["flush"] = e.flush_body_device(ct, st, 0, 1, 16, 10.0)
        del ct, st
        if before_destroy:
            before_destroy()
    return out


def test_redone_batches_equal_plain_ones(small_graph, inputs, monkeypatch):
    got = _cycle(small_graph, inputs, monkeypatch, pinned=True)
    want = _cycle(small_graph, inputs, monkeypatch, pinned=False)
    assert got.pop("attempts") > 1 and want.pop("attempts") == 1   # the pinned engine regrew and redid its batch
    assert got["counted_points"] == 20 * 60
    assert got["report_segments"] == [(CASE["code"], CASE["body"])]
    assert all(code == 200 for code, _ in got["report_batch"])
    assert got["window"][1] > 0 and got["pairs"][1]["records"] > 0 and got["flush"][1] > 0
    assert sorted(got) == sorted(want)
    for k in got:
        assert got[k] == want[k], k


def test_engine_cycles_hold_no_device_memory(small_graph, inputs, monkeypatch):
    """Six create / use / destroy cycles: free device memory after the last
    equals that after the second.  Measured on an MI355X, the drop from cycle
    2 to cycle 6 was 0 bytes with the hand-kept free lists the typed buffers
    replaced and 0 bytes with the typed buffers, so the equality is asserted.
    In use at the end of the first cycle's calls, before the destroy: printed,
    not asserted (2,455,764,992 bytes before and after the change,
    profiles/engine_buffers/memory.json)."""
    import torch
    torch.cuda.synchronize()
    start = torch.cuda.mem_get_info(0)[0]
    used, free = [], []

    def probe():
        torch.cuda.synchronize()
        used.append(start - torch.cuda.mem_get_info(0)[0])
    for k in range(6):
        _cycle(small_graph, inputs, monkeypatch, pinned=True, before_destroy=probe)
        torch.cuda.synchronize()
        free.append(torch.cuda.mem_get_info(0)[0])
    print("engine_buffers: in use before the first destroy %d bytes; free after cycles %s; drop 2 -> 6: %d bytes"
          % (used[0], free, free[1] - free[-1]))
    assert free[-1] == free[1], free
