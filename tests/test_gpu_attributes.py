"""Trace attributes (DESIGN.md §3 rule 7g, attributes.hip) through the C ABI,
under both launch plans: `Engine.attributes()` is byte for byte, body_off
included, tests/attributes_ref.py applied to the same batch's `points()`,
`scores()`, `traversals()` and `shape()` -- on every case of
tests/shape_cases.py and on hand_attr_zero (tests/attributes_cases.py), each
asserting what it reached; every body parses as JSON.

Then the masks, the switch (mask 15 against mask 0 changes no result and no
byte of the four other fetches), and the interface paths: a repeated fetch, the
device arrays, compact batches, clones, a two-member engine, what ends the
attributes (a JSON batch, a failed call, the next batch), empty batches and
traces without segments, regrown and resumed batches.  Batch shapes follow
tests/test_gpu_shape.py.
"""
import ctypes as C
import json

import numpy as np
import pytest

import attributes_cases
import attributes_ref as ar
import shape_cases
import specref_cases
import traversals_cases
from reporter_amd._lib import ATTR_ALL  # noqa: F401  (no such name before this API)
from test_gpu_shape import _dev_bytes, plan, star  # noqa: F401  (the launch plans' and the star graph's fixtures)

pytestmark = pytest.mark.gpu

ON = dict(matched_points=True, traversals=True, scores=True, shape=True)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    from reporter_amd import synth
    d = tmp_path_factory.mktemp("attributes_gpu")
    out = specref_cases.build(d, synth)
    out.update(traversals_cases.build(d))
    out.update(shape_cases.build(d))
    out.update(attributes_cases.build(d))
    return out


def restate(eng, trace_off, mask=ar.ALL):
    """The restatement on the engine's own records of its last batch -> (bodies, blob, body_off)."""
    pts, scr = eng.points(), eng.scores()
    tv, toff = eng.traversals()
    _, _, spans, toff2, poly, poly_off = eng.shape()
    assert toff.tobytes() == toff2.tobytes()
    bods = ar.bodies(mask, np.asarray(trace_off, np.int64), pts, scr, tv, toff, spans, poly, poly_off)
    return (bods,) + ar.blob(bods)


def check(eng, trace_off, what, mask=ar.ALL):
    """Engine.attributes() against the restatement, exactly.  -> the bodies."""
    got, off = eng.attributes()
    bods, want, want_off = restate(eng, trace_off, mask)
    assert isinstance(got, bytes) and off.dtype == np.int64 and len(off) == len(trace_off), what
    assert list(off) == list(want_off), what + " body_off"
    for t, b in enumerate(bods):
        assert got[off[t]:off[t + 1]] == b.encode("ascii"), "%s trace %d" % (what, t)
    assert got == want and len(got) == off[-1], what
    for b in bods:
        json.loads(b)
    return bods


@pytest.mark.parametrize("name", attributes_cases.ALL)
def test_case_against_restatement(cases, plan, name):
    from reporter_amd import Engine
    graph, batch, meili, _ = cases[name]
    with Engine(graph_path=graph, attributes=15, **ON, **meili) as eng:
        assert eng.attributes_info() == 15
        eng.match(batch)
        bods = check(eng, batch["trace_off"], name)
        pts, (tv, toff) = eng.points(), eng.traversals()
    text = "".join(bods)
    npts, ntrav = np.diff(batch["trace_off"]), np.diff(toff)
    print(name, "bodies:", len(bods), "bytes:", len(text), "longest:", max(map(len, bods)))
    # what the case is here for (tests/attributes_cases.py, tests/shape_cases.py, tests/specref_cases.py)
    if name == "hand_attr_zero":
        attributes_cases.assert_zero_reached(bods)
    if name in ("hand_shape", "hand_attr_zero", "stop_and_go", "seg_forms"):
        assert '"margin":null' in text
    if name == "hand_shape":
        assert ntrav[3] >= 65 and bods[3].count('{"id":') == ntrav[3]
    if name == "hand_many_short":
        assert ntrav.max() >= 65
    if name in ("stop_and_go", "seg_forms", "city_5s"):
        fl = pts["flags"]
        assert '{"type":"unmatched"' in text and ((fl & 1) == 0).any()
        assert text.count('"type":"interpolated"') == int((((fl & 1) != 0) & ((fl & 2) == 0)).sum())
        assert (fl & 16).any() and (fl & 64).any()                  # OTM_PT_ROUTE and OTM_PT_SAME_EDGE
    if name in ("stop_and_go", "seg_forms", "city_5s", "gaps_240s"):
        assert "\\\\" in text                                      # a polyline byte 92, doubled
    if name == "seg_forms":
        t = int(np.argmax(npts))
        assert npts[t] >= 257 and len(bods[t]) > 65536 and bods[t].count('"type":') == npts[t]


MASK_CASES = ["hand_shape", "stop_and_go"]


@pytest.mark.parametrize("name", MASK_CASES)
def test_masks(cases, plan, name):
    from reporter_amd import Engine, _lib
    graph, batch, meili, _ = cases[name]
    assert {8, 4, 5} <= set(ar.VALID_MASKS)                         # SHAPE alone, EDGES without SHAPE
    with Engine(graph_path=graph, **ON, **meili) as eng:
        for mask in ar.VALID_MASKS:
            eng.set_attributes(mask)
            assert eng.attributes_info() == mask
            eng.match(batch)
            bods = check(eng, batch["trace_off"], "%s mask %d" % (name, mask), mask)
            assert ('"shape":"' in bods[0]) == bool(mask & 8) and ('"edges":[' in bods[0]) == bool(mask & 4)
            for bad in ar.INVALID_MASKS:
                assert _lib.lib().otm_set_attributes(eng.h, bad) == -1 and "trace attributes" in _lib.last_error()
                assert eng.attributes_info() == mask


def test_mask_bits_run_their_kernels_alone(cases, plan):
    """With the four other switches off, the mask's bits run what they need; the other fetches stay off."""
    from reporter_amd import Engine, OtmError
    graph, batch, meili, _ = cases["stop_and_go"]
    with Engine(graph_path=graph, attributes=True, **ON, **meili) as eng:
        eng.match(batch)
        want = {15: eng.attributes()}
        for mask in (1, 4, 8):
            eng.set_attributes(mask)
            eng.match(batch)
            want[mask] = eng.attributes()
    for mask in (15, 1, 4, 8):
        with Engine(graph_path=graph, attributes=mask, **meili) as eng:
            eng.match(batch)
            got = eng.attributes()
            assert got[0] == want[mask][0] and got[1].tobytes() == want[mask][1].tobytes(), mask
            for fetch in (eng.points, eng.scores, eng.traversals, eng.shape):
                with pytest.raises(OtmError, match="off"):
                    fetch()
            eng.set_points(True)
            eng.set_traversals(True)
            with pytest.raises(OtmError, match="no batch"):
                eng.points()                                    # the batch ran with their switches off
            with pytest.raises(OtmError, match="no batch"):
                eng.traversals()


def test_mask_changed_between_batch_and_first_fetch(cases, plan):
    """The bodies are the batch's mask's, whatever the handle's mask is at the first call: with the other
    switches off only that mask's kernels wrote their arrays."""
    from reporter_amd import Engine, OtmError, _lib
    graph, batch, meili, _ = cases["stop_and_go"]
    want = {}
    for mask in (1, 3, 15):
        with Engine(graph_path=graph, attributes=mask, **meili) as eng:
            eng.match(batch)
            want[mask] = eng.attributes()
    assert len({w[0] for w in want.values()}) == 3
    for ran, later in ((1, 3), (1, 5), (1, 9), (1, 13), (1, 15), (3, 15), (15, 1), (15, 8), (3, 1)):
        with Engine(graph_path=graph, attributes=ran, **meili) as eng:
            eng.match(batch)
            eng.set_attributes(later)                           # before the first size, fetch or device call
            assert eng.attributes_info() == later
            got = eng.attributes()
            assert _same(got, want[ran]), (ran, later)
            assert eng.attributes_device()[3] == len(want[ran][0])
            eng.set_attributes(0)
            with pytest.raises(OtmError, match="off"):
                eng.attributes()
            eng.set_attributes(later)
            assert _same(eng.attributes(), want[ran]), (ran, later)  # still the batch's
            eng.match(batch)                                    # the next batch runs with the new mask
            if later in want:
                assert _same(eng.attributes(), want[later]), (ran, later)
            # NULL out-parameters on a live handle
            assert _lib.lib().otm_attributes_info(eng.h, None) == -1 and "NULL" in _lib.last_error()
            nb = C.c_int64()
            assert _lib.lib().otm_attributes_size(eng.h, None, C.byref(nb)) == -1 and "NULL" in _lib.last_error()


# ------------------------------------------------------------------ the switch
def test_off_by_default_and_changes_nothing_else(cases, plan, results_equal):
    from reporter_amd import Engine, OtmError, _lib
    graph, batch, meili, _ = cases["stop_and_go"]
    with Engine(graph_path=graph, **ON, **meili) as eng:
        assert eng.attributes_info() == 0
        plain = eng.match(batch)
        with pytest.raises(OtmError, match="off"):
            eng.attributes()
        with pytest.raises(OtmError, match="off"):
            eng.attributes_device()
        nb = C.c_int64()
        assert _lib.lib().otm_fetch_attributes(eng.h, None, 0, None, C.byref(nb)) == -1 and "off" in _lib.last_error()
        other = [eng.points().tobytes(), eng.scores().tobytes()] + [x.tobytes() for x in eng.traversals()] + [
            x if isinstance(x, bytes) else x.tobytes() for x in eng.shape()]
        eng.set_attributes(15)
        with pytest.raises(OtmError, match="no batch"):
            eng.attributes()                                    # the last batch ran with the mask 0
        res = eng.match(batch)
        blob, off = eng.attributes()
        assert len(blob) > 100000
        # a cap below the byte count: nothing is copied
        buf = np.zeros(len(blob) - 1, np.uint8)
        assert _lib.lib().otm_fetch_attributes(eng.h, buf.ctypes.data, len(buf), None, C.byref(nb)) == -1
        assert "cap" in _lib.last_error() and not buf.any()
        assert _lib.lib().otm_fetch_attributes(eng.h, None, 5, None, C.byref(nb)) == -1 and "NULL" in _lib.last_error()
        with_attr = [eng.points().tobytes(), eng.scores().tobytes()] + [x.tobytes() for x in eng.traversals()] + [
            x if isinstance(x, bytes) else x.tobytes() for x in eng.shape()]
        eng.set_attributes(False)
        with pytest.raises(OtmError, match="off"):
            eng.attributes()
    results_equal(plain, res, "attributes on")
    for key in ("traces", "segments", "reports", "way_ids"):
        assert getattr(res, key).tobytes() == getattr(plain, key).tobytes(), key
    assert with_attr == other


# ------------------------------------------------------------------ life cycle
def _same(a, b):
    return a[0] == b[0] and a[1].dtype == b[1].dtype and a[1].tobytes() == b[1].tobytes()


def test_compact_clone_device_and_members_agree(cases, plan):
    from reporter_amd import Engine, OtmError
    graph, batch, meili, _ = cases["stop_and_go"]    # whole-second times: a compact batch carries them
    nt = len(batch["trace_off"]) - 1
    with Engine(graph_path=graph, attributes=15, **meili) as eng:
        eng.match(batch)
        base = eng.attributes()
        assert _same(eng.attributes(), base)                               # a second fetch: the same bytes
        dev, doff, n_traces, n_bytes = eng.attributes_device()
        assert (n_traces, n_bytes) == (nt, len(base[0])) and dev and doff and n_bytes > 100000
        assert _dev_bytes(dev, n_bytes) == base[0] and _dev_bytes(doff, (nt + 1) * 8) == base[1].tobytes()
        assert _same(eng.attributes(), base)
        eng.match_compact(batch)
        assert _same(eng.attributes(), base)
        cl = eng.clone()
        try:
            assert cl.attributes_info() == 15 and cl.points_info() is False    # inherited when it was made
            cl.match(batch)
            assert _same(cl.attributes(), base)
        finally:
            cl.close()
        eng.set_attributes(5)
        cl = eng.clone()
        try:
            assert cl.attributes_info() == 5
        finally:
            cl.close()
    with Engine(graph_path=graph, devices=[0, 0], attributes=15, **meili) as grp:
        assert grp.members() == 2 and grp.attributes_info() == 15 and grp.member(1).attributes_info() == 15
        with pytest.raises(OtmError, match="no batch"):
            grp.attributes()
        res = grp.match(batch)
        assert len(res.traces) == nt
        for _ in range(2):
            assert _same(grp.attributes(), base)
        with pytest.raises(OtmError, match="member"):
            grp.attributes_device()
        with pytest.raises(OtmError, match="off"):
            grp.points()
        # a member view answers for its own share of the group's batch
        parts = [grp.member(i).attributes() for i in range(2)]
        assert sum(len(p[1]) - 1 for p in parts) == nt and min(len(p[1]) for p in parts) > 1
        assert sorted(base[0][base[1][t]:base[1][t + 1]] for t in range(nt)) == sorted(
            p[0][p[1][t]:p[1][t + 1]] for p in parts for t in range(len(p[1]) - 1))
        grp.set_attributes(0)
        assert grp.member(0).attributes_info() == 0


def test_what_ends_the_attributes(cases, plan):
    """A JSON batch, a failed call and the next batch each end them: never another batch's bodies."""
    from reporter_amd import Engine, OtmError, encode_request
    graph, batch, meili, _ = cases["stop_and_go"]
    off = batch["trace_off"]
    small = {k: (batch[k][:off[2]] if k != "trace_off" else off[:3]) for k in batch}
    other = {k: (batch[k][off[2]:off[5]] if k != "trace_off" else off[2:6] - off[2]) for k in batch}
    body = encode_request("veh0", batch["lat"][off[5]:off[6]], batch["lon"][off[5]:off[6]],
                          batch["time"][off[5]:off[6]].astype(np.int64),
                          batch["accuracy"][off[5]:off[6]].astype(np.int32))
    with Engine(graph_path=graph, attributes=15, **ON, **meili) as eng:
        eng.match(small)
        first = eng.attributes()
        assert len(first[1]) == 3 and len(first[0]) > 1000
        eng.match_json(body)
        with pytest.raises(OtmError, match="no batch"):
            eng.attributes()
        with pytest.raises(OtmError, match="no batch"):
            eng.attributes_device()
        eng.match(small)
        assert _same(eng.attributes(), first)
        assert len(eng.report_batch([body])) == 1
        with pytest.raises(OtmError, match="no batch"):
            eng.attributes()
        eng.match(small)
        assert _same(eng.attributes(), first)
        # a call that fails: offsets that run backwards
        bad = dict(small, trace_off=np.array([0, int(off[2]), int(off[1])], np.int64))
        with pytest.raises(OtmError):
            eng.match(bad)
        with pytest.raises(OtmError, match="no batch"):
            eng.attributes()
        # a call that its arguments fail: a NULL batch
        from reporter_amd import _lib
        eng.match(small)
        assert _same(eng.attributes(), first)
        r = _lib.Results()
        assert _lib.lib().otm_match_soa(eng.h, None, C.byref(r)) == -1
        with pytest.raises(OtmError, match="no batch"):
            eng.attributes()
        # the next batch: its own bodies
        eng.match(small)
        assert _same(eng.attributes(), first)
        eng.match(other)
        nxt = check(eng, other["trace_off"], "the next batch")
        assert len(nxt) == 3 and eng.attributes()[0] != first[0]


def test_empty_batches_and_traces_without_segments(star, plan, monkeypatch):
    from reporter_amd import Engine
    from test_gpu_traversals import _mixed_star_batch
    monkeypatch.setenv("OTM_CAND_MAX_LOG2", "0")    # no candidate HBM tier: a probe that needs it fails its trace
    meili = dict(search_radius=20.0, max_search_radius=20.0)
    b = _mixed_star_batch()
    empty = dict(trace_off=np.zeros(1, np.int64), lat=np.zeros(0, np.float32), lon=np.zeros(0, np.float32),
                 time=np.zeros(0), accuracy=np.zeros(0, np.float32))
    o = b["trace_off"]
    none = {k: (b[k][o[4]:o[6]] if k != "trace_off" else o[4:7] - o[4]) for k in b}
    with Engine(graph_path=star, attributes=15, **ON, **meili) as eng:
        eng.match(empty)
        blob, off = eng.attributes()
        assert blob == b"" and list(off) == [0]
        assert eng.attributes_device()[2:] == (0, 0)
        eng.match(none)
        bods = check(eng, none["trace_off"], "no segments")
        assert len(bods) == 2 and all(x.endswith('],"edges":[],"shape":""}') for x in bods)
        res = eng.match(b)
        assert list(res.traces["code"][:4]) == [500, 500, 500, 200]
        bods = check(eng, b["trace_off"], "mixed star")
    for t in (0, 1, 2, 4, 5):
        assert bods[t].endswith('],"edges":[],"shape":""}'), t
        if t < 3:                                               # answered 500: every point unmatched, none scored
            assert '"type":"matched"' not in bods[t] and '"score"' not in bods[t] and '"unmatched"' in bods[t]
    assert '{"id":' in bods[3] and '{"id":' in bods[6]
    for mask, text in ((4, '{"edges":[]}'), (8, '{"shape":""}'), (12, '{"edges":[],"shape":""}')):
        with Engine(graph_path=star, attributes=mask, **meili) as eng:
            eng.match(none)
            blob, off = eng.attributes()
            assert blob == text.encode("ascii") * 2 and list(off) == [0, len(text), 2 * len(text)]


def test_regrown_and_resumed_batches(cases, star, plan, monkeypatch):
    from reporter_amd import Engine
    from test_no_limits import RADIUS_100, star_batch
    # a tier's tables grown on demand: the first batch resumes at the candidate HBM tier, the second runs clean
    b = star_batch()
    with Engine(graph_path=star, attributes=15, **RADIUS_100) as eng:
        eng.match(b)
        first, st1 = eng.attributes(), eng.spill_stats()
        eng.match(b)
        clean, st2 = eng.attributes(), eng.spill_stats()
    assert st1["attempts"] >= 2 and st1["resumed"] >= 1 and st2["attempts"] == 1
    assert len(clean[0]) > 1000 and _same(first, clean)
    # tiny pinned capacities: the transition matrices and the path pool overflow and the batch is redone whole
    graph, batch, meili, _ = cases["stop_and_go"]
    with Engine(graph_path=graph, attributes=15, **meili) as eng:
        eng.match(batch)
        want = eng.attributes()
    monkeypatch.setenv("OTM_TRANS_CAP", "64")
    monkeypatch.setenv("OTM_POOL_CAP", "8")
    with Engine(graph_path=graph, attributes=15, **meili) as eng:
        eng.match(batch)
        got, st = eng.attributes(), eng.spill_stats()
    assert st["attempts"] >= 2
    assert _same(got, want)
