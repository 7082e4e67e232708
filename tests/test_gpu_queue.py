"""k_queue (DESIGN.md §3 rule 7b) through the C ABI: the hand roads of
tests/queue_cases.py against closed-form expectations, with no exclusion; a
long trace, batch shapes, unsorted times and the 1.5 km city against the
independent float64 reference (tests/queue_ref.py) run on the engine's own
stage arrays; every other field against the oracle, which stays at 0; and the
interface paths that carry the field (/report bodies, compact batches, clones,
multi-device engines).
"""
import json

import numpy as np
import numpy.testing as npt
import pytest

import queue_cases as qc
import queue_ref as qr

pytestmark = pytest.mark.gpu

_CASES = dict(qc.hand_cases(), multi_edge=qc.multi_case(), chain_break=qc.break_case())


@pytest.fixture(scope="module")
def roads(tmp_path_factory):
    return qc.graphs(tmp_path_factory.mktemp("queue_gpu"))


@pytest.fixture(scope="module")
def engines(roads):
    """One engine per hand road, threshold on; closed at module end."""
    from reporter_amd import Engine
    made = {}

    def get(key):
        if key not in made:
            made[key] = Engine(graph_path=roads[key], queue_speed_kph=qc.KPH)
        return made[key]

    yield get
    for e in made.values():
        e.close()


def _stages(eng):
    return {k: eng.debug(k) for k in ("state", "is_col", "route_dist", "ipos", "chain_start")}


def _ref(eng, b, res, v):
    return qr.queue_lengths(b, _stages(eng), res.traces, res.segments, v)


def _equal_but_queue(orc, res, what=""):
    """Every field other than queue_length equals the oracle's (run at its unchanged default)."""
    for f in orc["traces"].dtype.names:
        npt.assert_array_equal(orc["traces"][f], res.traces[f], err_msg="%s traces.%s" % (what, f))
    for key, got in (("segments", res.segments), ("reports", res.reports)):
        assert len(orc[key]) == len(got), "%s %s count" % (what, key)
        for f in got.dtype.names:
            if f != "queue_length":
                npt.assert_array_equal(orc[key][f], got[f], err_msg="%s %s.%s" % (what, key, f))
    npt.assert_array_equal(orc["way_ids"], res.way_ids, err_msg="%s way_ids" % what)


def _by_id(segs):
    return {int(i): int(v) for i, v in zip(segs["segment_id"], segs["queue_length"]) if v}


def _check_reports(res):
    """k_report copies the prior segment's value into its report."""
    sq = {(int(s["segment_id"]), float(s["start_time"])): int(s["queue_length"]) for s in res.segments}
    for r in res.reports:
        assert int(r["queue_length"]) == sq[(int(r["id"]), float(r["t0"]))]


# ------------------------------------------------------------------ hand roads
def test_off_by_default(roads, oracle, results_equal):
    from reporter_amd import Engine
    b = qc.batch([qc.hand_cases()["queue_1s"][1]])
    with Engine(graph_path=roads["road"]) as eng:
        res = eng.match(b)
        assert eng.queue_info() == 0.0
    assert len(res.segments) == 5
    assert (res.segments["queue_length"] == 0).all() and (res.reports["queue_length"] == 0).all()
    results_equal(oracle.match_batch(oracle.Graph(roads["road"]), b), res, "off")
    with Engine(graph_path=roads["road"], queue_speed_kph=0) as eng:
        assert not eng.match(b).segments["queue_length"].any()


@pytest.mark.parametrize("name", sorted(_CASES))
def test_hand_case(roads, engines, oracle, name):
    gk, tr, want = _CASES[name]
    b = qc.batch([tr])
    eng = engines(gk)
    res = eng.match(b)
    q, bnd, _ = _ref(eng, b, res, qc.KPH)
    got = _by_id(res.segments)
    print(name, "queue_length by segment:", got, "expected:", want)
    assert not bnd.any()   # no exclusion on the hand roads
    assert got == want
    npt.assert_array_equal(res.segments["queue_length"], q)
    _equal_but_queue(oracle.match_batch(oracle.Graph(roads[gk]), b), res, name)
    _check_reports(res)
    if name == "queue_1s":
        assert want == {16: 80}
        rep = res.reports[res.reports["id"] == 16]
        assert len(rep) == 1 and rep["queue_length"][0] == 80
    if name == "incomplete":
        assert res.segments["length"][0] == -1 and res.segments["length"][-1] == -1
        assert res.segments["queue_length"][0] == 0 and res.segments["queue_length"][-1] == 0
    if name == "whole_slow":
        s = res.segments[res.segments["segment_id"] == 16]
        assert s["queue_length"][0] == s["length"][0]
    if name == "chain_break":
        # both chains' segments at the break are incomplete, and stay 0
        for sid in (24, 72):
            s = res.segments[res.segments["segment_id"] == sid]
            assert len(s) == 1 and s["length"][0] == -1 and s["queue_length"][0] == 0
        assert eng.debug("chain_start").sum() == 2


def test_lane_striding_and_trace_length(roads, engines, oracle):
    gk, tr, _ = qc.fine_case()
    b = qc.batch([tr])
    eng = engines(gk)
    res = eng.match(b)
    assert len(tr) > 128 and len(res.segments) > 64
    q, bnd, dis = _ref(eng, b, res, qc.KPH)
    assert not bnd.any()
    nz = np.nonzero(q)[0]
    assert len(nz) >= 6 and (np.diff(nz) > 5).sum() == 2 and nz.max() >= 64   # three stretches, past lane 63
    npt.assert_array_equal(res.segments["queue_length"], q)
    _equal_but_queue(oracle.match_batch(oracle.Graph(roads[gk]), b), res, "fine")
    _check_reports(res)


def test_batch_shapes(roads, engines):
    eng = engines("road")
    empty = dict(trace_off=np.zeros(1, np.int64), lat=np.zeros(0, np.float32), lon=np.zeros(0, np.float32),
                 time=np.zeros(0), accuracy=np.zeros(0, np.float32))
    r = eng.match(empty)
    assert len(r.traces) == 0 and len(r.segments) == 0
    q1 = qc.hand_cases()["queue_1s"][1]
    alone = eng.match(qc.batch([q1]))
    b = qc.batch([[(100.0, qc.T0)], qc.drive(100.0, [(5, 15.0, 1.0)]), qc.zero_duration_trace(), q1])
    b["lat"][1:7] = 41.0   # trace 1: a hundred kilometres off the graph
    res = eng.match(b)
    assert list(res.traces["code"][[0, 2, 3]]) == [200, 500, 200]
    assert res.traces["seg_cnt"][0] == 0 and res.traces["seg_cnt"][1] == 0
    mine = res.segments[res.traces["seg_off"][3]:]
    assert len(mine) == res.traces["seg_cnt"][3] == len(alone.segments)
    npt.assert_array_equal(mine["queue_length"], alone.segments["queue_length"])
    assert _by_id(mine) == {16: 80}
    q, bnd, _ = _ref(eng, b, res, qc.KPH)
    assert not bnd.any()
    npt.assert_array_equal(res.segments["queue_length"], q)


@pytest.mark.parametrize("swap", [(45, 46), (60, 72), (28, 33)])
def test_unsorted_times(roads, engines, swap):
    tr = list(qc.hand_cases()["queue_1s"][1])
    i, j = swap
    tr[i], tr[j] = (tr[i][0], tr[j][1]), (tr[j][0], tr[i][1])
    b = qc.batch([tr])
    eng = engines("road")
    res = eng.match(b)   # the call returns
    q, bnd, _ = _ref(eng, b, res, qc.KPH)
    print("unsorted", swap, "queue_length", list(res.segments["queue_length"]), "reference", list(q), "excluded", bnd.sum())
    keep = ~bnd
    npt.assert_array_equal(res.segments["queue_length"][keep], q[keep])


# ------------------------------------------------------------------ interface paths
def _json_body(tr, uuid="veh"):
    return json.dumps({"uuid": uuid, "trace": [{"lat": qc.LAT, "lon": float(qc.lon_of(x)), "time": int(t),
                                                "accuracy": 5} for x, t in tr]})


def test_report_bodies_carry_the_value(roads, engines):
    eng = engines("road")
    body = _json_body(qc.hand_cases()["queue_1s"][1])
    for code, out in (eng.report(body), eng.report_batch([body])[0]):
        assert code == 200
        seg = out[out.index('"segment_id":16'):]
        assert '"queue_length":80' in seg[:seg.index("}")]
        rep = out[out.index('"reports":['):]
        rep = rep[rep.index('"id":16'):]
        assert '"queue_length":80' in rep[:rep.index("}")]
        d = json.loads(out)
        assert [s["queue_length"] for s in d["segment_matcher"]["segments"]] == [0, 80, 0, 0, 0]
        assert {r["id"]: r["queue_length"] for r in d["datastore"]["reports"]}[16] == 80


def test_compact_clone_and_members_agree(roads, engines):
    from reporter_amd import Engine
    c = qc.hand_cases()
    names = ("queue_1s", "incomplete", "queue_states", "whole_slow")   # whole-second times: compact batches carry those
    b = qc.batch([c[k][1] for k in names])
    eng = engines("road")
    assert eng.queue_info() == 10.0
    base = eng.match(b)
    assert [_by_id(base.segments[o:o + n]) for o, n in zip(base.traces["seg_off"], base.traces["seg_cnt"])] == \
        [c[k][2] for k in names]

    def same(res, what):
        for key in ("traces", "segments", "reports", "way_ids"):
            assert getattr(res, key).tobytes() == getattr(base, key).tobytes(), "%s %s" % (what, key)

    same(eng.match_compact(b), "match_compact")
    cl = eng.clone()
    try:
        assert cl.queue_info() == 10.0
        same(cl.match(b), "clone")
    finally:
        cl.close()
    with Engine(graph_path=roads["road"], devices=[0, 0], queue_speed_kph=qc.KPH) as grp:
        assert grp.members() == 2 and grp.queue_info() == 10.0
        assert grp.member(1).queue_info() == 10.0
        same(grp.match(b), "two members")


# ------------------------------------------------------------------ the city, stage-isolated
@pytest.fixture(scope="module")
def city(tmp_path_factory):
    from reporter_amd import synth
    g = synth.make_graph(str(tmp_path_factory.mktemp("queue_city_gpu") / "city.otmg"), width_m=1500, height_m=1500)
    return g, qc.city_batch(synth, g)


@pytest.fixture(scope="module")
def city_oracle(city, oracle):
    g, b = city
    return oracle.match_batch(oracle.Graph(g), b, nthreads=4)


@pytest.mark.parametrize("plan", ["large", "small"])
def test_city_against_reference(city, city_oracle, monkeypatch, plan):
    """Both launch plans, selected as tests/test_gpu_specref.py selects them."""
    from reporter_amd import Engine
    monkeypatch.setenv("OTM_SMALL_POINTS", "0" if plan == "large" else str(1 << 40))
    g, b = city
    with Engine(graph_path=g, queue_speed_kph=qc.CITY_KPH) as eng:
        assert eng.queue_info() == 20.0
        res = eng.match(b)
        q, bnd, dis = _ref(eng, b, res, qc.CITY_KPH)
    s = res.segments
    complete = (s["segment_id"] >= 0) & (s["length"] >= 0)
    print("city", plan, "segments", len(s), "complete", complete.sum(), "excluded", (bnd & complete).sum(),
          "non-zero", (q > 0).sum(), "discharge", (dis & (q > 0)).sum())
    assert (bnd & complete).sum() <= 0.01 * complete.sum()
    assert (q > 0).sum() >= 20
    assert (dis & (q > 0)).sum() >= 5
    _equal_but_queue(city_oracle, res, "city " + plan)
    keep = ~bnd
    npt.assert_array_equal(s["queue_length"][keep], q[keep])
    assert not s["queue_length"][~complete].any()
    _check_reports(res)
