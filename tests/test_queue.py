"""queue_length (DESIGN.md §3 rule 7b) where no GPU exists: the config key
through the C ABI, and the Python reference of the rule (tests/queue_ref.py)
pinned by hand -- on interval lists written out here, and on the CPU oracle's
stage arrays of the hand roads of tests/queue_cases.py (the kernels' stage
arrays are bit-identical to those, so the reference that tests/test_gpu_queue.py
compares the kernel with is itself checked against closed-form numbers here).
"""
import ctypes as C
import json

import numpy as np
import pytest

import queue_cases as qc
import queue_ref as qr


# ------------------------------------------------------------------ config key
def _config_queue(tmp_path, text):
    from reporter_amd import _lib
    p = tmp_path / "cfg.json"
    p.write_text(text)
    k = C.c_float(-7.0)
    rc = _lib.lib().otm_config_queue(str(p).encode(), C.byref(k))
    return rc, k.value, _lib.last_error()


@pytest.mark.parametrize("otm, want", [('{"graph":"g.otmg","queue_speed_kph":12.5}', 12.5),
                                       ('{"graph":"g.otmg","queue_speed_kph":0}', 0.0),
                                       ('{"graph":"g.otmg","queue_speed_kph":20}', 20.0),
                                       ('{"graph":"g.otmg"}', 0.0)])
def test_config_queue_accepts(tmp_path, otm, want):
    rc, k, err = _config_queue(tmp_path, '{"otm":%s,"meili":{"default":{}}}' % otm)
    assert rc == 0, err
    assert k == want


@pytest.mark.parametrize("v", ["-1", '"x"', "NaN", "Infinity", "-Infinity", "true", "[10]", "1e60"])
def test_config_queue_rejects(tmp_path, v):
    from reporter_amd import _lib
    rc, _, err = _config_queue(tmp_path, '{"otm":{"graph":"g.otmg","queue_speed_kph":%s}}' % v)
    assert rc == -1  # OTM_EINVAL
    assert "queue_speed_kph" in err


def test_write_config_names_the_key(tmp_path):
    # a named parameter: **meili must not swallow it into the meili section
    from reporter_amd.engine import write_config
    p = write_config(str(tmp_path / "c.json"), "g.otmg", queue_speed_kph=12.5, sigma_z=4.0)
    cfg = json.load(open(p))
    assert cfg["otm"]["queue_speed_kph"] == 12.5
    assert cfg["meili"]["default"] == {"sigma_z": 4.0}
    assert "queue_speed_kph" not in json.load(open(write_config(str(tmp_path / "d.json"), "g.otmg")))["otm"]


# ------------------------------------------------------------------ the reference on written-out intervals
def _seg(lo, hi, t0, t1, length=100, sid=8):
    return dict(segment_id=sid, length=length, start_time=t0, end_time=t1, begin_shape_index=lo, end_shape_index=hi)


V = 10.0  # km/h: slow is less than 2.78 m per second


def test_ref_trailing_slow_run_and_time_clip():
    # (first anchor, d, t_prev, t_next): fast, slow, slow, slow; the segment ends midway through the last
    iv = [(0, 15.0, 0.0, 1.0), (1, 2.0, 1.0, 2.0), (2, 2.0, 2.0, 3.0), (3, 2.0, 3.0, 4.0)]
    assert qr.segment_queue(iv, _seg(0, 3, 0.0, 3.5), V) == (5, False, False)   # 2 + 2 + 2 * 0.5
    # ... and starts midway through the first slow one (the clip at start_time)
    assert qr.segment_queue(iv, _seg(1, 3, 1.75, 4.0), V) == (5, True, False)   # 0.5 + 2 + 2 = 4.5 -> 5, on k + 0.5
    assert qr.segment_queue(iv, _seg(1, 3, 1.8, 4.0), V)[0] == 4                # 0.4 + 2 + 2
    # the cap at length
    assert qr.segment_queue(iv, _seg(0, 3, 0.0, 4.0, length=4), V)[0] == 4


def test_ref_discharge_and_its_limits():
    slow, fast = (2.0, 1.0), (15.0, 1.0)

    def ivs(kinds):
        return [(i, d, float(i), float(i) + dt) for i, (d, dt) in enumerate(kinds)]

    # the last interval fast, the one before slow: the discharge piece counts
    assert qr.segment_queue(ivs([fast, slow, slow, fast]), _seg(0, 3, 0.0, 4.0), V) == (19, False, True)
    # two fast ones at the end: no queue at the segment's end
    assert qr.segment_queue(ivs([slow, slow, fast, fast]), _seg(0, 3, 0.0, 4.0), V) == (0, False, False)
    # a single fast interval
    assert qr.segment_queue(ivs([fast]), _seg(0, 0, 0.0, 1.0), V) == (0, False, False)
    # stays (d = 0, dt > 0) are slow and continue a run
    stay = (0.0, 5.0)
    assert qr.segment_queue(ivs([fast, slow, stay, stay, slow]), _seg(0, 4, 0.0, 20.0), V)[0] == 4


def test_ref_ignored_and_run_ending_intervals():
    # an interval of no duration inside the range has no share (c <= 0): ignored, the run goes on
    iv = [(0, 2.0, 0.0, 1.0), (1, 2.0, 1.0, 1.0), (2, 2.0, 1.0, 2.0)]
    assert qr.segment_queue(iv, _seg(0, 2, 0.0, 2.0), V)[0] == 4
    # intervals outside [begin_shape_index, end_shape_index] do not count
    iv = [(0, 2.0, 0.0, 1.0), (1, 2.0, 1.0, 2.0), (2, 2.0, 2.0, 3.0)]
    assert qr.segment_queue(iv, _seg(1, 1, 0.0, 3.0), V)[0] == 2
    # no segment id, or an incomplete segment: 0
    assert qr.segment_queue(iv, _seg(0, 2, 0.0, 3.0, sid=-1), V)[0] == 0
    assert qr.segment_queue(iv, _seg(0, 2, 0.0, 3.0, length=-1), V)[0] == 0


def test_ref_boundaries_are_flagged():
    # exactly at the threshold: 10 km/h = 25 m in 9 s
    assert qr.segment_queue([(0, 25.0, 0.0, 9.0)], _seg(0, 0, 0.0, 9.0), V)[1]
    # the sum on k + 0.5
    assert qr.segment_queue([(0, 2.5, 0.0, 1.0)], _seg(0, 0, 0.0, 1.0), V) == (3, True, False)
    assert not qr.segment_queue([(0, 2.2, 0.0, 1.0)], _seg(0, 0, 0.0, 1.0), V)[1]


def test_ref_anchors_of_a_step():
    # one trace: states 0 and 4, between them ipos 3, 2 (behind: no anchor), -1 (unplaced); a new chain at 5
    state = np.array([0, -1, -1, -1, 0, 0, 0], np.int32)
    ipos = np.array([-1, 3.0, 2.0, -1, -1, -1, -1], np.float32)
    rd = np.array([0, 0, 0, 0, 10.0, 99.0, 7.0], np.float32)
    cs = np.array([1, 0, 0, 0, 0, 1, 0], np.uint8)
    tm = np.arange(7.0)
    iv = qr.trace_intervals(0, 7, tm, state, state >= 0, cs, rd, ipos)
    assert iv == [(0, 3.0, 0.0, 1.0), (1, 7.0, 1.0, 4.0), (5, 7.0, 5.0, 6.0)]


# ------------------------------------------------------------------ the reference on the oracle's stage arrays
@pytest.fixture(scope="module")
def roads(tmp_path_factory):
    return qc.graphs(tmp_path_factory.mktemp("queue"))


_CASES = dict(qc.hand_cases(), multi_edge=qc.multi_case(), chain_break=qc.break_case())


def _oracle_queue(oracle, graph, b, v):
    r = oracle.match_batch(oracle.Graph(graph), b, keep_stages=True)
    q, bnd, dis = qr.queue_lengths(b, qr.oracle_stages(b, r), r["traces"], r["segments"], v)
    return r, q, bnd, dis


@pytest.mark.parametrize("name", sorted(_CASES))
def test_reference_gives_the_closed_form_values(roads, oracle, name):
    gk, tr, want = _CASES[name]
    r, q, bnd, _ = _oracle_queue(oracle, roads[gk], qc.batch([tr]), qc.KPH)
    s = r["segments"]
    assert (r["traces"]["code"] == 200).all()
    assert (s["queue_length"] == 0).all()          # the oracle itself stays at 0
    assert not bnd.any()                           # the hand cases allow no exclusion
    got = {int(i): int(v) for i, v in zip(s["segment_id"], q) if v}
    assert got == want
    # off: everything 0
    assert not qr.queue_lengths(qc.batch([tr]), qr.oracle_stages(qc.batch([tr]), r), r["traces"], s, 0.0)[0].any()


def test_hand_cases_reach_what_they_name(roads, oracle):
    c = qc.hand_cases()
    # the 1 s queue: some slow points are placed interpolated points; the queue of states has none
    r = oracle.match_batch(oracle.Graph(roads["road"]), qc.batch([c["queue_1s"][1]]), keep_stages=True)
    assert (r["ipos"] >= 0).sum() > 0
    r = oracle.match_batch(oracle.Graph(roads["road"]), qc.batch([c["queue_states"][1]]), keep_stages=True)
    assert (r["state"] >= 0).all()
    # the discharge case takes the discharge branch
    r, q, _, dis = _oracle_queue(oracle, roads["road"], qc.batch([c["discharge"][1]]), qc.KPH)
    assert dis[r["segments"]["segment_id"] == 16].all()
    # incomplete: first and last segment
    r = oracle.match_batch(oracle.Graph(roads["road"]), qc.batch([c["incomplete"][1]]))
    assert r["segments"]["length"][0] == -1 and r["segments"]["length"][-1] == -1
    # the multi-edge queue is longer than the segment's last edge
    assert qc.multi_case()[2][16] > 345
    # the break: two chains
    gk, tr, _ = qc.break_case()
    b = qc.batch([tr])
    r = oracle.match_batch(oracle.Graph(roads[gk]), b, keep_stages=True)
    assert qr.chain_starts(b["trace_off"], r).sum() == 2


def test_fine_road_case(roads, oracle):
    gk, tr, _ = qc.fine_case()
    r, q, bnd, dis = _oracle_queue(oracle, roads[gk], qc.batch([tr]), qc.KPH)
    assert len(tr) > 128 and len(r["segments"]) > 64
    assert not bnd.any()
    # three slow stretches: queues in three separate groups of segments, beyond lane 63 too
    nz = np.nonzero(q)[0]
    assert len(nz) >= 6 and (np.diff(nz) > 5).sum() == 2 and nz.max() >= 64
    assert dis[nz].any()


def test_city_case_conditions(tmp_path_factory, oracle):
    from reporter_amd import synth
    city = synth.make_graph(str(tmp_path_factory.mktemp("queue_city") / "city.otmg"), width_m=1500, height_m=1500)
    b = qc.city_batch(synth, city)
    r, q, bnd, dis = _oracle_queue(oracle, city, b, qc.CITY_KPH)
    s = r["segments"]
    complete = (s["segment_id"] >= 0) & (s["length"] >= 0)
    assert (bnd & complete).sum() <= 0.01 * complete.sum()
    assert (q > 0).sum() >= 20
    assert (dis & (q > 0)).sum() >= 5
    assert not q[~complete].any()
