"""Matched points (DESIGN.md §3 rule 7c) without a GPU: the float64 reference
of tests/points_ref.py on hand graphs against closed-form answers (the
oracle's stage arrays are its inputs only: the oracle computes no matched
points), the record's layout, the errors that need no device, and the
ambiguity cap of the cases tests/test_gpu_points.py runs.
"""
import ctypes as C
import math

import numpy as np
import pytest

import points_ref as pr
import specref as sr
import specref_cases
from reporter_amd import _lib
from reporter_amd._lib import POINT_DTYPE, MatchedPoint  # noqa: F401  (the record: no such names before this API)

M, COL, NODE, CS, ROUTE, ANCHOR, SAME = (pr.MATCHED, pr.COLUMN, pr.NODE, pr.CHAIN_START, pr.ROUTE, pr.ANCHOR,
                                         pr.SAME_EDGE)
MLAT, MLON, LAT = specref_cases.MLAT, specref_cases.MLON, specref_cases.LAT


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    from reporter_amd import synth
    return specref_cases.build(tmp_path_factory.mktemp("points_cpu"), synth)


def _ref(oracle, graph, batch, meili):
    orc = oracle.match_batch(oracle.Graph(graph), batch, p=oracle.params(**meili), keep_stages=True)
    G, P = sr.Graph(graph), sr.params(**meili)
    return G, pr.matched_points(G, P, batch, pr.oracle_stages(batch, orc), orc["traces"]["code"]), orc


def _xy(G, r, batch, k):
    """Record k's place in the hand graphs' metres (x east, y north), and its distance."""
    la, lo, d = pr.coordinate(G, int(r.edge[k]), float(np.float32(r.off[k])), float(np.float32(batch["lat"][k])),
                              float(np.float32(batch["lon"][k])))
    return lo * MLON, (la - LAT) * MLAT, d


def _probe_xy(batch, k):
    return float(batch["lon"][k]) * MLON, (float(batch["lat"][k]) - LAT) * MLAT


def _edge_from(G, node):
    e = [int(x) for x in np.nonzero(G.efrom == node)[0]]
    assert len(e) == 1
    return e[0]


# ------------------------------------------------------------------ the record and the calls that need no device
def test_record_layout():
    assert C.sizeof(_lib.MatchedPoint) == 40 and C.alignment(_lib.MatchedPoint) == 8
    want = dict(edge=0, flags=4, lat=8, lon=16, offset=24, distance=28, way_id=32)
    assert {n: getattr(_lib.MatchedPoint, n).offset for n, _ in _lib.MatchedPoint._fields_} == want
    assert _lib.POINT_DTYPE.itemsize == 40
    assert {n: _lib.POINT_DTYPE.fields[n][1] for n in _lib.POINT_DTYPE.names} == want
    for n, t in _lib.MatchedPoint._fields_:
        assert getattr(_lib.MatchedPoint, n).offset % C.sizeof(t) == 0          # natural alignment
        assert _lib.POINT_DTYPE.fields[n][0].itemsize == C.sizeof(t)
    assert (_lib.PT_MATCHED, _lib.PT_COLUMN, _lib.PT_NODE, _lib.PT_CHAIN_START, _lib.PT_ROUTE, _lib.PT_ANCHOR,
            _lib.PT_SAME_EDGE) == (1, 2, 4, 8, 16, 32, 64) == (M, COL, NODE, CS, ROUTE, ANCHOR, SAME)
    hdr = open(_lib.os.path.join(_lib._HERE, "..", "include", "otmatch.h")).read()
    for name, v in (("MATCHED", 1), ("COLUMN", 2), ("NODE", 4), ("CHAIN_START", 8), ("ROUTE", 16), ("ANCHOR", 32),
                    ("SAME_EDGE", 64)):
        assert "#define OTM_PT_%s %du" % (name, v) in hdr


def test_null_engine_is_einval():
    L = _lib.lib()
    on, n, p = C.c_int(7), C.c_int64(7), C.c_void_p()
    buf = np.zeros(2, _lib.POINT_DTYPE)
    for rc in (L.otm_set_points(None, 1), L.otm_points_info(None, C.byref(on)),
               L.otm_fetch_points(None, buf.ctypes.data, 2, C.byref(n)), L.otm_fetch_points(None, None, 0, C.byref(n)),
               L.otm_points_device(None, C.byref(p), C.byref(n))):
        assert rc == -1                                     # OTM_EINVAL
        assert "NULL" in _lib.last_error()
    assert (on.value, n.value, p.value) == (7, 7, None) and not buf["flags"].any()


# ------------------------------------------------------------------ the reference against closed-form answers
def test_straight_road(cases, oracle):
    """hand_filter's one-way road east along y = 0 (40 m edges): trace 1 is
    placed at 4.3 m, then 1.7 m (behind: no anchor), then 9.5 m (past the node
    at 40), from q at x = 32."""
    graph, batch, meili, _ = cases["hand_filter"]
    G, r, orc = _ref(oracle, graph, batch, meili)
    assert not r.amb.any()
    a = int(batch["trace_off"][1])
    e0, e1 = _edge_from(G, 0), _edge_from(G, 1)
    want = [(M | COL | CS, e0, 32.0, 1.5), (M | ROUTE | ANCHOR, e0, 36.3, 1.0), (M | ROUTE, e0, 33.7, 1.5),
            (M | ROUTE | ANCHOR, e1, 1.5, 1.0), (M | COL, e1, 14.0, 1.5), (M | COL, _edge_from(G, 2), 15.0, 1.5)]
    for j, (fl, e, off, dist) in enumerate(want):
        k = a + j
        assert (int(r.flags[k]), int(r.edge[k])) == (fl, e), (j, r.flags[k], r.edge[k])
        assert abs(r.off[k] - off) < 0.01, (j, r.off[k])
        x, y, d = _xy(G, r, batch, k)
        # the f32 probe's own metres (a latitude near 40 is quantised to 0.42 m): the foot is straight below it
        x_in, y_in = _probe_xy(batch, k)
        assert abs(x - x_in) < 0.01 and abs(y) < 0.01 and abs(d - abs(y_in)) < 0.01 and abs(d - dist) < 0.25, \
            (j, x, y, d)
        assert r.way[k] == 4000 + (0 if e == e0 else 1 if e == e1 else 2)
    # the rebuilt position is the one ipos names: 4.3, 1.7, 9.5
    for j, pos in ((1, 4.3), (2, 1.7), (3, 9.5)):
        k = a + j
        assert abs(r.xs[k] + (r.off[k] - r.o0[k]) - pos) < 0.01 and abs(float(orc["ipos"][k]) - pos) < 0.01
    # the points no step holds: after the last state (trace 3), around an empty column (trace 4), before a
    # breakage (trace 5); the empty column itself is COLUMN alone
    off = [int(x) for x in batch["trace_off"]]
    assert list(r.flags[off[3] + 3:off[4]]) == [0, 0]
    assert [int(x) for x in r.flags[off[4] + 2:off[4] + 5]] == [0, COL, 0]
    assert list(r.flags[off[5] + 1:off[5] + 3]) == [0, 0]
    assert (r.edge[r.flags & M == 0] == -1).all() and not r.way[r.flags & M == 0].any()
    # p a node candidate at the edge's end (trace 0): NODE, offset 0 on the node's outgoing edge, on the node
    k = off[0] + 3
    assert int(r.flags[k]) == M | COL | NODE and int(r.edge[k]) == e1 and r.off[k] == 0.0
    x, y, d = _xy(G, r, batch, k)
    assert abs(x - 40.0) < 0.01 and abs(y) < 0.01 and d < 1e-6


def test_repeated_shape_point(cases, oracle):
    """hand_curve_interp, trace 1: the point outside the arc at its repeated
    shape point (45 degrees, 3 m out) is put on that vertex, whichever of the
    three shape segments that meet there names it."""
    graph, batch, meili, _ = cases["hand_curve_interp"]
    G, r, _ = _ref(oracle, graph, batch, meili)
    assert not r.amb.any()
    k = int(batch["trace_off"][1]) + 2
    curve = specref_cases.EDGE_IDS["curve"]
    assert int(r.flags[k]) & (M | ROUTE) == M | ROUTE and int(r.edge[k]) == curve
    chord = 2 * 100.0 * math.sin(math.radians(11.25 / 2))
    s0 = int(G.eshape[curve])
    # (the shape's f32 latitudes are quantised to 0.42 m near 40 degrees: the file's own vertex to the millimetre,
    # the drawn arc to a quarter of a metre)
    assert abs(r.off[k] - G.scum[s0 + 4]) < 1e-3 and abs(r.off[k] - 4 * chord) < 0.25
    x, y, d = _xy(G, r, batch, k)
    assert abs(x - float(G.slon[s0 + 4]) * MLON) < 1e-3 and abs(y - (float(G.slat[s0 + 4]) - LAT) * MLAT) < 1e-3
    assert abs(x - 100 * math.sin(math.pi / 4)) < 0.01 and abs(y - (100 - 100 * math.cos(math.pi / 4))) < 0.25
    assert abs(d - math.hypot(x - _probe_xy(batch, k)[0], y - _probe_xy(batch, k)[1])) < 1e-3 and abs(d - 3.0) < 0.25
    # the zero-length shape segment itself: t = 0 by the rule, no division by zero
    la, lo, _ = pr.coordinate(G, curve, float(G.scum[s0 + 4]), LAT, 0.0)
    assert (la, lo) == (float(G.slat[s0 + 4]), float(G.slon[s0 + 4])) and G.scum[s0 + 4] == G.scum[s0 + 5]
    # trace 0: the third point projects behind q on the arc, so it is placed far ahead, on `north` (22.5 m along
    # the route); the two after it (3.8 and 7.9 m) lie behind that maximum: ROUTE without ANCHOR
    a = int(batch["trace_off"][0])
    assert [int(x) for x in r.flags[a:a + 7]] == [M | COL | CS, M | COL, M | ROUTE | ANCHOR, M | ROUTE, M | ROUTE,
                                                  M | COL, M | COL]
    assert int(r.edge[a + 2]) == specref_cases.EDGE_IDS["north"] and int(r.edge[a + 3]) == curve


def test_node_candidate(cases, oracle):
    """hand_short_edges, trace 2: q exactly on the node at 60 m -- a node
    candidate, carried as the node's first outgoing edge (s1) at offset 0."""
    graph, batch, meili, _ = cases["hand_short_edges"]
    G, r, _ = _ref(oracle, graph, batch, meili)
    assert not r.amb.any()
    k = int(batch["trace_off"][2]) + 1
    ids = specref_cases.SHORT_IDS
    assert int(r.flags[k]) == M | COL | NODE and int(r.edge[k]) == ids["s1"] and r.off[k] == 0.0 and r.way[k] == 2001
    x, y, d = _xy(G, r, batch, k)
    assert abs(x - 60.0) < 0.01 and abs(y) < 0.01 and d < 1e-6
    # the points after it lie on s1, s2 and s3: middle pieces of the route, each 1.5 m into its 3 m edge
    for j, nm in ((2, "s1"), (3, "s2"), (4, "s3")):
        assert int(r.edge[k + j - 1]) == ids[nm] and abs(r.off[k + j - 1] - 1.5) < 0.01
        assert int(r.flags[k + j - 1]) == M | ROUTE | ANCHOR


def _road_batch(traces):
    return specref_cases._xy(traces, dt=2.0)


def test_same_edge_forward_run_and_stay(cases, oracle):
    """On the straight road: a forward run along one edge (feet at 8 and 12 m
    between the states at 5 and 30, and one behind q clamped to q's offset),
    and a stay (p 13 m behind q: a foot between them, one past q clamped)."""
    graph, _, meili, _ = cases["hand_filter"]
    b = _road_batch([[(5.0, 1.5), (8.0, 1.0), (12.0, -1.5), (3.0, 1.0), (30.0, 1.5)],
                     [(28.0, 1.5), (26.0, 1.0), (29.5, 1.5), (15.0, 1.5)]])
    G, r, orc = _ref(oracle, graph, b, meili)
    assert not r.amb.any() and (orc["ipos"] < 0).all()      # rule 7 places nothing in a same-edge step
    e0 = _edge_from(G, 0)
    want = [(M | COL | CS, 5.0), (M | SAME, 8.0), (M | SAME, 12.0), (M | SAME, 5.0), (M | COL, 30.0),
            (M | COL | CS, 28.0), (M | SAME, 26.0), (M | SAME, 28.0), (M | COL, 15.0)]
    for k, (fl, off) in enumerate(want):
        assert (int(r.flags[k]), int(r.edge[k])) == (fl, e0), (k, r.flags[k], r.edge[k])
        assert abs(r.off[k] - off) < 0.01, (k, r.off[k])
        x, y, d = _xy(G, r, b, k)
        x_in, y_in = _probe_xy(b, k)                         # (the clamped feet are not below their probes)
        assert abs(x - off) < 0.01 and abs(y) < 0.01 and abs(d - math.hypot(off - x_in, y_in)) < 0.01, (k, x, y, d)
        assert r.off_tol[k] < 1e-4


# ------------------------------------------------------------------ the cap of the GPU file's cases
@pytest.mark.parametrize("name", ["hand_short_edges", "hand_curve_interp", "hand_hairpin", "hand_filter",
                                  "hand_edge_cases", "stop_and_go", "stop_80", "seg_forms", "city_5s"])
def test_cases_stay_inside_the_cap(cases, oracle, name):
    """The same-edge rule and the route placements on the oracle's stage arrays:
    at most 5 % of a case's interpolated points are ambiguous, none on a hand
    graph (specref's caps)."""
    graph, batch, meili, max_excl = cases[name]
    _, r, _ = _ref(oracle, graph, batch, meili)
    n, amb = int(r.interp.sum()), int(r.amb.sum())
    print(name, "interpolated points with a place:", n, "ambiguous:", amb)
    assert amb <= (0.05 * n if max_excl is None else max_excl)
