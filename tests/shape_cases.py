"""Hand cases for rule 7f's kernel (tests/test_shape.py on the reference,
tests/test_gpu_shape.py on k_shape), in the form of tests/specref_cases.py:
(graph path, batch, meili overrides, max_excl).

hand_shape       one way east from (lat 40, lon 0), every edge its own OSMLR
                 segment; x east, y north in metres:
                   e2     2 shape points, (0,0) -> (60,0)
                   e3     3 shape points, a corner at (90,0), then to (110,-20)
                   e16    16 shape points (the format's maximum), 10 m apart along y = -20
                   dup0   its first shape point repeated (cum 0, 0, 30, 60)
                   dupi   an interior point repeated (cum 0, 30, 30, 60)
                   nw     north-east, then north-west, then south-east: negative
                          deltas on both axes
                   tail   60 m
                 and, 300 m north, a second road of 72 edges of 16 shape points
                 1 m apart (l0 .. l71).  Traces:
                   0  starts mid-segment on e16 and ends mid-segment on dupi two
                      edges later: partial begin and end, dup0 whole (its repeated
                      first point is dropped), dupi's repeated point never reached
                   1  its first state lies outside e3's corner, so both shape
                      segments clamp to the corner: begin_offset is cum[1] bit
                      for bit, and the strict compare leaves the corner to the
                      first vertex; it goes on over e16, dup0, dupi (both repeated
                      points kept), nw to the tail
                   2  two states inside e2's one shape segment: one record, two
                      vertices
                   3  eleven states 105 m apart along the second road: 71 records on
                      16-point edges, so its first chunk of 64 records expands to
                      far more than 64 vertices
hand_shape_sw    the first road alone at lat -33.45, lon -70.66 with traces 0-2:
                 the first delta from (0, 0) is negative on both axes and takes
                 6 chars.
hand_shape_jump  two 60 m roads 0.3 deg apart in latitude and 0.6 deg in
                 longitude; one trace with two states on each: two chains, a
                 5-char delta in mid-string, begin_vertex = the previous
                 end_vertex + 1.
The search radius is 5 m, so no probe sees a second road or a node.
"""
import math
import os

import numpy as np

import handgraph
from handgraph import MPD, SEG_BEGIN, SEG_END

MEILI = dict(search_radius=5.0, max_search_radius=5.0, gps_accuracy=5.0)
N_LONG, LONG_STATES, LONG_GAP = 72, 11, 105.0
IDS = {}    # case -> {edge name: id in the file}, filled by build()


def _frame(lat0, lon0):
    mlon = MPD * math.cos(math.radians(lat0))
    return lambda x, y: (lat0 + y / MPD, lon0 + x / mlon)


def _batch(pt, traces, dt=5.0, acc=5.0):
    """traces: lists of (x, y) in pt's frame, or of (x, y, frame) for a point in another one."""
    pts = [(p[2] if len(p) > 2 else pt)(p[0], p[1]) for tr in traces for p in tr]
    off = np.cumsum([0] + [len(tr) for tr in traces]).astype(np.int64)
    tm = np.concatenate([1500000000.0 + dt * np.arange(len(tr)) for tr in traces])
    return dict(trace_off=off, lat=np.array([p[0] for p in pts], np.float32),
                lon=np.array([p[1] for p in pts], np.float32), time=tm, accuracy=np.full(len(pts), acc, np.float32))


def _write(path, roads):
    """roads: (frame, [(name, [(x, y), ...]), ...]) each, a chain of edges (an
    edge starts where the one before ends).  -> {name: edge id}."""
    nodes, edges, segs, names = [], [], [], []
    for pt, road in roads:
        nodes.append(pt(*road[0][1][0]))
        for name, sh in road:
            nodes.append(pt(*sh[-1]))
            edges.append(dict(**{"from": len(nodes) - 2, "to": len(nodes) - 1}, way=9000 + len(edges), level=0,
                              seg=len(segs), seg_pos=0, flags=SEG_BEGIN | SEG_END, shape=[pt(x, y) for x, y in sh]))
            segs.append(((len(segs) + 1) << 3, None))
            names.append(name)
    ids = handgraph.write(path, nodes, edges, segs)
    return {nm: ids[k] for k, nm in enumerate(names)}


Y = -20.0
FIRST_ROAD = [
    ("e2", [(0.0, 0.0), (60.0, 0.0)]),
    ("e3", [(60.0, 0.0), (90.0, 0.0), (110.0, Y)]),
    ("e16", [(110.0 + 10.0 * k, Y) for k in range(16)]),
    ("dup0", [(260.0, Y), (260.0, Y), (290.0, Y), (320.0, Y)]),
    ("dupi", [(320.0, Y), (350.0, Y), (350.0, Y), (380.0, Y)]),
    ("nw", [(380.0, Y), (410.0, Y + 10.0), (400.0, Y + 20.0), (430.0, Y)]),
    ("tail", [(430.0, Y), (490.0, Y)]),
]
FIRST_TRACES = [
    [(165.0, Y + 1.0), (335.0, Y + 1.0)],
    [(91.5, 3.3), (205.0, Y + 1.0), (335.0, Y + 1.0), (460.0, Y + 1.0)],
    [(10.0, 1.0), (40.0, 1.0)],
]
LONG_Y = 300.0
LONG_ROAD = [("l%d" % k, [(15.0 * k + i, LONG_Y) for i in range(16)]) for k in range(N_LONG)]
LONG_TRACE = [(7.5 + LONG_GAP * k, LONG_Y + 1.0) for k in range(LONG_STATES)]


def build(tmpdir):
    """-> {name: (graph, batch, meili, max_excl)}."""
    d = str(tmpdir)
    cases = {}
    pt = _frame(40.0, 0.0)
    path = os.path.join(d, "shape_hand.otmg")
    IDS["hand_shape"] = _write(path, [(pt, FIRST_ROAD), (pt, LONG_ROAD)])
    cases["hand_shape"] = (path, _batch(pt, FIRST_TRACES + [LONG_TRACE]), dict(MEILI), 0)

    pt = _frame(-33.45, -70.66)
    path = os.path.join(d, "shape_hand_sw.otmg")
    IDS["hand_shape_sw"] = _write(path, [(pt, FIRST_ROAD)])
    cases["hand_shape_sw"] = (path, _batch(pt, FIRST_TRACES), dict(MEILI), 0)

    pt, far = _frame(40.0, 0.0), _frame(40.3, 0.6)
    path = os.path.join(d, "shape_hand_jump.otmg")
    IDS["hand_shape_jump"] = _write(path, [(pt, [("a", [(0.0, 0.0), (60.0, 0.0)])]),
                                           (far, [("b", [(0.0, 0.0), (60.0, 0.0)])])])
    cases["hand_shape_jump"] = (path, _batch(pt, [[(10.0, 1.0), (40.0, 1.0), (10.0, 1.0, far), (40.0, 1.0, far)]]),
                                dict(MEILI), 0)
    return cases


# ------------------------------------------------------------------ what each case reaches
ALL = ["hand_shape", "hand_shape_sw", "hand_shape_jump", "hand_many_short", "hand_long_edge", "stop_80",
       "stop_and_go", "seg_forms", "city_5s", "gaps_240s"]
TV_CHAIN_START, TV_FROM_START, TV_TO_END = 1, 4, 8


def value_lengths(poly):
    """The char count of each value of a polyline6 string (bytes)."""
    out, n = [], 0
    for c in poly:
        n += 1
        if not (c - 63) & 0x20:
            out.append(n)
            n = 0
    assert n == 0, "truncated polyline"
    return out


def assert_reached(name, G, edge, b, z, flags, toff, spans, vtx_off, polylines):
    """No case goes empty: what `name` is there for, asserted on the records
    (edge, begin_offset b and end_offset z as f32, flags, trav_off) and on a
    shape of them (spans (n, 2), vtx_off, one polyline per trace)."""
    nv = spans[:, 1] - spans[:, 0] + ((flags & TV_CHAIN_START) != 0)      # vertices each record emitted
    cnt = np.diff(toff)
    assert len(edge) > 0 and (nv >= 1).all(), name
    if name in ("hand_shape", "hand_shape_sw"):
        ids = IDS[name]
        r0 = int(toff[0])
        assert [int(e) for e in edge[r0:r0 + 3]] == [ids["e16"], ids["dup0"], ids["dupi"]] and cnt[0] == 3
        # a partial begin and a partial end; dup0 whole: one of its two interior points (the repeated first one dropped)
        assert not flags[r0] & TV_FROM_START and b[r0] > 0 and not flags[r0 + 2] & TV_TO_END
        assert flags[r0 + 1] & TV_FROM_START and flags[r0 + 1] & TV_TO_END and nv[r0 + 1] == 2
        r1 = int(toff[1])
        assert cnt[1] == 6 and int(edge[r1]) == ids["e3"] and int(edge[r1 + 3]) == ids["dupi"]
        corner = np.float32(G.scum[int(G.eshape[ids["e3"]]) + 1])
        assert np.float32(b[r1]).view(np.uint32) == corner.view(np.uint32)      # an end on a shape point, bit for bit
        assert nv[r1] == 2 and nv[r1 + 1] == 15 and nv[r1 + 3] == 3             # the corner only once; dupi: both kept
        assert cnt[2] == 1 and nv[int(toff[2])] == 2                            # one record, two vertices
        # the first values, from (0, 0): lat 40 and lon 0.002, or lat -33 and lon -70
        assert value_lengths(polylines[0])[:2] == ([6, 6] if name == "hand_shape_sw" else [6, 3])
    if name == "hand_shape_sw":
        assert (polylines[0][0] - 63) & 1 and (polylines[0][6] - 63) & 1        # both first deltas negative
    if name == "hand_shape":
        r3 = int(toff[3])
        assert cnt[3] == 71 > 64 and spans[r3 + 63, 1] + 1 > 64 * 8             # a record chunk of hundreds of vertices
        assert (G.eshape[edge[r3:r3 + 71] + 1] - G.eshape[edge[r3:r3 + 71]] == 16).all()
    if name == "hand_shape_jump":
        assert cnt[0] == 2 and spans.tolist() == [[0, 1], [2, 3]] and vtx_off[1] == 4
        vl = value_lengths(polylines[0])
        assert len(vl) == 8 and vl[0] == 6 and vl[4:6] == [4, 5]                # mid-string: 0.3 deg 4 chars, 0.6 deg 5
    if name == "hand_many_short":
        assert cnt.max() == 102                                                 # a step's records cross the chunk
    if name == "hand_long_edge":
        last = int(toff[2]) - 1
        assert not flags[last] & TV_TO_END and abs(float(z[last]) - 764.0) < 0.01    # the largest offset reached
    if name in ("stop_80", "stop_and_go", "seg_forms", "city_5s", "gaps_240s"):
        assert len(edge) >= (10 if name == "stop_80" else 100) and (nv > 2).any()
        assert ((flags & TV_FROM_START) == 0).any() and ((flags & TV_TO_END) == 0).any()
    if name == "gaps_240s":
        starts = np.add.reduceat(((flags & TV_CHAIN_START) != 0).astype(np.int64), toff[:-1][cnt > 0])
        assert (starts >= 2).any()                                              # chain breaks inside a trace
