"""The inputs of the spec-reference tests (tests/test_specref.py on the CPU
oracle, tests/test_gpu_specref.py on the kernels): a 1.5 x 1.5 km synthetic
city with batches that reach each rule of DESIGN.md §3, and hand graphs whose
probes are placed so that one named rule fires, clear of every decision
boundary (the reference must exclude nothing there).  The cases of rule 7's
interpolated points -- short edges, the curve, a hairpin, the filter road, a
stop of 80 samples, the three segment emitters -- are the smallest shapes on
which placement and the anchored boundaries can go wrong.  (Latitudes are f32:
at 40 degrees a probe's y is quantised to 0.42 m, so the metres in the
comments are approximate across the road and exact enough along it.)

A case is (graph path, batch, meili overrides, max_excl): max_excl None means
the caps of specref_checks (5 % of traces, 1 % of transition entries), 0 means
no exclusion at all.
"""
import math
import os

import numpy as np

import handgraph
from handgraph import SEG_BEGIN, SEG_END

LAT = 40.0
MLAT = handgraph.MPD
MLON = MLAT * math.cos(math.radians(LAT))
HAND = dict(search_radius=25.0, max_search_radius=25.0, gps_accuracy=5.0)
EDGE_IDS = {}   # edge name -> id in the edge-case graph's file, filled by build()


def _pt(x, y):
    return (LAT + y / MLAT, x / MLON)


def _batch(traces, dt=5.0, acc=5.0):
    """traces: lists of (lat, lon) points, one fix every dt seconds."""
    pts = [p for tr in traces for p in tr]
    off = np.cumsum([0] + [len(tr) for tr in traces]).astype(np.int64)
    tm = np.concatenate([1500000000.0 + dt * np.arange(len(tr)) for tr in traces])
    return dict(trace_off=off, lat=np.array([p[0] for p in pts], np.float32),
                lon=np.array([p[1] for p in pts], np.float32), time=tm,
                accuracy=np.full(len(pts), acc, np.float32))


def _xy(traces, **kw):
    return _batch([[_pt(x, y) for x, y in tr] for tr in traces], **kw)


def edge_case_graph(path):
    """Four components 1 km apart, every edge one-way and its own OSMLR
    segment (id (k + 1) << 3 for the k-th edge below, way 1000 + k):
      curve  C0 -> C1: a quarter circle of radius 100 m in 9 shape segments, its
             middle point repeated (a zero-length shape segment); C1 -> C2 north
      sink   S0 -> S1, nothing leaves S1
      ring   R0 -> R1 -> R2 -> R3 -> R0, 60 m a side, one way
      twins  T0 -> T1, two edges T1 -> T2 of one geometry, T2 -> T3
    Returns {name: edge id in the file}."""
    arc = [(100 * math.sin(math.radians(a)), 100 - 100 * math.cos(math.radians(a)))
           for a in (0, 11.25, 22.5, 33.75, 45, 45, 56.25, 67.5, 78.75, 90)]
    xy = {"C0": (0, 0), "C1": (100, 100), "C2": (100, 200), "S0": (1000, 0), "S1": (1100, 0),
          "R0": (2000, 0), "R1": (2060, 0), "R2": (2060, 60), "R3": (2000, 60),
          "T0": (3000, 0), "T1": (3060, 0), "T2": (3100, 0), "T3": (3160, 0)}
    names = list(xy)
    nodes = [_pt(*xy[n]) for n in names]
    spec = [("curve", "C0", "C1"), ("north", "C1", "C2"), ("sink", "S0", "S1"), ("r01", "R0", "R1"),
            ("r12", "R1", "R2"), ("r23", "R2", "R3"), ("r30", "R3", "R0"), ("t01", "T0", "T1"),
            ("twin_a", "T1", "T2"), ("twin_b", "T1", "T2"), ("t23", "T2", "T3")]
    edges, segs = [], []
    for k, (nm, a, b) in enumerate(spec):
        e = dict(**{"from": names.index(a), "to": names.index(b)}, way=1000 + k, seg=k, seg_pos=0,
                 flags=SEG_BEGIN | SEG_END, level=0)
        if nm == "curve":
            e["shape"] = [nodes[names.index("C0")]] + [_pt(x, y) for x, y in arc[1:-1]] + [nodes[names.index("C1")]]
        edges.append(e)
        segs.append(((k + 1) << 3, None))
    ids = handgraph.write(path, nodes, edges, segs)
    return {nm: ids[k] for k, (nm, _, _) in enumerate(spec)}


# the probes of the edge-case graph, one trace per rule (metres, x east, y north)
EDGE_TRACES = [
    [(32.8, 9.8), (74.9, 25.1), (103.0, 150.0)],      # curve: inside the arc; outside it at the repeated point
    [(1040.0, 3.0), (1108.0, 2.0)],                   # sink: the second probe 8 m past the dead end
    [(2040.0, -4.0), (2025.0, -5.0), (2064.0, 30.0)],  # ring: 15 m back along r01 (a stay), then r12
    [(3030.0, 3.0), (3130.0, -3.0)],                  # twins: the route crosses the twin edges
    [(3030.0, 3.0), (3080.0, 2.0), (3130.0, -3.0)],   # twins: a probe on them (two tied states)
]


# ---------------------------------------------------------------- rule 7: interpolated points
# Every interpolated point lies within interpolation_distance (10 m) of its
# column q, so it reaches a middle piece of a step's route only where edges are
# a few metres long.
SHORT_X = [0.0, 60.0, 63.0, 66.0, 69.0, 129.0]       # nodes of the short-edge chain, metres east
SHORT_EDGES = ["a", "s1", "s2", "s3", "b"]
SHORT_IDS = {}
SHORT_TRACES = [
    # q 1 m before the first short edge; points on the first piece, on s1, s2 and s3 (path edges in the
    # middle of the route); p on b.  The segment ends at 60, 63, 66 and 69 each lie between two anchors
    [(30.0, 1.5), (59.0, 1.5), (59.5, 1.5), (61.0, 1.5), (64.5, 1.5), (67.5, 1.5), (80.0, 1.5), (110.0, 1.0)],
    # q on s1: the first piece is the rest of a short edge, the last point lies on p's piece (b from 0)
    [(30.0, 1.5), (61.5, 1.5), (62.5, 1.5), (64.0, 1.5), (68.0, 1.5), (70.0, 1.5), (80.0, 1.5), (110.0, 1.0)],
    # q exactly on the node at 60 (filled in by build(): a node candidate, no first piece)
    [(30.0, 1.5), None, (61.5, 1.0), (64.5, -1.5), (67.5, 1.0), (80.0, 1.5), (110.0, 1.0)],
    # p exactly on the node at 69 (a node candidate, no last piece), then on along b
    [(30.0, 1.5), (58.5, 1.5), (59.5, -1.0), (61.5, 2.0), (64.5, -1.5), (67.5, 1.0), None, (85.0, 1.5), (110.0, 1.0)],
]


def short_edge_graph(path):
    """A one-way chain east along y = 0: a (60 m), s1, s2, s3 (3 m each, shaped
    like intersection-internal edges; s2 is flagged internal and carries no
    segment), b (60 m); every other edge its own OSMLR segment."""
    nodes = [_pt(x, 0.0) for x in SHORT_X]
    edges, segs = [], []
    for k, nm in enumerate(SHORT_EDGES):
        if nm == "s2":
            edges.append(dict(**{"from": k, "to": k + 1}, way=2000 + k, seg=-1, flags=handgraph.EDGE_INTERNAL, level=0))
        else:
            edges.append(dict(**{"from": k, "to": k + 1}, way=2000 + k, seg=len(segs), seg_pos=0,
                              flags=SEG_BEGIN | SEG_END, level=0))
            segs.append(((k + 1) << 3, None))
    ids = handgraph.write(path, nodes, edges, segs)
    return {nm: ids[k] for k, nm in enumerate(SHORT_EDGES)}


# the curve graph again: a state on the arc, interpolated points inside and outside it, a state on `north`
def _arc(a_deg, r):
    a = math.radians(a_deg)
    return (r * math.sin(a), 100.0 - r * math.cos(a))


CURVE_INTERP_TRACES = [
    # the third point lies behind q: its closest foot on the arc (shape segment 6) is behind q's offset, so the
    # first piece is not admissible -- although segment 7's clamped foot would lie inside the piece
    [_arc(60.0, 99.0), _arc(77.0, 99.0), _arc(74.5, 98.0), _arc(79.0, 96.5), _arc(81.5, 103.0), (101.5, 112.0),
     (99.0, 150.0)],
    # the second point sits outside the arc at its repeated shape point (45 degrees): its closest foot is that
    # vertex, the end of shape segment 3, the zero-length segment 4 and the start of segment 5 alike
    [_arc(20.0, 99.0), _arc(42.0, 101.0), _arc(45.0, 103.0), _arc(46.5, 98.0), (101.5, 112.0), (99.0, 150.0)],
]

# the hairpin: e runs east 40 m along y = 0, a 4 m connector north, w runs back west along y = 4
HAIRPIN_EDGES = ["e", "conn", "w"]
HAIRPIN_IDS = {}
HAIRPIN_TRACES = [
    # (36, 2.2) and (38, 2.1) are nearer to w than to e (the sqdist terms prefer w by 0.05 and 0.01), and
    # |pos - gc| / beta puts them on e (by 3.9 and 3.0); (27, 3.2) projects behind q on e: it lands on w
    [(15.0, -3.0), (33.0, 1.0), (36.0, 2.2), (38.0, 2.1), (27.0, 3.2), (22.0, 3.5), (8.0, 3.8)],
]


def hairpin_graph(path):
    nodes = [_pt(0.0, 0.0), _pt(40.0, 0.0), _pt(40.0, 4.0), _pt(0.0, 4.0)]
    edges = [dict(**{"from": k, "to": k + 1}, way=3000 + k, seg=k, seg_pos=0, flags=SEG_BEGIN | SEG_END, level=0)
             for k in range(3)]
    ids = handgraph.write(path, nodes, edges, [((k + 1) << 3, None) for k in range(3)])
    return {nm: ids[k] for k, nm in enumerate(HAIRPIN_EDGES)}


# the monotone filter and the points outside every step, on a one-way straight road of 40 m edges (nodes at
# x = 0, 40, ..., 280); breakage_distance is 60 m in this case
FILTER_TRACES = [
    # behind q on q's edge, and p a node candidate at the edge's end: the first piece is the only one
    [(5.0, 1.5), (28.0, 1.5), (25.5, 1.0), None, (62.0, 1.5)],
    # placed at 4.3, then at 1.7 behind it (the filter drops it), then at 9.5 past the node at 40 (position 8):
    # the boundary there lies between the first and the third, and must not see the second
    [(32.0, 1.5), (36.3, 1.0), (33.7, 1.5), (41.5, 1.0), (54.0, 1.5), (95.0, 1.5)],
    # two bit-equal copies in a row (not of q): both anchors, the later one names the boundary at 40
    [(5.0, 1.5), (30.0, 1.5), (35.0, 1.0), (35.0, 1.0), (55.0, 1.5), (96.0, 1.5)],
    # points after the chain's last state
    [(5.0, 1.5), (30.0, 1.5), (55.0, 1.5), (57.0, 1.0), (59.0, 1.5)],
    # an off-graph point (an empty column) and an interpolated point of it inside the trace: the chain breaks
    # there, the points on either side of it lie in no step
    [(30.0, 1.5), (55.0, 1.5), (57.0, 1.0), (30.0, 500.0), (33.0, 500.0), (57.0, 1.0), (59.0, 1.5), (100.0, 1.5)],
    # duplicates on both sides of a breakage break (65 m > 60 m): those before it lie in no step
    [(30.0, 1.5), (30.0, 1.5), (30.0, 1.5), (95.0, 1.5), (95.0, 1.5), (95.0, 1.5), (140.0, 1.5), (180.0, 1.5)],
]


def _insert_copies(b, at, n, dt=1.0):
    """A one-trace batch with n bit-equal copies of point `at` after it, dt
    seconds apart; the later points move on in time."""
    idx = np.concatenate([np.arange(at + 1), np.full(n, at), np.arange(at + 1, len(b["lat"]))])
    out = {k: np.asarray(b[k])[idx] for k in ("lat", "lon", "accuracy")}
    tm = np.asarray(b["time"], np.float64)[idx]
    tm[at + 1:at + 1 + n] += dt * np.arange(1, n + 1)
    tm[at + 1 + n:] += dt * n
    out["time"] = tm
    out["trace_off"] = np.array([0, len(idx)], np.int64)
    return out


def _concat(batches):
    out = {k: np.concatenate([np.asarray(b[k]) for b in batches]) for k in ("lat", "lon", "accuracy", "time")}
    out["trace_off"] = np.cumsum([0] + [len(b["lat"]) for b in batches]).astype(np.int64)
    return out


def _cut(b, n):
    out = {k: np.asarray(b[k])[:n] for k in ("lat", "lon", "accuracy", "time")}
    out["trace_off"] = np.array([0, n], np.int64)
    return out


STOP_AT, STOP_N = 11, 80           # stop_80: the point the vehicle stands on, and for how many samples
# seg_forms: the lead-in trace's length, and where the 129-point trace stands (its point 36 and 16 copies: the
# copies are points 249..264 of the batch)
FORMS = dict(lead=84, stop_at=36, stop_n=16)


def build(tmpdir, synth):
    """-> {name: (graph, batch, meili, max_excl)}."""
    d = str(tmpdir)
    city = synth.make_graph(os.path.join(d, "specref_city.otmg"), width_m=1500, height_m=1500)

    def tr(n, pts, interval, seed, sigma=15.0, acc=15.0):
        b = synth.make_traces(city, n, pts, interval_s=interval, noise_sigma_m=sigma, accuracy=acc, seed=seed)
        return {k: b[k] for k in ("trace_off", "lat", "lon", "time", "accuracy")}

    cases = {}
    cases["city_5s"] = (city, tr(40, 30, 5.0, 5), {}, None)
    cases["city_30s"] = (city, tr(40, 30, 30.0, 6), {}, None)
    cases["gaps_240s"] = (city, tr(24, 20, 240.0, 7), dict(breakage_distance=800.0), None)
    cases["radius_120"] = (city, tr(24, 4, 5.0, 8), dict(search_radius=120.0, max_search_radius=120.0), None)
    cases["radius_300"] = (city, tr(40, 2, 5.0, 13), dict(search_radius=300.0, max_search_radius=300.0,
                                                         max_candidates=32), None)
    cases["dense_1s"] = (city, tr(24, 40, 1.0, 10), {}, None)
    # stop and go: every point of a 5 s trace three times, a second apart (the copies are interpolated points)
    b = tr(24, 12, 5.0, 11)
    rep = np.repeat(np.arange(len(b["lat"])), 3)
    sg = {k: b[k][rep] for k in ("lat", "lon", "accuracy")}
    sg["time"] = b["time"][rep] + np.tile(np.arange(3.0), len(b["lat"]))
    sg["trace_off"] = b["trace_off"] * 3
    cases["stop_and_go"] = (city, sg, {}, None)
    cases["turn_factor_0"] = (city, tr(24, 20, 5.0, 17), dict(turn_penalty_factor=0.0), None)
    b = tr(24, 20, 5.0, 13)
    b["accuracy"] = np.tile(np.array([0.0, -5.0, 500.0, 15.0], np.float32), len(b["lat"]) // 4 + 1)[:len(b["lat"])]
    cases["accuracies"] = (city, b, {}, None)
    # the long trace: 140 points, past the 128-point Viterbi window of the kernels
    cases["long_140"] = (city, tr(1, 140, 5.0, 14), {}, None)

    hand = os.path.join(d, "specref_edge_cases.otmg")
    EDGE_IDS.update(edge_case_graph(hand))
    cases["hand_edge_cases"] = (hand, _xy(EDGE_TRACES), dict(HAND), 0)
    # probes exactly on shape points at radius 0: the hit test's "<=" decides (0 <= 0)
    import specref
    G = specref.Graph(hand)
    on = [[(float(np.float32(G.node_lat[v])), float(np.float32(G.node_lon[v]))) for v in (9, 10, 12)]]  # T0, T1, T3
    cases["hand_radius_0"] = (hand, _batch(on, acc=0.0), dict(search_radius=0.0, max_search_radius=25.0,
                                                              gps_accuracy=0.0), 0)
    # ---- rule 7
    short = os.path.join(d, "specref_short_edges.otmg")
    SHORT_IDS.update(short_edge_graph(short))
    Gs = specref.Graph(short)
    node = lambda v: (float(np.float32(Gs.node_lat[v])), float(np.float32(Gs.node_lon[v])))
    fix = {2: node(1), 3: node(4)}
    cases["hand_short_edges"] = (short, _batch([[fix[t] if pt is None else _pt(*pt) for pt in tr]
                                                for t, tr in enumerate(SHORT_TRACES)], dt=2.0),
                                 dict(HAND, turn_penalty_factor=0.0), 0)
    cases["hand_curve_interp"] = (hand, _xy(CURVE_INTERP_TRACES, dt=2.0), dict(HAND), 0)
    hair = os.path.join(d, "specref_hairpin.otmg")
    HAIRPIN_IDS.update(hairpin_graph(hair))
    cases["hand_hairpin"] = (hair, _xy(HAIRPIN_TRACES, dt=2.0), dict(HAND, turn_penalty_factor=0.0), 0)
    road = os.path.join(d, "specref_road.otmg")
    handgraph.write(road, [_pt(40.0 * k, 0.0) for k in range(8)],
                    [dict(**{"from": k, "to": k + 1}, way=4000 + k, seg=k, seg_pos=0, flags=SEG_BEGIN | SEG_END,
                          level=0) for k in range(7)], [((k + 1) << 3, None) for k in range(7)])
    Gr = specref.Graph(road)
    n40 = (float(np.float32(Gr.node_lat[1])), float(np.float32(Gr.node_lon[1])))
    cases["hand_filter"] = (road, _batch([[n40 if pt is None else _pt(*pt) for pt in tr] for tr in FILTER_TRACES],
                                         dt=2.0), dict(HAND, breakage_distance=60.0), 0)
    # one city trace that stands for 80 samples (more than one wavefront of K7a threads inside one step) and drives on
    cases["stop_80"] = (city, _insert_copies(tr(1, 30, 5.0, 21), STOP_AT, STOP_N), {}, None)
    # the three segment emitters: <= 128 points, <= 256 points, longer -- dense traces of 128, 129, 256 and 257
    # points in one batch behind a short lead-in trace; the 129-point one stands for 16 samples across point 256
    # of the batch (a 256-thread block boundary of K7a inside one step's run of interpolated points); and one trace
    # of <= 128 points with more than 160 traversals (30 s sampling, a copy after every fifth point)
    dense = lambda n, seed: _cut(tr(1, 257, 0.5, seed, sigma=3.0, acc=10.0), n)
    lead = FORMS["lead"]
    b129 = _insert_copies(dense(129 - FORMS["stop_n"], 32), FORMS["stop_at"], FORMS["stop_n"])
    slow = tr(1, 100, 30.0, 35)
    for at in range(95, 0, -5):
        slow = _insert_copies(slow, at, 1)
    forms = ([dense(lead, 36)] if lead else []) + [dense(128, 31), b129, dense(256, 33), dense(257, 34), slow]
    cases["seg_forms"] = (city, _concat(forms), {}, None)
    star = os.path.join(d, "specref_star.otmg")
    handgraph.star(star, lat=LAT, lon=0.0, n_spokes=20, length_m=90.0)
    a7 = 2.0 * math.pi * 7 / 20
    hub = [[(3.0, 50.0), (2.0, 1.0), (50 * math.sin(a7) + 2.0, 50 * math.cos(a7) + 2.0)]]
    cases["hand_star"] = (star, _xy(hub), dict(HAND), 0)
    return cases
