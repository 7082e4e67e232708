"""The inputs of the spec-reference tests (tests/test_specref.py on the CPU
oracle, tests/test_gpu_specref.py on the kernels): a 1.5 x 1.5 km synthetic
city with batches that reach each rule of DESIGN.md §3, and hand graphs whose
probes are placed so that one named rule fires, clear of every decision
boundary (the reference must exclude nothing there).

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
    star = os.path.join(d, "specref_star.otmg")
    handgraph.star(star, lat=LAT, lon=0.0, n_spokes=20, length_m=90.0)
    a7 = 2.0 * math.pi * 7 / 20
    hub = [[(3.0, 50.0), (2.0, 1.0), (50 * math.sin(a7) + 2.0, 50 * math.cos(a7) + 2.0)]]
    cases["hand_star"] = (star, _xy(hub), dict(HAND), 0)
    return cases
