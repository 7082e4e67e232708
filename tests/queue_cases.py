"""The inputs of the queue_length tests (tests/test_queue.py on the CPU oracle's
stage arrays, tests/test_gpu_queue.py on the kernel): straight hand roads at
lat 40 with probes exactly on the road, so that every expected queue length is
a closed-form function of the probe longitudes, and the 1.5 km city of
specref_cases with its times rewarped into slow stretches.

A hand case is (graph key, trace [(x metres east, t seconds)], {segment_id:
expected queue_length}).  Positions are metres along the road from lon 0 (the
equirectangular metres of tests/test_interp.py's _x()); NODE(step, k) is node
k of a road with step_deg = step.  The threshold of every hand case is KPH.
"""
import math

import numpy as np

import handgraph
from handgraph import SEG_BEGIN, SEG_END

LAT = 40.0
MLON = handgraph.MPD * math.cos(math.radians(LAT))
KPH = 10.0          # hand cases: slow is below 2.78 m/s
CITY_KPH = 20.0
STEP = 0.004        # edges of ~341 m, one OSMLR segment each
T0 = 1500000000.0


def lon_of(x):
    return np.float32(x / MLON)


def xq(x):
    """x as the engine sees it: through the probe's float32 longitude"""
    return float(lon_of(x)) * MLON


def NODE(step, k):
    return float(np.float32(k * step)) * MLON


def drive(x0, legs, t0=T0):
    """[(x, t)]: from x0 at t0, then per leg (steps, metres per step, seconds per step)"""
    pts = [(x0, t0)]
    for n, dx, dt in legs:
        for _ in range(n):
            x, t = pts[-1]
            pts.append((x + dx, t + dt))
    return pts


def batch(traces, acc=5.0):
    lon = np.array([lon_of(x) for tr in traces for x, _ in tr], np.float32)
    tm = np.array([t for tr in traces for _, t in tr], np.float64)
    off = np.cumsum([0] + [len(tr) for tr in traces]).astype(np.int64)
    return dict(trace_off=off, lat=np.full(len(lon), LAT, np.float32), lon=lon, time=tm,
                accuracy=np.full(len(lon), acc, np.float32))


def graphs(tmpdir):
    """-> {key: .otmg path}: "road" 6 nodes, one segment per edge; "multi" the same road with
    edges 1 and 2 joined into one segment; "long" 12 nodes (past breakage_distance
    end to end); "fine" 72 nodes 42.6 m apart."""
    d = str(tmpdir)
    g = {}
    g["road"], _ = handgraph.straight_road(d + "/q_road.otmg", lat=LAT, step_deg=STEP, n_nodes=6)
    # "multi": the 6-node road with edges 1 and 2 joined into one segment (id 16)
    nodes = [(LAT, i * STEP) for i in range(6)]
    segs = [(8, None), (16, None), (24, None), (32, None)]
    lay = [(0, 0, SEG_BEGIN | SEG_END), (1, 0, SEG_BEGIN), (1, 1, SEG_END), (2, 0, SEG_BEGIN | SEG_END),
           (3, 0, SEG_BEGIN | SEG_END)]
    edges = []
    for i, (sg, pos, fl) in enumerate(lay):
        edges.append(dict(**{"from": i, "to": i + 1}, way=100 + i, seg=sg, seg_pos=pos, flags=fl, level=0))
        edges.append(dict(**{"from": i + 1, "to": i}, way=100 + i, seg=-1, level=0))
    g["multi"] = d + "/q_multi.otmg"
    handgraph.write(g["multi"], nodes, edges, segs)
    g["long"], _ = handgraph.straight_road(d + "/q_long.otmg", lat=LAT, step_deg=STEP, n_nodes=12)
    g["fine"], _ = handgraph.straight_road(d + "/q_fine.otmg", lat=LAT, step_deg=0.0005, n_nodes=72)
    return g


N = lambda k: NODE(STEP, k)  # noqa: E731


def _r(v):
    """v rounded as the rule rounds; every hand expectation stays 0.2 m clear of a rounding boundary"""
    assert abs(v - math.floor(v) - 0.5) >= 0.2, v
    return int(math.floor(v + 0.5))


def hand_cases():
    """-> {name: (graph key, trace, {segment_id: queue_length})}; segment ids
    are (edge + 1) << 3.  Every segment of the trace not named in the dict is
    expected to carry 0."""
    c = {}
    L1 = _r(float(np.float32(N(2) - N(1))))  # about what the graph holds for a segment's length (341)
    # free flow: 15 m/s at 1 s
    c["free_flow"] = ("road", drive(72.0, [(85, 15.0, 1.0)]), {})
    # 15 m/s until 80 m before the end of edge 1, 2 m/s through the node and 20 m
    # into edge 2, then 15 m/s: the queue of edge 1's segment starts at that
    # sample; edge 2's slow part is not at its end
    a = N(2) - 80.0
    tr = drive(a - 30 * 15.0, [(30, 15.0, 1.0), (50, 2.0, 1.0), (50, 15.0, 1.0)])
    c["queue_1s"] = ("road", tr, {16: _r(N(2) - xq(a))})
    # the same with states only: 5 s sampling, 12.5 m apart (2.5 m/s: 9 km/h, 10 % under the
    # threshold; every point a column), 75 m apart when fast
    tr = drive(a - 6 * 75.0, [(6, 75.0, 5.0), (8, 12.5, 5.0), (10, 75.0, 5.0)])
    c["queue_states"] = ("road", tr, {16: _r(N(2) - xq(a))})
    # discharge: standing 15 m before the end of edge 1 (six identical points
    # 5 s apart), the next sample 1.4 s later 6 m past the node (15 m/s)
    s = N(2) - 15.0
    tr = drive(s - 30 * 15.0, [(30, 15.0, 1.0), (5, 0.0, 5.0), (1, 21.0, 1.4), (40, 15.0, 1.0)])
    c["discharge"] = ("road", tr, {16: _r(N(2) - xq(s))})
    tr = drive(s - 30 * 15.0, [(30, 15.0, 1.0), (1, 21.0, 1.4), (40, 15.0, 1.0)])
    c["no_standing"] = ("road", tr, {})
    # whole segment slow: the run starts 30 m before edge 1 and ends 29 m past it
    b = N(1) - 30.0
    tr = drive(b - 3 * 75.0, [(3, 75.0, 5.0), (32, 12.5, 5.0), (10, 75.0, 5.0)])
    c["whole_slow"] = ("road", tr, {16: L1})
    # crawled throughout, entered and left mid-segment: first and last incomplete
    tr = drive(200.0, [(47, 12.5, 5.0)])
    c["incomplete"] = ("road", tr, {16: L1})
    return c


def multi_case():
    """Edges 1 and 2 are one segment (id 16, ~682 m): slow from 50 m before node
    2 (on edge 1) until 20 m past node 3, so the queue is longer than the
    segment's last edge and the walk crosses the edge boundary inside it."""
    a = N(2) - 50.0
    n = int(math.ceil((N(3) + 20.0 - a) / 12.5))
    tr = drive(a - 7 * 75.0, [(7, 75.0, 5.0), (n, 12.5, 5.0), (8, 75.0, 5.0)])
    return "multi", tr, {16: _r(N(3) - xq(a))}


def zero_duration_trace():
    """Two points of one time a whole segment apart: edge 1's segment has
    start_time == end_time, its report divides by zero and the trace answers 500."""
    return [(100.0, T0), (N(2) + 100.0, T0), (N(3) + 100.0, T0 + 10.0), (N(4) + 100.0, T0 + 20.0)]


def break_case():
    """A gap of 2050 m (> breakage_distance) inside a slow run: chain 1 crawls
    from 60 m before node 2 to 20 m past it; chain 2 starts 2050 m on (edge 8),
    crawls 20 m past node 9, drives on, crawls the last 40 m of edge 9 and on.
    The segments at the break are incomplete; no interval crosses it."""
    a = N(2) - 60.0
    one = drive(a - 6 * 75.0, [(6, 75.0, 5.0), (6, 12.5, 5.0), (1, 5.0, 5.0)])   # ends at node 2 + 20
    x2 = one[-1][0] + 2050.0
    n1 = int((N(9) + 20.0 - x2) // 12.5) + 1
    two = drive(x2, [(n1, 12.5, 5.0)], t0=one[-1][1] + 5.0)
    d = N(10) - 40.0 - two[-1][0]
    two = two + drive(two[-1][0], [(4, d / 4.0, 5.0), (5, 12.0, 5.0), (4, 75.0, 5.0)], t0=two[-1][1])[1:]
    b = two[n1 + 4][0]
    return "long", one + two, {16: _r(N(2) - xq(a)), 80: _r(N(10) - xq(b))}


def fine_case():
    """72 nodes 42.6 m apart driven at 1 s sampling: more than 64 segments and
    more than 128 points in one trace, with three slow stretches (2 m/s)."""
    legs = []
    for _ in range(3):
        legs += [(55, 15.0, 1.0), (45, 2.0, 1.0)]
    legs += [(12, 15.0, 1.0)]
    return "fine", drive(20.0, legs), None


def city_batch(synth, city, seed=24):
    """40 traces x 30 points at 5 s on the 1.5 km city, sigma 15 m; runs of 3-6
    consecutive intervals last 8 x as long (about 7 km/h between about 54)."""
    b = synth.make_traces(city, 40, 30, interval_s=5.0, noise_sigma_m=15.0, accuracy=15.0, seed=5)
    b = {k: np.array(b[k]) for k in ("trace_off", "lat", "lon", "time", "accuracy")}
    rng = np.random.RandomState(seed)
    tm = b["time"].astype(np.float64).copy()
    off = b["trace_off"]
    for t in range(len(off) - 1):
        a, e = int(off[t]), int(off[t + 1])
        dt = np.diff(tm[a:e])
        k = 0
        while k < len(dt):
            k += rng.randint(3, 8)            # free-flowing intervals
            run = rng.randint(3, 7)           # 3-6 slow ones
            dt[k:k + run] *= 8.0
            k += run
        tm[a + 1:e] = tm[a] + np.cumsum(dt)
    b["time"] = tm
    return b
