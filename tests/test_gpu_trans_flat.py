"""k_trans_sub's flat pair loop, against the CPU oracle, bit
for bit: the pairs of a wave's columns are laid end to end over its 64 lanes,
so which lane answers which pair depends on the pair counts of the columns
that share the wave.

The graph is two bundles of parallel east-west roads 3 m apart, in 100 m edges,
joined at a node west of them.  A road ends where its bundle's next zone
(200 m of road) has fewer roads, so a probe on the bundle's centre line has
exactly its zone's number of edge candidates (a two-way road gives two, the odd
bundle's first road is one-way): 15, 9, 7, 5, 3, 1 and 16, 12, 10, 8, 6, 4, 2.
Under the natural-order plan (OTM_SMALL_POINTS huge) a wave's first pass takes
points 8w ... 8w + 7 (4w ... 4w + 3 at 16 lanes per column), so a batch lays
out which columns share a wave; every case asserts from the oracle's ncand and
col_prev that the wave totals it was built for occur, and runs under the
spatial-order plan too, with the work counters on and off.

The oracle never links a column to a point without candidates: the next point
of the trace starts a new chain.  "A column with Kp or Kq = 0" therefore shows
as unlinked groups between linked ones, which is what the off-graph case
asserts.
"""
import math

import numpy as np
import pytest

import handgraph
from test_gpu_graph_words import _batch, _check

pytestmark = pytest.mark.gpu

LAT0 = 40.0
MPD = handgraph.MPD
LS = MPD * math.cos(math.radians(LAT0))
ZONE, EDGE, GAP = 200.0, 100.0, 3.0
BUNDLES = {"o": (0.0, [15, 9, 7, 5, 3, 1]), "e": (2000.0, [16, 12, 10, 8, 6, 4, 2])}
R20 = dict(search_radius=20.0, max_search_radius=20.0)
FACTOR = 5.0  # meili's max_route_distance_factor: a column's bound is 5 x its great-circle step
OFF = ("o", 1, 100.0, 600.0)  # 600 m north of the odd bundle: no candidates
S1 = ("e", 2, 50.0)  # a one-point trace: an unlinked column


def _bundles(path):
    nodes, edges, segs = [], [], []

    def edge(a, b, seg):
        if seg:
            segs.append(((len(segs) + 1) << 3, None))
            edges.append(dict(**{"from": a, "to": b}, way=100 + len(edges), seg=len(segs) - 1, seg_pos=0,
                              flags=handgraph.SEG_BEGIN | handgraph.SEG_END, level=0))
        else:
            edges.append(dict(**{"from": a, "to": b}, way=100 + len(edges), seg=-1, level=0))

    for name, (north, counts) in BUNDLES.items():
        odd = counts[0] % 2
        nroads = (counts[0] + 1) // 2
        hub = len(nodes)
        nodes.append((LAT0 + north / MPD, -100.0 / LS))
        for r in range(nroads):
            # the road's share of a zone's count: road 0 of the odd bundle is
            # one-way (1), every other road two-way (2)
            need = 2 * r + 1 if odd else 2 * r + 2
            zones = sum(1 for c in counts if c >= need)
            y = north + (r - 0.5 * (nroads - 1)) * GAP
            prev = hub
            for i in range(int(zones * ZONE / EDGE) + 1):
                nodes.append((LAT0 + y / MPD, i * EDGE / LS))
                cur = len(nodes) - 1
                edge(prev, cur, True)
                if not (odd and r == 0):
                    edge(cur, prev, False)
                prev = cur
    handgraph.write(path, nodes, edges, segs)
    return path


def _pt(spec):
    """(bundle, zone count, metres into the zone[, metres north of the centre
    line]) -> (north m, east m); 25-75 and 125-175 m into a zone keep every node
    more than the search radius away: each road gives its one edge under the
    probe and no node candidate."""
    name, count, x = spec[:3]
    north, counts = BUNDLES[name]
    return (north + (spec[3] if len(spec) > 3 else 0.0), counts.index(count) * ZONE + x)


def _traces(specs):
    return [[_pt(s) + (5.0 * i,) for i, s in enumerate(t)] for t in specs]


def _pair(name, count, a=50.0, b=150.0):
    """two probes of one zone, 100 m apart: a count x count column"""
    return [(name, count, a), (name, count, b)]


# wave totals at 8 lanes per column, then at 16: {wave: pairs}
CASES = {
    # exactly 64, 63 and 65 pairs; 1 x 1 columns; 31 points
    "edges": dict(
        traces=[_pair("e", 8)] + [[S1]] * 6
        + [[("o", 7, 150.0), ("o", 5, 50.0), ("o", 5, 150.0)], [("o", 3, 150.0), ("o", 1, 50.0)]] + [[S1]] * 3
        + [_pair("e", 8), _pair("o", 1)] + [[S1]] * 4
        + [[("o", 9, 150.0), ("o", 7, 50.0)], [S1], [S1]]
        + [[("o", 1, 30.0), ("o", 1, 50.0), ("o", 1, 70.0)]],
        totals8={0: 64, 1: 63, 2: 65, 3: 2}, totals16={0: 64, 4: 65, 6: 63, 7: 2}, npoints=31),
    # 180 pairs in a wave, columns over [0,4) [4,52) [52,116) [116,180) with
    # unlinked groups between them; then a trace broken by an off-graph point
    "big": dict(
        traces=[_pair("e", 2), [S1], [S1], [("e", 6, 50.0), ("e", 8, 150.0), ("e", 8, 50.0), ("e", 8, 150.0)]]
        + [[("o", 5, 50.0), ("o", 5, 150.0), OFF, ("o", 3, 50.0), ("o", 3, 150.0)]] + [[S1]] * 2,
        totals8={0: 180, 1: 34}, totals16={0: 4, 1: 176, 2: 25, 3: 9}, npoints=15, offgraph=10),
    # ordinary columns beside one for the wide list (12 x 12) and one for the
    # search tiers (a 300 m step: bound 1500 m over an 800 m index)
    "mixed": dict(
        traces=[_pair("e", 8), _pair("e", 12), [("e", 4, 50.0), ("e", 2, 150.0)], _pair("e", 6)],
        totals8={0: 100}, totals16={0: 208, 1: 36}, npoints=8, spilled=[5], eng=dict(index_radius_m=800.0)),
    # the wide pass: six columns of 9-16 candidates a side, all of different
    # sizes; at 8 lanes the first wave has no pair of its own at all
    "wide": dict(
        traces=[_pair("e", 16), _pair("e", 12), _pair("e", 10), _pair("o", 9),
                [("o", 15, 150.0), ("o", 9, 50.0)], [("e", 12, 150.0), ("e", 10, 50.0)], _pair("e", 8)],
        totals8={0: 0, 1: 64}, totals16={0: 400, 1: 181, 2: 255, 3: 64}, npoints=14, nwide=6),
    # a near index of 150 m: 20 m steps (bound 100 m) and 100 m steps (bound
    # 500 m, the full index) in one wave
    "near": dict(
        traces=[_pair("e", 8, 40.0, 60.0), _pair("e", 6), _pair("o", 5, 40.0, 60.0), _pair("o", 3)],
        totals8={0: 134}, totals16={0: 100, 1: 34}, npoints=8, near=150.0, eng=dict(index_near_m=[150.0])),
}


def _wave_totals(orc, lanes, skip=()):
    """pairs per wave of the natural-order plan's first pass: the columns that
    the pass answers itself (linked, at most KC candidates a side, not in
    `skip`: the columns the index cannot answer)"""
    per, kc = 64 // lanes, (8 if lanes == 8 else 16)
    k, prev = orc["ncand"].astype(np.int64), orc["col_prev"]
    tot = {}
    for p in range(len(k)):
        q = prev[p]
        own = q >= 0 and k[p] <= kc and k[q] <= kc and p not in skip
        tot[p // per] = tot.get(p // per, 0) + (int(k[p] * k[q]) if own else 0)
    return tot


_ORACLE = {}


@pytest.fixture(scope="module")
def bundles(tmp_path_factory):
    return _bundles(str(tmp_path_factory.mktemp("bundles") / "bundles.otmg"))


@pytest.fixture(params=["natural", "spatial"])
def plan(request, monkeypatch):
    monkeypatch.setenv("OTM_SMALL_POINTS", str(1 << 40) if request.param == "natural" else "0")
    return request.param


@pytest.mark.parametrize("lanes", [8, 16])
@pytest.mark.parametrize("case", list(CASES))
def test_flat_pairs(bundles, oracle, results_equal, plan, case, lanes):
    c = CASES[case]
    b = _batch(_traces(c["traces"]), LAT0, LS)
    if case not in _ORACLE:  # computed once per case, shared, never changed
        _ORACLE[case] = oracle.match_batch(oracle.Graph(bundles), b, p=oracle.params(**R20), keep_stages=True,
                                           nthreads=4)
    orc = _ORACLE[case]
    # the case occurs: the batch's layout, by the oracle's own stage outputs
    k, prev, gc = orc["ncand"], orc["col_prev"], orc["gc"]
    assert len(k) == c["npoints"] and (orc["traces"]["error_kind"] == 0).all()
    spilled = c.get("spilled", ())
    tot = _wave_totals(orc, lanes, skip=spilled)
    for w, n in c["totals8" if lanes == 8 else "totals16"].items():
        assert tot[w] == n, "wave %d: %d pairs, built for %d (%s)" % (w, tot[w], n, tot)
    if case == "edges":
        assert c["npoints"] % 8 and ((k[prev[prev >= 0]] == 1) & (k[prev >= 0] == 1)).sum() >= 3  # 1 x 1 columns
    if "offgraph" in c:
        p = c["offgraph"]
        assert k[p] == 0 and prev[p] < 0 and prev[p + 1] < 0 and prev[p - 1] >= 0 and prev[p + 2] >= 0
    for p in spilled:
        assert FACTOR * gc[p] > 1.5 * c["eng"]["index_radius_m"] and prev[p] >= 0
        assert all(FACTOR * gc[x] < 0.75 * c["eng"]["index_radius_m"] for x in range(len(k)) if x != p and prev[x] >= 0)
    if "nwide" in c:
        lk = np.nonzero(prev >= 0)[0]
        wide = [int(k[p] * k[prev[p]]) for p in lk if 8 < max(k[p], k[prev[p]]) <= 16]
        assert len(wide) == c["nwide"] == len(set(wide))
    if "near" in c:
        for w0 in range(0, len(k), 64 // lanes):
            bounds = [FACTOR * gc[p] for p in range(w0, min(len(k), w0 + 64 // lanes)) if prev[p] >= 0]
            assert min(bounds) < 0.8 * c["near"] and max(bounds) > 1.25 * c["near"]
    # 1500 m: every bound of these batches (at most 5 x 100 m) but a spilled column's
    eng = dict(dict(index_radius_m=1500.0), **c.get("eng", {}))
    res, spill = _check(bundles, b, orc, results_equal, meili=R20, trans_lanes=lanes, **eng)
    assert spill["trans_online"] == len(spilled)  # those alone, answered by the search tiers once
