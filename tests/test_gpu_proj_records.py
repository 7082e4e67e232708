"""Projection and node snap from the packed graph records (DESIGN.md §4:
the per-edge projection record and the 16-byte shape-point records), against
the CPU oracle, bit for bit.

Every projection on the device -- the lane tier's snap pass, the wave tier's
snap pass and output, the interpolated points -- reads an edge record and then
a segment's two point records; the node a projection snaps to comes out of the
same words (the start node's representative edge from the edge record, the end
node's from the last point's end word).  The hand-built graphs below hold the
shapes where that can go wrong: edges of 1, 2 and 15 shape segments (the
format's most), probes at
the first, an interior and the last segment, at the first and the last shape
point, at an interior vertex from both sides, past a sink, at a T-junction
whose representative edge is not the probed one, and repeated shape points.
Each runs under both launch plans (the second puts every probe on the wave
tier) and with the work counters on and off.
"""
import math

import numpy as np
import pytest

import handgraph
from test_gpu_graph_words import R50, _batch, _check, _oracle, batch_path  # noqa: F401  (batch_path: a fixture)

MPD = handgraph.MPD
LAT0 = 40.0
LS = MPD * math.cos(math.radians(LAT0))


def _ll(n, e):
    """(lat, lon) of the point n metres north and e metres east of (LAT0, 0)."""
    return (LAT0 + n / MPD, e / LS)


def _cum(shape):
    """handgraph.write's cumulative metres of a shape, as float32."""
    sh = [(np.float32(a), np.float32(b)) for a, b in shape]
    out, cum = [np.float32(0.0)], 0.0
    for (pla, plo), (la, lo) in zip(sh, sh[1:]):
        dy = (float(la) - float(pla)) * MPD
        dx = (float(lo) - float(plo)) * MPD * math.cos(math.radians(0.5 * (float(la) + float(pla))))
        cum += math.hypot(dx, dy)
        out.append(np.float32(cum))
    return out


# nodes of the polyline graph, metres (north, east)
_A, _B, _C, _D, _E, _F, _G = (0, 0), (0, 200), (0, 320), (0, 512), (0, 600), (100, 200), (100, 320)
_V = (30, 260)    # the corner of B-C
_M = (115, 260)   # the repeated interior point of F-G, a corner
# C..D in 15 segments, OTM_MAX_EDGE_SHAPE_SEGS: the most the graph reader takes (an edge of 16 is refused at load)
_ARC = [(20.0 * math.sin(math.pi * i / 15.0), 320.0 + 12.8 * i) for i in range(16)]


def _poly_graph(path):
    """A-B one segment, two-way; B-C two segments with a corner, two-way; C->D
    15 segments, one-way; D->E one-way into the sink E; the stem B-F two-way
    (B's first outgoing edge is B->A: a T-junction whose representative is
    none of B->C, B->F); F->G with its first, an interior and its last shape
    point repeated (zero-length segments 0, 2 and 4), one-way; G->C."""
    pts = [_A, _B, _C, _D, _E, _F, _G]
    nodes = [_ll(*p) for p in pts]
    ix = {p: i for i, p in enumerate(pts)}
    shapes = {
        "AB": [_A, _B], "BA": [_B, _A], "BC": [_B, _V, _C], "CB": [_C, _V, _B], "CD": [_C] + _ARC[1:15] + [_D],
        "DE": [_D, _E], "BF": [_B, _F], "FB": [_F, _B], "FG": [_F, _F, _M, _M, _G, _G], "GC": [_G, _C],
    }
    ends = {"AB": (_A, _B), "BA": (_B, _A), "BC": (_B, _C), "CB": (_C, _B), "CD": (_C, _D), "DE": (_D, _E),
            "BF": (_B, _F), "FB": (_F, _B), "FG": (_F, _G), "GC": (_G, _C)}
    names = ["AB", "BA", "BC", "CB", "CD", "DE", "BF", "FB", "FG", "GC"]  # B's edges in this order: BA first
    edges = []
    for k, nm in enumerate(names):
        a, b = ends[nm]
        edges.append({"from": ix[a], "to": ix[b], "shape": [_ll(*p) for p in shapes[nm]], "way": 100 + k, "seg": k,
                      "seg_pos": 0, "flags": handgraph.SEG_BEGIN | handgraph.SEG_END, "level": 0})
    ids = handgraph.write(path, nodes, edges, [((k + 1) << 3, None) for k in range(len(names))])
    eid = {nm: ids[k] for k, nm in enumerate(names)}
    cum = {nm: _cum([_ll(*p) for p in shapes[nm]]) for nm in names}
    return eid, cum


# the probes, metres (north, east); consecutive points of a trace lie well over
# the interpolation distance apart, so every one is a column
_PROBES = {
    "ab_mid": (10, 100),       # the single segment's interior
    "a_before": (5, -20),      # before A: A->B at its first shape point, B->A at its last
    "b_tee": (-8, 192),        # before B->C's and B->F's start: node B, represented by B->A
    "bc_first": (12, 225),     # B-C's first segment
    "bc_last": (12, 295),      # ... its last
    "v_west": (45, 255),       # the corner's outer wedge: t == 1 on segment 0, t == 0 on segment 1,
    "v_east": (45, 265),       # from either side
    "arc_first": (8, 326),     # C->D's segment 0
    "arc_mid": (28, 416),      # ... segment 7
    "arc_last": (8, 506),      # ... segment 14
    "d_past": (-5, 518),       # past C->D's last shape point: node D (its edge D->E), D->E also at an offset
    "d_start": (6, 505),       # before D->E's start, beside C->D's last segment
    "e_past": (4, 615),        # past the sink E: D->E clamped to its length, an edge candidate
    "e_far": (0, 640),
    "f_before": (108, 190),    # before F: F->G's zero-length first segment
    "fg_first": (108, 230),    # F->G's segment 1
    "m_west": (128, 258),      # the outer wedge of the repeated interior point, from either side
    "m_east": (128, 262),
    "fg_last": (92, 300),      # segment 3
    "g_past": (105, 330),      # past G: the zero-length last segment
}
_TRACES = [["ab_mid", "a_before", "b_tee", "bc_first", "v_west", "bc_last"],
           ["v_east", "arc_first", "arc_mid", "arc_last", "d_past", "e_past"],
           ["d_start", "e_far"],
           ["f_before", "fg_first", "m_west", "fg_last", "g_past"],
           ["g_past", "m_east", "f_before"]]


@pytest.fixture(scope="module")
def poly(tmp_path_factory, oracle):
    path = str(tmp_path_factory.mktemp("proj") / "poly.otmg")
    eid, cum = _poly_graph(path)
    order = [nm for t in _TRACES for nm in t]
    b = _batch([[_PROBES[nm] + (5.0 * i,) for i, nm in enumerate(t)] for t in _TRACES], LAT0, LS)
    orc = _oracle(oracle, path, b, R50)
    P = len(b["lat"])
    edge = orc["cand_edge"].reshape(P, -1)
    off = orc["cand_off"].reshape(P, -1)
    cands = {}
    for p, nm in enumerate(order):
        cands.setdefault(nm, [(int(edge[p, j]), np.float32(off[p, j])) for j in range(int(orc["ncand"][p]))])
    return dict(path=path, eid=eid, cum=cum, batch=b, orc=orc, cands=cands)


def _offs(cands, e):
    return [o for (x, o) in cands if x == e]


def test_polyline_cases_hold(poly):
    """The oracle's candidates show each case the probes were placed for (a
    property of the spec and the fixture, not of the device code)."""
    eid, cum, c = poly["eid"], poly["cum"], poly["cands"]
    assert all(len(v) >= 1 for v in c.values())
    (o,) = _offs(c["ab_mid"], eid["AB"])
    assert 0.0 < o < cum["AB"][-1]
    # start-node snap; A's only outgoing edge is A->B
    assert c["a_before"] == [(eid["AB"], np.float32(0.0))]
    # the T-junction: B->C and B->F project at offset 0, node B is carried by B->A
    assert eid["BA"] not in (eid["BC"], eid["BF"])
    assert np.float32(0.0) in _offs(c["b_tee"], eid["BA"])
    assert not _offs(c["b_tee"], eid["BC"]) and not _offs(c["b_tee"], eid["BF"])
    (o,) = _offs(c["bc_first"], eid["BC"])
    assert 0.0 < o < cum["BC"][1]
    (o,) = _offs(c["bc_last"], eid["BC"])
    assert cum["BC"][1] < o < cum["BC"][2]
    # an interior vertex: no snap, the vertex's own cumulative metres
    for nm in ("v_west", "v_east"):
        assert _offs(c[nm], eid["BC"]) == [cum["BC"][1]] and _offs(c[nm], eid["CB"]) == [cum["CB"][1]]
    (o,) = _offs(c["arc_first"], eid["CD"])
    assert 0.0 < o < cum["CD"][1]
    (o,) = _offs(c["arc_mid"], eid["CD"])
    assert cum["CD"][7] < o < cum["CD"][8]
    (o,) = _offs(c["arc_last"], eid["CD"])
    assert len(cum["CD"]) == 16 and cum["CD"][14] < o < cum["CD"][15]
    # end-node snap: C->D becomes node D, carried by D->E; D->E is also an edge candidate
    assert not _offs(c["d_past"], eid["CD"])
    assert sorted(_offs(c["d_past"], eid["DE"]))[0] == 0.0 and len(_offs(c["d_past"], eid["DE"])) == 2
    assert _offs(c["d_start"], eid["DE"]) == [np.float32(0.0)] and len(_offs(c["d_start"], eid["CD"])) == 1
    # the sink: clamped to the edge's length, still an edge candidate
    for nm in ("e_past", "e_far"):
        assert c[nm] == [(eid["DE"], cum["DE"][-1])]
    # repeated shape points
    assert cum["FG"][0] == cum["FG"][1] and cum["FG"][2] == cum["FG"][3] and cum["FG"][4] == cum["FG"][5]
    assert not _offs(c["f_before"], eid["FG"])  # offset 0: node F
    (o,) = _offs(c["fg_first"], eid["FG"])
    assert 0.0 < o < cum["FG"][2]
    for nm in ("m_west", "m_east"):
        assert _offs(c[nm], eid["FG"]) == [cum["FG"][2]]
    (o,) = _offs(c["fg_last"], eid["FG"])
    assert cum["FG"][3] < o < cum["FG"][4]
    # past a repeated last point: segment 3 at t == 1 ties with the zero-length segment 4 and wins (the
    # smaller index), and is not the edge's last: no end-node snap, the edge at its full length
    assert _offs(c["g_past"], eid["FG"]) == [cum["FG"][5]]


@pytest.mark.gpu
def test_polyline(poly, results_equal, batch_path):
    _check(poly["path"], poly["batch"], poly["orc"], results_equal, meili=R50)


@pytest.mark.gpu
@pytest.mark.parametrize("grid_mult", [1, 2, 4])
def test_polyline_wave_tier_grids(poly, results_equal, monkeypatch, grid_mult):
    # the wave tier's scan reads cell_ent and ent_geo by entry index: the
    # entries' order changes with the device grid's cell size
    monkeypatch.setenv("OTM_SMALL_POINTS", str(1 << 40))
    _check(poly["path"], poly["batch"], poly["orc"], results_equal, meili=R50, grid_mult=grid_mult)


@pytest.mark.gpu
def test_bent_hub(tmp_path, oracle, results_equal, batch_path):
    # 5 two-way spokes of two shape segments each: 10 edges within the radius
    # of a probe at the hub, over the lane list's 8, so the "large" plan
    # reaches the wave tier through the spill list
    n, length = 5, 90.0
    nodes, edges = [_ll(0, 0)], []
    for i in range(n):
        a = 2.0 * math.pi * i / n
        tip = (length * math.cos(a), length * math.sin(a))
        mid = (45.0 * math.cos(a) - 6.0 * math.sin(a), 45.0 * math.sin(a) + 6.0 * math.cos(a))
        nodes.append(_ll(*tip))
        out = [_ll(0, 0), _ll(*mid), _ll(*tip)]
        edges.append({"from": 0, "to": i + 1, "shape": out, "way": 5000 + i, "seg": i, "seg_pos": 0,
                      "flags": handgraph.SEG_BEGIN | handgraph.SEG_END, "level": 0})
        edges.append({"from": i + 1, "to": 0, "shape": out[::-1], "way": 5000 + i, "seg": -1, "level": 0})
    path = str(tmp_path / "hub.otmg")
    handgraph.write(path, nodes, edges, [((i + 1) << 3, None) for i in range(n)])
    traces = []
    for i in range(2):
        a = 2.0 * math.pi * i / n
        at = lambda d, side=0.0: (d * math.cos(a) - side * math.sin(a), d * math.sin(a) + side * math.cos(a))
        pts = [(0.0, 0.0), at(40.0, 4.0), (3.0, 0.0), at(50.0, 9.0), (0.0, -2.0), at(88.0, 2.0)]
        traces.append([(x, y, 5.0 * k) for k, (x, y) in enumerate(pts)])
    b = _batch(traces, LAT0, LS)
    orc = _oracle(oracle, path, b, R50)
    res, spill = _check(path, b, orc, results_equal, meili=R50)
    P = len(b["lat"])
    off = orc["cand_off"].reshape(P, -1)
    valid = np.arange(off.shape[1])[None, :] < orc["ncand"][:, None]
    assert ((off > 0.0) & valid).any() and ((off == 0.0) & valid).any()  # edge and node candidates
    if batch_path == "large":
        assert spill["cand_wave"] > 0
