"""An independent restatement of rule 7f, the matched shape:
from a graph file and a batch's rule-7d records (edge, begin_offset,
end_offset, flags, trav_off) to each trace's vertex list, one span per record
and one polyline6 string.  Plain Python on numpy float64; the graph through
specref.Graph (float sections widened from f32, so a compare of two of them is
the f32 compare); its own encoder.  It shares no code with reporter_amd/.

Nothing here is decided differently in float64 than in the kernel: the interior
test compares f32 values, the end points are one ordered double expression
(rule 7c's Coordinate), and Python's round() on a float is round-half-even as
rint is.  So every comparison against this file is exact.
"""
import numpy as np

CHAIN_START = 1


def coordinate(G, e, off):
    """Rule 7c's Coordinate at offset `off` (a float holding an f32 value) on
    edge e: the lowest shape segment s with off <= cum[s + 1] (the last one
    when there is none), t = 0 on a segment of no length."""
    s0 = int(G.eshape[e])
    m = int(G.eshape[e + 1]) - s0 - 1
    s = 0
    while s + 1 < m and not off <= G.scum[s0 + s + 1]:
        s += 1
    c0, c1 = float(G.scum[s0 + s]), float(G.scum[s0 + s + 1])
    t = 0.0 if c1 == c0 else (off - c0) / (c1 - c0)
    la0, lo0 = float(G.slat[s0 + s]), float(G.slon[s0 + s])
    return la0 + t * (float(G.slat[s0 + s + 1]) - la0), lo0 + t * (float(G.slon[s0 + s + 1]) - lo0)


def interior(G, e, b, z):
    """The shape point indices 1..m-1 of edge e with b < cum[i] < z."""
    s0 = int(G.eshape[e])
    m = int(G.eshape[e + 1]) - s0 - 1
    return [i for i in range(1, m) if b < G.scum[s0 + i] and G.scum[s0 + i] < z]


def trace_vertices(G, recs):
    """recs: the trace's records as (edge, begin_offset, end_offset, flags).
    -> (vertices [(lat, lon)] unquantised, spans [(begin_vertex, end_vertex)])."""
    vs, spans = [], []
    for e, b, z, fl in recs:
        e, b, z = int(e), float(b), float(z)
        if int(fl) & CHAIN_START:
            vs.append(coordinate(G, e, b))
        first = len(vs) - 1
        s0 = int(G.eshape[e])
        for i in interior(G, e, b, z):
            vs.append((float(G.slat[s0 + i]), float(G.slon[s0 + i])))
        vs.append(coordinate(G, e, z))
        spans.append((first, len(vs) - 1))
    return vs, spans


def quantise(x):
    return int(round(x * 1e6))


def _value(d, out):
    v = (d << 1) ^ (d >> 31)
    while True:
        g, v = v & 31, v >> 5
        out.append((g | (0x20 if v else 0)) + 63)
        if not v:
            return


def encode(q):
    """[(lat_e6, lon_e6)] -> polyline6 bytes: deltas from (0, 0), lat then lon."""
    out, pla, plo = [], 0, 0
    for la, lo in q:
        _value(la - pla, out)
        _value(lo - plo, out)
        pla, plo = la, lo
    return bytes(out)


class Shape(object):
    """vertices: int32 (n, 2) lat_e6, lon_e6; raw: float64 (n, 2) before the
    quantisation; spans: int32 (n_records, 2); vtx_off / poly_off: int64
    [n_traces + 1]; polylines: one bytes per trace."""


def reference(G, edge, begin_offset, end_offset, flags, trav_off):
    res = Shape()
    raw, spans, polys = [], [], []
    res.vtx_off, res.poly_off = [0], [0]
    for t in range(len(trav_off) - 1):
        a, b = int(trav_off[t]), int(trav_off[t + 1])
        vs, sp = trace_vertices(G, zip(edge[a:b], begin_offset[a:b], end_offset[a:b], flags[a:b]))
        raw += vs
        spans += sp
        polys.append(encode([(quantise(la), quantise(lo)) for la, lo in vs]))
        res.vtx_off.append(len(raw))
        res.poly_off.append(res.poly_off[-1] + len(polys[-1]))
    res.raw = np.array(raw, np.float64).reshape(-1, 2)
    res.vertices = np.array([(quantise(la), quantise(lo)) for la, lo in raw], np.int32).reshape(-1, 2)
    res.spans = np.array(spans, np.int32).reshape(-1, 2)
    res.vtx_off, res.poly_off = np.array(res.vtx_off, np.int64), np.array(res.poly_off, np.int64)
    res.polylines = polys
    return res
