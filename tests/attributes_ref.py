"""Rule 7g restated in plain Python: each trace's JSON body as a
string, from numpy records (reporter_amd._lib's POINT_DTYPE, SCORE_DTYPE,
TRAVERSAL_DTYPE, SHAPE_SPAN_DTYPE), the polyline bytes, the offsets and the
section mask.  Numbers by int(round(float(x) * 1000.0)) and integer formatting;
nothing here is shared with the library.
"""
import numpy as np

POINTS, SCORES, EDGES, SHAPE, ALL = 1, 2, 4, 8, 15
PT_MATCHED, PT_COLUMN = 1, 2
SC_SCORED = 1
VALID_MASKS = [m for m in range(1, 16) if not (m & SCORES and not m & POINTS)]
INVALID_MASKS = [m for m in range(1, 16) if m & SCORES and not m & POINTS] + [16, 31, 1 << 31]


def fixed(x, d):
    """F3 (d = 3) or F6 (d = 6) of x."""
    v = float(x) * (1000.0 if d == 3 else 1e6)
    if not abs(v) < 2.0 ** 53:          # NaN and the infinities too
        return "null"
    n = int(round(v))                   # round half even, as an integer
    a = -n if n < 0 else n
    p = 10 ** d
    return "%s%d.%0*d" % ("-" if n < 0 else "", a // p, d, a % p)


def f3(x):
    return fixed(x, 3)


def f6(x):
    return fixed(x, 6)


def matched_point(p, sc):
    """One MP; sc: the point's score record, or None with the scores section off."""
    fl = int(p["flags"])
    if fl & PT_MATCHED:
        s = ('{"type":"%s","edge_id":%d,"way_id":%d,"lat":%s,"lon":%s,"distance_along_edge":%s,'
             '"distance_from_trace_point":%s,"flags":%d' % (
                 "matched" if fl & PT_COLUMN else "interpolated", int(p["edge"]), int(p["way_id"]), f6(p["lat"]),
                 f6(p["lon"]), f3(p["offset"]), f3(p["distance"]), fl))
    else:
        s = '{"type":"unmatched","flags":%d' % fl
    if sc is not None and int(sc["flags"]) & SC_SCORED:
        s += (',"score":{"cost":%s,"margin":%s,"chain_cost":%s,"emission":%s,"transition":%s,"ncand":%d,"state":%d,'
              '"alt":%d,"alt_edge":%d,"alt_offset":%s,"flags":%d}' % (
                  f6(sc["cost"]), f6(sc["margin"]), f6(sc["chain_cost"]), f6(sc["emission"]), f6(sc["transition"]),
                  int(sc["ncand"]), int(sc["state"]), int(sc["alt"]), int(sc["alt_edge"]), f3(sc["alt_offset"]),
                  int(sc["flags"])))
    return s + "}"


def edge(e, span):
    """One E; span: the traversal's span record, or None with the shape section off."""
    s = ('{"id":%d,"way_id":%d,"begin_offset":%s,"end_offset":%s,"enter_time":%s,"exit_time":%s,'
         '"begin_shape_index":%d,"end_shape_index":%d,"segment":%d' % (
             int(e["edge"]), int(e["way_id"]), f3(e["begin_offset"]), f3(e["end_offset"]), f3(e["enter_time"]),
             f3(e["exit_time"]), int(e["begin_shape_index"]), int(e["end_shape_index"]), int(e["segment"])))
    if span is not None:
        s += ',"begin_vertex":%d,"end_vertex":%d' % (int(span["begin_vertex"]), int(span["end_vertex"]))
    return s + ',"flags":%d}' % int(e["flags"])


def bodies(mask, trace_off, points=None, scores=None, travs=None, trav_off=None, spans=None, poly=None, poly_off=None):
    """-> the traces' bodies (str each).  Only what the mask's sections read is needed."""
    assert mask in VALID_MASKS
    out = []
    for t in range(len(trace_off) - 1):
        parts = []
        if mask & POINTS:
            parts.append('"matched_points":[%s]' % ",".join(
                matched_point(points[k], scores[k] if mask & SCORES else None)
                for k in range(int(trace_off[t]), int(trace_off[t + 1]))))
        if mask & EDGES:
            parts.append('"edges":[%s]' % ",".join(
                edge(travs[k], spans[k] if mask & SHAPE else None)
                for k in range(int(trav_off[t]), int(trav_off[t + 1]))))
        if mask & SHAPE:
            s = bytes(poly[int(poly_off[t]):int(poly_off[t + 1])]).decode("ascii")
            parts.append('"shape":"%s"' % s.replace("\\", "\\\\"))
        out.append("{%s}" % ",".join(parts))
    return out


def blob(bods):
    """-> (bytes, body_off) of a list of bodies."""
    enc = [b.encode("ascii") for b in bods]
    return b"".join(enc), np.cumsum([0] + [len(b) for b in enc]).astype(np.int64)
