"""Matched points by the written rule (DESIGN.md §3 rule 7c), in plain Python
and float64: one record per input point, restated from the text and sharing
no code with reporter_amd/.  The pieces of rule 7 it stands on -- the route of
a step, its pieces, the closest foot on an edge, the placement -- are
tests/specref.py's.

Stage-isolated, like tests/queue_ref.py: the inputs are the batch, the traces'
codes and an implementation's own stage arrays (`Engine.debug` on the GPU, the
oracle's keep_stages arrays on the CPU): state, cand_edge, cand_off, ipos,
is_col, chain_start, col_prev.  The output says per point what the record must
hold: flags, edge and way exactly; the offset of an interpolated point within a
bound; and which points a float64 reference cannot adjudicate (`amb`, by
specref's own rules: Placed.amb for a route placement, Foot.amb for a same-edge
foot).  The coordinate and the distance follow from a record's own (edge,
offset): `coordinate` returns them with their bounds.
"""
import math

import numpy as np

import specref as sr

MATCHED, COLUMN, NODE, CHAIN_START, ROUTE, ANCHOR, SAME_EDGE = 1, 2, 4, 8, 16, 32, 64
KMAX = sr.KMAX
DBL = 2.0 ** -53               # unit roundoff of a double


def tol_coord(c):
    """Bound on |implementation's coordinate - this module's|, degrees: both
    evaluate c_s + t * (c_{s+1} - c_s), t = (off - cum_s) / (cum_{s+1} - cum_s),
    in double from the same f32 inputs.  The two differences of f32 numbers are
    exact in double; the quotient (1), the product (1) and the sum (1) round,
    each relative to a quantity no larger than the coordinate: 3 * 2^-53 * |c|
    for one evaluation, and one more for an implementation whose product and
    sum differ in the last place: 4 * 2^-53 * max(|c|, 1)."""
    return 4 * DBL * max(abs(c), 1.0)


def tol_dist(d, lat, lon):
    """Bound on the distance, metres: the coordinate's own bound on each axis
    scaled to metres (tol_coord x one degree); then, relative to d, the
    double roundings of the scale -- degrees to radians (1), the cosine (2: a
    library cosine is within 2 ulp), its product with the constant (1) -- and
    of the two axis products, the squares and their sum, and the root (5):
    9 * 2^-53 * d; and the final rounding to f32, 2^-24 * d."""
    return sr.MPD * (tol_coord(lat) + tol_coord(lon)) + 9 * DBL * d + sr.U * d


def tol_rebuilt(nsum, pos):
    """Bound on |f32 ipos - the position rebuilt in float64 from the record's
    own (edge, offset)|: specref.tol_ipos with an exact foot (the offset is the
    implementation's own f32 number): start = len - off (1), the nsum path
    lengths (nsum), the subtraction of o0 (1), the final addition (1), each
    relative to a part of pos: (nsum + 3) * 2^-24 * pos."""
    return sr.tol_ipos(0.0, nsum, abs(pos))


def shape_segment(G, e, off):
    """The lowest shape segment s of edge e with off <= cum[s + 1] (the last
    one when none is: the edge's length is its last cum)."""
    s0 = int(G.eshape[e])
    n = int(G.eshape[e + 1]) - s0 - 1
    for s in range(n):
        if off <= G.scum[s0 + s + 1]:
            return s0 + s
    return s0 + n - 1


def coordinate(G, e, off, plat, plon):
    """(lat, lon, distance) of offset `off` (the f32 number, as a float) on edge
    e, the distance from the input point (plat, plon), all in float64."""
    a = shape_segment(G, e, off)
    c0, c1 = float(G.scum[a]), float(G.scum[a + 1])
    t = 0.0 if c1 == c0 else (off - c0) / (c1 - c0)
    lat = float(G.slat[a]) + t * (float(G.slat[a + 1]) - float(G.slat[a]))
    lon = float(G.slon[a]) + t * (float(G.slon[a + 1]) - float(G.slon[a]))
    ls = sr.MPD * math.cos(math.radians(plat))
    dx, dy = (lon - plon) * ls, (lat - plat) * sr.MPD
    return lat, lon, math.sqrt(dx * dx + dy * dy)


class Points(object):
    """Per point: flags (every OTM_PT_* bit; ANCHOR from the implementation's
    own f32 ipos by the running-maximum rule), edge (-1 none), off (float64;
    exact for a column), off_tol (0 for a column), way (0 none), interp (an
    interpolated point with a place), amb (not adjudicated: its edge and
    offset are not compared), and for a route placement the winning piece's
    xs, o0 and nsum (rebuild the position as xs + (off - o0))."""

    def __init__(self, n):
        self.flags = np.zeros(n, np.uint32)
        self.edge = np.full(n, -1, np.int64)
        self.off, self.off_tol = np.zeros(n), np.zeros(n)
        self.way = np.zeros(n, np.int64)
        self.interp, self.amb = np.zeros(n, bool), np.zeros(n, bool)
        self.xs, self.o0 = np.zeros(n), np.zeros(n)
        self.nsum = np.zeros(n, np.int64)


def matched_points(G, P, batch, st, codes):
    lat = np.asarray(batch["lat"], np.float32).astype(np.float64)
    lon = np.asarray(batch["lon"], np.float32).astype(np.float64)
    off = np.asarray(batch["trace_off"], np.int64)
    state, is_col, cstart, cprev = st["state"], st["is_col"], st["chain_start"], st["col_prev"]
    cedge, coff, ipos = st["cand_edge"], st["cand_off"], st["ipos"]
    Utab = sr._utab(G, P)
    out = Points(len(lat))

    def chosen(k):
        j = k * KMAX + int(state[k])
        return int(cedge[j]), float(coff[j])

    for t in range(len(off) - 1):
        a, e = int(off[t]), int(off[t + 1])
        cols = [k for k in range(a, e) if is_col[k]]
        for k in cols:
            out.flags[k] = COLUMN
        if int(codes[t]) != 200:
            continue
        for k in cols:
            if state[k] < 0:
                continue
            ed, of = chosen(k)
            out.edge[k], out.off[k], out.way[k] = ed, of, int(G.eway[ed])
            out.flags[k] |= MATCHED | (NODE if of == 0 else 0) | (CHAIN_START if cstart[k] else 0)
        for q, p in zip(cols, cols[1:]):
            if p - q < 2 or state[q] < 0 or state[p] < 0 or int(cprev[p]) != q or cstart[p]:
                continue                        # no step: the points between keep flags 0
            (ei, oi), (ej, oj) = chosen(q), chosen(p)
            s = sr.step(G, Utab, ei, oi, ej, oj)
            assert s.kind is not None, "chosen states without a route"
            if s.kind != "route":
                # a same-edge step: the closest foot on the whole edge, clamped between the two offsets.  The
                # clamp is continuous (it moves no two offsets apart), so the foot's own bound holds after it
                lo_, hi_ = min(oi, oj), max(oi, oj)
                for k in range(q + 1, p):
                    f = sr.foot_on_edge(G, ei, float(lat[k]), float(lon[k]))
                    out.flags[k] = MATCHED | SAME_EDGE
                    out.edge[k], out.way[k] = ei, int(G.eway[ei])
                    out.off[k], out.off_tol[k] = min(max(f.off, lo_), hi_), f.tol
                    out.interp[k], out.amb[k] = True, f.amb
                continue
            pcs = sr.step_pieces(G, s, ei, oi, ej, oj)
            run = None                          # the running maximum of the step's earlier placed positions (f32)
            for k in range(q + 1, p):
                x = np.float32(ipos[k])
                if not x >= 0:
                    continue                    # unplaced: flags 0
                out.flags[k] = MATCHED | ROUTE | (ANCHOR if run is None or x >= run else 0)
                run = x if run is None or x > run else run
                out.interp[k] = True
                r = sr.place_point(G, P, lat, lon, q, k, pcs)
                if r.pos is None:
                    out.amb[k] = True           # (placed by the implementation, by none of the reference's pieces)
                    continue
                pc = pcs[r.piece]
                f = sr.foot_on_edge(G, pc.edge, float(lat[k]), float(lon[k]))
                ident = pc.kind == "first" and lat[k] == lat[q] and lon[k] == lon[q]   # place_point's identity
                of, ft = (pc.o0, 0.0) if ident else (f.off, f.tol)
                # a second piece as cheap at the same place (the vertex two pieces share) widens Placed.tol: the
                # place is one, the edge either piece's -- not adjudicated here
                tie = r.tol > sr.tol_ipos(ft, pc.nsum, abs(r.pos)) * (1 + 1e-12) + 1e-300
                out.edge[k], out.way[k] = pc.edge, int(G.eway[pc.edge])
                out.off[k], out.off_tol[k] = of, ft
                out.xs[k], out.o0[k], out.nsum[k] = pc.xs, pc.o0, pc.nsum
                out.amb[k] = bool(r.amb or tie)
    return out


def oracle_stages(batch, r):
    """The stage arrays matched_points reads, from an oracle result made with
    keep_stages, which carries neither chain starts nor column flags: the
    first rebuilt as queue_ref does, the second as rule 1 shows in gc (a
    trace's first point, or gc > 0)."""
    import queue_ref
    toff = np.asarray(batch["trace_off"], np.int64)
    is_col = np.asarray(r["gc"]) > 0
    is_col[toff[:-1][np.diff(toff) > 0]] = True
    return dict(state=r["state"], cand_edge=r["cand_edge"], cand_off=r["cand_off"], ipos=r["ipos"],
                col_prev=r["col_prev"], chain_start=queue_ref.chain_starts(toff, r), is_col=is_col)
