"""An independent float64 reference of rule 7d: the traversals
of a trace, one per traversed edge, from an implementation's own stage arrays
(states, candidate edges and offsets, the interpolated points' positions).

Built from specref's pieces (step, Anchors, step_boundary, tol_time, tol_cut,
tol_route); the chain loop is restated here, so nothing of
specref.segments_of_chain's own grouping is reused: test_traversals.py regroups
these traversals by rule 7's join and compares the result with the oracle's
segment records, which pins this file to what is already pinned.  It shares no
code with reporter_amd/.

A boundary is (time, shape index, known, bound, inside): `known` False where
the reference cannot decide it (specref.step_boundary); `bound` the time's
error bound; `inside` 0, or the boundary lies inside a step with interpolated
points (1: none of them an anchor, 2: anchored).
"""
import math

import numpy as np

import specref as sr

KMAX = sr.KMAX
CHAIN_START, CHAIN_END, FROM_START, TO_END, INTERNAL, SEGMENT_FIRST = 1, 2, 4, 8, 16, 32


class Trav(object):
    __slots__ = ("edge", "off0", "off1", "begin", "end", "flags", "segment", "way_id")

    def __init__(self, edge, off0, off1, begin, end):
        self.edge, self.off0, self.off1, self.begin, self.end = int(edge), off0, off1, begin, end
        self.flags, self.segment, self.way_id = 0, -1, 0


def chain_traversals(G, P, t0, times, cols, states, cand_edge, cand_off, ipos, place, latlon):
    """The traversals of one chain (cols: its columns, states: their chosen
    slots; t0: the trace's first point), their boundaries made from `ipos`
    with `place`'s ambiguity and cut flags (specref.placements on the same
    states).  A chain of one state has none."""
    Utab = sr._utab(G, P)
    out = []
    if len(cols) < 2:
        return out
    p = cols[0]
    e, o = int(cand_edge[p * KMAX + states[0]]), float(cand_off[p * KMAX + states[0]])
    cur = Trav(e, o, None, (times[p], p - t0, True, 0.0, 0), None)
    curmax = o
    for k in range(1, len(cols)):
        q, p = cols[k - 1], cols[k]
        a, b = q * KMAX + states[k - 1], p * KMAX + states[k]
        ei, oi = int(cand_edge[a]), float(cand_off[a])
        ej, oj = int(cand_edge[b]), float(cand_off[b])
        s = sr.step(G, Utab, ei, oi, ej, oj)
        assert s.kind is not None, "chosen states without a route"
        if s.kind != "route":                                   # forward along the edge, or a stay
            curmax = max(curmax, oj)
            continue
        R, n = s.r, len(s.path)
        an = None
        if p - q >= 2:
            an = sr.Anchors(q, p, ipos, None, place.amb, place.cut, latlon[0], latlon[1])

        def bound(x, j, at_end=False, q=q, p=p, R=R, n=n, an=an):
            if an is None or len(an.pts) == 1 and not an.amb:   # the two-state rule
                dt = times[p] - times[q]
                tm = times[q] + dt * (x / R) if R > 0 else times[q]
                return (tm, (p if (at_end or R <= x) else q) - t0, True, sr.tol_time(n, dt), 0 if an is None else 1)
            tm, sh, ok, tt = sr.step_boundary(times, an, q, p, R, sr.tol_route(n, 0.0, R, 0.0), x,
                                              sr.tol_cut(j, x, 0.0), j, at_end)
            return (tm, sh - t0, ok, tt, 2 if len(an.pts) > 1 else 1)
        start = 0.0 if oi == 0 else G.elen[ei] - oi
        if oi != 0:                                             # a route from a node candidate starts at its node
            cur.off1, cur.end = float(G.elen[ei]), bound(start, 0, oj == 0 and n == 0)
            out.append(cur)
        d = 0.0
        for j, g in enumerate(s.path):
            xb = start + d
            d += G.elen[g]
            out.append(Trav(g, 0.0, float(G.elen[g]), bound(xb, j), bound(start + d, j + 1, oj == 0 and j == n - 1)))
        cur = Trav(ej, 0.0, None, bound(start + d, n, oj == 0), None)
        curmax = oj
    last = cols[-1]
    if curmax != 0.0:                                           # a chain ending on a node candidate ends at the node
        cur.off1, cur.end = curmax, (times[last], last - t0, True, 0.0, 0)
        out.append(cur)
    return out


def joins(G, pe, e):
    """Rule 7's join of a traversal on edge e to the one before it on pe."""
    if G.eseg[e] >= 0:
        return bool(G.eseg[pe] == G.eseg[e] and G.eseg_pos[e] == G.eseg_pos[pe] + 1)
    return bool(G.eseg[pe] < 0 and ((int(G.eflags[e]) ^ int(G.eflags[pe])) & sr.INTERNAL) == 0)


def finish_trace(G, chains):
    """chains: the lists chain_traversals returned for one trace, in order.
    Sets every record's flags, way id and `segment` (the trace's group index)
    -> the trace's records in order."""
    out, seg = [], -1
    for ch in chains:
        for k, tv in enumerate(ch):
            first = k == 0 or not joins(G, ch[k - 1].edge, tv.edge)
            seg += 1 if first else 0
            tv.segment = seg
            tv.way_id = int(G.eway[tv.edge])
            tv.flags = ((CHAIN_START if k == 0 else 0) | (CHAIN_END if k == len(ch) - 1 else 0) |
                        (FROM_START if tv.off0 == 0.0 else 0) | (TO_END if tv.off1 == float(G.elen[tv.edge]) else 0) |
                        (INTERNAL if G.eseg[tv.edge] < 0 and int(G.eflags[tv.edge]) & sr.INTERNAL else 0) |
                        (SEGMENT_FIRST if first else 0))
            out.append(tv)
    return out


def segments_of(G, recs):
    """The trace's records regrouped by `segment` into specref.Seg records."""
    segs, groups = [], {}
    for tv in recs:
        groups.setdefault(tv.segment, []).append(tv)
    for key in sorted(groups):
        gr = groups[key]
        f, l = gr[0], gr[-1]
        sg = int(G.eseg[f.edge])
        s = sr.Seg()
        if sg >= 0:
            s.start_valid = bool(f.off0 == 0.0 and G.eseg_pos[f.edge] == 0)
            s.end_valid = bool(l.off1 == G.elen[l.edge] and G.eseg_pos[l.edge] == G.gn[sg] - 1)
            s.segment_id, s.internal = int(G.gid[sg]), False
            s.length = int(math.floor(G.glen[sg] + 0.5)) if s.start_valid and s.end_valid else -1
        else:
            s.start_valid, s.end_valid = f.off0 == 0.0, bool(l.off1 == G.elen[l.edge])
            s.segment_id, s.length = None, -1
            s.internal = bool(int(G.eflags[f.edge]) & sr.INTERNAL)
        s.start_time = f.begin[0] if s.start_valid else None
        s.end_time = l.end[0] if s.end_valid else None
        s.begin_shape_index, s.begin_known, s.begin_tol, s.begin_in = f.begin[1:5]
        s.end_shape_index, s.end_known, s.end_tol, s.end_in = l.end[1:5]
        s.way_ids = []
        for tv in gr:
            if not s.way_ids or s.way_ids[-1] != tv.way_id:
                s.way_ids.append(tv.way_id)
        segs.append(s)
    return segs


def chains_from_stages(batch, is_col, state, chain_start):
    """Per trace the chains' columns, as the stage arrays show them."""
    off = np.asarray(batch["trace_off"])
    res = []
    for t in range(len(off) - 1):
        chs = []
        for p in range(int(off[t]), int(off[t + 1])):
            if not is_col[p] or state[p] < 0:
                continue
            if chain_start[p] or not chs:
                chs.append([])
            chs[-1].append(p)
        res.append(chs)
    return res


class Result(object):
    """by_trace: the records of each trace; the counts of the ambiguity caps:
    trav, bounds (2 a traversal), inside (boundaries inside steps with
    interpolated points), amb (ambiguous ones), compared_inside."""

    def __init__(self):
        self.by_trace, self.trav, self.bounds, self.inside, self.amb = [], 0, 0, 0, 0

    @property
    def compared_inside(self):
        return sum(1 for recs in self.by_trace for tv in recs for bd in (tv.begin, tv.end) if bd[4] and bd[2])


def reference(G, P, batch, chain_cols, state, cand_edge, cand_off, ipos, codes=None):
    """chain_cols: per trace the chains' columns; state / cand_edge / cand_off
    / ipos: the implementation's stage arrays; codes: per trace result codes
    (a trace not answered 200 has no records)."""
    off = np.asarray(batch["trace_off"])
    times = np.asarray(batch["time"], np.float64)
    with np.errstate(invalid="ignore"):             # (slots past ncand hold whatever the buffer held)
        co = np.asarray(cand_off, np.float64)
    ll = (np.asarray(batch["lat"], np.float32).astype(np.float64),
          np.asarray(batch["lon"], np.float32).astype(np.float64))
    sts = [[(cols, [int(state[p]) for p in cols]) for cols in chs] for chs in chain_cols]
    place = sr.placements(G, P, batch, sts, cand_edge, co)
    ip = np.asarray(ipos, np.float64)
    res = Result()
    for t, chs in enumerate(sts):
        if codes is not None and int(codes[t]) != 200:
            res.by_trace.append([])
            continue
        recs = finish_trace(G, [chain_traversals(G, P, int(off[t]), times, cols, st, cand_edge, co, ip, place, ll)
                                for cols, st in chs])
        res.by_trace.append(recs)
        res.trav += len(recs)
        for tv in recs:
            for bd in (tv.begin, tv.end):
                res.bounds += 1
                res.inside += 1 if bd[4] else 0
                res.amb += 0 if bd[2] else 1
    return res


def assert_caps(res, hand, what=""):
    """The ambiguity caps, asserted before anything is compared: none on a hand
    graph; else at most 2 % of all the case's traversal boundaries, and for a
    case with at least 100 boundaries inside steps with interpolated points
    also at most 5 % of those."""
    if hand:
        assert res.amb == 0, "%s: %d ambiguous boundaries on a hand graph" % (what, res.amb)
        return
    assert res.amb <= 0.02 * res.bounds, "%s: %d of %d boundaries ambiguous" % (what, res.amb, res.bounds)
    if res.inside >= 100:
        assert res.amb <= 0.05 * res.inside, \
            "%s: %d of %d boundaries inside steps ambiguous" % (what, res.amb, res.inside)
