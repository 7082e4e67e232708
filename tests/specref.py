"""An independent float64 reference of the written spec of `Match`
(rules 1-7), for tests.

The CPU oracle and the HIP kernels share an author, an evaluation order, a
grid scan and their label keys; a misreading of the spec shared by both passes
every bit-identity test.  This module is a third implementation, written from
the text of §3 and deliberately naive: plain Python and numpy in float64,
brute force over every shape segment of the graph (no grid), a textbook heap
Dijkstra over Python integers, no f32 emulation, and no helper shared with
`oracle/` or `reporter_amd/`.  It reads the `.otmg` file itself
(include/otm_graph_format.h).

Every stage function takes the previous stage's arrays as input, so a caller
can feed a stage with the reference's own upstream arrays (end to end) or
with an implementation's (stage-isolated: a disagreement upstream can neither
mask nor multiply one here).

A float64 reference and an f32 implementation may differ at decision
boundaries.  Each stage therefore also reports what is *ambiguous*, from the
reference's own values only (never from a disagreement), and the tolerances
are functions below with their derivation.

Rule 7's interpolated points are covered in full: `place_point` places a point
on its step's route (`ipos`, within tol_ipos), `Anchors` applies the monotone
filter, and `step_boundary` gives every boundary inside a step its shape index
(exact) and its time (within tol_time_anchored), from whichever `ipos` the
caller passes: the reference's own (end to end) or the implementation's
(stage-isolated).  What is ambiguous there is decided per interpolated point
and per boundary (see those three), and excludes that point or boundary alone.
The one thing a float64 reference cannot adjudicate is rule 7's tie between two
pieces of equal f32 cost at different positions ("ties: earliest piece"): it
sees such a pair as closer than its bounds and calls the point ambiguous;
that tie stays pinned by the oracle / kernel bit-identity alone.

Where the spec says "accuracy or gps_accuracy", a probe's accuracy counts when
it is positive.
"""
import heapq
import math
import struct

import numpy as np

U = 2.0 ** -24                 # unit roundoff of f32 (round to nearest: half an ulp, relative)
MPD = 111319.4954833           # metres per degree of rule 1 and rule 2
KMAX = 32                      # row stride of the candidate arrays
NONE = 1 << 62                 # "no predecessor edge": sorts after every edge id
INF = float("inf")
INTERNAL = 0x01                # edge flag: intersection-internal

DEFAULTS = dict(sigma_z=4.07, beta=3.0, max_route_distance_factor=5.0, breakage_distance=2000.0,
                interpolation_distance=10.0, search_radius=50.0, max_search_radius=100.0, gps_accuracy=5.0,
                max_candidates=32, turn_penalty_factor=200.0)


def params(**kw):
    """meili's defaults with overrides.  The engine's parameters are f32
    numbers, so the values are those f32 numbers (inputs, like the file's f32
    lengths), held as Python floats."""
    p = dict(DEFAULTS)
    p.update(kw)
    return {k: (int(v) if k == "max_candidates" else float(np.float32(v))) for k, v in p.items()}


# ------------------------------------------------------------------ tolerances
K_SQ = 12


def tol_sqdist(D):
    """Absolute bound on |f32 sqdist - float64 sqdist|: K_SQ * 2^-24 * D^2, D the
    largest |metre coordinate| of the segment's two ends relative to the probe.

    Roundings of the f32 evaluation, each relative 2^-24 on a quantity of
    magnitude <= D (or D^2 for the last three): cos of the latitude (degree to
    radian product, polynomial: 3), metres-per-degree constant (1), its product
    with the cosine (1), coordinate difference times scale (1), v = b - a (1),
    t * v (1), a + t * v (1), the two squares (1 each along its axis: 1), their
    sum (1), and the clamp parameter t (1: its error moves the foot along the
    segment, perpendicular to the residual, so it enters only through t * v).
    12 in all."""
    return K_SQ * U * D * D


def tol_emission(D, emis, sigma_z):
    """tol_sqdist / (2 sigma_z^2), plus the f32 division and the two products
    of the denominator (3 roundings relative to the emission itself)."""
    return tol_sqdist(D) / (2.0 * sigma_z * sigma_z) + 3 * U * emis


def tol_offset(length, D=0.0, v=0.0):
    """2^-24 * (7 max(edge length, 1) + 12 D + 6 D^2 / |v|), |v| the shape
    segment's length (the last term drops for a zero-length segment, t = 0).

    The offset is cum_a + t * (cum_b - cum_a) with t = -(a . v) / |v|^2, and an
    error dt moves the foot by dt |v|.  Per component a is off by <= 5 * 2^-24
    D (tol_sqdist's count) and v = b - a by <= 3 * 2^-24 D (two rounded
    products and the subtraction; the axis scale's error is relative to |v|).
    So a . v is off by |v| |da| + |a| |dv| <= 2^-24 (7 D |v| + 6 D^2) plus its
    own three roundings (4.3 * 2^-24 D |v|); divided by |v|: 2^-24 (11.3 D + 6
    D^2 / |v|).  |v|^2 and the division add 4 * 2^-24 |v|, the interpolation
    on cum three roundings on the edge length.  (The bound first written here,
    12 * 2^-24 max(edge length, 1), missed at a 300 m radius: the D^2 / |v|
    term does not shrink with the edge.)"""
    return U * (7.0 * max(length, 1.0) + 12.0 * D + (6.0 * D * D / v if v > 0 else 0.0))


def tol_gc(gc):
    """9 * 2^-24 * gc: cosine and scale (5, as in tol_sqdist), coordinate
    difference (1), product (1), squares and sum (1), square root (1)."""
    return 9 * U * gc


def tol_route(n, B, r, off_tol=0.0):
    """Bound on |f32 r - float64 r| for a route of n edges: start = len - off
    (1), n additions of lengths, + off_j (1), and B = factor * gc (1) when r is
    compared with it, one more for the difference to gc: (n + 4) * 2^-24 *
    max(B, r), plus the offsets' own tolerances when they are not the
    implementation's."""
    return (n + 4) * U * max(B, r) + off_tol


def tol_trans(n, B, r, beta, off_tol=0.0):
    """tol_route / beta: units / 64 is exact in f32 and <= B, the sum with
    |r - gc| and the division by beta are within the (n + 4) count."""
    return tol_route(n, B, r, off_tol) / beta


VIT_C = 2


def tol_viterbi(ncols, cost, input_tol=0.0):
    """columns * 2^-24 * chain cost * VIT_C: per column two f32 additions
    (transition, emission) on partial sums <= the chain cost; plus the sum of
    the inputs' own tolerances along a path when they are not the
    implementation's."""
    return ncols * U * cost * VIT_C + input_tol


def tol_time(n, dt):
    """A boundary time is t_q + dt * x / R with x <= R partial sums of the
    same n + 2 f32 terms: the quotient is within 2 (n + 4) 2^-24, the rest is
    float64.  (Steps without a placed anchor; tol_time_anchored otherwise.)"""
    return 2 * (n + 4) * U * abs(dt) + 1e-9


def tol_cut(n, x, off_tol=0.0):
    """Bound on |f32 x - float64 x| of a route position x = start + (the first
    n path lengths, summed in route order): start = len - off (1), n additions
    (n), each relative to a partial sum <= x: (n + 1) * 2^-24 * x, plus the
    offset's own tolerance when it is not the implementation's."""
    return (n + 1) * U * x + off_tol


def tol_ipos(foot_tol, n, pos, off_tol=0.0):
    """Bound on |f32 ipos - float64 ipos|, ipos = xs + (foot - o0) with xs =
    start + (n path lengths in route order): the foot's own tolerance
    (tol_offset; 0 for a foot that is exact, see Foot), start = len - off (1),
    the n additions (n), the subtraction of o0 (1) and the final addition (1),
    each relative to a quantity <= pos (every partial sum and foot - o0 are
    parts of pos): foot_tol + (n + 3) * 2^-24 * pos, plus the tolerance of q's
    offset (it enters start, or o0 on the first piece) when it is not the
    implementation's."""
    return foot_tol + (n + 3) * U * pos + off_tol


def tol_icost(D, emis, sigma_z, pos_tol, pos, gcd, beta):
    """Bound on a piece's cost sqdist / (2 sigma_z^2) + |pos - gc(q, k)| / beta:
    tol_emission of the first term; the position's and gc's own bounds, the
    subtraction and the division (2 roundings relative to |pos - gc|) over
    beta; the final sum (1, relative to the cost)."""
    d = abs(pos - gcd)
    return tol_emission(D, emis, sigma_z) + (pos_tol + tol_gc(gcd) + 2 * U * d) / beta + U * (emis + d / beta)


def tol_time_anchored(dt, den, ex, eL, eN, t=0.0):
    """A boundary time between anchors L and N is t_L + dt * (x - x_L) / (x_N -
    x_L), dt = t_N - t_L.  With x off by ex and the anchors by eL, eN, the
    quotient f <= 1 is off by (ex + eL) / den + f (eL + eN) / den <= (ex + 2 eL +
    eN) / den, den = x_N - x_L; the two f32 subtractions add 2 * 2^-24 (the
    quotient itself and the rest are float64).  The result is capped at |dt|:
    both values lie between t_L and t_N, because x lies between the anchors in
    either evaluation.  Fed the implementation's own ipos, eL = eN = 0 for
    placed anchors and only x (and R, for N = p) carries a bound.  The final
    sum is rounded to a double of magnitude |t| once in either evaluation:
    2 * 2^-53 * |t| on top (epoch seconds: 2.4e-7 s)."""
    cap = abs(dt)
    dbl = 2.0 ** -52 * abs(t)
    if not den > 0:
        return cap + dbl
    return min(cap * ((ex + 2 * eL + eN) / den + 2 * U), cap) + dbl


# ------------------------------------------------------------------ the graph file
_SECTIONS = [("node_lat", "<f4"), ("node_lon", "<f4"), ("out_off", "<i4"), ("efrom", "<i4"), ("eto", "<i4"),
             ("elen", "<f4"), ("eshape", "<i4"), ("eway", "<i8"), ("eseg", "<i4"), ("eseg_pos", "<i4"),
             ("eflags", "u1"), ("elevel", "u1"), ("espeed", "<f4"), ("eopp", "<i4"), ("slat", "<f4"),
             ("slon", "<f4"), ("scum", "<f4"), ("gid", "<u8"), ("glen", "<f4"), ("gfirst", "<i4"), ("gn", "<i4"),
             ("cell_off", "<i8"), ("cell_ent", "<u4"), ("head_out", "<u2"), ("head_in", "<u2")]
_HDR = "<8sII4i2iq3d4dQ"


class Graph(object):
    """The sections of an .otmg file as numpy arrays (floats widened to
    float64), plus per-shape-segment index arrays for the brute-force scan."""

    def __init__(self, path):
        raw = np.fromfile(path, dtype=np.uint8)
        hs = struct.calcsize(_HDR)
        hdr = struct.unpack_from(_HDR, raw, 0)
        assert hdr[0] == b"OTMGRAPH" and hdr[1] == 2, "not an .otmg version 2 file"
        for k, (name, dt) in enumerate(_SECTIONS):
            o, n = struct.unpack_from("<QQ", raw, hs + 16 * k)
            a = np.frombuffer(raw, dtype=dt, count=n // np.dtype(dt).itemsize, offset=o).copy()
            if a.dtype.kind == "f":
                a = a.astype(np.float64)
            elif a.dtype.kind in "iu" and name != "gid":
                a = a.astype(np.int64)
            setattr(self, name, a)
        self.n_nodes, self.n_edges = hdr[3], hdr[4]
        nseg = np.diff(self.eshape) - 1                   # shape segments per edge
        self.sg_edge = np.repeat(np.arange(self.n_edges), nseg)
        self.sg_first = np.cumsum(nseg) - nseg            # per edge: its first shape segment in the flat list
        self.sg_k = np.arange(len(self.sg_edge)) - self.sg_first[self.sg_edge]
        self.sg_a = self.eshape[self.sg_edge] + self.sg_k
        self.sg_b = self.sg_a + 1
        self.sg_last = self.sg_b == self.eshape[self.sg_edge + 1] - 1
        self.L = [int(math.floor(float(x) * 64.0 + 0.5)) for x in self.elen]   # rule 4: 1/64 m
        self._labels = {}
        self._utabs = {}

    def out(self, v):
        return range(int(self.out_off[v]), int(self.out_off[v + 1]))


# ------------------------------------------------------------------ rule 1
def _gc(la, lo, lb, lob):
    ls = MPD * math.cos(math.radians(0.5 * (la + lb)))
    return math.hypot((lob - lo) * ls, (lb - la) * MPD)


def columns(batch, P):
    """-> is_col (bool[P]), gc (float64[P]: distance to the previous column, 0
    for the first column and for interpolated points), amb (bool[P]: gc within
    tol_gc of interpolation_distance)."""
    off = np.asarray(batch["trace_off"])
    lat = np.asarray(batch["lat"], np.float32).astype(np.float64)
    lon = np.asarray(batch["lon"], np.float32).astype(np.float64)
    n = len(lat)
    is_col, gc, amb = np.zeros(n, bool), np.zeros(n), np.zeros(n, bool)
    for t in range(len(off) - 1):
        last = -1
        for p in range(int(off[t]), int(off[t + 1])):
            if last < 0:
                is_col[p] = True
                last = p
                continue
            d = _gc(lat[last], lon[last], lat[p], lon[p])
            amb[p] = abs(d - P["interpolation_distance"]) <= tol_gc(d)
            if d >= P["interpolation_distance"]:
                is_col[p], gc[p], last = True, d, p
    return is_col, gc, amb


def col_prev(batch, P, is_col, gc, ncand):
    """-> col_prev (int[P], -1 none), amb (bool[P]: gc within tol_gc of
    breakage_distance).  q = col_prev[p] is the column before p when both have
    candidates and gc <= breakage_distance."""
    off = np.asarray(batch["trace_off"])
    n = len(is_col)
    cp, amb = np.full(n, -1, np.int64), np.zeros(n, bool)
    for t in range(len(off) - 1):
        last = -1
        for p in range(int(off[t]), int(off[t + 1])):
            if not is_col[p]:
                continue
            if last >= 0 and ncand[p] > 0 and ncand[last] > 0:
                amb[p] = abs(gc[p] - P["breakage_distance"]) <= tol_gc(gc[p])
                if gc[p] <= P["breakage_distance"]:
                    cp[p] = last
            last = p
    return cp, amb


# ------------------------------------------------------------------ rules 2 and 3
def radius(P, acc):
    a = acc if acc > 0 else P["gps_accuracy"]
    return min(max(P["search_radius"], a), P["max_search_radius"])


class Cands(object):
    """One column's candidates: parallel lists edge, off, sqd, emis, node
    (is-node flag), D (for the tolerances), otol (the offset's tolerance), in
    rule 2's order; amb: the column
    sits on a decision boundary (see the module docstring); fired: which rules
    acted (names in a set), for tests that must see a rule fire."""

    def __init__(self):
        self.edge, self.off, self.sqd, self.emis, self.node, self.D, self.otol = [], [], [], [], [], [], []
        self.amb = False
        self.fired = set()

    def __len__(self):
        return len(self.edge)


def candidates_at(G, P, lat, lon, acc):
    r = radius(P, acc)
    r2 = r * r
    ls = MPD * math.cos(math.radians(lat))
    ax, ay = (G.slon[G.sg_a] - lon) * ls, (G.slat[G.sg_a] - lat) * MPD
    bx, by = (G.slon[G.sg_b] - lon) * ls, (G.slat[G.sg_b] - lat) * MPD
    vx, vy = bx - ax, by - ay
    l2 = vx * vx + vy * vy
    pos = l2 > 0
    traw = np.where(pos, -(ax * vx + ay * vy) / np.where(pos, l2, 1.0), 0.0)
    t = np.clip(traw, 0.0, 1.0)
    px, py = ax + t * vx, ay + t * vy
    sqd = px * px + py * py
    D = np.maximum(np.maximum(np.abs(ax), np.abs(ay)), np.maximum(np.abs(bx), np.abs(by)))
    off = np.minimum(G.scum[G.sg_a] + t * (G.scum[G.sg_b] - G.scum[G.sg_a]), G.elen[G.sg_edge])
    best = np.minimum.reduceat(sqd, G.sg_first)
    tol = tol_sqdist(D)
    out = Cands()
    near = np.nonzero(best <= r2 + np.maximum.reduceat(tol, G.sg_first))[0]
    hits, nodes = [], {}
    for e in near:
        s0 = int(G.sg_first[e])
        s1 = s0 + int(G.eshape[e + 1] - G.eshape[e] - 1)
        k = s0 + int(np.argmin(sqd[s0:s1]))                       # the first of the closest: lowest segment
        # hit test on its boundary -- unless both sides are exactly 0 (a probe on a
        # shape point at radius 0: a = 0 or b = 0, so every product and sum of
        # the projection is an exact 0 in any precision)
        if abs(sqd[k] - r2) <= tol[k] and not (sqd[k] == 0.0 and r2 == 0.0):
            out.amb = True
        if sqd[k] == r2:
            out.fired.add("hit_at_radius")
        if not sqd[k] <= r2:
            continue
        start = off[k] == 0.0
        end = (not start) and bool(G.sg_last[k]) and traw[k] >= 1.0
        # the same outcome from every segment of the edge that is as close within tolerance?
        # (around a shape point two segments are: the offset may then be either's)
        spread = 0.0
        for m in range(s0, s1):
            if not pos[m] and sqd[m] - sqd[k] <= tol[k] + tol[m]:
                out.fired.add("zero_length_segment")
            if m != k and sqd[m] - sqd[k] <= tol[k] + tol[m]:
                m_start = off[m] == 0.0
                m_end = (not m_start) and bool(G.sg_last[m]) and traw[m] >= 1.0
                if m_start != start or m_end != end:
                    out.amb = True
                else:                                             # the same candidate from either foot
                    spread = max(spread, abs(off[m] - off[k]))
        # a projection within 1e-6 of a first / last segment's end: node snap either way
        if (G.sg_k[k] == 0 and abs(traw[k]) < 1e-6 and traw[k] != 0.0 and pos[k]) or \
           (G.sg_last[k] and abs(traw[k] - 1.0) < 1e-6 and traw[k] != 1.0):
            out.amb = True
        v = -1
        if start:
            v = int(G.efrom[e])
        elif end:
            if G.out_off[G.eto[e] + 1] > G.out_off[G.eto[e]]:
                v = int(G.eto[e])
            else:
                out.fired.add("sink_end")
        if v >= 0:
            if v in nodes:
                out.fired.add("node_merge")
                if sqd[k] < nodes[v][0]:
                    nodes[v] = (sqd[k], D[k])
            else:
                nodes[v] = (sqd[k], D[k])
        else:
            hits.append((sqd[k], int(e), off[k], False, D[k], tol_offset(G.elen[e], D[k], math.sqrt(l2[k])) + spread))
    for v, (s, d) in nodes.items():
        hits.append((s, int(G.out_off[v]), 0.0, True, d, 0.0))
    hits.sort(key=lambda h: (h[0], h[1], h[2]))
    K = P["max_candidates"]
    if len(hits) > K:
        out.fired.add("cut")
        if hits[K][0] - hits[K - 1][0] <= tol_sqdist(hits[K][4]) + tol_sqdist(hits[K - 1][4]):
            out.amb = True
    ds = 2.0 * P["sigma_z"] * P["sigma_z"]
    for s, e, o, nd, d, ot in hits[:K]:
        out.otol.append(ot)
        out.edge.append(e)
        out.off.append(o)
        out.sqd.append(s)
        out.emis.append(s / ds)
        out.node.append(nd)
        out.D.append(d)
    return out


def candidates(G, batch, P, is_col):
    """-> {p: Cands} for every column p."""
    lat = np.asarray(batch["lat"], np.float32).astype(np.float64)
    lon = np.asarray(batch["lon"], np.float32).astype(np.float64)
    acc = np.asarray(batch["accuracy"], np.float32).astype(np.float64)
    return {int(p): candidates_at(G, P, lat[p], lon[p], acc[p]) for p in np.nonzero(is_col)[0]}


def cand_arrays(cands, npts):
    """{p: Cands} as the implementations' flat arrays (ncand, cand_edge,
    cand_off, cand_emis; rows of KMAX)."""
    nc = np.zeros(npts, np.int64)
    ce = np.zeros(npts * KMAX, np.int64)
    co = np.zeros(npts * KMAX)
    em = np.zeros(npts * KMAX)
    for p, c in cands.items():
        k = len(c)
        nc[p] = k
        ce[p * KMAX:p * KMAX + k] = c.edge
        co[p * KMAX:p * KMAX + k] = c.off
        em[p * KMAX:p * KMAX + k] = c.emis
    return nc, ce, co, em


# ------------------------------------------------------------------ rule 4
def turn_deg(hin, hout):
    d = (int(hout) - int(hin)) % 360
    return d if d <= 180 else 360 - d


def turn_table(factor, exp=math.exp):
    """U[0..180] = floor(factor * 64 / exp((180 - d) / 45) + 0.5)."""
    if not factor > 0:
        return [0] * 181
    return [int(math.floor(factor * 64.0 / exp((180 - d) / 45.0) + 0.5)) for d in range(181)]


def exp_series40(x):
    """The implementations' exp: 40 terms of the Taylor series in order."""
    term = total = 1.0
    for n in range(1, 41):
        term = term * x / n
        total = total + term
    return total


def labels(G, Utab, u, hin):
    """Rule 4's labels of the search from node u entered with heading hin
    (None: a node candidate), unbounded: (dep, arr), dep[g] / arr[v] = (cost,
    predecessor edge or NONE).  A bounded search's labels are these with cost
    <= the bound: a label's route only passes labels no dearer than itself."""
    key = (u, hin, Utab[0], Utab[180])
    if key in G._labels:
        return G._labels[key]
    dep, arr, heap = {}, {u: (0, NONE)}, []
    for g in G.out(u):
        c = 0 if hin is None else Utab[turn_deg(hin, G.head_out[g])]
        dep[g] = (c, NONE)
        heapq.heappush(heap, (c, NONE, g))
    while heap:
        c, pr, g = heapq.heappop(heap)
        if dep[g] != (c, pr):
            continue
        ca = c + G.L[g]
        v = int(G.eto[g])
        if (ca, g) < arr.get(v, (INF, NONE)):
            arr[v] = (ca, g)
        for h in G.out(v):
            k = (ca + Utab[turn_deg(G.head_in[g], G.head_out[h])], g)
            if k < dep.get(h, (INF, NONE)):
                dep[h] = k
                heapq.heappush(heap, (k[0], k[1], h))
    G._labels[key] = (dep, arr, Utab)
    return G._labels[key]


def _utab(G, P):
    f = P["turn_penalty_factor"]
    if f not in G._utabs:
        G._utabs[f] = turn_table(f)
    return G._utabs[f]


class Step(object):
    """The route from candidate i to candidate j: kind ("forward", "stay",
    "route" or None when unlabelled), cost (integer label cost), units, path
    (fully traversed edges in route order), r (float64 metres)."""
    __slots__ = ("kind", "cost", "units", "path", "r")

    def __init__(self, kind=None, cost=0, units=0, path=(), r=INF):
        self.kind, self.cost, self.units, self.path, self.r = kind, cost, units, path, r


def step(G, Utab, ei, oi, ej, oj):
    """Rule 4's route between two candidates, unbounded."""
    if ei == ej and oj >= oi:
        return Step("forward", 0, 0, (), oj - oi)
    if ei == ej and oi > 0 and oj > 0:
        return Step("stay", 0, 0, (), 0.0)
    if oi == 0:                                            # node candidate: at its node, no heading
        u, hin, start = int(G.efrom[ei]), None, 0.0
    else:                                                  # edge candidate: the rest of its edge first
        u, hin, start = int(G.eto[ei]), int(G.head_in[ei]), G.elen[ei] - oi
    dep, arr, _ = labels(G, Utab, u, hin)
    lab = arr.get(int(G.efrom[ej])) if oj == 0 else dep.get(ej)
    if lab is None:
        return Step()
    path, pr = [], lab[1]
    while pr != NONE:
        path.append(pr)
        pr = dep[pr][1]
    path.reverse()
    units, h, d = 0, hin, 0.0
    for g in path:
        units += 0 if h is None else Utab[turn_deg(h, G.head_out[g])]
        d += G.elen[g]
        h = int(G.head_in[g])
    if oj != 0:
        units += 0 if h is None else Utab[turn_deg(h, G.head_out[ej])]
    assert units + sum(G.L[g] for g in path) == lab[0], "label cost is not its route's cost"
    return Step("route", lab[0], min(units, (1 << 24) - 1), tuple(path), start + d + oj)


class Trans(object):
    """Column p's transition matrix from q = col_prev[p]: T (Kq x Kp float64,
    inf = none), tol (same shape: tol_trans per entry), amb (same shape:
    entries on a decision boundary), steps (Kq x Kp list of Step)."""


def transitions(G, P, ncand, cand_edge, cand_off, gc, cprev, off_tol=None, gc_own=False):
    """-> {p: Trans} for every p with col_prev[p] >= 0.  off_tol: per slot
    (flat, as cand_off) offset tolerances when the offsets are the
    reference's own, None when they are the implementation's (exact inputs);
    gc_own: gc is the reference's own too, so gc and B carry tol_gc."""
    Utab = _utab(G, P)
    out = {}
    for p in np.nonzero(np.asarray(cprev) >= 0)[0]:
        p = int(p)
        q = int(cprev[p])
        Kq, Kp = int(ncand[q]), int(ncand[p])
        B = P["max_route_distance_factor"] * float(gc[p])
        cmax = math.floor(B * 64.0)
        tr = Trans()
        tr.T, tr.tol = np.full((Kq, Kp), INF), np.zeros((Kq, Kp))
        tr.amb = np.zeros((Kq, Kp), bool)
        tr.steps = [[None] * Kp for _ in range(Kq)]
        tr.B, tr.gc = B, float(gc[p])
        gt = tol_gc(tr.gc) if gc_own else 0.0
        Bt = P["max_route_distance_factor"] * gt + U * B          # B = factor * gc, one f32 product
        for i in range(Kq):
            ei, oi = int(cand_edge[q * KMAX + i]), float(cand_off[q * KMAX + i])
            for j in range(Kp):
                ej, oj = int(cand_edge[p * KMAX + j]), float(cand_off[p * KMAX + j])
                ot = 0.0 if off_tol is None else off_tol[q * KMAX + i] + off_tol[p * KMAX + j]
                s = step(G, Utab, ei, oi, ej, oj)
                tr.steps[i][j] = s
                if s.kind is None:
                    continue
                if ei == ej and oi > 0 and oj > 0 and abs(oj - oi) <= ot and ot > 0:
                    tr.amb[i, j] = True                    # forward or stay: decided by rounding
                n = len(s.path)
                tr.tol[i, j] = tol_trans(n, B, s.r, P["beta"], ot + gt)
                if s.kind == "route" and abs(s.cost - B * 64.0) <= 64.0 * Bt:
                    tr.amb[i, j] = True                    # integer cost on the bound floor(B * 64)
                if abs(s.r - B) <= tol_route(n, B, s.r, ot) + Bt:
                    tr.amb[i, j] = True                    # r on the route bound
                if (s.kind != "route" or s.cost <= cmax) and s.r <= B:
                    tr.T[i, j] = (s.units / 64.0 + abs(s.r - tr.gc)) / P["beta"]
        out[p] = tr
    return out


# ------------------------------------------------------------------ rule 5
class Chain(object):
    """One Viterbi chain: cols (its columns), state (the optimum, lowest index
    on ties), cost, margin (per column: by how much the best complete path
    through the winning state beats the best through any other state; inf
    with one state), m (per column: best complete path cost through each
    state)."""


def viterbi(batch, is_col, ncand, emis, cprev, trans):
    """emis: flat per slot; trans: {p: matrix Kq x Kp}.  -> list of Chain per
    trace (list of lists).  A column with candidates but no reachable state,
    or without a link to the column before, starts a new chain."""
    off = np.asarray(batch["trace_off"])
    res = []
    for t in range(len(off) - 1):
        chains, cur = [], None
        for p in range(int(off[t]), int(off[t + 1])):
            if not is_col[p]:
                continue
            K = int(ncand[p])
            if K == 0:
                cur = None
                continue
            em = np.asarray(emis[p * KMAX:p * KMAX + K], np.float64)
            if cur is not None and cprev[p] == cur["cols"][-1]:
                T = np.asarray(trans[p], np.float64)
                v = cur["alpha"][-1][:, None] + T               # Kq x Kp
                best = v.min(axis=0)
                if np.isfinite(best).any():
                    cur["alpha"].append(best + em)
                    cur["bp"].append(v.argmin(axis=0))          # the first minimum: lowest index
                    cur["cols"].append(p)
                    cur["T"].append(T)
                    cur["em"].append(em)
                    continue
            cur = dict(cols=[p], alpha=[em.copy()], bp=[None], T=[None], em=[em])
            chains.append(cur)
        out = []
        for c in chains:
            n = len(c["cols"])
            beta = [None] * n
            beta[n - 1] = np.zeros(len(c["alpha"][-1]))
            for k in range(n - 2, -1, -1):
                beta[k] = (c["T"][k + 1] + (c["em"][k + 1] + beta[k + 1])[None, :]).min(axis=1)
            ch = Chain()
            ch.cols = c["cols"]
            ch.cost = float(c["alpha"][-1].min())
            ch.m = [c["alpha"][k] + beta[k] for k in range(n)]
            st = [0] * n
            st[n - 1] = int(c["alpha"][-1].argmin())
            for k in range(n - 1, 0, -1):
                st[k - 1] = int(c["bp"][k][st[k]])
            ch.state = st
            ch.margin = []
            for k in range(n):
                others = np.delete(ch.m[k], st[k])
                ch.margin.append(float(others.min() - ch.m[k][st[k]]) if len(others) else INF)
            ch.T, ch.em = c["T"], c["em"]
            out.append(ch)
        res.append(out)
    return res


def path_cost(chain, states):
    """The cost of a given state sequence over a chain's columns."""
    c = chain.em[0][states[0]]
    for k in range(1, len(states)):
        c = c + chain.T[k][states[k - 1], states[k]] + chain.em[k][states[k]]
    return float(c)


# ------------------------------------------------------------------ rule 7: interpolated points
class Foot(object):
    """The closest foot of a point on an edge's polyline (brute force over its
    shape segments, equirectangular at the point's latitude, ties to the lowest
    shape segment): sqd, off, D (for the tolerances), tol (the offset's bound:
    tol_offset of the winning segment, plus the spread of the offsets of the
    segments as close within tol_sqdist when they agree -- a foot on a shared
    vertex -- and 0 for an exact foot), amb (two segments as close within
    tol_sqdist whose offsets differ by more than their bounds), exact0 (the
    foot is the edge's first shape point by the clamp t = 0, decided by more
    than the bound: its offset is 0 in any precision)."""
    __slots__ = ("sqd", "off", "D", "tol", "amb", "exact0")


def foot_on_edge(G, e, lat, lon):
    s0 = int(G.eshape[e])
    n = int(G.eshape[e + 1]) - s0 - 1
    ls = MPD * math.cos(math.radians(lat))
    rows = []
    for s in range(n):
        a, b = s0 + s, s0 + s + 1
        ax, ay = (G.slon[a] - lon) * ls, (G.slat[a] - lat) * MPD
        bx, by = (G.slon[b] - lon) * ls, (G.slat[b] - lat) * MPD
        vx, vy = bx - ax, by - ay
        l2 = vx * vx + vy * vy
        traw = -(ax * vx + ay * vy) / l2 if l2 > 0 else 0.0
        t = min(max(traw, 0.0), 1.0)
        px, py = ax + t * vx, ay + t * vy
        D = max(abs(ax), abs(ay), abs(bx), abs(by))
        vlen = math.sqrt(l2)
        off = min(G.scum[a] + t * (G.scum[b] - G.scum[a]), G.elen[e])
        rows.append((px * px + py * py, s, off, D, vlen, traw))
    sqd, s, off, D, vlen, traw = min(rows)                       # (sqd, segment): ties to the lowest segment
    f = Foot()
    f.sqd, f.off, f.D = sqd, off, D
    f.tol = tol_offset(G.elen[e], D, vlen)
    f.amb = False
    for r in rows:
        if r[1] != s and r[0] - sqd <= tol_sqdist(r[3]) + tol_sqdist(D):
            if abs(r[2] - off) > tol_offset(G.elen[e], r[3], r[4]) + tol_offset(G.elen[e], D, vlen):
                f.amb = True
            else:
                f.tol = max(f.tol, tol_offset(G.elen[e], r[3], r[4])) + abs(r[2] - off)
    # t = 0 on the first shape segment by the clamp, the unclamped foot further
    # out than the bound: offset scum[first] + 0 * (...) = 0 whatever the precision
    f.exact0 = (not f.amb) and s == 0 and vlen > 0 and traw < 0 and -traw * vlen > f.tol and f.tol == \
        tol_offset(G.elen[e], D, vlen)
    if f.exact0:
        f.tol = 0.0
    return f


class Piece(object):
    """One piece of a step's route: edge, [o0, o1] on it, xs (the route
    position of o0), nsum (path lengths summed into xs), kind ("first": the
    rest of q's edge, "path", "last": p's edge up to its offset), cut (the index
    of the step's cut -- the route position start + the first `cut` path
    lengths -- where the piece begins; the first piece begins at q, cut -1)."""
    __slots__ = ("edge", "o0", "o1", "xs", "nsum", "kind", "cut")

    def __init__(self, edge, o0, o1, xs, nsum, kind, cut):
        self.edge, self.o0, self.o1, self.xs, self.nsum, self.kind, self.cut = edge, o0, o1, xs, nsum, kind, cut


def step_pieces(G, s, ei, oi, ej, oj):
    """The pieces of a "route" step (rule 7): the rest of q's edge unless q is
    a node candidate, each path edge whole, p's edge up to its offset unless p
    is a node candidate."""
    out = []
    start = 0.0 if oi == 0 else G.elen[ei] - oi
    if oi != 0:
        out.append(Piece(ei, oi, G.elen[ei], 0.0, 0, "first", -1))
    d = 0.0
    for n, g in enumerate(s.path):
        out.append(Piece(g, 0.0, G.elen[g], start + d, n, "path", n))
        d += G.elen[g]
    if oj != 0:
        out.append(Piece(ej, 0.0, oj, start + d, len(s.path), "last", len(s.path)))
    return out


class Placed(object):
    """An interpolated point on its step's route: pos (None: unplaced), tol
    (tol_ipos), amb (decided by less than the bounds, see place_point), piece,
    cut (>= 0: the position *is* that cut of the step in any precision -- the
    foot is the first shape point of a piece that starts there, so pos = xs +
    (0 - 0))."""
    __slots__ = ("pos", "tol", "amb", "piece", "cut")


def place_point(G, P, lat, lon, q, k, pieces, oi_tol=0.0, oj_tol=0.0):
    """Rule 7's placement of point k of step q -> p on the step's pieces: per
    piece the closest foot on the piece's edge, admissible iff its offset lies
    inside the piece (ends included), cost sqdist / (2 sigma_z^2) + |pos -
    gc(q, k)| / beta, the lowest cost wins, ties to the earliest piece.
    oi_tol / oj_tol: the tolerances of q's and p's offsets when they are the
    reference's own.

    One identity: a point whose f32 (lat, lon) equal q's projects onto q's edge
    at q's own offset (the same input through the same projection), so on the
    first piece its foot is o0 and its position exactly 0.  (The same would
    hold for a copy of p on p's edge, but a point between q and p lies within
    interpolation_distance of q and p does not: there is none.)

    Ambiguous, from the reference's values alone: a piece is *shaky* when its
    foot is (Foot.amb) or when the foot's offset is within its bound of the
    piece's o0 = off_q or o1 = off_p (an edge's own ends are no test: the
    projection is clamped into [0, len] in any precision); the point is
    ambiguous when a shaky piece is the winner, or could beat it within the
    cost bounds (tol_icost), or no other piece is admissible; and when two
    admissible pieces' costs are closer than the sum of their bounds -- unless
    their positions agree within their bounds (the vertex two consecutive
    pieces share: the same place either way)."""
    la, lo = float(lat[k]), float(lon[k])
    gcd = _gc(float(lat[q]), float(lon[q]), la, lo)
    same_q = lat[k] == lat[q] and lon[k] == lon[q]
    ds = 2.0 * P["sigma_z"] * P["sigma_z"]
    rows = []                                                   # (cost, m, pos, ptol, ctol, cut, adm, shaky)
    for m, pc in enumerate(pieces):
        f = foot_on_edge(G, pc.edge, la, lo)
        off, ftol, shaky = f.off, f.tol, f.amb
        ident = same_q and pc.kind == "first"
        if ident:
            off, ftol, shaky = pc.o0, 0.0, False
        else:
            if pc.kind == "first" and abs(off - pc.o0) <= ftol + oi_tol:
                shaky = True
            if pc.kind == "last" and abs(off - pc.o1) <= ftol + oj_tol:
                shaky = True
        adm = pc.o0 <= off <= pc.o1
        pos = pc.xs + (off - pc.o0)
        ptol = 0.0 if ident else tol_ipos(ftol, pc.nsum, abs(pos), oi_tol)
        emis = f.sqd / ds
        cost = emis + abs(pos - gcd) / P["beta"]
        ctol = tol_icost(f.D, emis, P["sigma_z"], ptol, pos, gcd, P["beta"])
        cut = pc.cut if (f.exact0 and pc.kind != "first" and pc.o0 == 0.0 and not ident) else -1
        rows.append((cost, m, pos, ptol, ctol, cut, adm, shaky))
    out = Placed()
    out.pos, out.tol, out.amb, out.piece, out.cut = None, 0.0, False, -1, -1
    firm = [r for r in rows if r[6]]
    best = min(firm) if firm else None                          # (cost, piece): ties to the earliest piece
    for r in rows:
        if r[7] and (best is None or r is best or r[0] - r[4] <= best[0] + best[4]):
            out.amb = True
    if best is None:
        return out
    out.pos, out.tol, out.piece, out.cut = best[2], best[3], best[1], best[5]
    for r in firm:
        if r is not best and r[0] - best[0] <= r[4] + best[4]:
            if abs(r[2] - best[2]) <= r[3] + best[3]:
                out.tol = max(out.tol, r[3]) + abs(r[2] - best[2])
                if r[5] != best[5]:
                    out.cut = -1
            else:
                out.amb = True
    return out


class Placements(object):
    """Rule 7's placement over a batch: pos (float64[P], -1 unplaced), tol,
    amb, cut (int, -1 none), piece (-1 none), in_step (bool: an interpolated
    point strictly inside a "route" step of a chain)."""

    def __init__(self, n):
        self.pos, self.tol = np.full(n, -1.0), np.zeros(n)
        self.amb, self.in_step = np.zeros(n, bool), np.zeros(n, bool)
        self.cut, self.piece = np.full(n, -1, np.int64), np.full(n, -1, np.int64)


def placements(G, P, batch, chains, cand_edge, cand_off, off_tol=None):
    """chains: per trace a list of (cols, states).  off_tol: per slot (flat)
    when the offsets are the reference's own, None when the implementation's.
    A same-edge step (forward or a stay) places nothing; a step into a chain
    start does not exist (chains are given apart); points after a chain's last
    state, before its first, or in a trace without a chain stay unplaced."""
    lat = np.asarray(batch["lat"], np.float32).astype(np.float64)
    lon = np.asarray(batch["lon"], np.float32).astype(np.float64)
    Utab = _utab(G, P)
    pl = Placements(len(lat))
    for chs in chains:
        for cols, states in chs:
            for c in range(1, len(cols)):
                q, p = int(cols[c - 1]), int(cols[c])
                if p - q < 2:
                    continue
                a, b = q * KMAX + states[c - 1], p * KMAX + states[c]
                ei, oi, ej, oj = int(cand_edge[a]), float(cand_off[a]), int(cand_edge[b]), float(cand_off[b])
                s = step(G, Utab, ei, oi, ej, oj)
                assert s.kind is not None, "chosen states without a route"
                if s.kind != "route":
                    continue
                pcs = step_pieces(G, s, ei, oi, ej, oj)
                ti = 0.0 if off_tol is None or oi == 0 else float(off_tol[a])
                tj = 0.0 if off_tol is None or oj == 0 else float(off_tol[b])
                for k in range(q + 1, p):
                    r = place_point(G, P, lat, lon, q, k, pcs, ti, tj)
                    pl.in_step[k], pl.amb[k], pl.tol[k], pl.cut[k], pl.piece[k] = True, r.amb, r.tol, r.cut, r.piece
                    if r.pos is not None:
                        pl.pos[k] = r.pos
    return pl


class Anchors(object):
    """A step's anchors (rule 7): q at 0, the placed points not behind an
    earlier anchor (position >= the running maximum, in trace order), p at R.
    pts: [(point, position, tolerance, cut)] from q on, p not included; amb:
    a point of the step is ambiguous in its placement, or its position is
    within the bounds of the running maximum (the filter is undecided), and
    then every boundary of the step is; dropped: placed points the filter
    removed.  Two points with bit-equal f32 (lat, lon) have the same position
    in any precision (the same input through the same projection), so a copy
    of the anchor that set the maximum is an anchor and not ambiguous."""

    def __init__(self, q, p, pos, tol, amb, cut, lat, lon):
        self.pts, self.amb, self.dropped = [(q, 0.0, 0.0, -1)], False, 0
        run, rtol, rk = 0.0, 0.0, q
        for k in range(q + 1, p):
            if amb is not None and amb[k]:
                self.amb = True
            v = float(pos[k])
            if not v >= 0.0:
                continue
            tv = 0.0 if tol is None else float(tol[k])
            copy = rk != q and lat[k] == lat[rk] and lon[k] == lon[rk]
            if copy:
                v = run
            elif tv + rtol > 0 and abs(v - run) <= tv + rtol:
                self.amb = True
            if v >= run:
                self.pts.append((k, v, tv, -1 if cut is None else int(cut[k])))
                run, rtol, rk = v, tv, k
            else:
                self.dropped += 1


def step_boundary(times, an, q, p, R, R_tol, x, x_tol, cut, at_end):
    """The boundary at route position x (the step's cut number `cut`) of step
    q -> p with anchors `an`: -> (time, shape point, not ambiguous, time bound).
    Shape index: the last anchor at or before x, p itself when x >= R (at_end:
    x is R by construction -- p a node candidate and x the end of the last path
    edge, the same f32 sum).  Time: linear between that anchor and the next
    (tol_time_anchored), the anchor's own time when the two coincide.
    Ambiguous: the step is (Anchors.amb); an anchor's position is within the
    bounds of x -- unless it is x by construction (Placed.cut); R within the
    bounds of x when not at_end."""
    amb = an.amb
    L = 0
    for i, (k, v, tv, c) in enumerate(an.pts):
        if i == 0:
            continue
        if c == cut and c >= 0:
            L = i                                               # at x in any precision: at or before it
            continue
        if abs(v - x) <= tv + x_tol:
            amb = True
        if v <= x:
            L = i
    kL, xL, eL, _ = an.pts[L]                                   # positions are nondecreasing: a prefix
    if L + 1 < len(an.pts):
        kN, xN, eN, _ = an.pts[L + 1]
    else:
        kN, xN, eN = p, R, R_tol
    if not at_end and abs(R - x) <= R_tol + x_tol:
        amb = True
    sh = p if (at_end or R <= x) else kL
    dt = times[kN] - times[kL]
    den = xN - xL
    tm = times[kL] + dt * ((x - xL) / den) if den > 0 else times[kL]
    return tm, sh, not amb, tol_time_anchored(dt, den, x_tol, eL, eN, tm)


# ------------------------------------------------------------------ rules 6 and 7
class Seg(object):
    """One matched segment.  segment_id None without association; start_time /
    end_time None when not valid; the *_known flags are False where the
    boundary is ambiguous (step_boundary); begin_tol / end_tol: the time
    bounds; begin_in / end_in: 0, or the boundary lies inside a step with
    interpolated points: 1 none of them an anchor (the two-state rule), 2 the
    step has anchors (tol_time_anchored)."""
    __slots__ = ("segment_id", "internal", "length", "way_ids", "start_valid", "end_valid", "start_time",
                 "end_time", "begin_shape_index", "end_shape_index", "begin_known", "end_known", "begin_tol",
                 "end_tol", "begin_in", "end_in")


def segments_of_chain(G, P, t0, times, cols, states, cand_edge, cand_off, gc, off_tol=None, ipos=None, place=None,
                      latlon=None):
    """cols: the chain's columns (point indices), states: their chosen slots,
    t0: the trace's first point; off_tol: per slot (flat) offset tolerances
    when the offsets are not the implementation's, else None.  ipos: the
    positions of the interpolated points (-1 unplaced) the boundaries are made
    from -- the implementation's own (stage-isolated: exact inputs) or, when
    None, the reference's own `place.pos` with `place.tol`; place: the
    reference's Placements on the same states (its amb and cut flags count
    either way); latlon: the batch's f32 (lat, lon) as float64 arrays.  ->
    (segments, route_dist per column (0 for the first), steps, {dropped: placed
    points the monotone filter removed, trav: traversals})."""
    Utab = _utab(G, P)
    # a traversal: [edge, off0, off1, begin, end], a boundary (t, sh, known, tol, inside: 0 no, 1 two-state, 2 anchored)
    trav = []
    rdist, steps = [0.0], []
    stats = dict(dropped=0)
    p = cols[0]
    e = int(cand_edge[p * KMAX + states[0]])
    o = float(cand_off[p * KMAX + states[0]])
    cur = [e, o, None, (times[p], p - t0, True, 0.0, False), None]
    curmax = o
    for k in range(1, len(cols)):
        q, p = cols[k - 1], cols[k]
        a, b = q * KMAX + states[k - 1], p * KMAX + states[k]
        ei, oi = int(cand_edge[a]), float(cand_off[a])
        ej, oj = int(cand_edge[b]), float(cand_off[b])
        s = step(G, Utab, ei, oi, ej, oj)
        assert s.kind is not None, "chosen states without a route"
        steps.append(s)
        rdist.append(s.r)
        if s.kind != "route":
            curmax = max(curmax, oj)
            continue
        R, n = s.r, len(s.path)
        ti = 0.0 if off_tol is None or oi == 0 else float(off_tol[a])
        tj = 0.0 if off_tol is None or oj == 0 else float(off_tol[b])
        an = None
        if p - q >= 2:                                          # interpolated points inside: the anchors decide
            if ipos is None:
                an = Anchors(q, p, place.pos, place.tol, place.amb, place.cut, latlon[0], latlon[1])
            else:
                an = Anchors(q, p, ipos, None, place.amb, place.cut, latlon[0], latlon[1])
            stats["dropped"] += an.dropped

        def bound(x, j, at_end=False):
            if an is None or len(an.pts) == 1 and not an.amb:   # the two-state rule
                tm = times[q] + (times[p] - times[q]) * (x / R) if R > 0 else times[q]
                tt = tol_time(n, times[p] - times[q]) + (abs(times[p] - times[q]) * 2 * max(ti, tj) / R if R > 0
                                                           else 0.0)
                return (tm, (p if (at_end or R <= x) else q) - t0, True, tt, 0 if an is None else 1)
            tm, sh, ok, tt = step_boundary(times, an, q, p, R, tol_route(n, 0.0, R, ti + tj), x,
                                           tol_cut(j, x, ti), j, at_end)
            return (tm, sh - t0, ok, tt, 2 if len(an.pts) > 1 else 1)
        start = 0.0 if oi == 0 else G.elen[ei] - oi
        if oi != 0:                                             # a route from a node candidate starts at its node
            cur[2], cur[4] = G.elen[ei], bound(start, 0, oj == 0 and n == 0)
            trav.append(cur)
        d = 0.0
        for j, g in enumerate(s.path):
            xb = start + d
            d += G.elen[g]
            trav.append([g, 0.0, G.elen[g], bound(xb, j), bound(start + d, j + 1, oj == 0 and j == n - 1)])
        cur = [ej, 0.0, None, bound(start + d, n, oj == 0), None]
        curmax = oj
    last = cols[-1]
    if curmax != 0.0:                                           # a chain ending on a node candidate ends at the node
        cur[2], cur[4] = curmax, (times[last], last - t0, True, 0.0, False)
        trav.append(cur)
    segs = []
    stats["trav"] = len(trav)
    if len(cols) < 2:
        return segs, rdist, steps, stats
    groups = []
    for k, tv in enumerate(trav):
        join = False
        if groups:
            pe, e = trav[k - 1][0], tv[0]
            if G.eseg[e] >= 0:
                join = G.eseg[pe] == G.eseg[e] and G.eseg_pos[e] == G.eseg_pos[pe] + 1
            else:
                join = G.eseg[pe] < 0 and ((G.eflags[e] ^ G.eflags[pe]) & INTERNAL) == 0
        if join:
            groups[-1].append(tv)
        else:
            groups.append([tv])
    for gr in groups:
        f, l = gr[0], gr[-1]
        sg = int(G.eseg[f[0]])
        s = Seg()
        if sg >= 0:
            s.start_valid = f[1] == 0.0 and G.eseg_pos[f[0]] == 0
            s.end_valid = l[2] == G.elen[l[0]] and G.eseg_pos[l[0]] == G.gn[sg] - 1
            s.segment_id = int(G.gid[sg])
            s.internal = False
            s.length = int(math.floor(G.glen[sg] + 0.5)) if s.start_valid and s.end_valid else -1
        else:
            s.start_valid, s.end_valid = f[1] == 0.0, l[2] == G.elen[l[0]]
            s.segment_id, s.length = None, -1
            s.internal = bool(G.eflags[f[0]] & INTERNAL)
        s.start_time = f[3][0] if s.start_valid else None
        s.end_time = l[4][0] if s.end_valid else None
        s.begin_shape_index, s.begin_known, s.begin_tol, s.begin_in = f[3][1], f[3][2], f[3][3], f[3][4]
        s.end_shape_index, s.end_known, s.end_tol, s.end_in = l[4][1], l[4][2], l[4][3], l[4][4]
        s.way_ids = []
        for tv in gr:
            w = int(G.eway[tv[0]])
            if not s.way_ids or s.way_ids[-1] != w:
                s.way_ids.append(w)
        segs.append(s)
    return segs, rdist, steps, stats
