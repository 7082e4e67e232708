"""Comparisons of an implementation of `Match` (the CPU oracle's stage arrays,
or the GPU engine's) with the float64 reference of the written spec
(tests/specref.py).  Shared by tests/test_specref.py (oracle, CPU) and
tests/test_gpu_specref.py (kernels).

Two ways, both through the same functions:
  stage-isolated  each reference stage is fed with the implementation's own
                  upstream arrays and compared with the implementation's
                  output of that stage;
  end to end      the reference runs all the way on its own arrays and its
                  segments are compared with the implementation's final
                  records, on the traces without an ambiguous decision.

Every check asserts its exclusion caps (at most 5 % of traces, 1 % of
transition entries, 5 % of a case's interpolated points and 5 % of its
boundaries inside steps with interpolated points; `max_excl=0` for hand
graphs) before it compares.  An ambiguous interpolated point or boundary
excludes itself only, never the rest of its trace.
RATIOS collects the largest observed error / bound per quantity, SHARES the
excluded shares of rule 7 per (check, case).
"""
import numpy as np

import specref as sr

KMAX = sr.KMAX
TRACE_CAP, ENTRY_CAP = 0.05, 0.01
RATIOS = {}
SHARES = {}


def _ratio(name, err, bound):
    r = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    if r > RATIOS.get(name, 0.0):
        RATIOS[name] = r
    return r


class Impl(object):
    """An implementation's stage arrays and final records under one face."""

    def __init__(self, stages, traces, segments, way_ids, npts):
        for k in ("ncand", "cand_edge", "cand_off", "cand_emis", "gc", "col_prev", "trans_off", "trans", "state",
                  "route_dist", "ipos"):
            n = {"trans_off": npts + 1, "trans": None, "cand_edge": npts * KMAX, "cand_off": npts * KMAX,
                 "cand_emis": npts * KMAX}.get(k, npts)
            setattr(self, k, np.asarray(stages[k])[:n])
        # slots past ncand hold whatever the buffers held: clear them
        live = (np.arange(KMAX)[None, :] < np.asarray(self.ncand)[:, None]).ravel()
        for k in ("cand_edge", "cand_off", "cand_emis"):
            setattr(self, k, np.where(live, getattr(self, k), 0))
        self.traces, self.segments, self.way_ids = traces, segments, way_ids

    @classmethod
    def from_oracle(cls, orc, npts):
        return cls(orc, orc["traces"], orc["segments"], orc["way_ids"], npts)

    @classmethod
    def from_engine(cls, eng, res, npts):
        names = ("ncand", "cand_edge", "cand_off", "cand_emis", "gc", "col_prev", "trans_off", "trans", "state",
                 "route_dist", "ipos")
        return cls({k: eng.debug(k) for k in names}, res.traces, res.segments, res.way_ids, npts)

    def is_col(self, batch):
        """Rule 1 as the arrays show it: a trace's first point, or gc > 0."""
        c = np.asarray(self.gc) > 0
        off = np.asarray(batch["trace_off"])
        c[off[:-1][np.diff(off) > 0]] = True
        return c

    def T(self, p, Kq, Kp):
        a = int(self.trans_off[p])
        return np.asarray(self.trans[a:a + Kq * Kp], np.float64).reshape(Kq, Kp)


def _trace_of(batch):
    off = np.asarray(batch["trace_off"])
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def _cap(what, dropped, total, cap, max_excl, why=None):
    assert len(dropped) <= (cap * total if max_excl is None else max_excl), \
        "%s: %d of %d excluded as ambiguous %s" % (what, len(dropped), total, why or "")


class Reference(object):
    """The reference all the way on its own arrays (end to end), with the
    traces it excludes: computed once per (graph, batch, params)."""

    def __init__(self, G, batch, P):
        self.G, self.batch, self.P = G, batch, P
        npts = len(batch["lat"])
        tr = _trace_of(batch)
        self.is_col, self.gc, amb = sr.columns(batch, P)
        drop = set(tr[amb])
        self.why = {int(t): 'columns' for t in drop}
        self.cands = sr.candidates(G, batch, P, self.is_col)
        drop |= set(tr[p] for p, c in self.cands.items() if c.amb)
        for t in drop:
            self.why.setdefault(int(t), 'candidates')
        self.ncand, self.ce, self.co, self.em = sr.cand_arrays(self.cands, npts)
        self.cprev, amb = sr.col_prev(batch, P, self.is_col, self.gc, self.ncand)
        drop |= set(tr[amb])
        otol, etol = np.zeros(npts * KMAX), np.zeros(npts * KMAX)
        for p, c in self.cands.items():
            for k in range(len(c)):
                otol[p * KMAX + k] = c.otol[k]
                etol[p * KMAX + k] = sr.tol_emission(c.D[k], c.emis[k], P["sigma_z"])
        self.trans = sr.transitions(G, P, self.ncand, self.ce, self.co, self.gc, self.cprev, off_tol=otol, gc_own=True)
        self.n_entries = sum(t.T.size for t in self.trans.values())
        self.amb_entries = sum(int(t.amb.sum()) for t in self.trans.values())
        drop |= set(tr[p] for p, t in self.trans.items() if t.amb.any())
        for t in drop:
            self.why.setdefault(int(t), 'col_prev or transitions')
        self.chains = sr.viterbi(batch, self.is_col, self.ncand, self.em, self.cprev,
                                 {p: t.T for p, t in self.trans.items()})
        # Viterbi margins against the inputs' tolerances.  Two paths differ by the sum
        # over the entries only one of them uses, so: raise the winner's entries by
        # their tolerances, lower every other entry, and a state whose best path
        # still does not beat the winner's cannot win in the implementation either.
        # Chains of one column yield no segment: their state decides nothing.
        em_mod, T_mod = self.em - etol, {p: t.T - t.tol for p, t in self.trans.items()}
        for chs in self.chains:
            for ch in chs:
                for k, p in enumerate(ch.cols):
                    w = ch.state[k]
                    em_mod[p * KMAX + w] = self.em[p * KMAX + w] + etol[p * KMAX + w]
                    if k:
                        T_mod[p][ch.state[k - 1], w] = self.trans[p].T[ch.state[k - 1], w] + \
                            self.trans[p].tol[ch.state[k - 1], w]
        mod = sr.viterbi(batch, self.is_col, self.ncand, em_mod, self.cprev, T_mod)
        for t, chs in enumerate(self.chains):
            assert [c.cols for c in chs] == [c.cols for c in mod[t]]
            for ch, cm in zip(chs, mod[t]):
                if len(ch.cols) < 2:
                    continue
                win = sr.path_cost(cm, ch.state)
                tol = sr.tol_viterbi(len(ch.cols), win)
                for k in range(len(ch.cols)):
                    others = np.delete(cm.m[k], ch.state[k])
                    if len(others) and others.min() - win <= tol and not _twin_tie(ch, k):
                        drop.add(t)
                        self.why.setdefault(int(t), 'viterbi')
        self.dropped = drop
        self.otol = otol
        # rule 7's placement on the reference's own states and offsets
        self.place = sr.placements(G, P, batch, [[(c.cols, c.state) for c in chs] for chs in self.chains], self.ce,
                                   self.co, off_tol=otol)
        self.fired = set()
        for c in self.cands.values():
            self.fired |= c.fired
        for t in self.trans.values():
            for row in t.steps:
                for s in row:
                    if s.kind == "stay":
                        self.fired.add("stay")
                    if s.kind == "route" and len(s.path) >= 3:
                        self.fired.add("multi_edge_route")


def _twins(ch, k, a, b):
    """States a and b of column k are exact twins: bitwise equal emission,
    incoming and outgoing transitions, so every precision ties them."""
    if ch.em[k][a] != ch.em[k][b]:
        return False
    if k > 0 and not np.array_equal(ch.T[k][:, a], ch.T[k][:, b]):
        return False
    if k + 1 < len(ch.cols) and not np.array_equal(ch.T[k + 1][a, :], ch.T[k + 1][b, :]):
        return False
    return True


def _twin_tie(ch, k):
    """The column's zero margin comes from exact twins of the winner only (rule
    5's tie rule decides, in any precision)."""
    w = ch.state[k]
    best = ch.m[k][w]
    tied = [s for s in range(len(ch.m[k])) if s != w and ch.m[k][s] == best]
    rest = [ch.m[k][s] for s in range(len(ch.m[k])) if s != w and s not in tied]
    return bool(tied) and all(_twins(ch, k, w, s) for s in tied) and (not rest or min(rest) > best)


# ---------------------------------------------------------------------- stage-isolated
def check_columns(batch, P, impl, max_excl=None):
    """Rule 1: the column flags and gc (reference from the raw points)."""
    is_col, gc, amb = sr.columns(batch, P)
    tr = _trace_of(batch)
    dropped = set(tr[amb])
    _cap("columns", dropped, len(batch["trace_off"]) - 1, TRACE_CAP, max_excl)
    keep = ~np.isin(tr, list(dropped))
    got = impl.is_col(batch)
    assert np.array_equal(got[keep], is_col[keep]), "column flags"
    for p in np.nonzero(keep & is_col)[0]:
        assert _ratio("gc", abs(float(impl.gc[p]) - gc[p]), sr.tol_gc(gc[p])) <= 1, "gc at point %d" % p


def check_candidates(G, batch, P, impl, max_excl=None):
    """Rules 2 and 3 at the implementation's own columns."""
    is_col = impl.is_col(batch)
    cands = sr.candidates(G, batch, P, is_col)
    tr = _trace_of(batch)
    dropped = set(tr[p] for p, c in cands.items() if c.amb)
    _cap("candidates", dropped, len(batch["trace_off"]) - 1, TRACE_CAP, max_excl)
    assert not np.asarray(impl.ncand)[~is_col].any(), "an interpolated point has candidates"
    for p, c in cands.items():
        if tr[p] in dropped:
            continue
        K = int(impl.ncand[p])
        assert K == len(c), "ncand at point %d: %d, reference %d" % (p, K, len(c))
        e = [int(x) for x in impl.cand_edge[p * KMAX:p * KMAX + K]]
        o = [float(x) for x in impl.cand_off[p * KMAX:p * KMAX + K]]
        em = [float(x) for x in impl.cand_emis[p * KMAX:p * KMAX + K]]
        ref = {(c.edge[k], c.node[k]): k for k in range(K)}
        assert len(ref) == K
        assert set(zip(e, [x == 0.0 for x in o])) == set(ref), "candidate (edge, is-node) set at point %d" % p
        prev = None
        for k in range(K):
            m = ref[(e[k], o[k] == 0.0)]
            if not c.node[m]:
                assert _ratio("offset", abs(o[k] - c.off[m]), c.otol[m]) <= 1, \
                    "offset of candidate %d at point %d" % (k, p)
            assert _ratio("emission", abs(em[k] - c.emis[m]), sr.tol_emission(c.D[m], c.emis[m], P["sigma_z"])) \
                <= 1, "emission of candidate %d at point %d: %r, reference %r" % (k, p, em[k], c.emis[m])
            # rule 2's order: by the reference's sqdist within tolerance
            if prev is not None:
                gap = c.sqd[m] - c.sqd[prev]
                assert gap >= -(sr.tol_sqdist(c.D[m]) + sr.tol_sqdist(c.D[prev])), "candidate order at point %d" % p
                # twin edges (one geometry, one direction: the same sqdist and offset in any
                # precision): rule 2's tie goes to the lower edge
                if gap == 0.0 and c.off[m] == c.off[prev] and not c.node[m] and not c.node[prev]:
                    assert e[k - 1] < e[k], "candidate tie order at point %d" % p
            prev = m
    return cands


def check_col_prev(batch, P, impl, max_excl=None):
    cp, amb = sr.col_prev(batch, P, impl.is_col(batch), np.asarray(impl.gc, np.float64), impl.ncand)
    tr = _trace_of(batch)
    dropped = set(tr[amb])
    _cap("col_prev", dropped, len(batch["trace_off"]) - 1, TRACE_CAP, max_excl)
    keep = ~np.isin(tr, list(dropped))
    assert np.array_equal(np.asarray(impl.col_prev)[keep], cp[keep]), "col_prev"


def check_transitions(G, P, impl, max_excl=None):
    """Rule 4 on the implementation's own candidates, gc and col_prev."""
    trans = sr.transitions(G, P, impl.ncand, impl.cand_edge, np.asarray(impl.cand_off, np.float64),
                           np.asarray(impl.gc, np.float64), impl.col_prev)
    total = sum(t.T.size for t in trans.values())
    namb = sum(int(t.amb.sum()) for t in trans.values())
    assert namb <= (ENTRY_CAP * total if max_excl is None else max_excl), \
        "transitions: %d of %d entries excluded as ambiguous" % (namb, total)
    toff = np.asarray(impl.trans_off)
    for p in range(len(impl.ncand)):
        want = trans[p].T.size if p in trans else 0
        assert toff[p + 1] - toff[p] == want, "transition matrix size at point %d" % p
    for p, t in trans.items():
        got = impl.T(p, *t.T.shape)
        ok = ~t.amb
        assert np.array_equal(np.isfinite(got)[ok], np.isfinite(t.T)[ok]), \
            "finite / no-transition pattern at point %d" % p
        for i, j in zip(*np.nonzero(ok & np.isfinite(t.T))):
            assert _ratio("T", abs(got[i, j] - t.T[i, j]), t.tol[i, j]) <= 1, \
                "T[%d, %d] at point %d: %r, reference %r (%s)" % (i, j, p, got[i, j], t.T[i, j], t.steps[i][j].kind)
    return trans


def check_viterbi(batch, impl, max_excl=None):
    """Rule 5 on the implementation's own emissions and transitions: its path
    costs the optimum within tolerance with the same chains; the states are
    equal where the margin exceeds the tolerance, the lowest index among exact
    twins."""
    is_col = impl.is_col(batch)
    mats = {}
    for p in np.nonzero(np.asarray(impl.col_prev) >= 0)[0]:
        mats[int(p)] = impl.T(p, int(impl.ncand[impl.col_prev[p]]), int(impl.ncand[p]))
    chains = sr.viterbi(batch, is_col, impl.ncand, np.asarray(impl.cand_emis, np.float64), impl.col_prev, mats)
    in_chain = np.zeros(len(is_col), bool)

    def decided(ch, k, tol):
        # the margin exceeds the bound; or exact twins tie (in any precision); or a
        # chain of one column, decided on the emissions as they stand: in each case
        # the state must be the reference's (the lowest index on a tie)
        return ch.margin[k] > tol or _twin_tie(ch, k) or len(ch.cols) == 1
    # nothing is dropped here (the cost check runs on every chain), but the states
    # must be comparable on all but a few columns: the cap first
    total = skipped = 0
    for chs in chains:
        for ch in chs:
            tol = sr.tol_viterbi(len(ch.cols), ch.cost)
            total += len(ch.cols)
            skipped += sum(1 for k in range(len(ch.cols)) if not decided(ch, k, tol))
    assert skipped <= (TRACE_CAP * total if max_excl is None else max_excl), \
        "viterbi: %d of %d columns too close to compare states" % (skipped, total)
    for t, chs in enumerate(chains):
        for ch in chs:
            in_chain[ch.cols] = True
            st = [int(impl.state[p]) for p in ch.cols]
            assert min(st) >= 0, "a chain column without a state (trace %d)" % t
            tol = sr.tol_viterbi(len(ch.cols), ch.cost)
            cost = sr.path_cost(ch, st)
            assert np.isfinite(cost), "the chosen path crosses a missing transition (trace %d)" % t
            assert _ratio("viterbi_cost", cost - ch.cost, max(tol, 1e-300)) <= 1 or cost == ch.cost, \
                "path cost %r, optimum %r (trace %d)" % (cost, ch.cost, t)
            for k, p in enumerate(ch.cols):
                if decided(ch, k, tol):
                    assert st[k] == ch.state[k], "state at point %d%s" % (
                        p, "" if ch.margin[k] > tol else ": tie not to the lowest index")
    assert (np.asarray(impl.state)[~in_chain] == -1).all(), "a state outside every chain"
    return chains


def _latlon(batch):
    return (np.asarray(batch["lat"], np.float32).astype(np.float64),
            np.asarray(batch["lon"], np.float32).astype(np.float64))


def _new_stats():
    return dict(pts=0, pts_amb=0, placed=0, unplaced=0, dropped=0, bounds_in=0, bounds_amb=0, sh_interp=0,
                t_anchored=0, bounds_by_trace={}, trav_by_trace={})


def _rule7_caps(what, st, max_excl, name=None):
    """The caps of rule 7, asserted before anything is compared."""
    assert st["pts_amb"] <= (TRACE_CAP * st["pts"] if max_excl is None else max_excl), \
        "%s: %d of %d interpolated points excluded as ambiguous" % (what, st["pts_amb"], st["pts"])
    assert st["bounds_amb"] <= (TRACE_CAP * st["bounds_in"] if max_excl is None else max_excl), \
        "%s: %d of %d boundaries inside steps with interpolated points excluded as ambiguous" % (
            what, st["bounds_amb"], st["bounds_in"])
    if name is not None:
        SHARES[(what, name)] = (st["pts_amb"], st["pts"], st["bounds_amb"], st["bounds_in"])


def _count_bounds(want, place, t, t_first, st):
    """Counts the boundaries that are compared; per trace those inside steps
    with interpolated points that are not ambiguous."""
    before = st["bounds_in"] - st["bounds_amb"]
    for w in want:
        for inside, known, sh in ((w.begin_in, w.begin_known, w.begin_shape_index),
                                  (w.end_in, w.end_known, w.end_shape_index)):
            if inside:
                st["bounds_in"] += 1
                st["bounds_amb"] += 0 if known else 1
                st["sh_interp"] += 1 if known and place.in_step[t_first + sh] else 0
                st["t_anchored"] += 1 if known and inside == 2 else 0
    st["bounds_by_trace"][t] = st["bounds_in"] - st["bounds_amb"] - before


def _compare_segments(G, impl, t, t_first, want, what):
    tr = impl.traces[t]
    assert tr["code"] == 200, "%s: trace %d answered %d" % (what, t, tr["code"])
    got = impl.segments[tr["seg_off"]:tr["seg_off"] + tr["seg_cnt"]]
    assert len(got) == len(want), "%s: trace %d has %d segments, reference %d" % (what, t, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        at = "%s: trace %d segment %d" % (what, t, k)
        assert int(g["segment_id"]) == (-1 if w.segment_id is None else w.segment_id), at + " id"
        assert bool(g["flags"] & 4) == w.internal, at + " internal"
        assert int(g["length"]) == w.length, at + " length"
        ways = [int(x) for x in impl.way_ids[g["way_off"]:g["way_off"] + g["way_cnt"]]]
        assert ways == w.way_ids, at + " way_ids"
        assert bool(g["flags"] & 1) == w.start_valid and bool(g["flags"] & 2) == w.end_valid, at + " validity"
        if w.begin_known:
            assert int(g["begin_shape_index"]) == w.begin_shape_index, at + " begin_shape_index: %d, reference %d" % (
                g["begin_shape_index"], w.begin_shape_index)
            if w.start_valid:
                nm = "time_anchored" if w.begin_in == 2 else "time"
                assert _ratio(nm, abs(float(g["start_time"]) - w.start_time), w.begin_tol) <= 1, \
                    at + " start_time %r, reference %r (bound %g)" % (float(g["start_time"]), w.start_time, w.begin_tol)
        if w.end_known:
            assert int(g["end_shape_index"]) == w.end_shape_index, at + " end_shape_index: %d, reference %d" % (
                g["end_shape_index"], w.end_shape_index)
            if w.end_valid:
                nm = "time_anchored" if w.end_in == 2 else "time"
                assert _ratio(nm, abs(float(g["end_time"]) - w.end_time), w.end_tol) <= 1, \
                    at + " end_time %r, reference %r (bound %g)" % (float(g["end_time"]), w.end_time, w.end_tol)


def check_placement(G, batch, P, impl, chains, max_excl=None, name=None):
    """Rule 7's placement (stage-isolated A) on the implementation's own states
    and offsets: the placed / unplaced pattern exactly and `ipos` within
    tol_ipos for every unambiguous point; columns and points outside every
    step are -1.  -> (the reference's Placements, statistics)."""
    place = sr.placements(G, P, batch, [[(ch.cols, [int(impl.state[p]) for p in ch.cols]) for ch in chs]
                                        for chs in chains], impl.cand_edge, np.asarray(impl.cand_off, np.float64))
    st = _new_stats()
    st["pts"], st["pts_amb"] = int(place.in_step.sum()), int((place.in_step & place.amb).sum())
    _rule7_caps("placement", st, max_excl)
    got = np.asarray(impl.ipos, np.float64)
    assert (got[~place.in_step] == -1.0).all(), "a column or a point outside every step has a position"
    for k in np.nonzero(place.in_step & ~place.amb)[0]:
        if place.pos[k] < 0:
            assert got[k] == -1.0, "point %d is placed at %r, the reference leaves it unplaced" % (k, got[k])
            st["unplaced"] += 1
        else:
            assert got[k] >= 0.0, "point %d is unplaced, the reference places it at %r" % (k, place.pos[k])
            assert _ratio("ipos", abs(got[k] - place.pos[k]), place.tol[k]) <= 1 or got[k] == place.pos[k], \
                "ipos of point %d: %r, reference %r (bound %g)" % (k, got[k], place.pos[k], place.tol[k])
            st["placed"] += 1
    return place, st


def check_segments(G, batch, P, impl, chains, max_excl=None, name=None):
    """Rules 6 and 7 on the implementation's own states (chains: the chain
    structure check_viterbi returned): route distances, rule 7's placement
    (check_placement), then the final segment records with the boundaries
    made from the implementation's own `ipos` (stage-isolated B)."""
    off = np.asarray(batch["trace_off"])
    times = np.asarray(batch["time"], np.float64)
    co = np.asarray(impl.cand_off, np.float64)
    place, st = check_placement(G, batch, P, impl, chains, max_excl, name)
    ipos, ll = np.asarray(impl.ipos, np.float64), _latlon(batch)
    wants = []
    for t, chs in enumerate(chains):
        want = []
        for ch in chs:
            sts = [int(impl.state[p]) for p in ch.cols]
            segs, rd, steps, s7 = sr.segments_of_chain(G, P, int(off[t]), times, ch.cols, sts, impl.cand_edge, co,
                                                      impl.gc, ipos=ipos, place=place, latlon=ll)
            st["dropped"] += s7["dropped"]
            st["trav_by_trace"][t] = st["trav_by_trace"].get(t, 0) + s7["trav"]
            for k in range(1, len(ch.cols)):
                B = P["max_route_distance_factor"] * float(impl.gc[ch.cols[k]])
                assert _ratio("route_dist", abs(float(impl.route_dist[ch.cols[k]]) - rd[k]),
                              sr.tol_route(len(steps[k - 1].path), B, rd[k])) <= 1, "route_dist at %d" % ch.cols[k]
            want += segs
        _count_bounds(want, place, t, int(off[t]), st)
        wants.append(want)
    _rule7_caps("stage-isolated", st, max_excl, name)
    for t, want in enumerate(wants):
        _compare_segments(G, impl, t, int(off[t]), want, "stage-isolated")
    return st


def check_isolated(G, batch, P, impl, max_excl=None, name=None):
    """-> rule 7's statistics (what the case reached)."""
    check_columns(batch, P, impl, max_excl)
    check_candidates(G, batch, P, impl, max_excl)
    check_col_prev(batch, P, impl, max_excl)
    check_transitions(G, P, impl, max_excl)
    chains = check_viterbi(batch, impl, max_excl)
    return check_segments(G, batch, P, impl, chains, max_excl, name)


# ---------------------------------------------------------------------- end to end
def check_end_to_end(ref, impl, max_excl=None, name=None):
    """The reference's own segments, their boundaries made from its own
    placements, against the implementation's final records, on the traces the
    reference did not exclude; and its placements against the implementation's
    `ipos` within tol_ipos on the same traces (its states are the
    implementation's there).  -> rule 7's statistics."""
    G, batch, P = ref.G, ref.batch, ref.P
    ntr = len(batch["trace_off"]) - 1
    _cap("end to end", ref.dropped, ntr, TRACE_CAP, max_excl, ref.why)
    assert ref.amb_entries <= (ENTRY_CAP * ref.n_entries if max_excl is None else max_excl), \
        "end to end: %d of %d transition entries ambiguous" % (ref.amb_entries, ref.n_entries)
    off = np.asarray(batch["trace_off"])
    times = np.asarray(batch["time"], np.float64)
    ll, place = _latlon(batch), ref.place
    keep = ~np.isin(_trace_of(batch), list(ref.dropped))
    st = _new_stats()
    st["pts"], st["pts_amb"] = int((place.in_step & keep).sum()), int((place.in_step & place.amb & keep).sum())
    wants = {}
    for t, chs in enumerate(ref.chains):
        if t in ref.dropped:
            continue
        want = []
        for ch in chs:
            segs, _, _, s7 = sr.segments_of_chain(G, P, int(off[t]), times, ch.cols, ch.state, ref.ce, ref.co, ref.gc,
                                                  off_tol=ref.otol, place=place, latlon=ll)
            st["dropped"] += s7["dropped"]
            want += segs
        _count_bounds(want, place, t, int(off[t]), st)
        wants[t] = want
    _rule7_caps("end to end", st, max_excl, name)
    got = np.asarray(impl.ipos, np.float64)
    for k in np.nonzero(place.in_step & ~place.amb & keep)[0]:
        if place.pos[k] < 0:
            assert got[k] == -1.0, "end to end: point %d is placed at %r, the reference leaves it unplaced" % (
                k, got[k])
            st["unplaced"] += 1
        else:
            assert got[k] >= 0.0, "end to end: point %d is unplaced, the reference places it at %r" % (k, place.pos[k])
            assert _ratio("ipos_end_to_end", abs(got[k] - place.pos[k]), place.tol[k]) <= 1 or got[k] == place.pos[k], \
                "end to end: ipos of point %d: %r, reference %r (bound %g)" % (k, got[k], place.pos[k], place.tol[k])
            st["placed"] += 1
    for t, want in wants.items():
        _compare_segments(G, impl, t, int(off[t]), want, "end to end")
    return st
