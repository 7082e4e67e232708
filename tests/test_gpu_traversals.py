"""k_traversals (DESIGN.md §3 rule 7d) through the C ABI, under both launch
plans: the matched route of the inputs of tests/specref_cases.py and
tests/traversals_cases.py,

 * exact against the batch's own segments: grouped by `segment`, a trace's
   records give its otm_segment records (count, shape indices, the two times
   bit for bit where valid, validity, segment id, way ids, INTERNAL);
 * exact chain invariants: bit-equal hand-over of times and shape indices,
   node connectivity, begin_offset 0 except with CHAIN_START, end_offset the
   edge's length bit for bit except with CHAIN_END, no records for a trace
   answered 500 or without segments, trav_off monotone and ending at n;
 * against the independent float64 reference (tests/traversals_ref.py) on the
   engine's own stage arrays (`Engine.debug`): edge, flags, `segment` and the
   chain ends' offsets exactly; every unambiguous boundary's shape index
   exactly and its time within the reference's bound.  The ambiguity caps
   (traversals_ref.assert_caps) are asserted before anything is compared.

The hand-over has one exception, found on the reference (test_traversals.py)
and asserted here in its exact form: across a state on a node candidate, whose
own traversal is not emitted, the record before ends in the step before (at
its R: the state's time and point) and the record after begins in the step
after (at 0), where interpolated points standing on the node are anchors and
a step of R = 0 names its end point.  There exit_time <= enter_time, and both
are the times of the points their shape indices name.

Batch shapes, the switch, and the interface paths that carry the records
(compact batches, clones, a repeated fetch, the device arrays, a two-member
engine, regrown and resumed batches) follow tests/test_gpu_points.py.
"""
import ctypes as C

import numpy as np
import numpy.testing as npt
import pytest

import specref as sr
import specref_cases
import traversals_cases
import traversals_ref as tr
from reporter_amd._lib import TRAVERSAL_DTYPE, Traversal  # noqa: F401  (the record: no such names before this API)

pytestmark = pytest.mark.gpu

KMAX = sr.KMAX
STAGES = ("state", "cand_edge", "cand_off", "ipos", "is_col", "chain_start")
HANDS = ("hand_edge_cases", "hand_radius_0", "hand_star", "hand_short_edges", "hand_curve_interp", "hand_hairpin",
         "hand_filter", "hand_long_edge", "hand_many_short")
RATIOS = {}     # quantity -> largest error / bound seen
_G = {}         # case -> (specref.Graph, params)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    from reporter_amd import synth
    d = tmp_path_factory.mktemp("traversals_gpu")
    out = specref_cases.build(d, synth)
    out.update(traversals_cases.build(d))
    return out


@pytest.fixture(params=["large", "small"])
def plan(request, monkeypatch):
    """The two launch plans of a batch, forced as tests/test_gpu_specref.py forces them."""
    monkeypatch.setenv("OTM_SMALL_POINTS", "0" if request.param == "large" else str(1 << 40))
    return request.param


def _ratio(name, err, bound):
    r = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    return r


def _graph(cases, name):
    if name not in _G:
        graph, _, meili, _ = cases[name]
        _G[name] = (sr.Graph(graph), sr.params(**meili))
    return _G[name]


def _bits(x):
    return np.asarray(x).view(np.uint32 if np.asarray(x).dtype.itemsize == 4 else np.uint64)


def check_exact(G, batch, res, recs, toff, st, what):
    """Everything that is exact without a reference: the records against the
    batch's own segments, and the chain invariants."""
    nt = len(batch["trace_off"]) - 1
    assert recs.dtype.itemsize == 56 and len(toff) == nt + 1, what
    assert toff[0] == 0 and (np.diff(toff) >= 0).all() and toff[-1] == len(recs), what + " trav_off"
    assert not recs["pad"].any(), what
    f = recs["flags"]
    elen32 = np.asarray(G.elen, np.float32)
    npt.assert_array_equal(recs["way_id"], G.eway[recs["edge"]], err_msg=what + " way_id")
    npt.assert_array_equal((f & tr.FROM_START) != 0, recs["begin_offset"] == 0, err_msg=what + " FROM_START")
    npt.assert_array_equal((f & tr.TO_END) != 0, _bits(recs["end_offset"]) == _bits(elen32[recs["edge"]]),
                           err_msg=what + " TO_END")
    assert ((f & (tr.FROM_START | tr.CHAIN_START)) != 0).all(), what + ": begin_offset 0 except with CHAIN_START"
    assert ((f & (tr.TO_END | tr.CHAIN_END)) != 0).all(), what + ": the edge's length except with CHAIN_END"
    npt.assert_array_equal((f & tr.INTERNAL) != 0,
                           (G.eseg[recs["edge"]] < 0) & ((G.eflags[recs["edge"]] & sr.INTERNAL) != 0),
                           err_msg=what + " INTERNAL")
    times = np.asarray(batch["time"], np.float64)
    for t in range(nt):
        r = recs[toff[t]:toff[t + 1]]
        trc = res.traces[t]
        segs = res.segments[trc["seg_off"]:trc["seg_off"] + trc["seg_cnt"]]
        at = "%s trace %d" % (what, t)
        if trc["code"] != 200 or len(segs) == 0:
            assert len(r) == 0, at + ": records without segments"
            continue
        t0 = int(batch["trace_off"][t])
        # ---- the groups are the segments
        sg = r["segment"]
        assert len(r) and sg[0] == 0 and sg[-1] == len(segs) - 1 and set(np.diff(sg)) <= {0, 1}, at + " segment"
        first = np.concatenate([[True], np.diff(sg) == 1])
        npt.assert_array_equal((r["flags"] & tr.SEGMENT_FIRST) != 0, first, err_msg=at + " SEGMENT_FIRST")
        for k, s in enumerate(segs):
            gr = r[sg == k]
            a, b = gr[0], gr[-1]
            ak = at + " segment %d" % k
            assert s["begin_shape_index"] == a["begin_shape_index"] and s["end_shape_index"] == b["end_shape_index"], ak
            es = G.eseg[gr["edge"]]
            if s["segment_id"] >= 0:
                assert (es >= 0).all() and (G.gid[es] == np.uint64(s["segment_id"])).all(), ak + " segment_id"
                p0 = int(G.eseg_pos[a["edge"]])
                assert list(G.eseg_pos[gr["edge"]]) == list(range(p0, p0 + len(gr))), ak
                sv = bool(a["flags"] & tr.FROM_START) and G.eseg_pos[a["edge"]] == 0
                ev = bool(b["flags"] & tr.TO_END) and G.eseg_pos[b["edge"]] == G.gn[es[0]] - 1
            else:
                assert (es < 0).all(), ak + " segment_id"
                sv, ev = bool(a["flags"] & tr.FROM_START), bool(b["flags"] & tr.TO_END)
            assert bool(s["flags"] & 1) == sv and bool(s["flags"] & 2) == ev, ak + " validity"
            if sv:
                assert _bits(s["start_time"]) == _bits(a["enter_time"]), ak + " start_time"
            if ev:
                assert _bits(s["end_time"]) == _bits(b["exit_time"]), ak + " end_time"
            ways = [int(x) for x in res.way_ids[s["way_off"]:s["way_off"] + s["way_cnt"]]]
            mine = [int(w) for i, w in enumerate(gr["way_id"]) if i == 0 or w != gr["way_id"][i - 1]]
            assert ways == mine, ak + " way_ids"
            internal = (gr["flags"] & tr.INTERNAL) != 0
            assert internal.all() == internal.any() == bool(s["flags"] & 4), ak + " INTERNAL"
        # ---- chains
        assert r[0]["flags"] & tr.CHAIN_START and r[-1]["flags"] & tr.CHAIN_END, at
        for i in range(len(r) - 1):
            a, b = r[i], r[i + 1]
            ai = at + " record %d" % i
            assert bool(a["flags"] & tr.CHAIN_END) == bool(b["flags"] & tr.CHAIN_START), ai
            if b["flags"] & tr.CHAIN_START:
                assert b["flags"] & tr.SEGMENT_FIRST, ai
                continue
            assert G.eto[a["edge"]] == G.efrom[b["edge"]], ai + " connectivity"
            same = _bits(a["exit_time"]) == _bits(b["enter_time"]) and a["end_shape_index"] == b["begin_shape_index"]
            if not same:
                # across node-candidate states only (the module docstring)
                lo, hi = t0 + int(a["end_shape_index"]), t0 + int(b["begin_shape_index"])
                assert lo < hi, ai
                for p in range(lo, hi):
                    on_node = st["state"][p] < 0 or st["cand_off"][p * KMAX + st["state"][p]] == 0
                    assert not st["is_col"][p] or on_node, ai
                assert a["exit_time"] == times[lo] <= b["enter_time"] <= times[hi], ai


def compare(G, P, batch, eng, res, hand, what):
    """The engine's records of its last batch: check_exact, then against the
    reference on its own stage arrays.  -> (records, trav_off, the reference's Result)."""
    st = {k: eng.debug(k) for k in STAGES}
    recs, toff = eng.traversals()
    check_exact(G, batch, res, recs, toff, st, what)
    chains = tr.chains_from_stages(batch, st["is_col"], st["state"], st["chain_start"])
    ref = tr.reference(G, P, batch, chains, st["state"], st["cand_edge"], st["cand_off"], st["ipos"],
                       res.traces["code"])
    print(what, "traversals:", ref.trav, "boundaries:", ref.bounds, "inside steps with interpolated points:",
          ref.inside, "ambiguous:", ref.amb)
    tr.assert_caps(ref, hand, what)              # the caps, before anything is compared
    for t, want in enumerate(ref.by_trace):
        got = recs[toff[t]:toff[t + 1]]
        at = "%s trace %d" % (what, t)
        assert len(got) == len(want), at + ": %d records, reference %d" % (len(got), len(want))
        for i, (g, w) in enumerate(zip(got, want)):
            ai = at + " record %d" % i
            assert (g["edge"], g["flags"], g["segment"], g["way_id"]) == (w.edge, w.flags, w.segment, w.way_id), ai
            assert _bits(g["begin_offset"]) == _bits(np.float32(w.off0)), ai + " begin_offset"
            assert _bits(g["end_offset"]) == _bits(np.float32(w.off1)), ai + " end_offset"
            for (tm, sh, known, tol, inside), gt, gs in ((w.begin, g["enter_time"], g["begin_shape_index"]),
                                                        (w.end, g["exit_time"], g["end_shape_index"])):
                if not known:
                    continue
                assert gs == sh, ai + " shape index %d, reference %d" % (gs, sh)
                nm = "time_anchored" if inside == 2 else "time"
                assert _ratio(nm, abs(float(gt) - tm), tol) <= 1, \
                    ai + " time %r, reference %r (bound %g)" % (gt, tm, tol)
    return recs, toff, ref


def _run(cases, name, **engine_kw):
    from reporter_amd import Engine
    graph, batch, meili, _ = cases[name]
    G, P = _graph(cases, name)
    with Engine(graph_path=graph, traversals=True, **engine_kw, **meili) as eng:
        assert eng.traversals_info() is True
        res = eng.match(batch)
        recs, toff, ref = compare(G, P, batch, eng, res, name in HANDS, name)
        sp = eng.spill_stats()
    return recs, toff, ref, batch, sp


ALL = ["city_5s", "city_30s", "gaps_240s", "radius_120", "radius_300", "dense_1s", "stop_and_go", "turn_factor_0",
       "accuracies", "long_140", "stop_80", "seg_forms"] + list(HANDS)


@pytest.mark.parametrize("name", ALL)
def test_case_against_reference(cases, plan, name):
    recs, toff, ref, batch, _ = _run(cases, name)
    n = np.diff(batch["trace_off"])
    if name == "stop_and_go":
        assert ref.compared_inside >= 200
    if name == "hand_short_edges":
        assert ref.compared_inside == 29
    if name == "seg_forms":
        # the three forms of k_segments: <= 128 points, <= 256, longer; and 253 traversals in <= 128 points
        assert ref.compared_inside >= 180
        assert list(n[1:5]) == [128, 129, 256, 257] and n[5] <= 128 and toff[6] - toff[5] == 253
        assert all(toff[k + 1] > toff[k] for k in range(1, 6))
    if name == "hand_long_edge":
        ids = traversals_cases.IDS[name]
        a, b = recs[toff[0]:toff[1]], recs[toff[1]:toff[2]]
        assert list(a["edge"]) == [ids["a"], ids["L"], ids["c"]] and list(b["edge"]) == [ids["a"], ids["L"]]
        # L: opened in the first chunk of 64 points, closed in the second (the carry, not a lane, holds its opener)
        assert a[1]["begin_shape_index"] <= 1 and a[1]["end_shape_index"] >= 70 and n[0] > 64
        assert b[1]["begin_shape_index"] <= 1 and b[1]["end_shape_index"] == n[1] - 1
        # the backward stay: the chain ends at the largest offset reached, 11 m past its last state's
        st_last = 65.0 + traversals_cases.LONG_GAP * (traversals_cases.LONG_STATES - 2) - 60.0
        assert abs(float(b[1]["end_offset"]) - (st_last + traversals_cases.LONG_GAP)) < 0.01
    if name == "hand_many_short":
        ids = traversals_cases.IDS[name]
        want = [ids["a"]] + [ids["s%d" % k] for k in range(traversals_cases.N_SHORT)] + [ids["b"]]
        for t in (0, 1):
            r = recs[toff[t]:toff[t + 1]]
            assert list(r["edge"]) == want and r[-1]["segment"] == 1 + 13 + 12 * 3


@pytest.mark.parametrize("name", ["stop_and_go", "hand_short_edges", "hand_many_short"])
def test_on_online_routes(cases, plan, name):
    # no route index: the path edges the records are made of come from the online route tiers
    _, _, _, _, sp = _run(cases, name, index_radius_m=0.0)
    assert sp["route_online"] > 0, sp


def test_report_headroom():
    """Not a check: prints the largest error / bound ratios seen (pytest -s)."""
    print("matched route, error / bound:", {k: float("%.3g" % v) for k, v in sorted(RATIOS.items())})


# ------------------------------------------------------------------ the switch
def test_off_by_default(cases, plan, oracle, results_equal):
    from reporter_amd import Engine, OtmError, _lib
    graph, batch, meili, _ = cases["stop_and_go"]
    orc = oracle.match_batch(oracle.Graph(graph), batch, p=oracle.params(**meili), nthreads=4)
    with Engine(graph_path=graph, **meili) as never:
        plain = never.match(batch)
    with Engine(graph_path=graph, **meili) as eng:
        assert eng.traversals_info() is False
        off = eng.match(batch)
        with pytest.raises(OtmError, match="off"):
            eng.traversals()
        with pytest.raises(OtmError, match="off"):
            eng.traversals_device()
        eng.set_traversals(True)
        with pytest.raises(OtmError, match="no batch"):
            eng.traversals()     # the last batch ran with the switch off
        on = eng.match(batch)
        recs, toff = eng.traversals()
        n = len(recs)
        assert n > 100 and toff[-1] == n
        buf = np.zeros(n - 1, dtype=_lib.TRAVERSAL_DTYPE)
        cnt = C.c_int64()
        assert _lib.lib().otm_fetch_traversals(eng.h, buf.ctypes.data, n - 1, None, C.byref(cnt)) == -1  # cap too small
        assert "cap" in _lib.last_error() and cnt.value == n and not buf["flags"].any()
        eng.set_traversals(False)
        with pytest.raises(OtmError, match="off"):
            eng.traversals()
    results_equal(orc, off, "switch off")
    results_equal(orc, on, "switch on")
    for key in ("traces", "segments", "reports", "way_ids"):
        assert getattr(on, key).tobytes() == getattr(off, key).tobytes() == getattr(plain, key).tobytes(), key


# ------------------------------------------------------------------ batch shapes
@pytest.fixture(scope="module")
def star(tmp_path_factory):
    import handgraph
    from test_no_limits import SPOKES, STAR_LON
    return handgraph.star(str(tmp_path_factory.mktemp("trav_star") / "star.otmg"), lon=STAR_LON, n_spokes=SPOKES,
                          length_m=90.0)[0]


def _mixed_star_batch():
    """tests/test_gpu_points.py's recipe (traces 0-2 hold a probe within 20 m of the hub: answered 500 without the
    candidate HBM tier), then a matched trace, a one-point trace, an off-graph trace and another matched one."""
    from test_no_limits import _star_point, star_batch
    b = star_batch()
    more = [[_star_point(5, 85), _star_point(5, 60), _star_point(6, 40)], [_star_point(7, 50)],
            [_star_point(0, 600), _star_point(0, 640)], [_star_point(20, 80), _star_point(20, 55), _star_point(20, 30)]]
    lat = np.array([p[0] for tr_ in more for p in tr_], np.float32)
    lon = np.array([p[1] for tr_ in more for p in tr_], np.float32)
    n = len(b["lat"])
    return dict(trace_off=np.concatenate([b["trace_off"], n + np.cumsum([len(tr_) for tr_ in more])]),
                lat=np.append(b["lat"], lat), lon=np.append(b["lon"], lon),
                time=np.append(b["time"], 5000.0 + np.arange(len(lat)) * 6.0),
                accuracy=np.append(b["accuracy"], np.full(len(lat), 5.0, np.float32)))


def test_mixed_and_empty_batches(star, plan, monkeypatch):
    from reporter_amd import Engine
    monkeypatch.setenv("OTM_CAND_MAX_LOG2", "0")    # no candidate HBM tier: a probe that needs it fails its trace
    meili = dict(search_radius=20.0, max_search_radius=20.0)
    b = _mixed_star_batch()
    G, P = sr.Graph(star), sr.params(**meili)
    empty = dict(trace_off=np.zeros(1, np.int64), lat=np.zeros(0, np.float32), lon=np.zeros(0, np.float32),
                 time=np.zeros(0), accuracy=np.zeros(0, np.float32))
    with Engine(graph_path=star, traversals=True, **meili) as eng:
        r = eng.match(empty)
        recs, toff = eng.traversals()
        assert len(r.traces) == 0 and len(recs) == 0 and list(toff) == [0] and eng.traversals_device()[2] == 0
        res = eng.match(b)
        assert list(res.traces["code"][:4]) == [500, 500, 500, 200]
        recs, toff, _ = compare(G, P, b, eng, res, True, "mixed star")
    cnt = list(np.diff(toff))
    assert cnt[:3] == [0, 0, 0] and cnt[3] >= 1 and cnt[4] == 0 and cnt[5] == 0 and cnt[6] >= 1, cnt


# ------------------------------------------------------------------ regrown and resumed batches
def test_regrown_and_resumed_batches(cases, star, plan, monkeypatch):
    from reporter_amd import Engine
    from test_no_limits import RADIUS_100, star_batch
    # a tier's tables grown on demand: the first batch resumes at the candidate HBM tier, the second runs clean
    b = star_batch()
    with Engine(graph_path=star, traversals=True, **RADIUS_100) as eng:
        eng.match(b)
        (first, foff), st1 = eng.traversals(), eng.spill_stats()
        eng.match(b)
        (clean, coff), st2 = eng.traversals(), eng.spill_stats()
    assert st1["attempts"] >= 2 and st1["resumed"] >= 1 and st2["attempts"] == 1
    assert len(clean) >= 6 and first.tobytes() == clean.tobytes() and foff.tobytes() == coff.tobytes()
    # tiny pinned capacities: the transition matrices and the path pool overflow and the batch is redone whole
    graph, batch, meili, _ = cases["stop_and_go"]
    with Engine(graph_path=graph, traversals=True, **meili) as eng:
        eng.match(batch)
        want, woff = eng.traversals()
    monkeypatch.setenv("OTM_TRANS_CAP", "64")
    monkeypatch.setenv("OTM_POOL_CAP", "8")
    with Engine(graph_path=graph, traversals=True, **meili) as eng:
        eng.match(batch)
        (got, goff), st = eng.traversals(), eng.spill_stats()
    assert st["attempts"] >= 2
    assert got.tobytes() == want.tobytes() and goff.tobytes() == woff.tobytes()


# ------------------------------------------------------------------ interface paths
class _DeviceBytes(object):
    """A device buffer under the CUDA array interface, for torch.as_tensor."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def test_compact_clone_device_and_members_agree(cases, plan):
    import torch
    from reporter_amd import Engine, OtmError, _lib
    graph, batch, meili, _ = cases["stop_and_go"]    # whole-second times: a compact batch carries them
    nt = len(batch["trace_off"]) - 1
    with Engine(graph_path=graph, traversals=True, **meili) as eng:
        eng.match(batch)
        base, boff = eng.traversals()
        again, aoff = eng.traversals()
        assert again.tobytes() == base.tobytes() and aoff.tobytes() == boff.tobytes()   # a second fetch: the same bytes
        ptr, optr, cnt = eng.traversals_device()
        assert ptr and optr and cnt == len(base) > 100
        dev = torch.as_tensor(_DeviceBytes(ptr, cnt * 56), device="cuda:0")
        assert dev.cpu().numpy().view(_lib.TRAVERSAL_DTYPE).tobytes() == base.tobytes()
        dev = torch.as_tensor(_DeviceBytes(optr, (nt + 1) * 8), device="cuda:0")
        assert dev.cpu().numpy().view(np.int64).tobytes() == boff.tobytes()
        eng.match_compact(batch)
        got, goff = eng.traversals()
        assert got.tobytes() == base.tobytes() and goff.tobytes() == boff.tobytes()
        cl = eng.clone()
        try:
            assert cl.traversals_info() is True                      # inherited when it was made
            cl.match(batch)
            got, goff = cl.traversals()
            assert got.tobytes() == base.tobytes() and goff.tobytes() == boff.tobytes()
        finally:
            cl.close()
        eng.set_traversals(False)
        cl = eng.clone()
        try:
            assert cl.traversals_info() is False
        finally:
            cl.close()
    with Engine(graph_path=graph, devices=[0, 0], traversals=True, **meili) as grp:
        assert grp.members() == 2 and grp.traversals_info() is True and grp.member(1).traversals_info() is True
        with pytest.raises(OtmError, match="no batch"):
            grp.traversals()
        res = grp.match(batch)
        assert len(res.traces) == nt
        for _ in range(2):
            got, goff = grp.traversals()
            assert got.tobytes() == base.tobytes() and goff.tobytes() == boff.tobytes()
        with pytest.raises(OtmError, match="member"):
            grp.traversals_device()
        # a member view answers for its own share of the group's batch, its arrays sized by the library
        parts = [grp.member(i).traversals() for i in range(2)]
        assert sum(len(o) - 1 for _, o in parts) == nt and all(o[-1] == len(r) for r, o in parts)
        assert min(len(o) for _, o in parts) > 1
        assert parts[0][0].tobytes() + parts[1][0].tobytes() == base.tobytes()
        assert list(parts[0][1]) + [int(x) + len(parts[0][0]) for x in parts[1][1][1:]] == list(boff)


def test_only_binary_batches_leave_records(cases, plan):
    """A JSON batch on the same handle writes no records.  Where it runs on the handle's own buffers it ends
    the last binary batch's records too; either way nothing of a batch with another trace count can be fetched."""
    from reporter_amd import Engine, OtmError, encode_request
    graph, batch, meili, _ = cases["stop_and_go"]
    off = batch["trace_off"]
    small = {k: (batch[k][:off[2]] if k != "trace_off" else off[:3]) for k in batch}
    bodies = [encode_request("veh%d" % t, batch["lat"][off[t]:off[t + 1]], batch["lon"][off[t]:off[t + 1]],
                             batch["time"][off[t]:off[t + 1]].astype(np.int64),
                             batch["accuracy"][off[t]:off[t + 1]].astype(np.int32)) for t in range(len(off) - 1)]
    with Engine(graph_path=graph, **meili) as plain:
        want = plain.report_batch(bodies)
    with Engine(graph_path=graph, traversals=True, **meili) as eng:
        eng.match(small)
        recs, toff = eng.traversals()
        assert len(toff) == 3 and len(recs) > 2
        def same_or_none():
            # the handle's own buffers were used: nothing to fetch; a batch context of its own: still `small`'s
            try:
                r, o = eng.traversals()
            except OtmError as e:
                assert "no batch" in str(e)
                with pytest.raises(OtmError, match="no batch"):
                    eng.traversals_device()
                return None
            assert len(o) == 3 and r.tobytes() == recs.tobytes() and o.tobytes() == toff.tobytes()
            return r
        assert eng.report_batch(bodies) == want                  # many more traces than `small` holds
        first = same_or_none()
        eng.match_json(bodies[0])
        second = same_or_none()
        print("after report_batch:", "none" if first is None else "kept", "after match_json:",
              "none" if second is None else "kept")
        eng.match(small)
        again, aoff = eng.traversals()
        assert again.tobytes() == recs.tobytes() and aoff.tobytes() == toff.tobytes()
