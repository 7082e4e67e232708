"""k_points (DESIGN.md §3 rule 7c) through the C ABI: the matched-point
records of the inputs of tests/specref_cases.py, under both launch plans,
against the independent float64 reference (tests/points_ref.py) run on the
engine's own stage arrays (`Engine.debug`); the switch off (nothing changes);
batch shapes; a trace answered 500 among matched ones; batches that regrow a
capacity or resume at a tier; and the interface paths that carry the records
(compact batches, clones, the device buffer, multi-device engines).

Exact: every flag (ANCHOR recomputed from the engine's own f32 ipos), ROUTE
<=> ipos >= 0, a column's (edge, offset) bit for bit, way_id, the all-zero
record of a point without a place, the edge of an interpolated point.  Within
a bound (points_ref.py, specref.py): an interpolated point's offset, the route
position rebuilt from (edge, offset) against ipos, the coordinate, the
distance.  The ambiguity cap (specref's: 5 % of a case's interpolated points,
none on hand graphs) is checked before anything is compared.
"""
import ctypes as C

import numpy as np
import numpy.testing as npt
import pytest

import points_ref as pr
import specref as sr
import specref_cases
from reporter_amd._lib import POINT_DTYPE, MatchedPoint  # noqa: F401  (the record: no such names before this API)

pytestmark = pytest.mark.gpu

KMAX = sr.KMAX
CAP = 0.05
STAGES = ("state", "cand_edge", "cand_off", "ipos", "is_col", "chain_start", "col_prev")
RATIOS = {}     # quantity -> largest error / bound seen
_G = {}         # case -> (specref.Graph, params)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    from reporter_amd import synth
    return specref_cases.build(tmp_path_factory.mktemp("points_gpu"), synth)


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


def _count(pts):
    f = pts["flags"]
    c = {n: int(((f & b) != 0).sum()) for n, b in (("matched", pr.MATCHED), ("column", pr.COLUMN), ("node", pr.NODE),
                                                   ("chain_start", pr.CHAIN_START), ("route", pr.ROUTE),
                                                   ("anchor", pr.ANCHOR), ("same_edge", pr.SAME_EDGE))}
    c["unmatched"] = int(((f & pr.MATCHED) == 0).sum())
    c["filtered"] = c["route"] - c["anchor"]
    return c


def compare(G, P, batch, eng, res, max_excl, what):
    """The engine's records of its last batch against the reference on its own stage arrays."""
    n = len(batch["lat"])
    st = {k: eng.debug(k) for k in STAGES}
    pts = eng.points()
    assert pts.dtype.itemsize == 40 and len(pts) == n, what
    ref = pr.matched_points(G, P, batch, st, res.traces["code"])
    # the cap, before anything is compared
    n_int, n_amb = int(ref.interp.sum()), int(ref.amb.sum())
    print(what, "interpolated points with a place:", n_int, "ambiguous:", n_amb, _count(pts))
    assert n_amb <= (CAP * n_int if max_excl is None else max_excl), \
        "%s: %d of %d interpolated points excluded as ambiguous" % (what, n_amb, n_int)
    f = pts["flags"]
    # exact: the flags (ANCHOR by the running-maximum rule on the engine's own f32 ipos), ROUTE <=> ipos >= 0
    npt.assert_array_equal(f, ref.flags, err_msg=what + " flags")
    npt.assert_array_equal((f & pr.ROUTE) != 0, st["ipos"][:n] >= 0, err_msg=what + " ROUTE <=> ipos >= 0")
    matched = (f & pr.MATCHED) != 0
    # exact: the all-zero record of a point without a place
    un = pts[~matched]
    assert (un["edge"] == -1).all() and not un["lat"].any() and not un["lon"].any() and not un["offset"].any() \
        and not un["distance"].any() and not un["way_id"].any(), what
    assert ((un["flags"] & ~np.uint32(pr.COLUMN)) == 0).all(), what
    # exact: a column's (edge, offset) is its chosen candidate, bit for bit
    col = matched & ((f & pr.COLUMN) != 0)
    k = np.nonzero(col)[0]
    slot = k * KMAX + st["state"][k]
    npt.assert_array_equal(pts["edge"][k], st["cand_edge"][slot], err_msg=what + " column edge")
    npt.assert_array_equal(pts["offset"][k].view(np.uint32), st["cand_off"][slot].view(np.uint32),
                           err_msg=what + " column offset")
    npt.assert_array_equal(((f[k] & pr.NODE) != 0), pts["offset"][k] == 0, err_msg=what + " NODE")
    # exact: way_id is the record's own edge's way
    npt.assert_array_equal(pts["way_id"][matched], G.eway[pts["edge"][matched]], err_msg=what + " way_id")
    # interpolated points the reference adjudicates: the edge exactly, the offset within the foot's bound,
    # the rebuilt route position within tol_rebuilt of ipos
    for i in np.nonzero(ref.interp & ~ref.amb)[0]:
        assert pts["edge"][i] == ref.edge[i], "%s point %d: edge %d, reference %d" % (what, i, pts["edge"][i], ref.edge[i])
        err = abs(float(pts["offset"][i]) - ref.off[i])
        assert _ratio("offset", err, ref.off_tol[i]) <= 1.0, \
            "%s point %d: offset %r, reference %r, bound %g" % (what, i, pts["offset"][i], ref.off[i], ref.off_tol[i])
        if f[i] & pr.ROUTE:
            x = float(st["ipos"][i])
            reb = ref.xs[i] + (float(pts["offset"][i]) - ref.o0[i])
            assert _ratio("rebuilt ipos", abs(reb - x), pr.tol_rebuilt(int(ref.nsum[i]), x)) <= 1.0, \
                "%s point %d: rebuilt %r, ipos %r" % (what, i, reb, x)
    # every place: the coordinate and the distance of the record's own (edge, offset)
    lat32, lon32 = np.asarray(batch["lat"], np.float32), np.asarray(batch["lon"], np.float32)
    for i in np.nonzero(matched)[0]:
        la, lo, d = pr.coordinate(G, int(pts["edge"][i]), float(pts["offset"][i]), float(lat32[i]), float(lon32[i]))
        assert _ratio("lat", abs(pts["lat"][i] - la), pr.tol_coord(la)) <= 1.0, (what, i, pts["lat"][i], la)
        assert _ratio("lon", abs(pts["lon"][i] - lo), pr.tol_coord(lo)) <= 1.0, (what, i, pts["lon"][i], lo)
        assert _ratio("distance", abs(float(pts["distance"][i]) - d), pr.tol_dist(d, la, lo)) <= 1.0, \
            (what, i, pts["distance"][i], d)
    return pts, ref


# what each case is built for (counts of the records that carry the flag), so none can go empty
REACH = {
    "hand_short_edges": dict(route=15, anchor=15, node=2, chain_start=4),
    "hand_curve_interp": dict(route=5, anchor=3, filtered=2),
    "hand_hairpin": dict(route=3, anchor=3),
    "hand_filter": dict(route=8, anchor=7, filtered=1, node=1, unmatched=8, chain_start=8),
    "hand_edge_cases": dict(matched=13, chain_start=5),
    "stop_and_go": dict(route=200, anchor=200, same_edge=250, node=20, unmatched=20),
    "stop_80": dict(route=specref_cases.STOP_N, anchor=specref_cases.STOP_N),
    "seg_forms": dict(route=100, anchor=100, filtered=4, same_edge=250, node=30, unmatched=5),
    "city_5s": dict(route=5, same_edge=5, node=100, unmatched=1),
}


def _run(cases, name, **engine_kw):
    from reporter_amd import Engine
    graph, batch, meili, max_excl = cases[name]
    G, P = _graph(cases, name)
    with Engine(graph_path=graph, matched_points=True, **engine_kw, **meili) as eng:
        assert eng.points_info() is True
        res = eng.match(batch)
        pts, ref = compare(G, P, batch, eng, res, max_excl, name)
        sp = eng.spill_stats()
    c = _count(pts)
    assert all(c[k] >= v for k, v in REACH[name].items()), (name, REACH[name], c)
    return pts, ref, batch, sp


@pytest.mark.parametrize("name", sorted(REACH))
def test_case_against_reference(cases, plan, name):
    pts, ref, batch, _ = _run(cases, name)
    f = pts["flags"]
    off = [int(x) for x in batch["trace_off"]]
    if name == "stop_80":
        # 80 copies in one step: the max-scan's run crosses the 64-point chunk of its trace, and every copy
        # (equal positions count) is an anchor on both sides of it
        at, n = specref_cases.STOP_AT, specref_cases.STOP_N
        run = pts[at + 1:at + 1 + n]
        assert at + 1 < 64 < at + n and ((run["flags"] & pr.ANCHOR) != 0).all()
        assert (run["edge"] == run["edge"][0]).all() and (run["offset"] == run["offset"][0]).all()
    if name == "seg_forms":
        assert [off[k + 1] - off[k] for k in range(1, 5)] == [128, 129, 256, 257]
        F = specref_cases.FORMS
        first = off[2] + F["stop_at"] + 1
        run = pts[first:first + F["stop_n"]]
        assert first < 256 < first + F["stop_n"] - 1 and ((run["flags"] & pr.MATCHED) != 0).all()
        assert (run.tobytes() == run[:1].tobytes() * F["stop_n"])   # 16 copies of one point: one record, 16 times
    if name == "hand_filter":
        # trace 1: the second interpolated point lies behind the first (the filter drops it: ROUTE without
        # ANCHOR); trace 3: points after the last state; trace 4: an empty column (COLUMN alone) and the
        # points around it; trace 5: a breakage
        a = off[1]
        assert f[a + 1] & pr.ANCHOR and (f[a + 2] & (pr.ROUTE | pr.ANCHOR)) == pr.ROUTE and f[a + 3] & pr.ANCHOR
        assert list(f[off[3] + 3:off[4]]) == [0, 0]
        assert f[off[4] + 3] == pr.COLUMN and f[off[4] + 2] == 0 and f[off[4] + 4] == 0
        assert list(f[off[5] + 1:off[5] + 3]) == [0, 0]
    if name == "hand_edge_cases":
        # the dead-end sink: the probe past the end is put at the edge's end, no node candidate there
        e = specref_cases.EDGE_IDS["sink"]
        G, _ = _graph(cases, name)
        k = off[1] + 1
        assert pts["edge"][k] == e and pts["offset"][k] == np.float32(G.elen[e]) and not f[k] & pr.NODE
        assert pts["way_id"][k] == 1002


@pytest.mark.parametrize("name", ["stop_and_go", "hand_short_edges"])
def test_points_on_online_routes(cases, name):
    # no route index: the paths the placements walk come from the online route tiers
    _, _, _, sp = _run(cases, name, index_radius_m=0.0)
    assert sp["route_online"] > 0, sp


def test_report_headroom():
    """Not a check: prints the largest error / bound ratios seen (pytest -s)."""
    print("matched points, error / bound:", {k: float("%.3g" % v) for k, v in sorted(RATIOS.items())})


# ------------------------------------------------------------------ the switch
def test_off_by_default(cases, oracle, results_equal):
    from reporter_amd import Engine, OtmError, _lib
    graph, batch, meili, _ = cases["stop_and_go"]
    orc =oracle.match_batch(oracle.Graph(graph), batch, p=oracle.params(**meili), nthreads=4)
    with Engine(graph_path=graph, **meili) as eng:
        assert eng.points_info() is False
        off = eng.match(batch)
        with pytest.raises(OtmError, match="off"):
            eng.points()
        with pytest.raises(OtmError, match="off"):
            eng.points_device()
        eng.set_points(True)
        with pytest.raises(OtmError, match="no batch"):
            eng.points()     # the last batch ran with the switch off
        on = eng.match(batch)
        n = len(batch["lat"])
        assert len(eng.points()) == n
        buf = np.zeros(n - 1, dtype=_lib.POINT_DTYPE)
        cnt = C.c_int64()
        assert _lib.lib().otm_fetch_points(eng.h, buf.ctypes.data, n - 1, C.byref(cnt)) == -1   # cap below the count
        assert "cap" in _lib.last_error() and cnt.value == n
        eng.set_points(False)
        with pytest.raises(OtmError, match="off"):
            eng.points()
    results_equal(orc, off, "switch off")
    results_equal(orc, on, "switch on")
    for key in ("traces", "segments", "reports", "way_ids"):
        assert getattr(on, key).tobytes() == getattr(off, key).tobytes(), key


# ------------------------------------------------------------------ batch shapes
def _concat(batches):
    out = {k: np.concatenate([np.asarray(b[k]) for b in batches]) for k in ("lat", "lon", "accuracy", "time")}
    out["trace_off"] = np.cumsum([0] + [len(b["lat"]) for b in batches]).astype(np.int64)
    return out


def test_batch_shapes(cases):
    from reporter_amd import Engine, synth
    graph, _, meili, _ = cases["city_5s"]
    G, P = _graph(cases, "city_5s")
    dense = lambda n, seed: specref_cases._cut(  # noqa: E731
        {k: v for k, v in synth.make_traces(graph, 1, 80, interval_s=0.5, noise_sigma_m=3.0, accuracy=10.0,
                                            seed=seed).items() if k in ("trace_off", "lat", "lon", "time", "accuracy")}, n)
    empty = dict(trace_off=np.zeros(1, np.int64), lat=np.zeros(0, np.float32), lon=np.zeros(0, np.float32),
                 time=np.zeros(0), accuracy=np.zeros(0, np.float32))
    parts = [dense(63, 41), empty, dense(1, 42), dense(64, 43), dense(65, 44)]
    b = _concat(parts)
    assert list(np.diff(b["trace_off"])) == [63, 0, 1, 64, 65]
    with Engine(graph_path=graph, matched_points=True, **meili) as eng:
        r = eng.match(empty)
        assert len(r.traces) == 0 and len(eng.points()) == 0 and eng.points_device() == (0, 0)
        res = eng.match(b)
        pts, _ = compare(G, P, b, eng, res, None, "shapes")
        c = _count(pts)
        assert c["same_edge"] + c["route"] >= 30 and c["matched"] >= 100, c
        one = pts[63]
        assert one["flags"] & pr.MATCHED and one["flags"] & pr.COLUMN and one["flags"] & pr.CHAIN_START
        # a trace's records do not depend on where it lies in the batch
        eng.match(parts[4])
        assert eng.points().tobytes() == pts[128:].tobytes()


# ------------------------------------------------------------------ a trace answered 500; regrown and resumed batches
@pytest.fixture(scope="module")
def star(tmp_path_factory):
    import handgraph
    from test_no_limits import SPOKES, STAR_LON
    return handgraph.star(str(tmp_path_factory.mktemp("points_star") / "star.otmg"), lon=STAR_LON, n_spokes=SPOKES,
                          length_m=90.0)[0]


def _star_batch_with_a_far_trace():
    """tests/test_no_limits.py's cap case: traces 0-2 each hold a probe within 20 m of the hub, trace 3 none."""
    from test_no_limits import _star_point, star_batch
    b = star_batch()
    lat, lon = zip(*[_star_point(5, 85), _star_point(5, 60), _star_point(6, 40)])
    return dict(trace_off=np.append(b["trace_off"], len(b["lat"]) + 3),
                lat=np.append(b["lat"], np.array(lat, np.float32)), lon=np.append(b["lon"], np.array(lon, np.float32)),
                time=np.append(b["time"], 5000.0 + np.arange(3) * 6.0),
                accuracy=np.append(b["accuracy"], np.full(3, 5.0, np.float32)))


def test_trace_answered_500(star, monkeypatch):
    from reporter_amd import Engine
    monkeypatch.setenv("OTM_CAND_MAX_LOG2", "0")    # no candidate HBM tier: a probe that needs it fails its trace
    meili = dict(search_radius=20.0, max_search_radius=20.0)
    b = _star_batch_with_a_far_trace()
    G, P = sr.Graph(star), sr.params(**meili)
    with Engine(graph_path=star, matched_points=True, **meili) as eng:
        res = eng.match(b)
        assert list(res.traces["code"]) == [500, 500, 500, 200]
        pts, _ = compare(G, P, b, eng, res, 0, "star 500")
        is_col = eng.debug("is_col")
    a = int(b["trace_off"][3])
    bad, good = pts[:a], pts[a:]
    assert (bad["edge"] == -1).all() and ((bad["flags"] & ~np.uint32(pr.COLUMN)) == 0).all()
    npt.assert_array_equal((bad["flags"] & pr.COLUMN) != 0, is_col[:a] != 0)
    assert not any(bad[k].any() for k in ("lat", "lon", "offset", "distance", "way_id"))
    assert ((good["flags"] & pr.MATCHED) != 0).all()


def test_regrown_and_resumed_batches(cases, star, monkeypatch):
    from reporter_amd import Engine
    from test_no_limits import RADIUS_100, star_batch
    # a tier's tables grown on demand: the first batch resumes at the candidate HBM tier, the second runs clean
    b = star_batch()
    with Engine(graph_path=star, matched_points=True, **RADIUS_100) as eng:
        eng.match(b)
        first, st1 = eng.points(), eng.spill_stats()
        eng.match(b)
        clean, st2 = eng.points(), eng.spill_stats()
    assert st1["attempts"] >= 2 and st1["resumed"] >= 1 and st2["attempts"] == 1
    assert ((clean["flags"] & pr.MATCHED) != 0).all()
    assert first.tobytes() == clean.tobytes()
    # tiny pinned capacities: the transition matrices and the path pool overflow and the batch is redone whole
    graph, batch, meili, _ = cases["stop_and_go"]
    with Engine(graph_path=graph, matched_points=True, **meili) as eng:
        eng.match(batch)
        want = eng.points()
    monkeypatch.setenv("OTM_TRANS_CAP", "64")
    monkeypatch.setenv("OTM_POOL_CAP", "8")
    with Engine(graph_path=graph, matched_points=True, **meili) as eng:
        eng.match(batch)
        got, st = eng.points(), eng.spill_stats()
    assert st["attempts"] >= 2
    assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------ interface paths
class _DeviceBytes(object):
    """A device buffer under the CUDA array interface, for torch.as_tensor."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def test_compact_clone_device_and_members_agree(cases):
    import torch
    from reporter_amd import Engine, _lib
    graph, batch, meili, _ = cases["stop_and_go"]    # whole-second times: a compact batch carries them
    n = len(batch["lat"])
    with Engine(graph_path=graph, matched_points=True, **meili) as eng:
        eng.match(batch)
        base = eng.points()
        assert eng.points().tobytes() == base.tobytes()          # a second fetch: the same bytes
        ptr, cnt = eng.points_device()
        assert ptr and cnt == n
        dev = torch.as_tensor(_DeviceBytes(ptr, n * 40), device="cuda:0")
        assert dev.cpu().numpy().view(_lib.POINT_DTYPE).tobytes() == base.tobytes()
        eng.match_compact(batch)
        assert eng.points().tobytes() == base.tobytes()
        cl = eng.clone()
        try:
            assert cl.points_info() is True                      # inherited when it was made
            cl.match(batch)
            assert cl.points().tobytes() == base.tobytes()
        finally:
            cl.close()
        eng.set_points(False)
        cl = eng.clone()
        try:
            assert cl.points_info() is False
        finally:
            cl.close()
    c = _count(base)
    assert c["route"] >= 200 and c["same_edge"] >= 250
    with Engine(graph_path=graph, devices=[0, 0], matched_points=True, **meili) as grp:
        assert grp.members() == 2 and grp.points_info() is True and grp.member(1).points_info() is True
        from reporter_amd import OtmError
        with pytest.raises(OtmError, match="no batch"):
            grp.points()
        res = grp.match(batch)
        assert len(res.traces) == len(batch["trace_off"]) - 1
        assert grp.points().tobytes() == base.tobytes()
        assert grp.points().tobytes() == base.tobytes()
        with pytest.raises(OtmError, match="member"):
            grp.points_device()
