"""k_shape (DESIGN.md §3 rule 7f) through the C ABI, under both launch plans:
`Engine.shape()` is exactly tests/shape_ref.py applied to the engine's own
`Engine.traversals()` records -- vertices, vtx_off, spans, trav_off, poly_off
equal and the polyline byte-equal, with no tolerance -- on the hand cases of
tests/shape_cases.py and the cases it names from tests/specref_cases.py and
tests/traversals_cases.py (each asserting what it reached).

Then the switch (alone, it changes nothing else of a match and does not turn
the matched route's fetch on), and the interface paths that carry the arrays:
a repeated fetch, the device arrays, clones, compact batches, a two-member
engine, regrown and resumed batches, empty batches and traces without
segments, a JSON batch on the handle.  Batch shapes follow
tests/test_gpu_traversals.py.
"""
import ctypes as C

import numpy as np
import numpy.testing as npt
import pytest

import shape_cases
import shape_ref
import specref as sr
import specref_cases
import traversals_cases
from reporter_amd._lib import SHAPE_SPAN_DTYPE, SHAPE_VERTEX_DTYPE  # noqa: F401  (no such names before this API)

pytestmark = pytest.mark.gpu

_G = {}         # case -> specref.Graph


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    from reporter_amd import synth
    d = tmp_path_factory.mktemp("shape_gpu")
    out = specref_cases.build(d, synth)
    out.update(traversals_cases.build(d))
    out.update(shape_cases.build(d))
    return out


@pytest.fixture(params=["large", "small"])
def plan(request, monkeypatch):
    """The two launch plans of a batch, forced as tests/test_gpu_traversals.py forces them."""
    monkeypatch.setenv("OTM_SMALL_POINTS", "0" if request.param == "large" else str(1 << 40))
    return request.param


def _graph(cases, name):
    if name not in _G:
        _G[name] = sr.Graph(cases[name][0])
    return _G[name]


def _same(a, b):
    """Two Engine.shape() results, byte for byte."""
    return len(a) == len(b) == 6 and all(
        (x == y) if isinstance(x, bytes) else (x.dtype == y.dtype and x.tobytes() == y.tobytes()) for x, y in zip(a, b))


def compare(G, recs, toff, got, what):
    """An Engine.shape() result against the restatement on the records (recs, toff).  -> the reference."""
    vtx, vtx_off, spans, trav_off, poly, poly_off = got
    nt = len(toff) - 1
    ref = shape_ref.reference(G, recs["edge"].astype(np.int64), recs["begin_offset"], recs["end_offset"],
                              recs["flags"], toff)
    assert vtx.dtype == SHAPE_VERTEX_DTYPE and spans.dtype == SHAPE_SPAN_DTYPE and isinstance(poly, bytes), what
    assert len(vtx_off) == len(trav_off) == len(poly_off) == nt + 1, what
    npt.assert_array_equal(trav_off, toff, err_msg=what + " trav_off")
    npt.assert_array_equal(vtx_off, ref.vtx_off, err_msg=what + " vtx_off")
    npt.assert_array_equal(poly_off, ref.poly_off, err_msg=what + " poly_off")
    npt.assert_array_equal(np.stack([vtx["lat_e6"], vtx["lon_e6"]], 1).reshape(-1, 2), ref.vertices,
                           err_msg=what + " vertices")
    npt.assert_array_equal(np.stack([spans["begin_vertex"], spans["end_vertex"]], 1).reshape(-1, 2), ref.spans,
                           err_msg=what + " spans")
    for t in range(nt):
        assert poly[poly_off[t]:poly_off[t + 1]] == ref.polylines[t], "%s trace %d polyline" % (what, t)
    assert len(poly) == poly_off[-1] and len(vtx) == vtx_off[-1] and len(spans) == trav_off[-1], what
    return ref


def _run(cases, name, **engine_kw):
    from reporter_amd import Engine
    graph, batch, meili, _ = cases[name]
    G = _graph(cases, name)
    with Engine(graph_path=graph, traversals=True, shape=True, **engine_kw, **meili) as eng:
        assert eng.shape_info() is True
        eng.match(batch)
        recs, toff = eng.traversals()
        got = eng.shape()
        ref = compare(G, recs, toff, got, name)
        sp = eng.spill_stats()
    shape_cases.assert_reached(name, G, recs["edge"].astype(np.int64), recs["begin_offset"], recs["end_offset"],
                               recs["flags"], toff, ref.spans, ref.vtx_off, ref.polylines)
    print(name, "records:", len(recs), "vertices:", len(got[0]), "bytes:", len(got[4]))
    return got, sp


@pytest.mark.parametrize("name", shape_cases.ALL)
def test_case_against_reference(cases, plan, name):
    _run(cases, name)


@pytest.mark.parametrize("name", ["stop_and_go", "hand_shape"])
def test_on_online_routes(cases, plan, name):
    # no route index: the path edges the records are made of come from the online route tiers
    _, sp = _run(cases, name, index_radius_m=0.0)
    assert sp["route_online"] > 0, sp


# ------------------------------------------------------------------ the switch
def test_off_by_default(cases, plan):
    from reporter_amd import Engine, OtmError
    graph, batch, meili, _ = cases["stop_and_go"]
    with Engine(graph_path=graph, **meili) as eng:
        assert eng.shape_info() is False
        eng.match(batch)
        with pytest.raises(OtmError, match="off"):
            eng.shape()
        with pytest.raises(OtmError, match="off"):
            eng.shape_device()
        eng.set_shape(True)
        with pytest.raises(OtmError, match="no batch"):
            eng.shape()              # the last batch ran with the switch off
        eng.match(batch)
        got = eng.shape()
        assert len(got[0]) > 100 and got[1][-1] == len(got[0])
        # a cap below its count: nothing is copied
        from reporter_amd import _lib
        buf = np.zeros(len(got[0]) - 1, dtype=SHAPE_VERTEX_DTYPE)
        dst = _lib.ShapeOut(buf.ctypes.data, len(buf), None, None, 0, None, None, 0, None)
        assert _lib.lib().otm_fetch_shape(eng.h, C.byref(dst)) == -1 and "cap" in _lib.last_error()
        assert not buf["lat_e6"].any()
        eng.set_shape(False)
        with pytest.raises(OtmError, match="off"):
            eng.shape()


def test_shape_alone_changes_nothing_else(cases, plan, results_equal):
    """With the shape on and the matched route off, k_traversals runs for the shape alone: the same shape,
    no route to fetch, and results, points and scores as without the switch."""
    from reporter_amd import Engine, OtmError
    graph, batch, meili, _ = cases["stop_and_go"]
    with Engine(graph_path=graph, traversals=True, shape=True, **meili) as eng:
        eng.match(batch)
        both = eng.shape()
    with Engine(graph_path=graph, matched_points=True, scores=True, **meili) as eng:
        plain = eng.match(batch)
        ppts, psc = eng.points(), eng.scores()
    with Engine(graph_path=graph, matched_points=True, scores=True, shape=True, **meili) as eng:
        assert eng.traversals_info() is False
        res = eng.match(batch)
        alone = eng.shape()
        with pytest.raises(OtmError, match="off"):
            eng.traversals()
        with pytest.raises(OtmError, match="off"):
            eng.traversals_device()
        pts, sc = eng.points(), eng.scores()
        eng.set_traversals(True)
        with pytest.raises(OtmError, match="no batch"):
            eng.traversals()         # the batch ran with the route's switch off
    assert _same(alone, both) and len(alone[0]) > 100
    results_equal(plain, res, "shape alone")
    for key in ("traces", "segments", "reports", "way_ids"):
        assert getattr(res, key).tobytes() == getattr(plain, key).tobytes(), key
    assert pts.tobytes() == ppts.tobytes() and sc.tobytes() == psc.tobytes()


# ------------------------------------------------------------------ batch shapes
@pytest.fixture(scope="module")
def star(tmp_path_factory):
    import handgraph
    from test_no_limits import SPOKES, STAR_LON
    return handgraph.star(str(tmp_path_factory.mktemp("shape_star") / "star.otmg"), lon=STAR_LON, n_spokes=SPOKES,
                          length_m=90.0)[0]


def test_empty_batches_and_traces_without_segments(star, plan, monkeypatch):
    from reporter_amd import Engine
    from test_gpu_traversals import _mixed_star_batch
    monkeypatch.setenv("OTM_CAND_MAX_LOG2", "0")    # no candidate HBM tier: a probe that needs it fails its trace
    meili = dict(search_radius=20.0, max_search_radius=20.0)
    b = _mixed_star_batch()
    G = sr.Graph(star)
    empty = dict(trace_off=np.zeros(1, np.int64), lat=np.zeros(0, np.float32), lon=np.zeros(0, np.float32),
                 time=np.zeros(0), accuracy=np.zeros(0, np.float32))
    # one-point and off-graph traces only: no trace has a segment
    o = b["trace_off"]
    none = {k: (b[k][o[4]:o[6]] if k != "trace_off" else o[4:7] - o[4]) for k in b}
    with Engine(graph_path=star, traversals=True, shape=True, **meili) as eng:
        eng.match(empty)
        vtx, vtx_off, spans, trav_off, poly, poly_off = eng.shape()
        assert len(vtx) == len(spans) == 0 and poly == b"" and list(vtx_off) == list(trav_off) == list(poly_off) == [0]
        dev, z = eng.shape_device()
        assert (z.n_traces, z.n_traversals, z.n_vertices, z.n_bytes) == (0, 0, 0, 0)
        eng.match(none)
        vtx, vtx_off, spans, trav_off, poly, poly_off = eng.shape()
        assert len(vtx) == len(spans) == 0 and poly == b""
        assert list(vtx_off) == list(trav_off) == list(poly_off) == [0, 0, 0]
        res = eng.match(b)
        assert list(res.traces["code"][:4]) == [500, 500, 500, 200]
        recs, toff = eng.traversals()
        got = eng.shape()
        compare(G, recs, toff, got, "mixed star")
    cnt = list(np.diff(got[1]))
    assert cnt[:3] == [0, 0, 0] and cnt[3] >= 2 and cnt[4] == 0 and cnt[5] == 0 and cnt[6] >= 2, cnt
    assert [int(x) for x in np.diff(got[5])][:3] == [0, 0, 0] and got[5][4] > got[5][3]


# ------------------------------------------------------------------ regrown and resumed batches
def test_regrown_and_resumed_batches(cases, star, plan, monkeypatch):
    from reporter_amd import Engine
    from test_no_limits import RADIUS_100, star_batch
    # a tier's tables grown on demand: the first batch resumes at the candidate HBM tier, the second runs clean
    b = star_batch()
    with Engine(graph_path=star, shape=True, **RADIUS_100) as eng:
        eng.match(b)
        first, st1 = eng.shape(), eng.spill_stats()
        eng.match(b)
        clean, st2 = eng.shape(), eng.spill_stats()
    assert st1["attempts"] >= 2 and st1["resumed"] >= 1 and st2["attempts"] == 1
    assert len(clean[0]) >= 6 and _same(first, clean)
    # tiny pinned capacities: the transition matrices and the path pool overflow and the batch is redone whole
    graph, batch, meili, _ = cases["stop_and_go"]
    with Engine(graph_path=graph, shape=True, **meili) as eng:
        eng.match(batch)
        want = eng.shape()
    monkeypatch.setenv("OTM_TRANS_CAP", "64")
    monkeypatch.setenv("OTM_POOL_CAP", "8")
    with Engine(graph_path=graph, shape=True, **meili) as eng:
        eng.match(batch)
        got, st = eng.shape(), eng.spill_stats()
    assert st["attempts"] >= 2
    assert _same(got, want)


# ------------------------------------------------------------------ interface paths
class _DeviceBytes(object):
    """A device buffer under the CUDA array interface, for torch.as_tensor."""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def _dev_bytes(ptr, nbytes):
    import torch
    return torch.as_tensor(_DeviceBytes(ptr, nbytes), device="cuda:0").cpu().numpy().tobytes()


def test_compact_clone_device_and_members_agree(cases, plan):
    from reporter_amd import Engine, OtmError
    graph, batch, meili, _ = cases["stop_and_go"]    # whole-second times: a compact batch carries them
    nt = len(batch["trace_off"]) - 1
    with Engine(graph_path=graph, shape=True, **meili) as eng:
        eng.match(batch)
        base = eng.shape()
        assert _same(eng.shape(), base)                                   # a second fetch: the same bytes
        vtx, vtx_off, spans, trav_off, poly, poly_off = base
        dev, z = eng.shape_device()
        assert (z.n_traces, z.n_traversals, z.n_vertices, z.n_bytes) == (nt, len(spans), len(vtx), len(poly))
        assert (dev.vertices_cap, dev.spans_cap, dev.polyline_cap) == (len(vtx), len(spans), len(poly))
        assert len(vtx) > 100 and dev.vertices and dev.spans and dev.polyline
        assert _dev_bytes(dev.vertices, len(vtx) * 8) == vtx.tobytes()
        assert _dev_bytes(dev.spans, len(spans) * 8) == spans.tobytes()
        assert _dev_bytes(dev.polyline, len(poly)) == poly
        for ptr, off in ((dev.vtx_off, vtx_off), (dev.trav_off, trav_off), (dev.poly_off, poly_off)):
            assert _dev_bytes(ptr, (nt + 1) * 8) == off.tobytes()
        assert _same(eng.shape(), base)
        eng.match_compact(batch)
        assert _same(eng.shape(), base)
        cl = eng.clone()
        try:
            assert cl.shape_info() is True and cl.traversals_info() is False   # inherited when it was made
            cl.match(batch)
            assert _same(cl.shape(), base)
        finally:
            cl.close()
        eng.set_shape(False)
        cl = eng.clone()
        try:
            assert cl.shape_info() is False
        finally:
            cl.close()
    with Engine(graph_path=graph, devices=[0, 0], shape=True, **meili) as grp:
        assert grp.members() == 2 and grp.shape_info() is True and grp.member(1).shape_info() is True
        with pytest.raises(OtmError, match="no batch"):
            grp.shape()
        res = grp.match(batch)
        assert len(res.traces) == nt
        for _ in range(2):
            assert _same(grp.shape(), base)
        with pytest.raises(OtmError, match="member"):
            grp.shape_device()
        with pytest.raises(OtmError, match="off"):
            grp.traversals()
        # a member view answers for its own share of the group's batch
        parts = [grp.member(i).shape() for i in range(2)]
        assert sum(len(p[1]) - 1 for p in parts) == nt and min(len(p[1]) for p in parts) > 1
        assert parts[0][0].tobytes() + parts[1][0].tobytes() == vtx.tobytes()
        assert parts[0][2].tobytes() + parts[1][2].tobytes() == spans.tobytes()
        assert parts[0][4] + parts[1][4] == poly


def test_a_json_batch_ends_the_shape(cases, plan):
    """A JSON batch on the handle writes no shape and ends the last binary batch's: never another batch's shape."""
    from reporter_amd import Engine, OtmError, encode_request
    graph, batch, meili, _ = cases["stop_and_go"]
    off = batch["trace_off"]
    small = {k: (batch[k][:off[2]] if k != "trace_off" else off[:3]) for k in batch}
    body = encode_request("veh0", batch["lat"][off[5]:off[6]], batch["lon"][off[5]:off[6]],
                          batch["time"][off[5]:off[6]].astype(np.int64),
                          batch["accuracy"][off[5]:off[6]].astype(np.int32))
    with Engine(graph_path=graph, shape=True, **meili) as eng:
        eng.match(small)
        first = eng.shape()
        assert len(first[1]) == 3 and len(first[0]) > 2
        eng.match_json(body)
        with pytest.raises(OtmError, match="no batch"):
            eng.shape()
        with pytest.raises(OtmError, match="no batch"):
            eng.shape_device()
        eng.match(small)
        assert _same(eng.shape(), first)
