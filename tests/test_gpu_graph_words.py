"""The lane candidate tier's kept offsets and the per-edge source records of
the route index, against the CPU oracle, bit for bit.

k_cand_lane projects each kept entry once, in its node-snap pass, and carries
the offset through the node merge (which moves the last entry into a freed
slot) and the selection sort (which swaps entries) to the output loop;
k_trans_sub and k_route_index read a source's row descriptor and its edge's
length out of one per-edge record (both rows an edge can stand for: its own,
and its from node's for a node candidate).  Every stage array and the final
records are compared exactly, with the work counters on and off (the two
instances of the lane kernel), on the smallest shapes that reach that code.
"""
import math

import numpy as np
import pytest

import handgraph
from reporter_amd import Engine, synth
from test_gpu_parity import _stage_compare

pytestmark = pytest.mark.gpu

MPD = 20037581.187 / 180.0
R50 = dict(search_radius=50.0, max_search_radius=50.0)


@pytest.fixture(params=["large", "small"])
def batch_path(request, monkeypatch):
    """Both launch plans (test_gpu_parity.py batch_path): "large" = spatial
    order and the lane tier, "small" = every probe on the wave tier."""
    monkeypatch.setenv("OTM_SMALL_POINTS", "0" if request.param == "large" else str(1 << 40))
    return request.param


_ORACLE = {}


def _oracle(oracle, graph, batch, meili, key=None):
    """The oracle's stages for (graph, batch, meili): computed once per key
    and shared, never changed (the engine's index and launch parameters do
    not enter it)."""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    orc = oracle.match_batch(oracle.Graph(graph), batch, p=oracle.params(**meili), keep_stages=True, nthreads=4)
    if key is not None:
        _ORACLE[key] = orc
    return orc


def _check(graph, batch, orc, results_equal, meili=None, **eng_kw):
    """test_gpu_parity._run_both with the oracle's result given: every stage,
    the final records and the counters, then the stages and records again with
    counting off (k_cand_lane<false>, the instance the benchmark runs)."""
    with Engine(graph_path=graph, **eng_kw, **(meili or {})) as eng:
        spill = None
        for counters in (True, False):
            eng.set_counting(counters)
            res = eng.match(batch)
            _stage_compare(eng, orc, batch)
            results_equal(orc, res, "final (counters %s)" % counters)
            if counters:
                c = eng.counters()
                same_grid = eng.grid_info()["mult"] == 1
                for k, v in orc["counters"].items():
                    if (k in ("cells_visited", "cell_entries_scanned") and not same_grid) or k not in c:
                        continue
                    assert c[k] == v, "counter %s gpu %d oracle %d" % (k, c[k], v)
            spill = eng.spill_stats()
        return res, spill


def _batch(traces, lat0, ls, acc=5.0):
    """traces: lists of (north m, east m, t) about (lat0, lon 0)."""
    lat = np.concatenate([np.array([lat0 + p[0] / MPD for p in t], np.float32) for t in traces])
    lon = np.concatenate([np.array([p[1] / ls for p in t], np.float32) for t in traces])
    tm = np.concatenate([np.array([p[2] for p in t], np.float64) for t in traces])
    off = np.concatenate([[0], np.cumsum([len(t) for t in traces])]).astype(np.int64)
    return dict(trace_off=off, lat=lat, lon=lon, time=tm, accuracy=np.full(len(lat), acc, np.float32))


# 7, 8 and 9 spokes, and -- a spoke being two directed edges -- 3, 4 and 5:
# 6, 8 and 10 distinct edges within the radius of a probe at the hub, under, at
# and over the lane list's 8-edge cap
@pytest.mark.parametrize("maxc", [None, 3], ids=["kdefault", "k3"])
@pytest.mark.parametrize("spokes", [3, 4, 5, 7, 8, 9])
def test_star_hub_and_spoke(tmp_path, oracle, results_equal, batch_path, spokes, maxc):
    # probes at the hub: every entry snaps to the one node, so the merge
    # repeats, each time moving the last entry (and its offset) into the freed
    # slot; probes 40 m out along a spoke: that spoke's two edges project at
    # offsets > 0 among the node candidates of the others, whose nearest point
    # is the hub; with max_candidates 3 the sort drops projected entries
    lat0 = 40.0
    ls = MPD * math.cos(math.radians(lat0))
    path, _, _ = handgraph.star(str(tmp_path / "star.otmg"), lat=lat0, n_spokes=spokes)
    traces = []
    for k in range(spokes):
        a, b = 2.0 * math.pi * k / spokes, 2.0 * math.pi * ((k + 1) % spokes) / spokes
        out = lambda d, ang, side=0.0: (d * math.cos(ang) - side * math.sin(ang), d * math.sin(ang) + side * math.cos(ang))
        pts = [(0.0, 0.0), out(40.0, a), (3.0, 0.0), out(40.0, a, 5.0), (0.0, 0.0), out(60.0, b), out(40.0, b, -3.0),
               (0.0, -2.0)]
        traces.append([(n, e, 5.0 * i) for i, (n, e) in enumerate(pts)])
    b = _batch(traces, lat0, ls)
    meili = dict(R50)
    if maxc:
        meili["max_candidates"] = maxc
    orc = _oracle(oracle, path, b, meili)
    res, spill = _check(path, b, orc, results_equal, meili=meili)
    P = len(b["lat"])
    k = orc["ncand"]
    off = orc["cand_off"].reshape(P, -1)
    valid = np.arange(off.shape[1])[None, :] < k[:, None]
    assert ((off > 0.0) & valid).any() and ((off == 0.0) & valid).any()  # edge and node candidates
    assert k.min() >= 1 and (not maxc or k.max() == maxc)
    if batch_path == "large":
        # the lane tier keeps a probe of up to 8 distinct edges; more spill
        assert (spill["cand_wave"] == 0) == (2 * spokes <= 8)


@pytest.mark.parametrize("two_way", [True, False], ids=["two_way", "one_way"])
def test_road_ends(tmp_path, oracle, results_equal, batch_path, two_way):
    # probes past the last node project onto the last edge's end: at_end, the
    # offset clamped to the edge's length (an edge candidate on the one-way
    # road, whose end node has no outgoing edge; that node's candidate on the
    # two-way one); probes before the first node project at offset 0
    lat0 = 40.0
    ls = MPD * math.cos(math.radians(lat0))
    path, _ = handgraph.straight_road(str(tmp_path / "road.otmg"), lat=lat0, n_nodes=5, two_way=two_way)
    end = 0.004 * ls  # the last node, metres east
    traces = [[(8.0, end - 120.0, 0.0), (6.0, end - 40.0, 5.0), (5.0, end + 15.0, 10.0), (-4.0, end + 30.0, 15.0)],
              [(3.0, -25.0, 0.0), (-6.0, -12.0, 5.0), (4.0, 30.0, 10.0), (5.0, 110.0, 15.0)],
              [(0.0, end + 20.0, 0.0), (0.0, end + 35.0, 5.0)]]
    b = _batch(traces, lat0, ls)
    orc = _oracle(oracle, path, b, R50)
    _check(path, b, orc, results_equal, meili=R50)
    P = len(b["lat"])
    off = orc["cand_off"].reshape(P, -1)
    assert orc["ncand"][2] >= 1 and orc["ncand"][3] >= 1
    if not two_way:
        # past the end: the last edge at its full length (~85 m)
        assert off[3, :orc["ncand"][3]].max() > 80.0


@pytest.mark.parametrize("maxc", [None, 3], ids=["kdefault", "k3"])
def test_city_traces(small_graph, oracle, results_equal, batch_path, maxc):
    b = synth.make_traces(small_graph, 150, 60, interval_s=5.0, noise_sigma_m=15.0, accuracy=15.0, seed=61)
    meili = dict(max_candidates=maxc) if maxc else {}
    orc = _oracle(oracle, small_graph, b, meili, key=("city", maxc))
    _check(small_graph, b, orc, results_equal, meili=meili)
    if maxc:
        assert orc["ncand"].max() == maxc


@pytest.mark.parametrize("lanes", [8, 16])
@pytest.mark.parametrize("radius", [None, 300.0, 0.0], ids=["index_default", "index300", "no_index"])
@pytest.mark.parametrize("near", [[], [300.0], [150.0, 300.0, 600.0]], ids=["near0", "near1", "near3"])
def test_source_records(small_graph, oracle, results_equal, near, radius, lanes):
    # 15 s sampling spreads the bounds (5 x gc) over the near levels and past a
    # 300 m index (those columns take the search tiers); radius 0 has no
    # records at all
    b = synth.make_traces(small_graph, 200, 60, interval_s=15.0, noise_sigma_m=15.0, accuracy=15.0, seed=63)
    orc = _oracle(oracle, small_graph, b, {}, key="records")
    # both halves of a record are read: node and edge candidates among the sources
    P = len(b["lat"])
    linked = np.nonzero(orc["col_prev"] >= 0)[0]
    q = orc["col_prev"][linked]
    off = orc["cand_off"].reshape(P, -1)[q]
    valid = np.arange(off.shape[1])[None, :] < orc["ncand"][q][:, None]
    assert ((off == 0.0) & valid).sum() > 100 and ((off > 0.0) & valid).sum() > 100
    res, spill = _check(small_graph, b, orc, results_equal, index_radius_m=radius, index_near_m=near,
                        trans_lanes=lanes)
    if radius is not None:
        assert spill["trans_online"] > 0  # columns the index (or none) cannot answer
