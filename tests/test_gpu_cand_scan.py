"""k_cand_lane's two-phase scan against the CPU oracle, bit
for bit.

The lane tier takes a grid row's entries in chunks of OTM_CAND_CHUNK (1..64,
default 64): it first scans a chunk, setting one bit of a per-lane mask per
entry within the radius, and then drains the mask in ascending order through
the unchanged insert body.  The order of inserts is the order of the entries,
so every stage array, the final records, the work counters and the spill
decision must be what the oracle gives, wherever the chunk boundaries fall.
Small chunk widths put them everywhere: between two hits on one edge, before
and after a hit, inside the drain in which a lane spills.  Only the large
launch plan runs this kernel.
"""
import math

import numpy as np
import pytest

import handgraph
from reporter_amd import synth
from test_gpu_graph_words import MPD, R50, _batch, _check, _oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def large_plan(monkeypatch):
    monkeypatch.setenv("OTM_SMALL_POINTS", "0")


def _chunk(monkeypatch, chunk):
    monkeypatch.setenv("OTM_CAND_CHUNK", str(chunk))


@pytest.mark.parametrize("chunk", [1, 2, 3, 64])
@pytest.mark.parametrize("spokes", [3, 4, 5])
def test_star_mixed_wave(tmp_path, oracle, results_equal, monkeypatch, spokes, chunk):
    # one batch of under 64 columns: probes at the hub (2 x spokes distinct
    # edges in range, every one a hit), probes 40 to 60 m out along a spoke, and
    # probes with no edge in range, so that the lanes of one wave drain masks
    # of very different sizes; with 5 spokes the hub probes spill inside a
    # drain while the other lanes go on
    _chunk(monkeypatch, chunk)
    lat0 = 40.0
    ls = MPD * math.cos(math.radians(lat0))
    path, _, _ = handgraph.star(str(tmp_path / "star.otmg"), lat=lat0, n_spokes=spokes)
    out = lambda d, ang, side=0.0: (d * math.cos(ang) - side * math.sin(ang), d * math.sin(ang) + side * math.cos(ang))
    traces = []
    for k in range(spokes):
        a, b = 2.0 * math.pi * k / spokes, 2.0 * math.pi * ((k + 1) % spokes) / spokes
        pts = [(0.0, 0.0), out(40.0, a), (3.0, 0.0), out(55.0, a, 5.0), (0.0, 0.0), out(60.0, b), out(40.0, b, -3.0),
               (0.0, -2.0)]
        traces.append([(n, e, 5.0 * i) for i, (n, e) in enumerate(pts)])
    # no edge within 50 m of (400, 400) or (-500, 300): columns without candidates between matched ones
    far = [(0.0, 0.0), (400.0, 400.0), out(45.0, 0.0), (-500.0, 300.0), (2.0, 1.0), out(50.0, 2.0 * math.pi / spokes)]
    traces.append([(n, e, 5.0 * i) for i, (n, e) in enumerate(far)])
    bt = _batch(traces, lat0, ls)
    P = len(bt["lat"])
    assert P < 64
    orc = _oracle(oracle, path, bt, R50, key=("scan_star", spokes))
    k = orc["ncand"]
    # the two probes without an edge, hub probes (every hit merged into the hub's one node) and spoke probes
    assert (k == 0).sum() == 2 and (k == 1).any() and k.max() >= 3
    res, spill = _check(path, bt, orc, results_equal, meili=R50)
    assert (spill["cand_wave"] == 0) == (2 * spokes <= 8)


@pytest.mark.parametrize("chunk", [2, 5, 64])
@pytest.mark.parametrize("mult", [1, 2, 4, 8])
def test_city_traces_by_grid(small_graph, oracle, results_equal, monkeypatch, mult, chunk):
    # coarser cells: row ranges longer than 64 entries (several chunks at any
    # width), odd row lengths, rows without a hit; with grid_mult 1 _check also
    # compares cells_visited and cell_entries_scanned with the oracle's
    _chunk(monkeypatch, chunk)
    bt = synth.make_traces(small_graph, 150, 60, interval_s=5.0, noise_sigma_m=15.0, accuracy=15.0, seed=61)
    orc = _oracle(oracle, small_graph, bt, {}, key=("scan_city",))
    _check(small_graph, bt, orc, results_equal, grid_mult=mult)


@pytest.mark.parametrize("chunk", [1, 64])
@pytest.mark.parametrize("two_way", [True, False], ids=["two_way", "one_way"])
def test_road_ends(tmp_path, oracle, results_equal, monkeypatch, two_way, chunk):
    # probes before the first and past the last node of a straight road: cells
    # that hold a single entry, and a hit at bit 0 and at the last bit of a
    # chunk (the road's first and last edge end their rows)
    _chunk(monkeypatch, chunk)
    lat0 = 40.0
    ls = MPD * math.cos(math.radians(lat0))
    path, _ = handgraph.straight_road(str(tmp_path / "road.otmg"), lat=lat0, n_nodes=5, two_way=two_way)
    end = 0.004 * ls  # the last node, metres east
    traces = [[(8.0, end - 120.0, 0.0), (6.0, end - 40.0, 5.0), (5.0, end + 15.0, 10.0), (-4.0, end + 30.0, 15.0)],
              [(3.0, -25.0, 0.0), (-6.0, -12.0, 5.0), (4.0, 30.0, 10.0), (5.0, 110.0, 15.0)],
              [(0.0, end + 20.0, 0.0), (0.0, end + 35.0, 5.0)],
              [(0.0, -40.0, 0.0), (0.0, -20.0, 5.0)]]
    bt = _batch(traces, lat0, ls)
    orc = _oracle(oracle, path, bt, R50, key=("scan_road", two_way))
    assert orc["ncand"].min() >= 1
    res, spill = _check(path, bt, orc, results_equal, meili=R50)
    assert spill["cand_wave"] == 0
