"""The spatial work order as the engine built it: a counting
sort of the batch's columns by the Hilbert index of their tile, cut into 8
groups.

k_columns counts the tiles and k_order_scatter hands out the slots with
wave-aggregated atomics whose lanes are matched by tile in registers first.
Every case compares all stage arrays and the final records with the CPU oracle
bit for bit (through test_gpu_graph_words' _batch / _oracle / _check), and
checks the order itself as fetched after each batch: `item` is a permutation
of the columns, the tiles are non-decreasing along it, `grp` is monotone, cuts
the run at tile boundaries and ends at the column count.  The shapes are the
smallest at which the sort can go wrong; OTM_SMALL_POINTS=0 makes the large
plan run at these sizes.
"""
import math
import struct

import numpy as np
import pytest

import handgraph
import test_gpu_graph_words as gw
from reporter_amd import Engine, synth
from test_gpu_graph_words import _batch, _check, _oracle

pytestmark = pytest.mark.gpu

MPD = handgraph.MPD
GROUPS = 8
EMPTY = dict(trace_off=np.zeros(1, np.int64), lat=np.zeros(0, np.float32), lon=np.zeros(0, np.float32),
             time=np.zeros(0), accuracy=np.zeros(0, np.float32))


def check_order(eng, batch):
    """The fetched order of the engine's last batch; returns (item, tile per
    point, is_col)."""
    P = len(batch["lat"])
    is_col = eng.debug("is_col")[:P].astype(bool)
    item = eng.debug("order_item")
    key = eng.debug("order_tile")[:P].astype(np.int64)
    grp = eng.debug("order_grp")
    cols = np.nonzero(is_col)[0]
    assert np.array_equal(np.sort(item), cols), "item is not a permutation of the columns"
    k = key[item]
    assert (np.diff(k) >= 0).all(), "tiles decrease along the order"
    assert len(grp) == GROUPS + 1 and grp[0] == 0 and grp[-1] == len(cols) and (np.diff(grp) >= 0).all()
    for c in grp[1:-1]:
        assert c == 0 or c == len(cols) or k[c - 1] != k[c], "a group cut inside a tile's run"
    return item, key, is_col


class OrderEngine(Engine):
    """Engine that checks the fetched order after every batch (takes Engine's
    place in _check) and keeps the last one."""
    last = None

    def match(self, batch):
        res = super().match(batch)
        OrderEngine.last = check_order(self, batch)
        return res


@pytest.fixture(autouse=True)
def large_plan(monkeypatch):
    monkeypatch.setenv("OTM_SMALL_POINTS", "0")
    monkeypatch.setattr(gw, "Engine", OrderEngine)
    OrderEngine.last = None


def header(graph):
    """rows, cols, grid lat0, lon0, cell_deg, node bbox of an .otmg file."""
    with open(graph, "rb") as f:
        h = struct.unpack(handgraph._HDR, f.read(struct.calcsize(handgraph._HDR)))
    return dict(rows=h[7], cols=h[8], lat0=h[10], lon0=h[11], cell=h[12], bbox=h[13:17])


def singles(lat, lon, acc=5.0):
    """One single-point trace per position."""
    n = len(lat)
    return dict(trace_off=np.arange(n + 1, dtype=np.int64), lat=np.asarray(lat, np.float32),
                lon=np.asarray(lon, np.float32), time=np.zeros(n), accuracy=np.full(n, acc, np.float32))


def concat(parts):
    off = [np.zeros(1, np.int64)]
    base = 0
    for p in parts:
        off.append(np.asarray(p["trace_off"][1:], np.int64) + base)
        base += len(p["lat"])
    out = {k: np.concatenate([np.asarray(p[k]) for p in parts]) for k in ("lat", "lon", "time", "accuracy")}
    out["trace_off"] = np.concatenate(off)
    return out


def tile_centre(h, tx, ty):
    b = h["bbox"]
    return b[0] + (ty + 0.5) / 64.0 * (b[2] - b[0]), b[1] + (tx + 0.5) / 64.0 * (b[3] - b[1])


def test_one_bucket_several_waves(small_graph, oracle, results_equal):
    # 300 probes within 2 m of the centre of one tile (78 m): one bucket, so
    # five waves and both scatter blocks add to one cursor
    h = header(small_graph)
    spot = tile_centre(h, 31, 33)
    rng = np.random.default_rng(5)
    ls = MPD * math.cos(math.radians(spot[0]))
    b = singles(spot[0] + rng.uniform(-2, 2, 300) / MPD, spot[1] + rng.uniform(-2, 2, 300) / ls)
    orc = _oracle(oracle, small_graph, b, {})
    _check(small_graph, b, orc, results_equal)
    item, key, is_col = OrderEngine.last
    assert is_col.all() and len(np.unique(key)) == 1


def test_one_column_per_bucket(small_graph, oracle, results_equal):
    # 200 probes at the centres of tiles four apart: a bucket each
    h = header(small_graph)
    pos = [tile_centre(h, 2 + 4 * i, 2 + 4 * j) for j in range(16) for i in range(16)][:200]
    b = singles([p[0] for p in pos], [p[1] for p in pos])
    orc = _oracle(oracle, small_graph, b, {})
    _check(small_graph, b, orc, results_equal)
    item, key, is_col = OrderEngine.last
    assert len(np.unique(key)) == 200
    # five columns: at least three of the eight groups are empty
    b5 = singles([p[0] for p in pos[:5]], [p[1] for p in pos[:5]])
    _check(small_graph, b5, _oracle(oracle, small_graph, b5, {}), results_equal)
    with OrderEngine(graph_path=small_graph) as eng:
        eng.match(b5)
        assert (np.diff(eng.debug("order_grp")) == 0).sum() >= 3
    # an empty batch on an engine of its own
    with OrderEngine(graph_path=small_graph) as eng:
        r = eng.match(EMPTY)
        assert len(r.traces) == 0 and len(eng.debug("order_item")) == 0


def test_outside_the_bbox(tmp_path, oracle, results_equal):
    # a star of 60 spokes; probes 300 m out on every side lie outside the node
    # bbox (tile row / column clamped to 0 and 63) and outside the cell grid,
    # beside probes at the hub and in the grid's empty corners
    lat0 = 40.0
    ls = MPD * math.cos(math.radians(lat0))
    path, _, _ = handgraph.star(str(tmp_path / "star.otmg"), lat=lat0, n_spokes=60)
    hub = [[(0.0, 0.0, 0.0), (40.0, 0.0, 5.0), (3.0, 20.0, 10.0), (0.0, -45.0, 15.0)], [(1.0, 1.0, 0.0)]]
    corners = [[(s * d, t * d, 0.0)] for d in (120.0, 150.0) for s in (-1, 1) for t in (-1, 1)]
    outside = [[(300.0, 0.0, 0.0)], [(-300.0, 0.0, 0.0)], [(0.0, 300.0, 0.0)], [(0.0, -300.0, 0.0)],
               [(300.0, 300.0, 0.0)], [(-300.0, -300.0, 0.0)]]
    b = _batch(hub + corners + outside, lat0, ls)
    orc = _oracle(oracle, path, b, gw.R50)
    _check(path, b, orc, results_equal, meili=gw.R50)
    item, key, is_col = OrderEngine.last
    assert is_col.all()
    n_in = sum(len(t) for t in hub) + len(corners)
    assert len(np.unique(key[n_in:])) == len(outside)  # the clamped corner and edge tiles, all different


def test_long_trace(small_graph, oracle, results_equal):
    # 300 points, above COL_PTS = 256: k_columns' serial path counts the
    # tiles, beside ordinary traces that cross the same tiles
    long = synth.make_traces(small_graph, 1, 300, interval_s=5.0, noise_sigma_m=15.0, accuracy=15.0, seed=71)
    rest = synth.make_traces(small_graph, 40, 60, interval_s=5.0, noise_sigma_m=15.0, accuracy=15.0, seed=72)
    b = concat([rest, long, rest])
    assert b["trace_off"][41] - b["trace_off"][40] == 300
    orc = _oracle(oracle, small_graph, b, {})
    _check(small_graph, b, orc, results_equal)
    item, key, is_col = OrderEngine.last
    a, e = b["trace_off"][40], b["trace_off"][41]
    lt = np.unique(key[a:e][is_col[a:e]])
    other = np.unique(np.concatenate([key[:a][is_col[:a]], key[e:][is_col[e:]]]))
    assert len(np.intersect1d(lt, other)) > 0


@pytest.mark.parametrize("mult", [1, None], ids=["g1", "auto"])
def test_city_batch(small_graph, oracle, results_equal, mult):
    # (the batch and oracle result test_gpu_cand_scan.py uses): waves of 60-point
    # traces that cross several tiles each, 36 scatter blocks
    bt = synth.make_traces(small_graph, 150, 60, interval_s=5.0, noise_sigma_m=15.0, accuracy=15.0, seed=61)
    orc = _oracle(oracle, small_graph, bt, {}, key=("scan_city",))
    _check(small_graph, bt, orc, results_equal, grid_mult=mult)
    item, key, is_col = OrderEngine.last
    off = bt["trace_off"]
    assert max(len(np.unique(key[off[t]:off[t + 1]])) for t in range(150)) >= 8  # many keys in one wave


def test_batch_redone(small_graph, oracle, results_equal, monkeypatch):
    # the transition matrices overflow: the whole batch runs twice, the tile
    # counts zeroed and rebuilt
    monkeypatch.setenv("OTM_TRANS_CAP", "64")
    monkeypatch.setenv("OTM_POOL_CAP", str(1 << 22))
    bt = synth.make_traces(small_graph, 150, 60, interval_s=5.0, noise_sigma_m=15.0, accuracy=15.0, seed=61)
    orc = _oracle(oracle, small_graph, bt, {}, key=("scan_city",))
    with OrderEngine(graph_path=small_graph) as eng:
        res = eng.match(bt)
        assert eng.spill_stats()["attempts"] == 2
        gw._stage_compare(eng, orc, bt)
        results_equal(orc, res, "redone")
