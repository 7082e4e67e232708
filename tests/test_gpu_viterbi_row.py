"""K5's row form (kernels.hip k_viterbi_row: four traces per wavefront, one
per 16-lane DPP row, OTM_VIT_FORM=4) against the CPU oracle, bit for bit,
through the comparison of tests/test_gpu_parity.py, at the smallest shapes
where it can go wrong: idle rows and a last wave that is not full, traces it
rejects (more than 128 points, a column wider than 16 candidates) beside
traces it takes in one wave, column pairs from 16 -> 1 to 1 -> 16 candidates
(the DPP broadcast reads source lanes past the target column's count), chain
breaks, empty columns, interpolated points, and chunks whose transition
blocks overflow the LDS window (OTM_VR_WIN forces the per-step path).

Every batch's shape is asserted from the oracle's stage arrays, so a case
cannot quietly stop reaching what it is there for.
"""
import numpy as np
import pytest

import specref_cases
from test_gpu_parity import _run_both, stop_and_go
from test_gpu_specref import _check

from reporter_amd import Engine, synth

pytestmark = pytest.mark.gpu

KEYS = ("lat", "lon", "time", "accuracy")


@pytest.fixture(autouse=True)
def row_form(monkeypatch):
    monkeypatch.setenv("OTM_VIT_FORM", "4")


def take(b, idx, lens=None):
    """Traces `idx` of a batch, in that order, each cut to its first lens[k]
    points (None: whole)."""
    off = b["trace_off"]
    spans = []
    for k, t in enumerate(idx):
        a, e = int(off[t]), int(off[t + 1])
        if lens is not None and lens[k] is not None:
            e = min(e, a + lens[k])
        spans.append((a, e))
    out = {f: np.concatenate([b[f][a:e] for a, e in spans]) for f in KEYS}
    out["trace_off"] = np.concatenate([[0], np.cumsum([e - a for a, e in spans])]).astype(np.int64)
    return out


def cat(parts):
    out = {f: np.concatenate([p[f] for p in parts]) for f in KEYS}
    offs, base = [np.zeros(1, np.int64)], 0
    for p in parts:
        offs.append(p["trace_off"][1:] + base)
        base += int(p["trace_off"][-1])
    out["trace_off"] = np.concatenate(offs)
    return out


def interleave(x, y):
    """Traces of x and y alternating (x0 y0 x1 y1 ...; the longer one's rest
    at the end), so every wave of four holds both kinds."""
    nx, ny = len(x["trace_off"]) - 1, len(y["trace_off"]) - 1
    both = cat([x, y])
    order = []
    for k in range(max(nx, ny)):
        if k < nx:
            order.append(k)
        if k < ny:
            order.append(nx + k)
    return take(both, order)


def trace_max_ncand(orc, b):
    nc, off = orc["ncand"], b["trace_off"]
    return np.array([nc[off[t]:off[t + 1]].max() if off[t + 1] > off[t] else 0 for t in range(len(off) - 1)])


def linked_pairs(orc):
    """(Kq, Kp) of every linked column pair."""
    cp, nc = orc["col_prev"], orc["ncand"]
    p = np.nonzero(cp >= 0)[0]
    return nc[cp[p]], nc[p]


def waves_mixed(taken):
    """Waves (four consecutive traces) that hold a taken and a rejected trace."""
    n = len(taken)
    return sum(1 for w in range(0, n, 4) if taken[w:w + 4].any() and not taken[w:w + 4].all())


@pytest.mark.parametrize("n_traces", [1, 3, 4, 5])
def test_batch_sizes(small_graph, oracle, results_equal, n_traces):
    # idle rows (1, 3), one full wave (4), a second wave with one row (5)
    b = take(synth.make_traces(small_graph, 5, 40, seed=51), list(range(n_traces)))
    res, _ = _run_both(small_graph, b, oracle, results_equal, counters=False)
    assert len(res.traces) == n_traces and len(res.segments) > 0


def test_empty_batch(small_graph):
    with Engine(graph_path=small_graph) as eng:
        r = eng.match(dict(trace_off=np.zeros(1, np.int64), lat=np.zeros(0, np.float32),
                           lon=np.zeros(0, np.float32), time=np.zeros(0), accuracy=np.zeros(0, np.float32)))
        assert len(r.traces) == 0 and len(r.segments) == 0


def test_one_and_two_point_traces(small_graph, oracle, results_equal):
    # beside whole traces in their waves, and as a last wave of their own
    base = synth.make_traces(small_graph, 10, 30, seed=52)
    b = take(base, list(range(10)), [1, None, 2, None, None, 2, 1, None, 1, 2])
    assert sorted(np.diff(b["trace_off"]).tolist())[:6] == [1, 1, 1, 2, 2, 2]
    _run_both(small_graph, b, oracle, results_equal, counters=False)


def test_128_and_129_points(small_graph, oracle, results_equal):
    # the longest trace the form takes and the shortest it hands to the wave
    # form's list, beside each other and short ones in the same waves
    long_b = synth.make_traces(small_graph, 6, 129, seed=53)
    short_b = synth.make_traces(small_graph, 5, 30, seed=54)
    b = interleave(take(long_b, list(range(6)), [128, 129, 129, 128, 128, 129]), short_b)
    n = np.diff(b["trace_off"])
    assert (n == 128).sum() == 3 and (n == 129).sum() == 3
    assert waves_mixed(n <= 128) >= 2
    _, orc = _run_both(small_graph, b, oracle, results_equal, counters=False)
    # (every point of the 128-point traces is a column or an interpolated one: no trace was cut by an error)
    assert (orc["traces"]["error_kind"] == 0).all()


@pytest.mark.parametrize("kmax", [16, 17])
def test_16_and_17_candidates(small_graph, oracle, results_equal, kmax):
    # a 300 m radius in the city finds 20 edges and more at nearly every
    # point, so max_candidates is what columns hold: exactly 16 (all of a
    # row's lanes are states; every trace is taken) or 17 (a trace with such
    # a column is rejected); narrow traces (a 20 m radius) share their waves
    wide = synth.make_traces(small_graph, 12, 30, interval_s=5.0, noise_sigma_m=25.0, accuracy=300.0, seed=55)
    narrow = synth.make_traces(small_graph, 12, 30, interval_s=5.0, noise_sigma_m=5.0, accuracy=5.0, seed=56)
    b = interleave(wide, narrow)
    _, orc = _run_both(small_graph, b, oracle, results_equal, counters=False,
                       meili=dict(search_radius=20.0, max_search_radius=300.0, max_candidates=kmax))
    nc = orc["ncand"]
    assert nc.max() == kmax and (nc == kmax).sum() > 50
    mx = trace_max_ncand(orc, b)
    if kmax == 17:
        assert waves_mixed(mx <= 16) >= 3, mx
    else:
        kq, kp = linked_pairs(orc)
        assert ((kq == 16) & (kp == 16)).sum() > 50


def ladder(path, lat0=40.0, rows=16, nodes_per_row=12, gap_m=5.0, step_deg=0.001):
    """`rows` parallel one-way roads running east, gap_m apart, joined by
    two-way rungs at every node: a probe on the southernmost or northernmost
    road sees that road's edge alone within 1 m and every road within 100 m.
    Returns (path, metres per degree of longitude)."""
    import handgraph
    ls = handgraph.MPD * np.cos(np.radians(lat0))
    nodes = [(lat0 + r * gap_m / handgraph.MPD, i * step_deg) for r in range(rows) for i in range(nodes_per_row)]
    edges, segs = [], []
    for r in range(rows):
        for i in range(nodes_per_row - 1):
            segs.append(((len(segs) + 1) << 3, None))
            edges.append(dict(**{"from": r * nodes_per_row + i, "to": r * nodes_per_row + i + 1}, way=100 + r,
                              seg=len(segs) - 1, seg_pos=0, flags=handgraph.SEG_BEGIN | handgraph.SEG_END, level=0))
    for r in range(rows - 1):
        for i in range(nodes_per_row):
            u, v = r * nodes_per_row + i, (r + 1) * nodes_per_row + i
            edges.append(dict(**{"from": u, "to": v}, way=900 + i))
            edges.append(dict(**{"from": v, "to": u}, way=900 + i))
    handgraph.write(path, nodes, edges, segs)
    return path, ls


def alternating(path):
    """Traces along the ladder's outer roads whose points alternate between a
    100 m and a 1 m search radius (the radius rule: the point's accuracy,
    between search_radius and max_search_radius), in runs of one and of two
    points: columns of 16 candidates (max_candidates) beside columns of one,
    in both orders."""
    import handgraph
    graph, ls = ladder(path)
    rng = np.random.default_rng(57)
    lat, lon, tm, acc, off = [], [], [], [], [0]
    for t in range(14):
        north = 0.0 if t % 2 == 0 else 15 * 5.0
        x = 12.0 + 3.0 * t
        for k in range(18):
            narrow = (k % 2 == 1) if t % 4 < 2 else (k % 4 >= 2)
            lat.append(40.0 + (north + rng.uniform(-0.3, 0.3)) / handgraph.MPD)
            lon.append(x / ls)
            tm.append(5.0 * k)
            acc.append(1.0 if narrow else 100.0)
            x += 45.0 + rng.uniform(-3.0, 3.0)
        off.append(len(lat))
    b = dict(trace_off=np.array(off, np.int64), lat=np.array(lat, np.float32), lon=np.array(lon, np.float32),
             time=np.array(tm, np.float64), accuracy=np.array(acc, np.float32))
    return graph, b, dict(search_radius=1.0, max_search_radius=100.0, max_candidates=16)


@pytest.mark.parametrize("win", [None, "0"], ids=["window", "per_step"])
def test_wide_and_narrow_column_pairs(tmp_path, oracle, results_equal, monkeypatch, win):
    # the disabled-source-lane hazard: Kq >> Kp and Kp >> Kq, at 16 -> 1 and
    # 1 -> 16; blocks of 16 x 16 floats beside blocks of 16 and of one
    if win is not None:
        monkeypatch.setenv("OTM_VR_WIN", win)
    graph, b, meili = alternating(str(tmp_path / "ladder.otmg"))
    res, orc = _run_both(graph, b, oracle, results_equal, counters=False, meili=meili)
    kq, kp = linked_pairs(orc)
    assert ((kq == 16) & (kp == 1)).sum() >= 20, "16 -> 1"
    assert ((kq == 1) & (kp == 16)).sum() >= 20, "1 -> 16"
    assert ((kq == 16) & (kp == 16)).sum() >= 20 and ((kq == 1) & (kp == 1)).sum() >= 20
    assert orc["ncand"].max() == 16
    # the chains hold: finite costs through the narrow columns
    assert (orc["state"] >= 0).mean() > 0.9 and len(res.segments) > 0


@pytest.mark.parametrize("win", [None, "64", "0"], ids=["window", "win64", "per_step"])
def test_wide_radius_batch(small_graph, oracle, results_equal, monkeypatch, win):
    # test_viterbi_forms' wide batch (120 m radius, 25 m noise): columns of 2
    # to 16 candidates, wide beside narrow; with a 64-float window many chunks
    # overflow it and many fit, with none every linked step copies its block
    # at the step
    if win is not None:
        monkeypatch.setenv("OTM_VR_WIN", win)
    wide = synth.make_traces(small_graph, 120, 50, interval_s=5.0, noise_sigma_m=25.0, accuracy=25.0, seed=31)
    _, orc = _run_both(small_graph, wide, oracle, results_equal, counters=False,
                       meili=dict(search_radius=120.0, max_search_radius=120.0))
    kq, kp = linked_pairs(orc)
    print("Kq >= 2 Kp: %d, Kp >= 2 Kq: %d, widest %d" % ((kq >= 2 * kp).sum(), (kp >= 2 * kq).sum(), orc["ncand"].max()))
    assert (kq >= 2 * kp).sum() >= 5 and (kp >= 2 * kq).sum() >= 5
    assert orc["ncand"].max() >= 15 and (kq > 8).sum() > 100 and (kq <= 4).sum() > 20
    # chunks of four columns under and over 64 floats
    blocks = kq.astype(np.int64) * kp
    assert (blocks > 64).sum() > 100 and (blocks <= 12).sum() > 100


def test_chain_breaks_and_empty_columns(small_graph, oracle, results_equal):
    # 240 s gaps past an 800 m breakage distance (test_viterbi_forms' batch),
    # and traces with off-graph points (columns without a candidate) inside
    gaps = synth.make_traces(small_graph, 60, 40, interval_s=240.0, noise_sigma_m=15.0, accuracy=15.0, seed=41)
    holes = synth.make_traces(small_graph, 12, 30, seed=58)
    lat = holes["lat"].copy()
    off = holes["trace_off"]
    for t in range(12):
        a = int(off[t])
        lat[a + 7] += 1.0           # one empty column inside a chain
        lat[a + 15:a + 17] += 1.0   # two in a row
        if t % 3 == 0:
            lat[a] += 1.0           # the first point
        if t % 3 == 1:
            lat[a + 29] += 1.0      # the last
    holes["lat"] = lat
    b = interleave(gaps, holes)
    _, orc = _run_both(small_graph, b, oracle, results_equal, counters=False, meili=dict(breakage_distance=800.0))
    nc, cp = orc["ncand"], orc["col_prev"]
    assert (nc == 0).sum() >= 12 * 3
    # chain breaks between two columns that both have candidates
    state = orc["state"]
    assert ((cp < 0) & (nc > 0) & (state >= 0)).sum() > len(b["trace_off"]) - 1


def test_stationary_duplicates(small_graph, oracle, results_equal):
    # interpolated points (no column) between columns, at stops of 2 to 20 samples
    b = stop_and_go(synth.make_traces(small_graph, 40, 30, interval_s=5.0, noise_sigma_m=15.0, accuracy=15.0,
                                      seed=59), seed=60)
    b = take(b, [t for t in range(40) if b["trace_off"][t + 1] - b["trace_off"][t] <= 128])
    assert len(b["trace_off"]) - 1 >= 30
    _, orc = _run_both(small_graph, b, oracle, results_equal, counters=False)
    assert (orc["ipos"] >= 0).sum() > 100


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return specref_cases.build(tmp_path_factory.mktemp("specref_row"), synth)


@pytest.mark.parametrize("name", ["radius_120", "long_140", "gaps_240s"])
def test_against_spec(cases, name):
    # the float64 reference of the written spec, no oracle in the loop
    # (tests/test_gpu_specref.py test_viterbi_forms' cases and comparison)
    _check(cases, name)
