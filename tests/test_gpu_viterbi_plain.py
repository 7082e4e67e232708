"""The plain-step fast path of K5's row form (kernels.hip k_viterbi_row,
OTM_VIT_FORM=4) against the CPU oracle, bit for bit, with the
fast path on (OTM_VR_FAST unset) and off (OTM_VR_FAST=0: every step through
the general body).

A wave holds four consecutive traces, one per 16-lane row, and steps them
together.  A step is plain when every row is idle (past its trace's end), at
an interpolated point, or at a column with candidates that links to the
previous column; only then does the wave take the fast path, and it leaves it
again inside the step when a linked row has no state left alive.  The cases
are the smallest batches that are all plain, that leave the fast path and
return to it in every wave, that die inside a plain-looking step, that carry
interpolated points through plain chains, and that use every guarded four of
the recurrence; the all-plain and the wide ones also with the LDS window
forced small (OTM_VR_WIN), and one with the transition allocation ending
where the batch's floats end (the chunk prefetch's clamped loads).

`plain_steps` restates "step s of wave w is plain" over the oracle's stage
arrays, and every case asserts its shape with it, so a case cannot quietly
stop reaching what it is there for.
"""
import numpy as np
import pytest

import queue_ref
from test_gpu_parity import _run_both, stop_and_go
from test_gpu_viterbi_row import cat, interleave, linked_pairs, take

from reporter_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def row_form(monkeypatch):
    monkeypatch.setenv("OTM_VIT_FORM", "4")


@pytest.fixture(params=[None, "0"], ids=["fast", "general"], autouse=True)
def fast(request, monkeypatch):
    if request.param is None:
        monkeypatch.delenv("OTM_VR_FAST", raising=False)
    else:
        monkeypatch.setenv("OTM_VR_FAST", request.param)
    return request.param


def columns(orc, b):
    """Rule 1's columns from the oracle's stage arrays, which carry no flag
    for them: a trace's first point, or gc > 0."""
    off = np.asarray(b["trace_off"], np.int64)
    is_col = np.asarray(orc["gc"]) > 0
    is_col[off[:-1][np.diff(off) > 0]] = True
    return is_col


def plain_steps(orc, b):
    """Per wave (four consecutive traces), a bool per step up to the longest
    trace's end: every row idle, at an interpolated point, or at a column
    with candidates that is linked to the previous one."""
    off = np.asarray(b["trace_off"], np.int64)
    is_col, nc, cp = columns(orc, b), orc["ncand"], orc["col_prev"]
    T = len(off) - 1
    out = []
    for w0 in range(0, T, 4):
        rows = range(w0, min(w0 + 4, T))
        steps = max(int(off[t + 1] - off[t]) for t in rows)
        pl = np.ones(steps, bool)
        for s in range(steps):
            for t in rows:
                p = int(off[t]) + s
                if p < off[t + 1] and is_col[p] and not (nc[p] > 0 and cp[p] >= 0):
                    pl[s] = False
        out.append(pl)
    return out


def returns(pl):
    """Steps that are not plain and are followed by a plain one."""
    return int((~pl[:-1] & pl[1:]).sum())


# ---- the batches (built from the graph alone, so their shapes can be checked without a GPU)
def plain_batch(graph, n_traces=40, n_points=43, seed=71):
    """Low-noise traces at a 5 s interval: every point after a trace's first
    is a column with candidates linked to the one before."""
    return synth.make_traces(graph, n_traces, n_points, interval_s=5.0, noise_sigma_m=3.0, accuracy=10.0, seed=seed)


ALL_PLAIN = {
    # traces, and the lengths 4k, 4k + 1, 4k + 2, 4k + 3 (the chunk is four
    # points) in turn; a full wave, a second wave of one row, of three
    "4": ([0, 1, 2, 3], [40, 41, 42, 43]),
    "5": ([0, 1, 2, 3, 4], [41, 42, 43, 40, 42]),
    "7": ([0, 1, 2, 3, 4, 5, 6], [42, 43, 40, 41, 43, 40, 41]),
    # one wave whose rows go idle one after the other
    "ragged": ([7, 8, 9, 10], [3, 8, 21, 40]),
}


def all_plain_batch(graph, shape):
    idx, lens = ALL_PLAIN[shape]
    return take(plain_batch(graph), idx, lens)


def odd_row_batch(graph):
    """test_chain_breaks_and_empty_columns' traces with holes (empty columns)
    and with 240 s gaps, one to a wave of four beside three plain traces."""
    gaps = synth.make_traces(graph, 60, 40, interval_s=240.0, noise_sigma_m=15.0, accuracy=15.0, seed=41)
    holes = synth.make_traces(graph, 12, 30, seed=58)
    lat = holes["lat"].copy()
    off = holes["trace_off"]
    for t in range(12):
        a = int(off[t])
        lat[a + 7] += 1.0
        lat[a + 15:a + 17] += 1.0
        if t % 3 == 0:
            lat[a] += 1.0
        if t % 3 == 1:
            lat[a + 29] += 1.0
    holes["lat"] = lat
    odd = interleave(take(holes, list(range(7))), take(gaps, list(range(7))))
    plain = plain_batch(graph, 42, 36, seed=72)
    order = []
    for w in range(14):
        # the odd row in another place from wave to wave
        rows = [14 + 3 * w, 14 + 3 * w + 1, 14 + 3 * w + 2]
        rows.insert(w % 4, w)
        order += rows
    return take(cat([odd, plain]), order), dict(breakage_distance=800.0)


def two_roads(path, gap_m=30.0, n_nodes=14, step_deg=0.001):
    """Two parallel one-way roads running east, gap_m apart, that never meet.
    Returns (path, metres per degree of longitude)."""
    import handgraph
    ls = handgraph.MPD * np.cos(np.radians(40.0))
    nodes = [(40.0 + r * gap_m / handgraph.MPD, i * step_deg) for r in range(2) for i in range(n_nodes)]
    edges, segs = [], []
    for r in range(2):
        for i in range(n_nodes - 1):
            segs.append(((len(segs) + 1) << 3, None))
            edges.append(dict(**{"from": r * n_nodes + i, "to": r * n_nodes + i + 1}, way=100 + r,
                              seg=len(segs) - 1, seg_pos=0, flags=handgraph.SEG_BEGIN | handgraph.SEG_END, level=0))
    handgraph.write(path, nodes, edges, segs)
    return path, ls


def hopping_batch(path):
    """Traces that run east and hop between the two roads, each to its own
    pattern, within 1 m of the road they are on: every column has its road's
    one candidate within the 10 m radius and links to the column before, and
    no route leads from one road to the other."""
    import handgraph
    graph, ls = two_roads(path)
    rng = np.random.default_rng(73)
    lat, lon, tm, acc, off = [], [], [], [], [0]
    for t in range(8):
        x = 20.0 + 7.0 * t
        for k in range(20):
            # runs of 2 + t % 3 points on a road, shifted from trace to trace
            road = ((k + t) // (2 + t % 3)) % 2
            lat.append(40.0 + (30.0 * road + rng.uniform(-1.0, 1.0)) / handgraph.MPD)
            lon.append(x / ls)
            tm.append(5.0 * k)
            acc.append(10.0)
            x += 45.0 + rng.uniform(-3.0, 3.0)
        off.append(len(lat))
    b = dict(trace_off=np.array(off, np.int64), lat=np.array(lat, np.float32), lon=np.array(lon, np.float32),
             time=np.array(tm, np.float64), accuracy=np.array(acc, np.float32))
    return graph, b, dict(search_radius=10.0, max_search_radius=10.0)


def dead_pairs(orc):
    """Linked column pairs, both with candidates, whose block has no finite cost."""
    nc, cp, toff, trans = orc["ncand"], orc["col_prev"], orc["trans_off"], orc["trans"]
    out = []
    for p in np.nonzero((cp >= 0) & (nc > 0))[0]:
        q = int(cp[p])
        if nc[q] > 0:
            blk = trans[int(toff[p]):int(toff[p]) + int(nc[q]) * int(nc[p])]
            if len(blk) and not np.isfinite(blk).any():
                out.append(int(p))
    return np.array(out, np.int64)


def stops_batch(graph):
    b = stop_and_go(plain_batch(graph, 24, 20, seed=74), seed=75, stops_per_trace=3, max_stop=12)
    assert np.diff(b["trace_off"]).max() <= 60
    return b


def wide_batch(graph):
    """test_16_and_17_candidates' 300 m-radius traces (16 candidates at nearly
    every point) and, sharing their waves, traces whose radius follows an
    accuracy of 55 to 150 m: columns of 5 to 15 candidates."""
    wide = synth.make_traces(graph, 12, 30, interval_s=5.0, noise_sigma_m=25.0, accuracy=300.0, seed=55)
    parts = [synth.make_traces(graph, 4, 30, interval_s=5.0, noise_sigma_m=10.0, accuracy=a, seed=76 + k)
             for k, a in enumerate((55.0, 110.0, 150.0))]
    return interleave(wide, cat(parts)), dict(search_radius=20.0, max_search_radius=300.0, max_candidates=16)


def check_all_plain(orc, b):
    pl = np.concatenate(plain_steps(orc, b))
    assert pl.mean() >= 0.95, pl.mean()
    # and no other step than a trace's first: every other point is a linked column
    assert (~pl).sum() == (len(b["trace_off"]) + 2) // 4


def check_odd_rows(orc, b):
    waves = plain_steps(orc, b)
    assert len(waves) == 14
    for w, pl in enumerate(waves):
        assert returns(pl) >= 3, (w, returns(pl))
    # (the fast path runs in between: in a wave with a holes trace for most of
    # its steps, in one with a 240 s-gap trace, which breaks at most steps, for some)
    assert min(int(pl.sum()) for pl in waves) >= 5 and max(pl.mean() for pl in waves) > 0.75


def check_dead(orc, b):
    dead = dead_pairs(orc)
    assert len(dead) >= 10, len(dead)
    cs = queue_ref.chain_starts(np.asarray(b["trace_off"], np.int64), orc)
    assert (cs[dead] == 1).all() and (orc["state"][dead] >= 0).all()
    # they sit in steps that look plain: all but the traces' first points
    pl = np.concatenate(plain_steps(orc, b))
    assert (~pl).sum() == 2
    # and beside them pairs that hold
    assert ((orc["col_prev"] >= 0) & (cs == 0) & (orc["state"] >= 0)).sum() >= 10


def check_stops(orc, b):
    assert (orc["ipos"] >= 0).sum() > 50
    pl = np.concatenate(plain_steps(orc, b))
    assert pl.mean() >= 0.9
    assert (~columns(orc, b)).sum() > 50


def check_wide(orc, b):
    kq, kp = linked_pairs(orc)
    assert ((kq == 16) & (kp == 16)).sum() >= 50
    for lo, hi in ((5, 8), (9, 12), (13, 16)):
        assert ((kq >= lo) & (kq <= hi)).sum() >= 5, (lo, hi)
    assert orc["ncand"].max() == 16
    pl = np.concatenate(plain_steps(orc, b))
    assert pl.mean() >= 0.9


# ---- the cases
WIN = pytest.mark.parametrize("win", [None, "64", "0"], ids=["window", "win64", "per_step"])


@WIN
@pytest.mark.parametrize("shape", list(ALL_PLAIN))
def test_all_plain(small_graph, oracle, results_equal, monkeypatch, shape, win):
    # a row whose chunk overflows the window (win64: some, per_step: all)
    # leaves the fast path to the general body's copy of the step's block
    if win is not None:
        monkeypatch.setenv("OTM_VR_WIN", win)
    b = all_plain_batch(small_graph, shape)
    assert np.diff(b["trace_off"]).tolist() == ALL_PLAIN[shape][1]
    _, orc = _run_both(small_graph, b, oracle, results_equal, counters=False)
    check_all_plain(orc, b)
    assert (orc["state"] >= 0).all()


def test_one_odd_row_per_wave(small_graph, oracle, results_equal):
    b, meili = odd_row_batch(small_graph)
    assert len(b["trace_off"]) - 1 == 56 and np.diff(b["trace_off"]).max() <= 60
    _, orc = _run_both(small_graph, b, oracle, results_equal, counters=False, meili=meili)
    check_odd_rows(orc, b)


def test_dead_chain_in_a_plain_looking_step(tmp_path, oracle, results_equal):
    graph, b, meili = hopping_batch(str(tmp_path / "two_roads.otmg"))
    _, orc = _run_both(graph, b, oracle, results_equal, counters=False, meili=meili)
    check_dead(orc, b)


def test_interpolated_points_inside_plain_chains(small_graph, oracle, results_equal):
    b = stops_batch(small_graph)
    _, orc = _run_both(small_graph, b, oracle, results_equal, counters=False)
    check_stops(orc, b)


@WIN
def test_wide_plain_steps(small_graph, oracle, results_equal, monkeypatch, win):
    if win is not None:
        monkeypatch.setenv("OTM_VR_WIN", win)
    b, meili = wide_batch(small_graph)
    _, orc = _run_both(small_graph, b, oracle, results_equal, counters=False, meili=meili)
    check_wide(orc, b)


@pytest.mark.parametrize("spare", [0, 100, 256])
def test_window_at_the_allocations_end(small_graph, oracle, results_equal, monkeypatch, spare):
    # A chunk's window is prefetched whole, 256 floats from its first on, and
    # element by element with clamped indices where that would leave the
    # transition allocation.  Its capacity pinned to the batch's own floats
    # (+ 0: every trace's last chunks are clamped, and the window the kernel
    # prefetches behind a trace's last chunk too; + 100: some; + 256: the
    # first capacity at which no load is clamped).
    b = all_plain_batch(small_graph, "7")
    total = int(oracle.match_batch(oracle.Graph(small_graph), b, keep_stages=True, nthreads=4)["trans_off"][-1])
    assert total > 7 * 256
    monkeypatch.setenv("OTM_TRANS_CAP", str(total + spare))
    _, orc = _run_both(small_graph, b, oracle, results_equal, counters=False)
    assert int(orc["trans_off"][-1]) == total
    check_all_plain(orc, b)
