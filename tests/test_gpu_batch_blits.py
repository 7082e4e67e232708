"""A batch's memsets and status copy, folded into kernels that run anyway
(DESIGN.md §5): K1 zeroes seg_base per trace (K7a adds each trace's segment
bound there, the scan turns it into the regions' offsets), k_order_plan zeroes
the tile counts it has read, k_status writes the host's status record itself.

What could go wrong is a stale value: a bound, a tile count or a status left by
an earlier batch or an aborted attempt.  So batches of different sizes and
trace counts run back to back on one engine, on clones at once, and through a
redone and a resumed attempt; trans_off is compared with the exclusive cumsum
of Kq x Kp rebuilt from the stage arrays, and every batch's final records with
the CPU oracle's, bit for bit.

(trans_off and seg_base are scanned by the library's scans, as before: a scan
inside k_links and k_seg_bound was measured and not kept,
profiles/launch_diet/README.md.  The trans_off cases here run unchanged
kernels; they are the shapes such a scan would have to pass, kept for a later
attempt, and are no coverage of one.)
"""
import threading

import numpy as np
import numpy.testing as npt
import pytest

from reporter_amd import Engine, synth

from test_no_limits import RADIUS_100, star, star_batch  # noqa: F401  (star: a fixture)
from test_gpu_viterbi_row import cat, take

pytestmark = pytest.mark.gpu

TILE = 256  # k_links' and k_seg_bound's block
KEYS = ("traces", "segments", "reports", "way_ids")

_cache = {}


def base(graph):
    """200 traces of 60 points; every batch below is cut from it."""
    if "base" not in _cache:
        _cache["base"] = synth.make_traces(graph, 200, 60, interval_s=5.0, noise_sigma_m=10.0, accuracy=10.0, seed=91)
    return _cache["base"]


def points_batch(graph, n_points):
    """The first n_points points of the base batch, as whole traces and one cut one."""
    full, rest = divmod(n_points, 60)
    idx = list(range(full + (1 if rest else 0)))
    return take(base(graph), idx, [None] * full + ([rest] if rest else []))


def orc_of(oracle, graph, b, key, meili=None):
    if key not in _cache:
        _cache[key] = oracle.match_batch(oracle.Graph(graph), b, p=oracle.params(**(meili or {})), keep_stages=True,
                                         nthreads=4)
    return _cache[key]


def check_trans_off(eng, b, breakage=2000.0):
    P = len(b["lat"])
    nc, cp, gc = eng.debug("ncand")[:P].astype(np.int64), eng.debug("col_prev")[:P], eng.debug("gc")[:P]
    linked = cp >= 0
    assert (gc[linked] <= breakage).all() and (nc[linked] > 0).all()
    cnt = np.where(linked, nc[np.maximum(cp, 0)] * nc, 0)
    want = np.concatenate([[0], np.cumsum(cnt)])
    npt.assert_array_equal(eng.debug("trans_off")[:P + 1], want, err_msg="trans_off")
    return int(want[-1])


@pytest.mark.parametrize("n_points", [1, TILE - 1, TILE, TILE + 1, 2 * TILE, 40 * TILE + 77])
def test_trans_off_batch_sizes(small_graph, oracle, results_equal, n_points):
    # one block whose last thread holds the total (255), the total alone in a second block (256), a second
    # block of one point (257), and ~40 blocks
    b = points_batch(small_graph, n_points)
    assert len(b["lat"]) == n_points
    orc = orc_of(oracle, small_graph, b, ("pts", n_points))
    with Engine(graph_path=small_graph) as eng:
        results_equal(orc, eng.match(b), "%d points" % n_points)
        total = check_trans_off(eng, b)
        npt.assert_array_equal(eng.debug("trans_off")[:n_points + 1], orc["trans_off"])
        assert total > 0 or n_points == 1


def test_empty_batch_and_one_point_traces(small_graph, oracle, results_equal):
    empty = dict(trace_off=np.zeros(1, np.int64), lat=np.zeros(0, np.float32), lon=np.zeros(0, np.float32),
                 time=np.zeros(0), accuracy=np.zeros(0, np.float32))
    ones = take(base(small_graph), list(range(200)), [1] * 200)  # every count is 0
    orc = orc_of(oracle, small_graph, ones, "ones")
    with Engine(graph_path=small_graph) as eng:
        r = eng.match(empty)
        assert len(r.traces) == 0 and len(r.segments) == 0
        npt.assert_array_equal(eng.debug("trans_off")[:1], [0])
        results_equal(orc, eng.match(ones), "one-point traces")
        assert check_trans_off(eng, ones) == 0
        r = eng.match(empty)  # ... and after a batch that left words behind
        assert len(r.traces) == 0
        npt.assert_array_equal(eng.debug("trans_off")[:1], [0])


def test_sizes_back_to_back(small_graph, oracle, results_equal):
    # a large batch, a small one, the large one again, a middle one: every batch finds the tile counts,
    # bounds and status of the one before
    sizes = [40 * TILE + 77, TILE + 1, 40 * TILE + 77, 2 * TILE]
    with Engine(graph_path=small_graph) as eng:
        for n in sizes:
            b = points_batch(small_graph, n)
            results_equal(orc_of(oracle, small_graph, b, ("pts", n)), eng.match(b), "%d points" % n)
            check_trans_off(eng, b)


def test_clones_in_flight(small_graph, oracle, results_equal):
    # four contexts on four streams from four threads, each with its own tile counts, bounds and
    # status record (12,000 and 18,000 points; 200 and 300 traces)
    b = base(small_graph)
    big = cat([b, take(b, list(range(100)))])
    orcs = [orc_of(oracle, small_graph, b, "orc_base"), orc_of(oracle, small_graph, big, "orc_big")]
    want = [[o[k].tobytes() for k in KEYS] for o in orcs]
    with Engine(graph_path=small_graph) as eng:
        clones = [eng.clone() for _ in range(4)]
        try:
            got = [None] * 4

            def run(i):
                out = []
                for k in range(4):
                    r = clones[i].match([b, big][(i + k) % 2])
                    out.append([getattr(r, f).tobytes() for f in KEYS] == want[(i + k) % 2])
                got[i] = out
            th = [threading.Thread(target=run, args=(i,)) for i in range(4)]
            for t in th:
                t.start()
            for t in th:
                t.join()
            assert got == [[True] * 4] * 4, got
        finally:
            for c in clones:
                c.close()


@pytest.mark.parametrize("n_traces", [1, 255, 256, 257, 3000])
def test_seg_base_trace_counts(small_graph, oracle, results_equal, n_traces):
    # K1 zeroes one bound a trace (a block a trace) and the total's element; through the final
    # records, whose regions seg_base places
    src = base(small_graph)
    idx = [k % 200 for k in range(n_traces)]
    lens = [4 + (k * 7) % 9 for k in range(n_traces)]
    b = take(src, idx, lens)
    orc = orc_of(oracle, small_graph, b, ("traces", n_traces))
    with Engine(graph_path=small_graph) as eng:
        res = eng.match(b)
        results_equal(orc, res, "%d traces" % n_traces)
        assert len(res.segments) > 0
        results_equal(orc, eng.match(b), "again")  # (K1 zeroed the scanned array)


def test_redone_and_resumed_batches(small_graph, star, oracle, results_equal, monkeypatch):  # noqa: F811
    # a resumed attempt (the candidate HBM tier's tables grow): K1 does not run again, k_seg_bound
    # runs for the first time on bounds K1 zeroed an attempt ago
    path = star[0]
    sb = star_batch()
    with Engine(graph_path=path, **RADIUS_100) as eng:
        results_equal(orc_of(oracle, path, sb, "star", RADIUS_100), eng.match(sb), "star, resumed")
        st = eng.spill_stats()
        assert st["attempts"] >= 2 and st["resumed"] >= 1
        check_trans_off(eng, sb)
    # a whole redo (the transition matrices overflow)
    monkeypatch.setenv("OTM_TRANS_CAP", "64")
    monkeypatch.setenv("OTM_POOL_CAP", str(1 << 22))
    b = points_batch(small_graph, 40 * TILE + 77)
    with Engine(graph_path=small_graph) as eng:
        results_equal(orc_of(oracle, small_graph, b, ("pts", 40 * TILE + 77)), eng.match(b), "redone")
        assert eng.spill_stats()["attempts"] == 2
        check_trans_off(eng, b)
