"""Tiers on demand (kernels.h TierGroup): a batch context stops
launching a group of kernels whose device list stayed empty TIER_QUIET = 2
completed batches in a row; a batch that then pushes onto such a list aborts,
the host makes the group live for good and runs the batch again.

Every result is compared with the CPU oracle bit for bit.  The groups, the
launches each one saves, and the batch that needs it:

  cand_big      1  the 200-spoke star of test_no_limits.py (400 edges in a radius)
  trans_online  3  120 s sampling (bounds past the route index), with ...
  route_online  3  ... the route tiers, which a woken transition group takes along
  vit_lists     1  under OTM_VIT_FORM=4: a column of 17 candidates, a trace of 129 points
  seg_large     1  a trace of 129 points (the small segment plan holds 128)
"""
import threading

import numpy as np
import pytest

from reporter_amd import Engine, synth

from test_no_limits import RADIUS_100, _star_point, star, star_batch  # noqa: F401  (star: a fixture)
from test_gpu_viterbi_row import interleave, take

pytestmark = pytest.mark.gpu

QUIET = 2
ALL = {"cand_big", "trans_online", "route_online", "vit_lists", "seg_large"}
KEYS = ("traces", "segments", "reports", "way_ids")


@pytest.fixture(params=["large", "small"])
def batch_path(request, monkeypatch):
    monkeypatch.setenv("OTM_SMALL_POINTS", "0" if request.param == "large" else str(1 << 40))
    return request.param


@pytest.fixture
def roomy(monkeypatch):
    """Transition matrices and a path pool that hold any batch here (120 s gaps make long routes: the pool sized
    from the batch overflows and the batch is redone for that, on a fresh engine too)."""
    monkeypatch.setenv("OTM_TRANS_CAP", str(1 << 24))
    monkeypatch.setenv("OTM_POOL_CAP", str(1 << 22))


_orc = {}


def orc_of(oracle, graph, b, key, meili=None):
    """The oracle's result of a batch, computed once a session."""
    if key not in _orc:
        _orc[key] = oracle.match_batch(oracle.Graph(graph), b, p=oracle.params(**(meili or {})), nthreads=4)
    return _orc[key]


def quiet_batch(graph, seed=81):
    return synth.make_traces(graph, 40, 50, interval_s=5.0, noise_sigma_m=5.0, accuracy=5.0, seed=seed)


def long_batch(graph):
    """Traces of 128 and 129 points among short ones: the 129-point ones are past the small segment plan
    (and past Viterbi's row form)."""
    long_b = synth.make_traces(graph, 6, 129, seed=53)
    short_b = synth.make_traces(graph, 5, 30, seed=54)
    return interleave(take(long_b, list(range(6)), [128, 129, 129, 128, 128, 129]), short_b)


def settle(eng, b, orc, results_equal, want=ALL):
    """QUIET quiet batches: equal, one attempt each, then `want` dormant."""
    for k in range(QUIET):
        assert not (eng.tiers()["dormant"] & want), "dormant before batch %d" % k
        results_equal(orc, eng.match(b), "quiet batch %d" % k)
        st = eng.spill_stats()
        assert st["attempts"] == 1
        assert all(st[g] == 0 for g in ("cand_big", "trans_online", "route_online") if g in want)
    assert eng.tiers()["dormant"] >= want


# groups that wake in one extra attempt: the online route tiers wake with the transition tiers
UNITS = [{"cand_big"}, {"trans_online", "route_online"}, {"vit_lists"}, {"seg_large"}]


def woken(eng, b, orc, results_equal, groups):
    """A batch that needs exactly the dormant `groups`: equal, those groups
    and no others live afterwards, one extra attempt for each unit of them
    (attempts == 2 for one unit); the same batch again in one run."""
    before = eng.tiers()["dormant"]
    assert groups <= before
    results_equal(orc, eng.match(b), "the batch that wakes %s" % sorted(groups))
    woke = before - eng.tiers()["dormant"]
    print("woke", sorted(woke), "attempts", eng.spill_stats()["attempts"])
    assert woke == groups, woke
    assert eng.spill_stats()["attempts"] == 1 + sum(1 for u in UNITS if u & groups)
    results_equal(orc, eng.match(b), "the same batch again")
    assert eng.spill_stats()["attempts"] == 1
    assert not (eng.tiers()["dormant"] & groups)


def test_quiet_batches(small_graph, oracle, results_equal, batch_path):
    b1, b2 = quiet_batch(small_graph, 81), quiet_batch(small_graph, 82)
    o1, o2 = orc_of(oracle, small_graph, b1, "q81"), orc_of(oracle, small_graph, b2, "q82")
    disp = []
    with Engine(graph_path=small_graph) as eng:
        for k, (b, o) in enumerate([(b1, o1), (b2, o2), (b1, o1), (b2, o2)]):
            results_equal(o, eng.match(b), "batch %d" % k)
            assert eng.spill_stats()["attempts"] == 1
            t = eng.tiers()
            assert t["dormant"] == (set() if k + 1 < QUIET else ALL), (k, t)
            disp.append(t["dispatches"])
    # batches 0 .. QUIET-1 were launched in full (the mask changes after a batch), the others
    # without k_candidates<true>, k_transitions<0..2>, k_route<0..2> and the large k_segments plan
    # (small batches run the wave form of Viterbi: it has no list pass)
    assert disp[0] == disp[1] and disp[2] == disp[3] == disp[0] - 8, disp


def test_wake_online_tiers(small_graph, oracle, results_equal, batch_path, roomy):
    q = quiet_batch(small_graph)
    gaps = synth.make_traces(small_graph, 60, 30, interval_s=120.0, noise_sigma_m=10.0, accuracy=10.0, seed=9)
    og = orc_of(oracle, small_graph, gaps, "gaps120")
    long_b = long_batch(small_graph)
    with Engine(graph_path=small_graph) as eng:
        settle(eng, q, orc_of(oracle, small_graph, q, "q81"), results_equal)
        # steps that long make routes of more traversals than the small segment plan holds, so the large
        # plan is woken first, by a batch that needs nothing else: the gaps then wake one unit, in one
        # extra attempt
        woken(eng, long_b, orc_of(oracle, small_graph, long_b, "p129"), results_equal, {"seg_large"})
        woken(eng, gaps, og, results_equal, {"trans_online", "route_online"})
        st = eng.spill_stats()
        assert st["trans_online"] > 0 and st["route_online"] > 0
        # the groups nothing needed are dormant still, the woken ones stay live through quiet batches
        for _ in range(QUIET + 1):
            eng.match(q)
        assert eng.tiers()["dormant"] == {"cand_big", "vit_lists"}


def star_quiet_batch():
    """Probes 150 m from the hub, 60 m past their spoke's tip: some 90 edges in the 100 m radius."""
    lat, lon, off = [], [], [0]
    for i in (0, 50, 100, 150):
        for d in (140.0, 150.0, 160.0):
            la, lo = _star_point(i, d)
            lat.append(la)
            lon.append(lo)
        off.append(len(lat))
    n = len(lat)
    return dict(trace_off=np.array(off, np.int64), lat=np.array(lat, np.float32), lon=np.array(lon, np.float32),
                time=np.arange(n) * 6.0 + 100.0, accuracy=np.full(n, 5.0, np.float32))


def test_wake_cand_big(star, oracle, results_equal, batch_path, roomy):  # noqa: F811
    path = star[0]
    q, b = star_quiet_batch(), star_batch()
    with Engine(graph_path=path, **RADIUS_100) as eng:
        settle(eng, q, orc_of(oracle, path, q, "starq", RADIUS_100), results_equal, want={"cand_big"})
        # one step of the star's routes is past the index too (test_no_limits.py STAR_SPILLS: route_online
        # 1), and the quiet batch left the online route tiers dormant (its transitions use the online
        # tiers, its routes do not): two units, two extra attempts, the candidate tier's a resumed one
        woken(eng, b, orc_of(oracle, path, b, "star", RADIUS_100), results_equal, {"cand_big", "route_online"})
        assert eng.spill_stats()["resumed"] == 0  # (the same batch again: one run)
        assert eng.spill_stats()["cand_big"] == len(b["lat"])
        # (the candidate stage had finished when the tier woke: the batch resumed there, and the tables
        # it needed were made in the same step)
        eng.match(q)


def test_wake_seg_large_then_viterbi_lists(small_graph, oracle, results_equal, monkeypatch, roomy):
    q = quiet_batch(small_graph)
    b = long_batch(small_graph)
    ob = orc_of(oracle, small_graph, b, "p129")
    with Engine(graph_path=small_graph) as eng:
        settle(eng, q, orc_of(oracle, small_graph, q, "q81"), results_equal)
        # the wave form of Viterbi (small batches) has no lists: the 129-point traces need the large plan alone
        woken(eng, b, ob, results_equal, {"seg_large"})
        assert "vit_lists" in eng.tiers()["dormant"]
        # ... and under the row form the list pass of the wave form
        monkeypatch.setenv("OTM_VIT_FORM", "4")
        woken(eng, b, ob, results_equal, {"vit_lists"})


def test_wake_viterbi_lists_wide_column(small_graph, oracle, results_equal, monkeypatch, roomy):
    monkeypatch.setenv("OTM_VIT_FORM", "4")
    meili = dict(search_radius=20.0, max_search_radius=300.0, max_candidates=17)
    narrow = synth.make_traces(small_graph, 12, 30, interval_s=5.0, noise_sigma_m=5.0, accuracy=5.0, seed=56)
    wide = synth.make_traces(small_graph, 12, 30, interval_s=5.0, noise_sigma_m=25.0, accuracy=300.0, seed=55)
    b = interleave(wide, narrow)
    ob = orc_of(oracle, small_graph, b, "wide17", meili)
    with Engine(graph_path=small_graph, **meili) as eng:
        settle(eng, narrow, orc_of(oracle, small_graph, narrow, "narrow", meili), results_equal, want={"vit_lists"})
        # the wide traces' probes (25 m of noise, a 300 m radius) also take steps the route index cannot
        # answer, which the narrow ones did not: three groups in two units, two extra attempts
        woken(eng, b, ob, results_equal, {"vit_lists", "trans_online", "route_online"})


def test_tiers_always(small_graph, oracle, results_equal, monkeypatch, roomy):
    monkeypatch.setenv("OTM_TIERS_ALWAYS", "1")
    q = quiet_batch(small_graph)
    gaps = synth.make_traces(small_graph, 60, 30, interval_s=120.0, noise_sigma_m=10.0, accuracy=10.0, seed=9)
    oq, og = orc_of(oracle, small_graph, q, "q81"), orc_of(oracle, small_graph, gaps, "gaps120")
    with Engine(graph_path=small_graph) as eng:
        disp = set()
        for _ in range(QUIET + 2):
            results_equal(oq, eng.match(q), "quiet")
            t = eng.tiers()
            assert t["mask"] == 0 and eng.spill_stats()["attempts"] == 1
            disp.add(t["dispatches"])
        assert len(disp) == 1
        results_equal(og, eng.match(gaps), "gaps")
        assert eng.spill_stats()["attempts"] == 1 and eng.tiers()["mask"] == 0


def test_clone_learns_on_its_own(small_graph, oracle, results_equal, roomy):
    q = quiet_batch(small_graph)
    oq = orc_of(oracle, small_graph, q, "q81")
    with Engine(graph_path=small_graph) as eng:
        settle(eng, q, oq, results_equal)
        cl = eng.clone()
        try:
            assert cl.tiers()["mask"] == 0  # a fresh context: every group live
            settle(cl, q, oq, results_equal)
            gaps = synth.make_traces(small_graph, 60, 30, interval_s=120.0, noise_sigma_m=10.0, accuracy=10.0, seed=9)
            long_b = long_batch(small_graph)
            woken(cl, long_b, orc_of(oracle, small_graph, long_b, "p129"), results_equal, {"seg_large"})
            woken(cl, gaps, orc_of(oracle, small_graph, gaps, "gaps120"), results_equal,
                  {"trans_online", "route_online"})
            assert eng.tiers()["dormant"] == ALL  # the parent did not hear of it
            # both contexts at once, from two threads: one dormant, one partly live
            got = {}

            def run(e, key):
                got[key] = [getattr(e.match(q), k).tobytes() for k in KEYS]
            th = [threading.Thread(target=run, args=(eng, "parent")), threading.Thread(target=run, args=(cl, "clone"))]
            for t in th:
                t.start()
            for t in th:
                t.join()
            want = [oq[k].tobytes() for k in KEYS]
            assert got["parent"] == want and got["clone"] == want
        finally:
            cl.close()


def test_timing_keeps_every_name(small_graph, oracle, results_equal):
    q = quiet_batch(small_graph)
    oq = orc_of(oracle, small_graph, q, "q81")
    with Engine(graph_path=small_graph) as eng:
        eng.set_timing(True)
        eng.match(q)
        names = set(eng.kernel_ms())
        settle(eng, q, oq, results_equal, want=set())
        assert eng.tiers()["dormant"] == ALL
        results_equal(oq, eng.match(q), "timed, dormant")
        ms = eng.kernel_ms()
        assert set(ms) == names
        # an empty begin/end pair on the stream: the two event records' own span, as "spatial_order"
        # reads in the small launch plan (4.5 - 5.5 us measured; a launched kernel's span starts there)
        print({k: round(v * 1e3, 2) for k, v in ms.items()})
        for k in ("k_transitions", "k_transitions_big", "k_route", "k_route_big"):
            assert 0.0 <= ms[k] < 0.008, (k, ms[k])
        assert ms["k_columns"] > 0 and ms["k_segments"] > 0


def test_counting_equal_to_always_live(small_graph, oracle, results_equal, monkeypatch):
    q = quiet_batch(small_graph)
    oq = orc_of(oracle, small_graph, q, "q81")
    with Engine(graph_path=small_graph) as eng:
        eng.set_counting(True)
        settle(eng, q, oq, results_equal)
        results_equal(oq, eng.match(q), "counted, dormant")
        c_dormant, s_dormant = eng.counters(), eng.spill_stats()
    monkeypatch.setenv("OTM_TIERS_ALWAYS", "1")
    with Engine(graph_path=small_graph) as eng:
        eng.set_counting(True)
        results_equal(oq, eng.match(q), "counted, live")
        assert eng.counters() == c_dormant and eng.spill_stats() == s_dormant


def test_capacity_redo_while_dormant(small_graph, oracle, results_equal, monkeypatch):
    # the transition matrices overflow with every group dormant: the whole batch runs twice
    monkeypatch.setenv("OTM_TRANS_CAP", "64")
    monkeypatch.setenv("OTM_POOL_CAP", str(1 << 22))
    q, q2 = quiet_batch(small_graph), synth.make_traces(small_graph, 150, 60, interval_s=5.0, noise_sigma_m=5.0,
                                                        accuracy=5.0, seed=83)
    oq, o2 = orc_of(oracle, small_graph, q, "q81"), orc_of(oracle, small_graph, q2, "q83")
    with Engine(graph_path=small_graph) as eng:
        results_equal(oq, eng.match(q), "first")
        assert eng.spill_stats()["attempts"] == 2  # (the pinned capacity grew)
        results_equal(oq, eng.match(q), "second")
        assert eng.tiers()["dormant"] == ALL
        results_equal(o2, eng.match(q2), "larger, redone")
        assert eng.spill_stats()["attempts"] == 2 and eng.tiers()["dormant"] == ALL
