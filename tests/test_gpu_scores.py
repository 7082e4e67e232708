"""k_scores (DESIGN.md §3 rule 7e) through the C ABI: the match scores of the
inputs of tests/specref_cases.py and of the shapes at which the packed form
can go wrong, under both launch plans and both forms (OTM_SCORE_FORM 1 and 4),
bit for bit against the ordered-float32 reference (tests/score_ref.py) run on
the engine's own stage arrays (`Engine.debug`), and inside the derived bounds
of the float64 reference; the switch off (nothing changes); a trace answered
500; batches that regrow a capacity or resume at a tier; and the interface
paths that carry the records (compact batches, clones, the device buffer,
multi-device engines).

Every batch's shape is asserted from the stage arrays before anything is
compared, so a case cannot quietly stop reaching what it is there for.
"""
import ctypes as C

import numpy as np
import numpy.testing as npt
import pytest

import score_ref as sc
import specref_cases
from reporter_amd._lib import SCORE_DTYPE, PointScore  # noqa: F401  (the record: no such names before this API)
from test_gpu_viterbi_row import alternating, interleave, take

pytestmark = pytest.mark.gpu

EMPTY = dict(trace_off=np.zeros(1, np.int64), lat=np.zeros(0, np.float32), lon=np.zeros(0, np.float32),
             time=np.zeros(0), accuracy=np.zeros(0, np.float32))
ZERO = np.zeros(1, sc.DTYPE)
ZERO["alt"], ZERO["alt_edge"] = -1, -1


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    from reporter_amd import synth
    return specref_cases.build(tmp_path_factory.mktemp("scores_gpu"), synth)


@pytest.fixture(params=["large", "small"])
def plan(request, monkeypatch):
    """The two launch plans of a batch, forced as tests/test_gpu_points.py forces them."""
    monkeypatch.setenv("OTM_SMALL_POINTS", "0" if request.param == "large" else str(1 << 40))
    return request.param


@pytest.fixture(params=[1, 4], ids=["general", "packed"])
def form(request, monkeypatch):
    monkeypatch.setenv("OTM_SCORE_FORM", str(request.param))
    return request.param


def stages(eng):
    return {k: eng.debug(k) for k in sc.STAGES}


def compare(eng, batch, what, st=None, codes=None):
    """The engine's records of its last batch against the float32 reference on
    its own stage arrays (and the traces' result codes, where a trace may have
    failed), bit for bit, and both exact consequences of the rule from the
    records alone.  -> (records, stage arrays)."""
    st = st or stages(eng)
    rec = eng.scores()
    assert rec.dtype == SCORE_DTYPE and len(rec) == len(batch["lat"]), what
    ref = sc.scores(batch, st, codes)
    for f in sc.DTYPE.names:
        a, b = rec[f], ref[f]
        if a.dtype.kind == "f":
            a, b = a.view(np.uint32), b.view(np.uint32)
        npt.assert_array_equal(a, b, err_msg="%s %s" % (what, f))
    assert rec.tobytes() == ref.tobytes(), what
    sc.fold_chain_costs(rec)
    return rec, st


def widths(st, n):
    """Candidate counts of the scored columns."""
    k = np.nonzero(st["state"][:n] >= 0)[0]
    return st["ncand"][k]


def linked_pairs(st, n):
    p = np.nonzero((st["state"][:n] >= 0) & (st["chain_start"][:n] == 0))[0]
    return st["ncand"][st["col_prev"][p]], st["ncand"][p]


# ------------------------------------------------------------------ the case subset
@pytest.mark.parametrize("name", ["city_5s", "gaps_240s", "radius_120", "radius_300", "long_140", "stop_and_go",
                                  "hand_edge_cases", "hand_star"])
def test_case_against_references(cases, plan, form, name):
    from reporter_amd import Engine
    graph, batch, meili, max_excl = cases[name]
    n = len(batch["lat"])
    with Engine(graph_path=graph, scores=True, **meili) as eng:
        assert eng.scores_info() is True
        eng.match(batch)
        st = stages(eng)
        # what the case is there for, from the stage arrays
        w = widths(st, n)
        assert len(w) > 0
        if name == "radius_300":
            assert w.max() > 16
        if name == "long_140":
            assert n > 128 and (st["state"][:n] >= 0).sum() > 128
        if name == "gaps_240s":
            assert (st["chain_start"][:n] != 0).sum() > len(batch["trace_off"]) - 1
        rec, _ = compare(eng, batch, name, st)
    if name == "gaps_240s":
        tie = (rec["flags"] & sc.TIE) != 0
        assert tie.sum() >= 1 and (rec["margin"][tie] == 0).all() and not np.signbit(rec["margin"][tie]).any()
    stats = sc.check_f64(batch, st, rec, name, max_excl=None if max_excl is None else 0)
    print(name, plan, form, stats)
    assert stats["scored"] == len(w)


# ------------------------------------------------------------------ batch sizes, trace lengths, column widths
@pytest.mark.parametrize("n_traces", [1, 3, 4, 5])
def test_batch_sizes(small_graph, form, n_traces):
    # idle rows (1, 3), one full wave (4), a second wave with one row (5)
    from reporter_amd import Engine, synth
    b = take(synth.make_traces(small_graph, 5, 40, seed=51), list(range(n_traces)))
    with Engine(graph_path=small_graph, scores=True) as eng:
        eng.match(b)
        rec, st = compare(eng, b, "%d traces" % n_traces)
    assert len(b["trace_off"]) - 1 == n_traces and ((rec["flags"] & sc.SCORED) != 0).sum() >= 20 * n_traces


def test_128_and_129_points(small_graph, form):
    # the longest trace the packed form takes and the shortest it hands to the
    # general form's list, beside each other and short ones in the same waves
    from reporter_amd import Engine, synth
    long_b = synth.make_traces(small_graph, 6, 129, seed=53)
    short_b = synth.make_traces(small_graph, 5, 30, seed=54)
    b = interleave(take(long_b, list(range(6)), [128, 129, 129, 128, 128, 129]), short_b)
    n = np.diff(b["trace_off"])
    assert (n == 128).sum() == 3 and (n == 129).sum() == 3 and (n == 30).sum() == 5
    with Engine(graph_path=small_graph, scores=True) as eng:
        eng.match(b)
        rec, st = compare(eng, b, "128 and 129 points")
    # the long traces are scored to their last point
    for t in np.nonzero(n >= 128)[0]:
        last = rec[int(b["trace_off"][t + 1]) - 1]
        assert last["flags"] & sc.SCORED and last["flags"] & sc.CHAIN_END


def test_one_and_two_point_traces(small_graph, form):
    from reporter_amd import Engine, synth
    base = synth.make_traces(small_graph, 10, 30, seed=52)
    b = take(base, list(range(10)), [1, None, 2, None, None, 2, 1, None, 1, 2])
    assert sorted(np.diff(b["trace_off"]).tolist())[:6] == [1, 1, 1, 2, 2, 2]
    with Engine(graph_path=small_graph, scores=True) as eng:
        eng.match(b)
        rec, st = compare(eng, b, "one- and two-point traces")
    one = rec[0]
    assert one["flags"] & sc.SCORED and one["flags"] & sc.CHAIN_START and one["flags"] & sc.CHAIN_END
    assert one["cost"] == one["emission"] == one["chain_cost"]


@pytest.mark.parametrize("kmax", [16, 17])
def test_16_and_17_candidates(small_graph, form, kmax):
    # columns of exactly 16 candidates (all of a row's lanes are states) or 17
    # (the packed form hands the trace to the general form through its list),
    # narrow traces in the same waves
    from reporter_amd import Engine, synth
    wide = synth.make_traces(small_graph, 12, 30, interval_s=5.0, noise_sigma_m=25.0, accuracy=300.0, seed=55)
    narrow = synth.make_traces(small_graph, 12, 30, interval_s=5.0, noise_sigma_m=5.0, accuracy=5.0, seed=56)
    b = interleave(wide, narrow)
    n = len(b["lat"])
    with Engine(graph_path=small_graph, scores=True, search_radius=20.0, max_search_radius=300.0,
                max_candidates=kmax) as eng:
        eng.match(b)
        st = stages(eng)
        w = widths(st, n)
        assert w.max() == kmax and (w == kmax).sum() > 50 and (w <= 8).sum() > 50
        kq, kp = linked_pairs(st, n)
        assert ((kq == kmax) & (kp == kmax)).sum() > 50
        compare(eng, b, "max_candidates %d" % kmax, st)


def test_wide_and_narrow_column_pairs(tmp_path, form):
    # the ladder's 16 -> 1 and 1 -> 16 column pairs: a lane past a column's
    # count must read +inf, never a neighbour's cost (the packed form has no
    # transition window to force off: it reads each block at its step)
    from reporter_amd import Engine
    graph, b, meili = alternating(str(tmp_path / "ladder.otmg"))
    n = len(b["lat"])
    with Engine(graph_path=graph, scores=True, **meili) as eng:
        eng.match(b)
        st = stages(eng)
        kq, kp = linked_pairs(st, n)
        assert ((kq == 16) & (kp == 1)).sum() >= 20, "16 -> 1"
        assert ((kq == 1) & (kp == 16)).sum() >= 20, "1 -> 16"
        assert ((kq == 16) & (kp == 16)).sum() >= 20 and ((kq == 1) & (kp == 1)).sum() >= 20
        rec, _ = compare(eng, b, "ladder", st)
    alone = (rec["flags"] & sc.ALONE) != 0
    assert alone.sum() >= 40 and (rec["ncand"][alone] == 1).sum() >= 40
    sc.check_f64(b, st, rec, "ladder")


def _breaks_batch(graph):
    """tests/test_gpu_viterbi_row.py test_chain_breaks_and_empty_columns' batch."""
    from reporter_amd import synth
    gaps = synth.make_traces(graph, 60, 40, interval_s=240.0, noise_sigma_m=15.0, accuracy=15.0, seed=41)
    holes = synth.make_traces(graph, 12, 30, seed=58)
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
    return interleave(gaps, holes)


def test_chain_breaks_and_empty_columns(small_graph, form):
    from reporter_amd import Engine
    b = _breaks_batch(small_graph)
    n = len(b["lat"])
    with Engine(graph_path=small_graph, scores=True, breakage_distance=800.0) as eng:
        eng.match(b)
        st = stages(eng)
        nc, state, cs, is_col = st["ncand"][:n], st["state"][:n], st["chain_start"][:n], st["is_col"][:n]
        assert ((is_col != 0) & (nc == 0)).sum() >= 12 * 3
        assert ((st["col_prev"][:n] < 0) & (nc > 0) & (state >= 0)).sum() > len(b["trace_off"]) - 1
        rec, _ = compare(eng, b, "breaks", st)
    scored = (rec["flags"] & sc.SCORED) != 0
    npt.assert_array_equal(scored, state >= 0)
    # the records around the breaks are zero
    assert rec[~scored].tobytes() == ZERO.tobytes() * int((~scored).sum())
    # CHAIN_START sits where K5 started a chain, CHAIN_END on the scored column before the next start (or the
    # trace's last scored column)
    npt.assert_array_equal((rec["flags"] & sc.CHAIN_START) != 0, scored & (cs != 0))
    k = np.nonzero(scored)[0]
    tr = np.searchsorted(b["trace_off"], k, side="right")
    end = np.ones(len(k), bool)
    end[:-1] = (cs[k[1:]] != 0) | (tr[1:] != tr[:-1])
    npt.assert_array_equal((rec["flags"][k] & sc.CHAIN_END) != 0, end)


# ------------------------------------------------------------------ the empty batch, a trace answered 500, redone batches
def test_empty_batch(small_graph, form):
    from reporter_amd import Engine
    with Engine(graph_path=small_graph, scores=True) as eng:
        r = eng.match(EMPTY)
        assert len(r.traces) == 0 and len(eng.scores()) == 0 and eng.scores_device() == (0, 0)


@pytest.fixture(scope="module")
def star(tmp_path_factory):
    import handgraph
    from test_no_limits import SPOKES, STAR_LON
    return handgraph.star(str(tmp_path_factory.mktemp("scores_star") / "star.otmg"), lon=STAR_LON, n_spokes=SPOKES,
                          length_m=90.0)[0]


def test_trace_answered_500(star, monkeypatch, form):
    from reporter_amd import Engine
    from test_gpu_points import _star_batch_with_a_far_trace
    meili = dict(search_radius=20.0, max_search_radius=20.0)
    b = _star_batch_with_a_far_trace()
    a = int(b["trace_off"][3])
    with Engine(graph_path=star, scores=True, **meili) as eng:
        eng.match(take(b, [3]))
        alone = eng.scores()
    monkeypatch.setenv("OTM_CAND_MAX_LOG2", "0")    # no candidate HBM tier: a probe that needs it fails its trace
    with Engine(graph_path=star, scores=True, **meili) as eng:
        res = eng.match(b)
        assert list(res.traces["code"]) == [500, 500, 500, 200]
        rec, _ = compare(eng, b, "star 500", codes=res.traces["code"])
    assert rec[:a].tobytes() == ZERO.tobytes() * a               # the failed traces: all zero
    assert ((rec[a:]["flags"] & sc.SCORED) != 0).all()
    assert rec[a:].tobytes() == alone.tobytes()                  # the neighbour: unchanged


@pytest.fixture(scope="module")
def dense_grid(tmp_path_factory):
    """tests/test_no_limits.py's dense grid: 600 s gaps on it need the huge search tier."""
    from reporter_amd import synth
    d = tmp_path_factory.mktemp("scores_dense")
    return synth.make_graph(str(d / "grid32.otmg"), width_m=12000, height_m=12000, block_m=32, jitter_m=0,
                            arterial_every=8, highway_every=1000, complex_every=4, seg_max_m=300)


def test_trace_failed_by_a_search_after_a_scored_batch(dense_grid, monkeypatch, form):
    """The huge search tier barred (test_no_limits' cap case): the traces with
    600 s gaps fail in the transition or the route stage -- the second after
    K5 gave their columns states -- on an engine whose last batch left scored
    records at the same points.  Their records are all zero, never the last
    batch's, whichever stage failed them."""
    from reporter_amd import Engine, synth
    from test_no_limits import GRID_MEILI, grid_batch
    monkeypatch.setenv("OTM_HUGE_MAX_LOG2", "0")
    far = grid_batch(dense_grid)
    near = synth.make_traces(dense_grid, 2, 6, interval_s=5.0, noise_sigma_m=5.0, accuracy=5.0, seed=6)
    b = {k: np.concatenate([far[k], near[k]]) for k in ("lat", "lon", "time", "accuracy")}
    b["trace_off"] = np.concatenate([far["trace_off"], far["trace_off"][-1] + near["trace_off"][1:]])
    prev = synth.make_traces(dense_grid, 5, 6, interval_s=5.0, noise_sigma_m=5.0, accuracy=5.0, seed=61)
    prev = {k: prev[k] for k in ("trace_off", "lat", "lon", "time", "accuracy")}
    assert list(prev["trace_off"]) == list(b["trace_off"])
    with Engine(graph_path=dense_grid, scores=True, **GRID_MEILI) as eng:
        r0 = eng.match(prev)
        assert (r0.traces["code"] == 200).all()
        before, _ = compare(eng, prev, "before", codes=r0.traces["code"])
        assert ((before["flags"] & sc.SCORED) != 0).all()          # every point of the last batch holds a score
        res = eng.match(b)
        code = res.traces["code"]
        bad = np.nonzero(code != 200)[0]
        assert len(bad) >= 1 and (code[bad] == 500).all() and (code[3:] == 200).all()
        st = stages(eng)
        rec, _ = compare(eng, b, "huge tier barred", st, codes=code)
    off = b["trace_off"]
    for t in bad:
        a, e = int(off[t]), int(off[t + 1])
        print("failed trace", t, "columns left with a state:", int((st["state"][a:e] >= 0).sum()))
        assert rec[a:e].tobytes() == ZERO.tobytes() * (e - a)
    a = int(off[3])
    assert ((rec[a:]["flags"] & sc.SCORED) != 0).all()


def test_regrown_and_resumed_batches(cases, star, monkeypatch, form):
    from reporter_amd import Engine
    from test_no_limits import RADIUS_100, star_batch
    # a tier's tables grown on demand: the first batch resumes at the candidate HBM tier, the second runs clean
    b = star_batch()
    with Engine(graph_path=star, scores=True, **RADIUS_100) as eng:
        eng.match(b)
        first, st1 = eng.scores(), eng.spill_stats()
        eng.match(b)
        clean, st2 = compare(eng, b, "star clean")[0], eng.spill_stats()
    assert st1["attempts"] >= 2 and st1["resumed"] >= 1 and st2["attempts"] == 1
    assert ((clean["flags"] & sc.SCORED) != 0).all() and clean["ncand"].max() == 32
    assert first.tobytes() == clean.tobytes()
    # tiny pinned capacities: the transition matrices and the path pool overflow and the batch is redone whole
    graph, batch, meili, _ = cases["stop_and_go"]
    with Engine(graph_path=graph, scores=True, **meili) as eng:
        eng.match(batch)
        want = eng.scores()
    monkeypatch.setenv("OTM_TRANS_CAP", "64")
    monkeypatch.setenv("OTM_POOL_CAP", "8")
    with Engine(graph_path=graph, scores=True, **meili) as eng:
        eng.match(batch)
        got, st = eng.scores(), eng.spill_stats()
    assert st["attempts"] >= 2
    assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------ the switch
def test_off_by_default(cases):
    from reporter_amd import Engine, OtmError, _lib, encode_request
    graph, batch, meili, _ = cases["stop_and_go"]
    n = len(batch["lat"])
    names = sorted(Engine._DEBUG)
    with Engine(graph_path=graph, **meili) as eng:
        assert eng.scores_info() is False
        off = eng.match(batch)
        st_off = {k: eng.debug(k).tobytes() for k in names}
        with pytest.raises(OtmError, match="off"):
            eng.scores()
        with pytest.raises(OtmError, match="off"):
            eng.scores_device()
        eng.set_scores(True)
        with pytest.raises(OtmError, match="no batch"):
            eng.scores()     # the last batch ran with the switch off
        on = eng.match(batch)
        st_on = {k: eng.debug(k).tobytes() for k in names}
        assert len(eng.scores()) == n
        buf = np.zeros(n - 1, dtype=SCORE_DTYPE)
        cnt = C.c_int64()
        assert _lib.lib().otm_fetch_scores(eng.h, buf.ctypes.data, n - 1, C.byref(cnt)) == -1   # cap below the count
        assert "cap" in _lib.last_error() and cnt.value == n
        # a JSON batch on the handle ends the binary batch's records
        o = batch["trace_off"]
        body = encode_request("veh0", batch["lat"][o[0]:o[1]], batch["lon"][o[0]:o[1]],
                              batch["time"][o[0]:o[1]].astype(np.int64), batch["accuracy"][o[0]:o[1]].astype(np.int32))
        assert len(eng.report_batch([body])) == 1
        with pytest.raises(OtmError, match="no batch"):
            eng.scores()
        with pytest.raises(OtmError, match="no batch"):
            eng.scores_device()
        eng.match(batch)
        assert len(eng.scores()) == n
        eng.set_scores(False)
        with pytest.raises(OtmError, match="off"):
            eng.scores()
    for key in ("traces", "segments", "reports", "way_ids"):
        assert getattr(on, key).tobytes() == getattr(off, key).tobytes(), key
    for k in names:
        assert st_on[k] == st_off[k], k


# ------------------------------------------------------------------ interface paths
def test_compact_clone_device_and_members_agree(cases):
    import torch
    from reporter_amd import Engine, OtmError
    from test_gpu_points import _DeviceBytes
    graph, batch, meili, _ = cases["stop_and_go"]    # whole-second times: a compact batch carries them
    n = len(batch["lat"])
    with Engine(graph_path=graph, scores=True, **meili) as eng:
        eng.match(batch)
        base, _ = compare(eng, batch, "base")
        assert eng.scores().tobytes() == base.tobytes()          # a second fetch: the same bytes
        ptr, cnt = eng.scores_device()
        assert ptr and cnt == n
        dev = torch.as_tensor(_DeviceBytes(ptr, n * 32), device="cuda:0")
        assert dev.cpu().numpy().view(SCORE_DTYPE).tobytes() == base.tobytes()
        eng.match_compact(batch)
        assert eng.scores().tobytes() == base.tobytes()
        cl = eng.clone()
        try:
            assert cl.scores_info() is True                      # inherited when it was made
            cl.match(batch)
            assert cl.scores().tobytes() == base.tobytes()
        finally:
            cl.close()
        eng.set_scores(False)
        cl = eng.clone()
        try:
            assert cl.scores_info() is False
        finally:
            cl.close()
    assert ((base["flags"] & sc.SCORED) != 0).sum() >= 250
    with Engine(graph_path=graph, devices=[0, 0], scores=True, **meili) as grp:
        assert grp.members() == 2 and grp.scores_info() is True and grp.member(1).scores_info() is True
        with pytest.raises(OtmError, match="no batch"):
            grp.scores()
        res = grp.match(batch)
        assert len(res.traces) == len(batch["trace_off"]) - 1
        assert grp.scores().tobytes() == base.tobytes()
        assert grp.scores().tobytes() == base.tobytes()
        with pytest.raises(OtmError, match="member"):
            grp.scores_device()
