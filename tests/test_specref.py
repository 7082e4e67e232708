"""The CPU oracle against the independent float64 reference of the written
spec (DESIGN.md §3 rules 1-7; tests/specref.py), stage by stage and end to
end.  The GPU parity suite pins the kernels to the oracle bit for bit; this
file pins the oracle to the text, so a misreading shared by oracle and kernels
no longer passes.  tests/test_gpu_specref.py runs the same comparisons on the
kernels' own stage arrays.

Every case runs two ways (specref_checks): stage-isolated, each reference
stage fed with the oracle's own upstream arrays; and end to end, the
reference on its own arrays against the oracle's final segments.  Each check
asserts its exclusion caps before it compares; the hand graphs allow none.

Rule 7's interpolated points are compared in full (placement, monotone filter,
shape indices and times of every boundary inside a step); the cases made for
them are RULE7 below, and test_rule7_cases_reach_their_targets asserts that
each reached what it exists for.  DESIGN.md §2 lists the oracle mutations
these tests were checked to fail on.
"""
import math

import numpy as np
import pytest

import specref as sr
import specref_cases
import specref_checks as ck

CITY = ["city_5s", "city_30s", "gaps_240s", "radius_120", "radius_300", "dense_1s", "stop_and_go", "turn_factor_0",
        "accuracies", "long_140"]
HANDS = ["hand_edge_cases", "hand_radius_0", "hand_star"]
# rule 7's interpolated points (specref_cases): hand graphs with no exclusion allowed, and city traces
RULE7 = ["hand_short_edges", "hand_curve_interp", "hand_hairpin", "hand_filter", "stop_80", "seg_forms"]
STATS = {}      # (check, case) -> rule 7's statistics, filled by the two tests below


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    from reporter_amd import synth
    return specref_cases.build(tmp_path_factory.mktemp("specref"), synth)


@pytest.fixture(scope="module")
def run(cases, oracle):
    """name -> (Graph, batch, params, Impl of the oracle, max_excl), once per case."""
    memo = {}

    def get(name):
        if name not in memo:
            graph, batch, meili, max_excl = cases[name]
            orc = oracle.match_batch(oracle.Graph(graph), batch, p=oracle.params(**meili), keep_stages=True)
            memo[name] = (sr.Graph(graph), batch, sr.params(**meili), ck.Impl.from_oracle(orc, len(batch["lat"])),
                          max_excl)
        return memo[name]
    return get


@pytest.fixture(scope="module")
def reference(run):
    memo = {}

    def get(name):
        if name not in memo:
            G, batch, P, _, _ = run(name)
            memo[name] = ck.Reference(G, batch, P)
        return memo[name]
    return get


def test_turn_table_series_rounds_as_exp():
    # U[d] is defined with exp; the implementations' fixed 40-term series must round to the same table
    for f in (200.0, 1.0, 37.5, 1000.0):
        assert sr.turn_table(f) == sr.turn_table(f, exp=sr.exp_series40)
    assert sr.turn_table(0.0) == [0] * 181
    assert sr.turn_table(200.0)[180] == 12800 and sr.turn_table(200.0)[0] == int(math.floor(12800 / math.e ** 4 + 0.5))


@pytest.mark.parametrize("name", CITY + HANDS + RULE7)
def test_stage_isolated(run, name):
    G, batch, P, impl, max_excl = run(name)
    STATS["isolated", name] = ck.check_isolated(G, batch, P, impl, max_excl, name)


@pytest.mark.parametrize("name", CITY + HANDS + RULE7)
def test_end_to_end(run, reference, name):
    _, _, _, impl, max_excl = run(name)
    STATS["end to end", name] = ck.check_end_to_end(reference(name), impl, max_excl, name)


@pytest.fixture(scope="module")
def stats(run, reference):
    """(check, case) -> rule 7's statistics, from the two tests above when they ran."""
    def get(check, name):
        if (check, name) not in STATS:
            G, batch, P, impl, max_excl = run(name)
            STATS[check, name] = ck.check_isolated(G, batch, P, impl, max_excl, name) if check == "isolated" else \
                ck.check_end_to_end(reference(name), impl, max_excl, name)
        return STATS[check, name]
    return get


def _ipos(run, name, t):
    _, b, _, impl, _ = run(name)
    return [float(x) for x in impl.ipos[b["trace_off"][t]:b["trace_off"][t + 1]]]


def _shape(run, name, t):
    _, b, _, impl, _ = run(name)
    tr = impl.traces[t]
    s = impl.segments[tr["seg_off"]:tr["seg_off"] + tr["seg_cnt"]]
    return [int(x) for x in s["begin_shape_index"]], [int(x) for x in s["end_shape_index"]]


def test_rule7_cases_reach_their_targets(run, reference, stats):
    """No case of rule 7 can quietly go empty: each asserts what it exists for,
    on what was compared (ambiguous points and boundaries do not count)."""
    for check in ("isolated", "end to end"):
        # the two city cases whose boundaries were out of scope before
        s = stats(check, "stop_and_go")
        assert s["placed"] >= 200 and s["t_anchored"] >= 60 and s["sh_interp"] >= 40, s
        s = stats(check, "dense_1s")
        assert s["placed"] >= 10 and s["unplaced"] >= 1 and s["t_anchored"] >= 5, s
        # short edges: every interpolated point placed; the ends of a, s1, s2, s3 inside each of the four steps
        s = stats(check, "hand_short_edges")
        assert s["placed"] == 15 and s["sh_interp"] >= 16 and s["t_anchored"] >= 16, s
        s = stats(check, "hand_curve_interp")
        assert s["placed"] == 5 and s["sh_interp"] >= 4, s
        s = stats(check, "hand_hairpin")
        assert s["placed"] == 3 and s["t_anchored"] >= 4, s
        s = stats(check, "hand_filter")
        assert s["placed"] == 8 and s["unplaced"] == 1 and s["dropped"] == 1 and s["sh_interp"] >= 6, s
        s = stats(check, "stop_80")
        assert s["placed"] >= specref_cases.STOP_N and s["t_anchored"] >= 2 and s["sh_interp"] >= 2, s
        s = stats(check, "seg_forms")
        assert s["placed"] >= 100 and s["unplaced"] >= 2 and s["dropped"] >= 4, s
        assert all(s["bounds_by_trace"][t] >= 2 for t in range(1, 6)), s
    # which piece took each point (the reference's own placement)
    G, b, _, impl, _ = run("hand_short_edges")
    pc, off = reference("hand_short_edges").place.piece, b["trace_off"]
    state_off = lambda p: float(impl.cand_off[p * ck.KMAX + int(impl.state[p])])
    assert [int(x) for x in pc[off[0] + 2:off[0] + 6]] == [0, 1, 2, 3]     # first piece, s1, s2, s3
    assert [int(x) for x in pc[off[1] + 2:off[1] + 6]] == [0, 1, 2, 3]     # rest of s1, s2, s3, p's piece on b
    assert state_off(off[1] + 1) > 0 and impl.cand_edge[(off[1] + 1) * ck.KMAX + int(impl.state[off[1] + 1])] == \
        specref_cases.SHORT_IDS["s1"]
    assert state_off(off[2] + 1) == 0.0 and [int(x) for x in pc[off[2] + 2:off[2] + 5]] == [0, 1, 2]   # q a node
    assert state_off(off[3] + 6) == 0.0 and int(pc[off[3] + 5]) == 3       # p a node: s3 is the last piece
    # begin / end shape indices name interpolated points: one segment end between each pair of anchors
    assert _shape(run, "hand_short_edges", 0) == ([0, 2, 3, 4, 5], [2, 3, 4, 5, 7])
    # the curve: the point outside the arc at the repeated shape point lands on that vertex
    G, b, _, impl, _ = run("hand_curve_interp")
    q = int(b["trace_off"][1]) + 1
    curve = specref_cases.EDGE_IDS["curve"]
    assert impl.cand_edge[q * ck.KMAX + int(impl.state[q])] == curve
    vertex = float(G.scum[G.eshape[curve] + 4])
    assert G.scum[G.eshape[curve] + 5] == vertex                            # the zero-length shape segment
    assert abs(state_off(q) + impl.ipos[q + 1] - vertex) < 1e-3
    # the point behind q on the arc goes to the start of `north` (the last piece), not onto the arc ahead of q
    assert [int(x) for x in reference("hand_curve_interp").place.piece[2:5]] == [1, 0, 0]
    assert abs(impl.ipos[2] - (G.elen[curve] - state_off(1))) < 1e-3
    # the hairpin: |pos - gc| / beta keeps two points on e that are nearer to w; the third lands on w
    assert [int(x) for x in reference("hand_hairpin").place.piece[2:5]] == [0, 0, 2]
    # the filter road, trace by trace
    ip = lambda t: _ipos(run, "hand_filter", t)
    assert ip(0) == [-1.0] * 5                                              # behind q, and no other piece
    assert ip(1)[1] > ip(1)[2] > 0 and ip(1)[3] > ip(1)[1]                  # placed behind an anchor: dropped
    assert _shape(run, "hand_filter", 1) == ([0, 1, 4], [1, 4, 5])
    assert ip(2)[2] == ip(2)[3] > 0 and _shape(run, "hand_filter", 2)[1][0] == 3   # two copies: the later one
    assert ip(3) == [-1.0] * 5                                              # after the last state
    assert ip(4)[:6] == [-1.0] * 6 and ip(4)[6] > 0                         # around the empty column
    assert ip(5) == [-1.0, -1.0, -1.0, -1.0, 0.0, 0.0, -1.0, -1.0]          # copies across the breakage break
    _, b, _, impl, _ = run("hand_filter")
    assert impl.ncand[int(b["trace_off"][4]) + 3] == 0 and impl.col_prev[int(b["trace_off"][5]) + 3] < 0
    # the stop: 80 copies at position 0 in one step, its last copy names a boundary, two more segments end after it
    at, n = specref_cases.STOP_AT, specref_cases.STOP_N
    assert _ipos(run, "stop_80", 0)[at + 1:at + 1 + n] == [0.0] * n
    begin, end = _shape(run, "stop_80", 0)
    assert at + n in end and sum(1 for x in end if x > at + n) >= 2
    # the emitter forms: lengths around the 128- and 256-point plans, the 129-point trace standing across point
    # 256 of the batch, and a trace of <= 128 points with more traversals than the small plan holds (160)
    _, b, _, impl, _ = run("seg_forms")
    off = [int(x) for x in b["trace_off"]]
    assert [off[k + 1] - off[k] for k in range(1, 5)] == [128, 129, 256, 257] and off[6] - off[5] <= 128
    assert stats("isolated", "seg_forms")["trav_by_trace"][5] > 160
    F = specref_cases.FORMS
    first = off[2] + F["stop_at"] + 1
    run_ = impl.ipos[first:first + F["stop_n"]]                             # one step's run of placed copies
    assert first < 256 < first + F["stop_n"] - 1 and run_[0] >= 0 and (run_ == run_[0]).all()


def test_cases_reach_their_rules(run, reference):
    """Each input exists for a rule; the reference says whether it fired."""
    _, b, _, impl, _ = run("gaps_240s")
    cols = impl.is_col(b) & (impl.ncand > 0)
    first = np.zeros(len(cols), bool)
    first[b["trace_off"][:-1]] = True
    assert (cols & ~first & (impl.col_prev < 0)).sum() >= 10, "no chain breaks at 240 s"
    assert (impl.col_prev >= 0).sum() >= 10
    assert run("radius_120")[3].ncand.max() > 8
    assert run("radius_300")[3].ncand.max() == 32 and "cut" in reference("radius_300").fired
    assert (run("radius_300")[3].ncand > 16).any()
    for name in ("dense_1s", "stop_and_go"):
        _, b, _, impl, _ = run(name)
        assert (~impl.is_col(b)).sum() >= 20, "%s has no interpolated points" % name
    assert "multi_edge_route" in reference("city_30s").fired
    assert {"node_merge", "stay"} <= reference("city_5s").fired
    _, b, _, impl, _ = run("long_140")
    assert impl.is_col(b).sum() > 128


def test_hand_graph_rules_fire(run, reference):
    ref = reference("hand_edge_cases")
    assert {"zero_length_segment", "sink_end", "stay"} <= ref.fired
    G, batch, P, impl, _ = run("hand_edge_cases")
    ids = specref_cases.EDGE_IDS
    assert (np.diff(G.eshape) - 1).max() == 9                      # the curved edge's shape segments
    tr = impl.traces
    seg = lambda t: [int(x) for x in impl.segments["segment_id"][tr["seg_off"][t]:tr["seg_off"][t] + tr["seg_cnt"][t]]]
    sid = lambda nm: int(G.gid[G.eseg[ids[nm]]])
    assert seg(0) == [sid("curve"), sid("north")]
    assert seg(1) == [sid("sink")]
    # the stay: back along r01, not around the block
    assert seg(2) == [sid("r01"), sid("r12")]
    # equal integer costs through either twin: the lower predecessor edge wins
    assert ids["twin_a"] < ids["twin_b"] and G.L[ids["twin_a"]] == G.L[ids["twin_b"]]
    assert seg(3) == [sid("t01"), sid("twin_a"), sid("t23")]
    # two tied states on the twins: the lower index
    assert seg(4) == [sid("t01"), sid("twin_a"), sid("t23")]
    p = int(batch["trace_off"][4]) + 1
    k = int(impl.state[p])
    assert impl.cand_edge[p * ck.KMAX + k] == ids["twin_a"]
    twin = [j for j in range(int(impl.ncand[p])) if impl.cand_edge[p * ck.KMAX + j] == ids["twin_b"]]
    assert twin and impl.cand_emis[p * ck.KMAX + twin[0]] == impl.cand_emis[p * ck.KMAX + k]
    assert {"hit_at_radius", "sink_end", "node_merge"} <= reference("hand_radius_0").fired
    assert (run("hand_radius_0")[3].ncand == 1).all()
    assert "node_merge" in reference("hand_star").fired
    assert run("hand_star")[3].ncand[1] > 8


def test_report_headroom(run):
    """Not a check: prints the largest error / bound ratios seen so far (pytest -s)."""
    print("specref error/bound ratios:", {k: round(float(v), 3) for k, v in sorted(ck.RATIOS.items())})
    print("rule 7, excluded as ambiguous (points, of; boundaries, of):",
          {"%s %s" % k: v for k, v in sorted(ck.SHARES.items()) if v[1] or v[3]})
