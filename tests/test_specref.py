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


@pytest.mark.parametrize("name", CITY + HANDS)
def test_stage_isolated(run, name):
    G, batch, P, impl, max_excl = run(name)
    ck.check_isolated(G, batch, P, impl, max_excl)


@pytest.mark.parametrize("name", CITY + HANDS)
def test_end_to_end(run, reference, name):
    _, _, _, impl, max_excl = run(name)
    ck.check_end_to_end(reference(name), impl, max_excl)


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
