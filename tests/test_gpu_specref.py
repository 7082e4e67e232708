"""The HIP kernels against the independent float64 reference of the written
spec (DESIGN.md §3 rules 1-7; tests/specref.py), with no oracle in the loop:
the engine's own stage arrays (`Engine.debug`) and final records go through
the comparisons of tests/specref_checks.py, stage-isolated and end to end, on
the inputs of tests/test_specref.py (tests/specref_cases.py).

Parametrised over what changes which kernel or tier runs: both launch plans,
the route index on and off, the device grid's merge factor, the transition
kernel's lane count and the Viterbi forms.  Rule 7's interpolated points (K7a
`k_seg_bound` / `interp_pos`, and `step_bound` in the three segment emitters)
are compared in full: `ipos` against the reference's placement, and every
boundary made from it.  The Python reference of a (graph, batch, params) is
computed once per module.
"""
import pytest

import specref as sr
import specref_cases
import specref_checks as ck

pytestmark = pytest.mark.gpu

ALL = ["city_5s", "city_30s", "gaps_240s", "radius_120", "radius_300", "dense_1s", "stop_and_go", "turn_factor_0",
       "accuracies", "long_140", "hand_edge_cases", "hand_radius_0", "hand_star",
       # rule 7's interpolated points
       "hand_short_edges", "hand_curve_interp", "hand_hairpin", "hand_filter", "stop_80", "seg_forms"]
_REF = {}
_STATS = {}     # case -> rule 7's statistics (stage-isolated, end to end) of its last run


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    from reporter_amd import synth
    return specref_cases.build(tmp_path_factory.mktemp("specref_gpu"), synth)


@pytest.fixture(params=["large", "small"])
def plan(request, monkeypatch):
    """The two launch plans of a batch, forced as in test_gpu_parity.batch_path."""
    monkeypatch.setenv("OTM_SMALL_POINTS", "0" if request.param == "large" else str(1 << 40))
    return request.param


def _check(cases, name, **engine_kw):
    """One batch through an engine; its arrays and records against the reference.
    Returns the engine's spill statistics."""
    from reporter_amd import Engine
    graph, batch, meili, max_excl = cases[name]
    if name not in _REF:
        G, P = sr.Graph(graph), sr.params(**meili)
        _REF[name] = (G, P, ck.Reference(G, batch, P))
    G, P, ref = _REF[name]
    with Engine(graph_path=graph, **engine_kw, **meili) as eng:
        res = eng.match(batch)
        impl = ck.Impl.from_engine(eng, res, len(batch["lat"]))
        spill = eng.spill_stats()
    _STATS[name] = (ck.check_isolated(G, batch, P, impl, max_excl, name),
                    ck.check_end_to_end(ref, impl, max_excl, name), impl)
    return spill


@pytest.mark.parametrize("name", ALL)
def test_kernels_against_spec(cases, plan, name):
    _check(cases, name)


@pytest.mark.parametrize("name", ["city_30s", "gaps_240s"])
def test_online_search_tiers(cases, plan, name):
    # no route index: every transition and route comes from the online searches.
    # A search of more than 192 labels leaves the LDS tables for the global-table
    # tier; the bounds of 30 s and 240 s gaps cover most of the 472-edge city, so
    # both batches reach it (24 traces at 240 s: every linked column does).
    sp = _check(cases, name, index_radius_m=0.0)
    print(name, "spill", sp)
    assert sp["trans_online"] > 0 and sp["route_online"] > 0, sp
    assert sp["trans_global"] > 0, sp


@pytest.mark.parametrize("name", ["stop_and_go", "hand_short_edges", "stop_80"])
def test_interpolated_points_on_online_routes(cases, name):
    # no route index: the paths K7a walks come from the online route tiers, which
    # fill path_pool themselves (k_route_index does not run)
    sp = _check(cases, name, index_radius_m=0.0)
    assert sp["route_online"] > 0, sp
    iso, e2e, _ = _STATS[name]
    assert iso["placed"] >= 15 and e2e["placed"] >= 15 and iso["t_anchored"] >= 2, (iso, e2e)


def test_rule7_cases_reach_their_targets(cases, plan):
    """What tests/test_specref.py asserts of the oracle's run, of the kernels'
    (the statistics count what was compared): no case goes empty."""
    want = {"stop_and_go": dict(placed=200, t_anchored=60, sh_interp=40),
            "hand_short_edges": dict(placed=15, t_anchored=16, sh_interp=16),
            "hand_curve_interp": dict(placed=5, sh_interp=4, dropped=2),
            "hand_hairpin": dict(placed=3, t_anchored=4),
            "hand_filter": dict(placed=8, unplaced=1, dropped=1, sh_interp=6),
            "stop_80": dict(placed=specref_cases.STOP_N, t_anchored=2, sh_interp=2),
            "seg_forms": dict(placed=100, unplaced=2, dropped=4)}
    for name, w in want.items():
        _check(cases, name)
        for st in _STATS[name][:2]:
            assert all(st[k] >= v for k, v in w.items()), (name, w, st)
    iso, _, impl = _STATS["seg_forms"]
    batch = cases["seg_forms"][1]
    off = [int(x) for x in batch["trace_off"]]
    # the three emitters: k_segments<128,160> takes the 128-point trace, k_segments<256,512> the 129- and the
    # 256-point ones, the serial walk the 257-point one.  The small plan also spills on its traversal count
    # (nt > TR in k_segments): the last trace has <= 128 points and more than 160 traversals.
    assert [off[k + 1] - off[k] for k in range(1, 5)] == [128, 129, 256, 257] and off[6] - off[5] <= 128
    assert iso["trav_by_trace"][5] > 160
    assert all(iso["bounds_by_trace"][t] >= 2 for t in range(1, 6)), iso
    # the 129-point trace stands across point 256 of the batch: one step's run of interpolated points lies in
    # two blocks of k_seg_bound
    F = specref_cases.FORMS
    first = off[2] + F["stop_at"] + 1
    run = impl.ipos[first:first + F["stop_n"]]
    assert first < 256 < first + F["stop_n"] - 1 and run[0] >= 0 and (run == run[0]).all()
    # the stop of 80 samples: more than one wavefront of k_seg_bound threads in one step, all at position 0
    impl = _STATS["stop_80"][2]
    at, n = specref_cases.STOP_AT, specref_cases.STOP_N
    assert (impl.ipos[at + 1:at + 1 + n] == 0.0).all()


@pytest.mark.parametrize("grid_mult", [1, 3])
@pytest.mark.parametrize("name", ["city_5s", "radius_300", "hand_star"])
def test_device_grid_merge(cases, plan, name, grid_mult):
    # the reference scans every shape segment and knows no grid
    _check(cases, name, grid_mult=grid_mult)


@pytest.mark.parametrize("lanes", [8, 16])
@pytest.mark.parametrize("name", ["radius_120", "radius_300"])
def test_transition_lanes(cases, name, lanes):
    _check(cases, name, trans_lanes=lanes)


@pytest.mark.parametrize("form", ["8", "16", "64"])
@pytest.mark.parametrize("name", ["radius_120", "long_140", "gaps_240s"])
def test_viterbi_forms(cases, monkeypatch, name, form):
    monkeypatch.setenv("OTM_VIT_FORM", form)
    _check(cases, name)


def test_report_headroom():
    """Not a check: prints the largest error / bound ratios seen (pytest -s)."""
    print("specref error/bound ratios (kernels):", {k: round(float(v), 3) for k, v in sorted(ck.RATIOS.items())})
    print("rule 7, excluded as ambiguous (points, of; boundaries, of):",
          {"%s %s" % k: v for k, v in sorted(ck.SHARES.items()) if v[1] or v[3]})
