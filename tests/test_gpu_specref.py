"""The HIP kernels against the independent float64 reference of the written
spec (DESIGN.md §3 rules 1-7; tests/specref.py), with no oracle in the loop:
the engine's own stage arrays (`Engine.debug`) and final records go through
the comparisons of tests/specref_checks.py, stage-isolated and end to end, on
the inputs of tests/test_specref.py (tests/specref_cases.py).

Parametrised over what changes which kernel or tier runs: both launch plans,
the route index on and off, the device grid's merge factor, the transition
kernel's lane count and the Viterbi forms.  The Python reference of a (graph,
batch, params) is computed once per module.
"""
import pytest

import specref as sr
import specref_cases
import specref_checks as ck

pytestmark = pytest.mark.gpu

ALL = ["city_5s", "city_30s", "gaps_240s", "radius_120", "radius_300", "dense_1s", "stop_and_go", "turn_factor_0",
       "accuracies", "long_140", "hand_edge_cases", "hand_radius_0", "hand_star"]
_REF = {}


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
    ck.check_isolated(G, batch, P, impl, max_excl)
    ck.check_end_to_end(ref, impl, max_excl)
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
