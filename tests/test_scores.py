"""Match scores (DESIGN.md §3 rule 7e) without a GPU: the record's layout, the
errors that need no device, the ordered-float32 reference of
tests/score_ref.py on hand graphs against closed-form answers, and that
reference against tests/specref.py's float64 Viterbi on the oracle's stage
arrays, inside bounds derived from the roundings (score_ref.tol_m).
"""
import ctypes as C

import numpy as np
import pytest

import score_ref as sc
import specref as sr
import specref_cases
from reporter_amd import _lib
from reporter_amd._lib import SCORE_DTYPE, PointScore  # noqa: F401  (the record: no such names before this API)

CASES = ["city_5s", "city_30s", "gaps_240s", "radius_120", "radius_300", "dense_1s", "stop_and_go", "long_140",
         "hand_edge_cases", "hand_star", "hand_hairpin"]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    from reporter_amd import synth
    return specref_cases.build(tmp_path_factory.mktemp("scores_cpu"), synth)


# ------------------------------------------------------------------ the record and the calls that need no device
def test_record_layout():
    assert C.sizeof(PointScore) == 32 and C.alignment(PointScore) == 4
    want = dict(cost=0, margin=4, chain_cost=8, emission=12, transition=16, alt_edge=20, alt_offset=24, flags=28,
                ncand=29, state=30, alt=31)
    assert {n: getattr(PointScore, n).offset for n, _ in PointScore._fields_} == want
    assert SCORE_DTYPE.itemsize == 32 and sc.DTYPE == SCORE_DTYPE
    assert {n: SCORE_DTYPE.fields[n][1] for n in SCORE_DTYPE.names} == want
    for n, t in PointScore._fields_:
        assert SCORE_DTYPE.fields[n][0].itemsize == C.sizeof(t)
    assert (_lib.SC_SCORED, _lib.SC_CHAIN_START, _lib.SC_CHAIN_END, _lib.SC_ALONE, _lib.SC_TIE) == (1, 2, 4, 8, 16) \
        == (sc.SCORED, sc.CHAIN_START, sc.CHAIN_END, sc.ALONE, sc.TIE)
    hdr = open(_lib.os.path.join(_lib._HERE, "..", "include", "otmatch.h")).read()
    for name, v in (("SCORED", 1), ("CHAIN_START", 2), ("CHAIN_END", 4), ("ALONE", 8), ("TIE", 16)):
        assert "#define OTM_SC_%s %du" % (name, v) in hdr
    assert "typedef struct otm_point_score { /* 32 bytes */" in hdr


def test_null_engine_is_einval():
    L = _lib.lib()
    on, n, p = C.c_int(7), C.c_int64(7), C.c_void_p()
    buf = np.zeros(2, SCORE_DTYPE)
    for rc in (L.otm_set_scores(None, 1), L.otm_scores_info(None, C.byref(on)),
               L.otm_fetch_scores(None, buf.ctypes.data, 2, C.byref(n)), L.otm_fetch_scores(None, None, 0, C.byref(n)),
               L.otm_scores_device(None, C.byref(p), C.byref(n))):
        assert rc == -1                                     # OTM_EINVAL
        assert "NULL" in _lib.last_error()
    assert (on.value, n.value, p.value) == (7, 7, None) and not buf.tobytes().strip(b"\0")


# ------------------------------------------------------------------ closed forms on hand graphs
@pytest.fixture(scope="module")
def two_roads(tmp_path_factory):
    """Two parallel one-way roads running east, 5 m apart (rungs every 85 m)."""
    from test_gpu_viterbi_row import ladder
    return ladder(str(tmp_path_factory.mktemp("scores_ladder") / "two.otmg"), rows=2)


def _probes(ls, pts, trace_off):
    """Points (metres east, metres north of the southern road)."""
    return dict(trace_off=np.array(trace_off, np.int64),
                lat=np.array([40.0 + y / sr.MPD for _, y in pts], np.float32),
                lon=np.array([x / ls for x, _ in pts], np.float32),
                time=np.arange(len(pts)) * 5.0, accuracy=np.full(len(pts), 5.0, np.float32))


def _hand(oracle, graph, batch, meili):
    orc = oracle.match_batch(oracle.Graph(graph), batch, p=oracle.params(**meili), keep_stages=True)
    st = sc.stages_of(batch, orc)
    rec = sc.scores(batch, st)
    stats = sc.check_f64(batch, st, rec, "hand", max_excl=0)           # hand graphs have none
    assert stats["excluded"] == 0 and stats["state_diff"] == 0
    return sr.Graph(graph), orc, st, rec


def test_single_column_chain_on_two_roads(two_roads, oracle):
    """One probe between two parallel roads, at d1 from the nearer and d2 from
    the farther: margin = (d2^2 - d1^2) / (2 sigma_z^2), the runner-up is the
    farther road."""
    graph, ls = two_roads
    meili = dict(search_radius=10.0, max_search_radius=10.0)
    batch = _probes(ls, [(130.0, 1.0)], [0, 1])                    # mid-edge: the rungs are 40 m away
    G, orc, st, rec = _hand(oracle, graph, batch, meili)
    r = rec[0]
    assert orc["ncand"][0] == 2 and r["ncand"] == 2
    assert r["flags"] == sc.SCORED | sc.CHAIN_START | sc.CHAIN_END
    # the f32 coordinates' own distances (a latitude near 40 is quantised to 0.42 m)
    plat = float(batch["lat"][0])
    d1 = abs(plat - float(G.node_lat[0])) * sr.MPD
    d2 = abs(float(G.node_lat[12]) - plat) * sr.MPD
    assert 0.5 < d1 < 1.5 and 3.5 < d2 < 4.5
    sz = sr.DEFAULTS["sigma_z"]
    e1, e2 = d1 * d1 / (2 * sz * sz), d2 * d2 / (2 * sz * sz)
    tol = sr.tol_emission(d1, e1, sz) + sr.tol_emission(d2, e2, sz) + sr.U * (e2 - e1)   # (+ the subtraction)
    assert abs(float(r["margin"]) - (e2 - e1)) <= tol, (r["margin"], e2 - e1, tol)
    assert abs(float(r["emission"]) - e1) <= sr.tol_emission(d1, e1, sz)
    assert r["cost"] == r["emission"] == r["chain_cost"] and r["transition"] == 0
    chosen = int(st["cand_edge"][int(r["state"])])
    assert G.eway[chosen] == 100 and G.eway[int(r["alt_edge"])] == 101 and r["alt"] == 1 - r["state"]
    assert r["alt_offset"] == st["cand_off"][int(r["alt"])]
    assert sc.fold_chain_costs(rec) == 1


def test_one_candidate_column_is_alone(two_roads, oracle):
    graph, ls = two_roads
    batch = _probes(ls, [(130.0, 1.0)], [0, 1])
    _, orc, _, rec = _hand(oracle, graph, batch, dict(search_radius=2.0, max_search_radius=2.0))
    r = rec[0]
    assert orc["ncand"][0] == 1
    assert r["flags"] == sc.SCORED | sc.CHAIN_START | sc.CHAIN_END | sc.ALONE
    assert np.isinf(r["margin"]) and r["margin"] > 0 and r["alt"] == -1 and r["alt_edge"] == -1
    assert r["alt_offset"] == 0 and r["ncand"] == 1 and r["state"] == 0


def test_two_column_chain_follows_its_four_transitions(two_roads, oracle):
    """Two probes 45 m apart along the southern road, both roads in reach of
    both: the through-costs are the minima over the four paths."""
    graph, ls = two_roads
    meili = dict(search_radius=10.0, max_search_radius=10.0)
    batch = _probes(ls, [(100.0, 1.0), (145.0, 1.5)], [0, 2])
    G, orc, st, rec = _hand(oracle, graph, batch, meili)
    assert list(orc["ncand"]) == [2, 2] and orc["col_prev"][1] == 0
    T = sc.block(st, 1).astype(np.float64)
    em = np.asarray(st["cand_emis"], np.float64)
    e0, e1 = em[0:2], em[sr.KMAX:sr.KMAX + 2]
    cost = e0[:, None] + T + e1[None, :]                            # the four paths
    assert np.isfinite(cost).sum() >= 2 and np.isfinite(T[0, 0]) and np.isfinite(T[1, 1])
    i, j = np.unravel_index(np.argmin(cost), cost.shape)
    assert (int(rec["state"][0]), int(rec["state"][1])) == (i, j)
    m0, m1 = cost.min(axis=1), cost.min(axis=0)
    tol = 2 * sc.tol_m(2, float(cost[np.isfinite(cost)].max()))
    for r, m, s in ((rec[0], m0, i), (rec[1], m1, j)):
        assert abs(float(r["cost"]) - cost[i, j]) <= tol
        if np.isfinite(m[1 - s]):
            assert abs(float(r["margin"]) - (m[1 - s] - m[s])) <= tol, (r["margin"], m)
            assert r["alt"] == 1 - s and not r["flags"] & sc.ALONE
        else:
            assert np.isinf(r["margin"]) and r["flags"] & sc.ALONE
    assert rec["flags"][0] & sc.CHAIN_START and rec["flags"][1] & sc.CHAIN_END
    assert not rec["flags"][0] & sc.CHAIN_END and not rec["flags"][1] & sc.CHAIN_START
    assert rec["transition"][1] == np.float32(T[i, j]) and rec["transition"][0] == 0
    assert sc.fold_chain_costs(rec) == 1


# ------------------------------------------------------------------ float32 against float64 on the oracle's stages
@pytest.mark.parametrize("name", CASES)
def test_float32_reference_against_float64(cases, oracle, name):
    graph, batch, meili, max_excl = cases[name]
    orc = oracle.match_batch(oracle.Graph(graph), batch, p=oracle.params(**meili), keep_stages=True)
    st = sc.stages_of(batch, orc)
    rec = sc.scores(batch, st)
    # what a case is there for, before anything is compared
    if name == "gaps_240s":
        assert ((rec["flags"] & sc.TIE) != 0).sum() >= 1 and (rec["margin"][(rec["flags"] & sc.TIE) != 0] == 0).all()
    if name == "radius_300":
        assert rec["ncand"].max() > 16
    if name == "long_140":
        assert len(batch["lat"]) > 128
    stats = sc.check_f64(batch, st, rec, name, max_excl=None if max_excl is None else 0)
    print(name, stats, "ties:", int(((rec["flags"] & sc.TIE) != 0).sum()))
    assert stats["scored"] > 0 and stats["state_diff"] == 0
    # the records without a score are all zero
    un = rec[(rec["flags"] & sc.SCORED) == 0]
    z = np.zeros(1, sc.DTYPE)
    z["alt"], z["alt_edge"] = -1, -1
    assert un.tobytes() == z.tobytes() * len(un)
    assert sc.fold_chain_costs(rec) >= 1
