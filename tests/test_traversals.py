"""Rule 7d without a device: the float64 reference of the
matched route (tests/traversals_ref.py) pinned to the CPU oracle -- its
traversals, regrouped by rule 7's join, are the oracle's segment records on
every case of tests/specref_cases.py and the two cases of
tests/traversals_cases.py; the ambiguity caps and what each case reaches,
asserted from the reference alone on the oracle's stage arrays; the record's
layout and the NULL-engine errors of the four calls; synth.route_agreement.

The caps (traversals_ref.assert_caps), asserted before anything is compared:
none on a hand graph; else at most 2 % of a case's traversal boundaries, and
with at least 100 boundaries inside steps with interpolated points also at
most 5 % of those.  An ambiguous boundary excludes its own time and shape
index only.  tests/test_gpu_traversals.py compares k_traversals' records with
the same reference on the engine's own stage arrays.
"""
import ctypes as C

import numpy as np
import pytest

import specref as sr
import specref_cases
import specref_checks as ck
import traversals_cases
import traversals_ref as tr
from reporter_amd import _lib, synth

CITY = ["city_5s", "city_30s", "gaps_240s", "radius_120", "radius_300", "dense_1s", "stop_and_go", "turn_factor_0",
        "accuracies", "long_140", "stop_80", "seg_forms"]
HANDS = ["hand_edge_cases", "hand_radius_0", "hand_star", "hand_short_edges", "hand_curve_interp", "hand_hairpin",
         "hand_filter", "hand_long_edge", "hand_many_short"]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("traversals")
    out = specref_cases.build(d, synth)
    out.update(traversals_cases.build(d))
    return out


@pytest.fixture(scope="module")
def run(cases, oracle):
    """name -> (Graph, batch, params, Impl of the oracle, the reference's Result), once per case."""
    memo = {}

    def get(name):
        if name not in memo:
            graph, batch, meili, max_excl = cases[name]
            orc = oracle.match_batch(oracle.Graph(graph), batch, p=oracle.params(**meili), keep_stages=True)
            G, P = sr.Graph(graph), sr.params(**meili)
            impl = ck.Impl.from_oracle(orc, len(batch["lat"]))
            chains = ck.check_viterbi(batch, impl, max_excl)
            res = tr.reference(G, P, batch, [[ch.cols for ch in chs] for chs in chains], impl.state, impl.cand_edge,
                               impl.cand_off, impl.ipos, impl.traces["code"])
            memo[name] = (G, batch, P, impl, res)
        return memo[name]
    return get


@pytest.mark.parametrize("name", CITY + HANDS)
def test_reference_regrouped_is_the_oracle(run, name):
    G, batch, _, impl, res = run(name)
    print("%s: %d traversals, %d boundaries, %d inside steps with interpolated points, %d ambiguous" % (
        name, res.trav, res.bounds, res.inside, res.amb))
    tr.assert_caps(res, name in HANDS, name)
    off = batch["trace_off"]
    for t, recs in enumerate(res.by_trace):
        if impl.traces[t]["code"] != 200:
            assert impl.traces[t]["seg_cnt"] == 0 and not recs
            continue
        ck._compare_segments(G, impl, t, int(off[t]), tr.segments_of(G, recs), "traversals regrouped")
        # rule 7d's consequences, in the reference itself
        for a, b in zip(recs, recs[1:]):
            if b.flags & tr.CHAIN_START:
                assert a.flags & tr.CHAIN_END
                continue
            assert G.eto[a.edge] == G.efrom[b.edge] and b.off0 == 0.0 and a.off1 == float(G.elen[a.edge])
            if a.end[:2] != b.begin[:2]:
                # the one place where the two sides are not one boundary of one step: a state on a node
                # candidate (its own traversal is not emitted).  The step before ends there at its R, the
                # step after starts there at 0, where interpolated points standing on the node (position
                # 0) are anchors, and a step of R = 0 names its end point: the vehicle waits on the node
                lo, hi = int(off[t]) + a.end[1], int(off[t]) + b.begin[1]
                assert lo < hi
                for p in range(lo, hi):                                  # every state from lo to before hi: on the node
                    assert impl.state[p] < 0 or float(impl.cand_off[p * sr.KMAX + int(impl.state[p])]) == 0.0
                assert a.end[0] == batch["time"][lo] <= b.begin[0] <= batch["time"][hi]


def test_cases_reach_their_targets(run):
    """No case goes empty: the compared boundaries inside steps with interpolated points."""
    assert run("stop_and_go")[4].compared_inside >= 200
    assert run("seg_forms")[4].compared_inside >= 180
    assert run("hand_short_edges")[4].compared_inside == 29


def test_hand_long_edge(run):
    G, batch, _, _, res = run("hand_long_edge")
    ids = traversals_cases.IDS["hand_long_edge"]
    assert res.amb == 0
    a, b = res.by_trace
    assert [r.edge for r in a] == [ids["a"], ids["L"], ids["c"]] and [r.edge for r in b] == [ids["a"], ids["L"]]
    # the traversal of L is opened at point 1 and closed past point 64: more than one chunk of the kernel's walk
    assert a[1].begin[1] <= 1 and a[1].end[1] >= 70 and a[1].flags & tr.TO_END
    assert len(batch["lat"]) == 2 * (traversals_cases.LONG_STATES + 2)
    # trace 1 ends on L after a backward stay: at the largest offset reached, not the last state's
    far = (65.0 + traversals_cases.LONG_GAP * (traversals_cases.LONG_STATES - 1)) - 60.0
    assert abs(b[1].off1 - far) < 0.01 and b[1].flags & tr.CHAIN_END and not b[1].flags & tr.TO_END
    assert b[1].end[1] == traversals_cases.LONG_STATES + 1 and b[1].begin[1] <= 1


def test_hand_many_short(run):
    G, _, _, _, res = run("hand_many_short")
    ids = traversals_cases.IDS["hand_many_short"]
    assert res.amb == 0
    want = [ids["a"]] + [ids["s%d" % k] for k in range(traversals_cases.N_SHORT)] + [ids["b"]]
    for recs in res.by_trace:
        assert [r.edge for r in recs] == want                   # one step, a path of 100 edges
        # a, 13 segments of four, 12 x (plain, internal pair, plain), b
        assert recs[-1].segment == 1 + 13 + 12 * 3
        assert sum(1 for r in recs if r.flags & tr.INTERNAL) == 24
    inside = [bd for r in res.by_trace[1] for bd in (r.begin, r.end) if bd[4]]
    assert len(inside) >= 200 and all(bd[2] for bd in inside)   # the copy with interpolated points inside the step
    assert not [bd for r in res.by_trace[0] for bd in (r.begin, r.end) if bd[4]]
    # ... whose boundaries name the interpolated points: more than the step's two states
    assert len(set(bd[1] for r in res.by_trace[1] for bd in (r.begin, r.end))) > 3
    assert len(set(bd[1] for r in res.by_trace[0] for bd in (r.begin, r.end))) == 2


def test_seg_forms_holds_253_traversals_in_128_points(run):
    _, batch, _, _, res = run("seg_forms")
    assert np.diff(batch["trace_off"])[5] <= 128 and len(res.by_trace[5]) == 253


# ------------------------------------------------------------------ the record and the calls that need no device
def test_record_layout():
    assert C.sizeof(_lib.Traversal) == 56 and C.alignment(_lib.Traversal) == 8
    want = dict(edge=0, flags=4, begin_offset=8, end_offset=12, enter_time=16, exit_time=24, begin_shape_index=32,
                end_shape_index=36, segment=40, pad=44, way_id=48)
    assert {n: getattr(_lib.Traversal, n).offset for n, _ in _lib.Traversal._fields_} == want
    assert _lib.TRAVERSAL_DTYPE.itemsize == 56
    assert {n: _lib.TRAVERSAL_DTYPE.fields[n][1] for n in _lib.TRAVERSAL_DTYPE.names} == want
    for n, t in _lib.Traversal._fields_:
        assert getattr(_lib.Traversal, n).offset % C.sizeof(t) == 0             # natural alignment
        assert _lib.TRAVERSAL_DTYPE.fields[n][0].itemsize == C.sizeof(t)
    assert (_lib.TV_CHAIN_START, _lib.TV_CHAIN_END, _lib.TV_FROM_START, _lib.TV_TO_END, _lib.TV_INTERNAL,
            _lib.TV_SEGMENT_FIRST) == (1, 2, 4, 8, 16, 32) == (tr.CHAIN_START, tr.CHAIN_END, tr.FROM_START, tr.TO_END,
                                                               tr.INTERNAL, tr.SEGMENT_FIRST)
    hdr = open(_lib.os.path.join(_lib._HERE, "..", "include", "otmatch.h")).read()
    for name, v in (("CHAIN_START", 1), ("CHAIN_END", 2), ("FROM_START", 4), ("TO_END", 8), ("INTERNAL", 16),
                    ("SEGMENT_FIRST", 32)):
        assert "#define OTM_TV_%s %du" % (name, v) in hdr


def test_null_engine_is_einval():
    L = _lib.lib()
    on, n, p, o = C.c_int(7), C.c_int64(7), C.c_void_p(), C.c_void_p()
    buf = np.zeros(2, _lib.TRAVERSAL_DTYPE)
    off = np.full(3, 7, np.int64)
    for rc in (L.otm_set_traversals(None, 1), L.otm_traversals_info(None, C.byref(on)),
               L.otm_fetch_traversals(None, buf.ctypes.data, 2, off.ctypes.data, C.byref(n)),
               L.otm_fetch_traversals(None, None, 0, None, C.byref(n)),
               L.otm_traversals_device(None, C.byref(p), C.byref(o), C.byref(n)),
               L.otm_traversals_size(None, C.byref(n), C.byref(n))):
        assert rc == -1                                     # OTM_EINVAL
        assert "NULL" in _lib.last_error()
    assert (on.value, n.value, p.value, o.value) == (7, 7, None, None) and not buf["flags"].any() and (off == 7).all()


# ------------------------------------------------------------------ synth.route_agreement
def _records(seqs):
    off = np.cumsum([0] + [len(s) for s in seqs]).astype(np.int64)
    recs = np.zeros(int(off[-1]), _lib.TRAVERSAL_DTYPE)
    recs["edge"] = [e for s in seqs for e in s]
    return recs, off


def test_route_agreement():
    truth = [[1, 2, 3, 4], [5, 6, 7], [8, 9, 10], [11, 12]]
    toff = np.cumsum([0] + [len(s) for s in truth]).astype(np.int64)
    tedges = np.array([e for s in truth for e in s], np.int32)
    # equal; one inserted; one dropped; empty
    recs, off = _records([[1, 2, 3, 4], [5, 6, 99, 7], [8, 10], []])
    c = synth.route_agreement(toff, tedges, recs, off)
    assert c["traces"] == 4 and c["truth"] == 12 and c["matched"] == 10
    assert c["paired"] == 4 + 3 + 2 + 0 and c["missed"] == 3 and c["extra"] == 1
    assert c["exact"] == 1 and c["empty"] == 1
    assert c["recall"] == 9 / 12 and c["precision"] == 9 / 10
    # a chain break re-enters its edge: the repeat is folded
    recs, off = _records([[1, 2, 2, 3, 4]])
    c = synth.route_agreement(toff[:2], tedges, recs, off)
    assert c["exact"] == 1 and c["matched"] == 4
    # nothing matched at all
    c = synth.route_agreement(toff, tedges, np.zeros(0, _lib.TRAVERSAL_DTYPE), np.zeros(5, np.int64))
    assert c["paired"] == 0 and c["precision"] == 1.0 and c["recall"] == 0.0 and c["empty"] == 4
