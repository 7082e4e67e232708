"""Rule 7g without a device.

 * The formatter pinned: otm_debug_attr_fixed, the host face of
   reporter_amd/csrc/attrfmt.h, against attributes_ref.fixed on 200k+ doubles.
 * The restatement (tests/attributes_ref.py) on reference records: matched
   points (points_ref), scores (score_ref), traversals (traversals_ref) and the
   shape (shape_ref) made from the oracle's stage arrays.  Every body parses,
   its integers are the records', its F3 / F6 numbers lie within half a unit of
   the last place of the record's number (plus the one rounding of the product
   x * 10^d, at most 2^-53 |x|: the text rounds that product, not x), and the
   shape string decodes to the vertices.
 * The calls' argument errors that need no device.
 * tests/native/attrfmt_main.cpp built with -fsanitize=address,undefined and
   run as a program: the edge values again, and the longest objects in buffers
   of exactly their documented maxima.

tests/test_gpu_attributes.py compares the GPU's bytes with the same
restatement on the engine's own records, exactly.
"""
import ctypes as C
import json
import os
import shutil
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import attributes_ref as ar
import points_ref as pr
import score_ref as sc
import shape_cases
import shape_ref
import specref as sr
import specref_cases
import specref_checks as ck
import traversals_cases
import traversals_ref as tr
from reporter_amd import _lib, synth, tracegen

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


# ------------------------------------------------------------------ the formatter
def _doubles():
    rng = np.random.default_rng(7)
    with np.errstate(invalid="ignore"):             # (signalling NaNs among the f32 patterns)
        f32 = rng.integers(0, 1 << 32, 40000, dtype=np.uint64).astype(np.uint32).view(np.float32).astype(np.float64)
    parts = [
        rng.integers(0, 1 << 64, 60000, dtype=np.uint64).view(np.float64),              # random bit patterns
        f32,                                                                            # f32 patterns, widened
        (rng.standard_normal(20000) * 1000.0).astype(np.float32).astype(np.float64),    # f32 widened, metres
        rng.uniform(-0.001, 0.0, 10000),                                                # negatives in (-0.001, 0)
        rng.uniform(-0.000001, 0.0, 5000),
        1.5e9 + rng.uniform(0, 1e8, 20000),                                             # epoch times
        np.round(1.5e9 + rng.uniform(0, 1e8, 5000)),
        rng.uniform(-180.0, 180.0, 10000),                                              # degrees
    ]
    # within one ulp of k + 0.5 units of the last place, both scales and both signs
    k = rng.integers(0, 1 << 40, 5000).astype(np.float64)
    for p in (1000.0, 1e6):
        m = (k + 0.5) / p
        for v in (np.nextafter(m, -np.inf), m, np.nextafter(m, np.inf)):
            parts += [v, -v]
    # 2^53 / 10^d and its neighbours
    edge = []
    for p in (1000.0, 1e6):
        v = np.float64(2.0 ** 53) / p
        for _ in range(8):
            v = np.nextafter(v, 0.0)
        for _ in range(17):
            edge += [v, -v]
            v = np.nextafter(v, np.inf)
    parts.append(np.array(edge + [0.0, -0.0, np.nan, np.inf, -np.inf, 12.0, -0.0004, -0.0015, 5e-324, 1e300, -1e300]))
    return np.concatenate(parts)


def test_fixed_against_the_restatement():
    L = _lib.lib()
    xs = _doubles()
    assert len(xs) >= 200000
    buf = C.create_string_buffer(32)
    nulls = negzero = 0
    for x in xs.tolist():
        for d in (3, 6):
            n = L.otm_debug_attr_fixed(x, d, buf)
            want = ar.fixed(x, d)
            assert buf.value.decode("ascii") == want and n == len(want), (x.hex(), d, buf.value, want)
            nulls += want == "null"
            negzero += x < 0 and not want.startswith("-")
    assert nulls > 1000 and negzero > 1000
    # the issue's own examples
    assert [ar.f3(x) for x in (-0.0004, -0.0015, 12)] == ["0.000", "-0.002", "12.000"]
    assert ar.f6(float("inf")) == ar.f3(float("nan")) == "null"


def test_argument_errors():
    L = _lib.lib()
    buf = C.create_string_buffer(32)
    for rc in (L.otm_debug_attr_fixed(1.0, 4, buf), L.otm_debug_attr_fixed(1.0, 3, None)):
        assert rc == -1 and "decimals" in _lib.last_error()
    m, a, b, p, q = C.c_uint32(7), C.c_int64(7), C.c_int64(7), C.c_void_p(), C.c_void_p()
    for rc in (L.otm_set_attributes(None, 15), L.otm_attributes_info(None, C.byref(m)),
               L.otm_attributes_size(None, C.byref(a), C.byref(b)),
               L.otm_fetch_attributes(None, None, 0, None, C.byref(a)),
               L.otm_attributes_device(None, C.byref(p), C.byref(q), C.byref(a), C.byref(b))):
        assert rc == -1 and "NULL" in _lib.last_error()
    assert (m.value, a.value, b.value, p.value, q.value) == (7, 7, 7, None, None)
    # a bad mask is refused before the handle is looked at, so it needs no device
    for bad in ar.INVALID_MASKS:
        assert L.otm_set_attributes(None, bad) == -1 and "trace attributes" in _lib.last_error(), bad
    assert "above" in _lib.last_error() and L.otm_set_attributes(None, 2) == -1 and "needs" in _lib.last_error()
    for ok in [0] + ar.VALID_MASKS:
        assert L.otm_set_attributes(None, ok) == -1 and "engine is NULL" in _lib.last_error(), ok
    assert (_lib.ATTR_POINTS, _lib.ATTR_SCORES, _lib.ATTR_EDGES, _lib.ATTR_SHAPE, _lib.ATTR_ALL) == (1, 2, 4, 8, 15)
    hdr = open(os.path.join(ROOT, "include", "otmatch.h")).read()
    for name, v in (("POINTS", 1), ("SCORES", 2), ("EDGES", 4), ("SHAPE", 8), ("ALL", 15)):
        assert "#define OTM_ATTR_%s %du" % (name, v) in hdr
    assert ar.VALID_MASKS == [1, 3, 4, 5, 7, 8, 9, 11, 12, 13, 15]


# ------------------------------------------------------------------ the stand-alone sanitizer program
def test_formatter_under_sanitizers(tmp_path):
    gxx = shutil.which("g++") or shutil.which("clang++")
    assert gxx, "no C++ compiler found"
    exe = str(tmp_path / "attrfmt_main")
    # the sanitizer runtimes linked into the program itself (tests/test_flush_host.py): it runs as it
    # stands, in the environment the test inherits, with only the sanitizers' options added
    static = ["-static-libsan"] if "clang" in os.path.basename(gxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.run([gxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] + static + [
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "reporter_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "attrfmt_main.cpp"), "-o", exe], check=True)
    env = dict(os.environ)
    env.update(ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and not r.stderr, r.stderr
    lines = r.stdout.splitlines()
    assert "MISMATCH" not in r.stdout
    seen = 0
    for ln in lines:
        w = ln.split(" ")
        if w[0] in ("MP", "E"):
            assert int(w[1]) == int(w[2]) == len(w[3]) == (493 if w[0] == "MP" else 332), ln   # the maxima, reached
            json.loads(w[3])
            continue
        x = struct.unpack("<d", struct.pack("<Q", int(w[0], 16)))[0]
        assert w[2] == ar.fixed(x, int(w[1])), ln
        seen += 1
    assert seen >= 2 * 100 and sum(1 for ln in lines if ln[:2] in ("MP", "E ")) == 2


# ------------------------------------------------------------------ the restatement on reference records
@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("attributes")
    out = specref_cases.build(d, synth)
    out.update(traversals_cases.build(d))
    out.update(shape_cases.build(d))
    return out


def _reference_records(cases, oracle, name):
    """The four outputs' records of a case, from the oracle's stage arrays by the four references."""
    graph, batch, meili, max_excl = cases[name]
    orc = oracle.match_batch(oracle.Graph(graph), batch, p=oracle.params(**meili), keep_stages=True)
    G, P = sr.Graph(graph), sr.params(**meili)
    codes = orc["traces"]["code"]
    n = len(batch["lat"])
    # matched points (tests/test_points.py)
    st = pr.oracle_stages(batch, orc)
    pp = pr.matched_points(G, P, batch, st, codes)
    pts = np.zeros(n, _lib.POINT_DTYPE)
    pts["edge"], pts["flags"], pts["way_id"] = pp.edge, pp.flags, pp.way
    for k in np.nonzero(pp.flags & 1)[0]:
        off = np.float32(pp.off[k])
        la, lo, dist = pr.coordinate(G, int(pp.edge[k]), float(off), float(np.float32(batch["lat"][k])),
                                     float(np.float32(batch["lon"][k])))
        pts["offset"][k], pts["lat"][k], pts["lon"][k], pts["distance"][k] = off, la, lo, dist
    # scores (tests/test_scores.py)
    scr = sc.scores(batch, sc.stages_of(batch, orc), codes)
    # traversals (tests/test_traversals.py) and the shape (tests/test_shape.py)
    impl = ck.Impl.from_oracle(orc, n)
    chains = ck.check_viterbi(batch, impl, max_excl)
    res = tr.reference(G, P, batch, [[ch.cols for ch in chs] for chs in chains], impl.state, impl.cand_edge,
                       impl.cand_off, impl.ipos, impl.traces["code"])
    recs = [r for rs in res.by_trace for r in rs]
    tv = np.zeros(len(recs), _lib.TRAVERSAL_DTYPE)
    for k, r in enumerate(recs):
        tv[k] = (r.edge, r.flags, r.off0, r.off1, r.begin[0], r.end[0], r.begin[1], r.end[1], r.segment, 0, r.way_id)
    toff = np.cumsum([0] + [len(rs) for rs in res.by_trace]).astype(np.int64)
    sh = shape_ref.reference(G, tv["edge"].astype(np.int64), tv["begin_offset"], tv["end_offset"], tv["flags"], toff)
    spans = np.zeros(len(recs), _lib.SHAPE_SPAN_DTYPE)
    if len(recs):
        spans["begin_vertex"], spans["end_vertex"] = sh.spans[:, 0], sh.spans[:, 1]
    return batch, pts, scr, tv, toff, spans, sh


def _near(text, x, d, what):
    """A parsed F3 / F6 number (a Fraction, or None for null) against the record's number."""
    x = float(x)
    if text is None:
        assert not abs(x * 10.0 ** d) < 2.0 ** 53, what
        return
    bound = Fraction(1, 2 * 10 ** d) + abs(Fraction(x)) / 2 ** 53
    assert abs(text - Fraction(x)) <= bound, (what, str(text), x)


@pytest.mark.parametrize("name", ["hand_shape", "stop_and_go", "gaps_240s", "seg_forms"])
def test_restatement_on_reference_records(cases, oracle, name):
    batch, pts, scr, tv, toff, spans, sh = _reference_records(cases, oracle, name)
    poly = b"".join(sh.polylines)
    off = np.asarray(batch["trace_off"], np.int64)
    bods = ar.bodies(ar.ALL, off, pts, scr, tv, toff, spans, poly, sh.poly_off)
    assert len(bods) == len(off) - 1
    kinds, scored, nulls = set(), 0, 0
    for t, body in enumerate(bods):
        assert " " not in body and "\n" not in body
        doc = json.loads(body, parse_float=Fraction)
        assert list(doc) == ["matched_points", "edges", "shape"]
        mps, es = doc["matched_points"], doc["edges"]
        assert len(mps) == off[t + 1] - off[t] and len(es) == toff[t + 1] - toff[t]
        for k, mp in zip(range(int(off[t]), int(off[t + 1])), mps):
            p, s, at = pts[k], scr[k], "%s point %d" % (name, k)
            kinds.add(mp["type"])
            assert mp["flags"] == int(p["flags"])
            if mp["type"] == "unmatched":
                assert not int(p["flags"]) & 1 and set(mp) <= {"type", "flags", "score"}
            else:
                assert mp["type"] == ("matched" if int(p["flags"]) & 2 else "interpolated") and int(p["flags"]) & 1
                assert (mp["edge_id"], mp["way_id"]) == (int(p["edge"]), int(p["way_id"])), at
                _near(mp["lat"], p["lat"], 6, at)
                _near(mp["lon"], p["lon"], 6, at)
                _near(mp["distance_along_edge"], p["offset"], 3, at)
                _near(mp["distance_from_trace_point"], p["distance"], 3, at)
            assert ("score" in mp) == bool(int(s["flags"]) & 1), at
            if "score" in mp:
                g = mp["score"]
                scored += 1
                nulls += g["margin"] is None
                assert (g["ncand"], g["state"], g["alt"], g["alt_edge"], g["flags"]) == (
                    int(s["ncand"]), int(s["state"]), int(s["alt"]), int(s["alt_edge"]), int(s["flags"])), at
                assert (g["margin"] is None) == bool(int(s["flags"]) & sc.ALONE), at
                for key in ("cost", "margin", "chain_cost", "emission", "transition"):
                    _near(g[key], s[key], 6, at + " " + key)
                _near(g["alt_offset"], s["alt_offset"], 3, at)
        for k, e in zip(range(int(toff[t]), int(toff[t + 1])), es):
            r, at = tv[k], "%s traversal %d" % (name, k)
            assert list(e) == ["id", "way_id", "begin_offset", "end_offset", "enter_time", "exit_time",
                               "begin_shape_index", "end_shape_index", "segment", "begin_vertex", "end_vertex", "flags"]
            assert (e["id"], e["way_id"], e["begin_shape_index"], e["end_shape_index"], e["segment"], e["flags"]) == (
                int(r["edge"]), int(r["way_id"]), int(r["begin_shape_index"]), int(r["end_shape_index"]),
                int(r["segment"]), int(r["flags"])), at
            assert (e["begin_vertex"], e["end_vertex"]) == (int(spans[k]["begin_vertex"]), int(spans[k]["end_vertex"]))
            for key in ("begin_offset", "end_offset", "enter_time", "exit_time"):
                _near(e[key], r[key], 3, at + " " + key)
        v = sh.vertices[sh.vtx_off[t]:sh.vtx_off[t + 1]]
        assert doc["shape"].encode("ascii") == sh.polylines[t]              # (json.loads undid the escapes)
        assert tracegen.decode(doc["shape"]) == [[float("%.6f" % (lo * 1e-6)), float("%.6f" % (la * 1e-6))]
                                                 for la, lo in v.tolist()]
    assert "matched" in kinds and scored > 0
    if name in ("stop_and_go", "seg_forms"):
        assert "interpolated" in kinds              # the copies of a standing point
    # a section that is off is absent with its comma; SHAPE without EDGES keeps the string
    for mask in ar.VALID_MASKS:
        some = ar.bodies(mask, off, pts, scr, tv, toff, spans, poly, sh.poly_off)
        for t in (0, len(off) - 2):
            doc = json.loads(some[t])
            assert list(doc) == [k for k, b in (("matched_points", 1), ("edges", 4), ("shape", 8)) if mask & b]
            if mask & 8:
                assert doc["shape"].encode("ascii") == sh.polylines[t]
            if mask & 4 and len(doc["edges"]):
                assert ("begin_vertex" in doc["edges"][0]) == bool(mask & 8)
            if mask & 1 and len(doc["matched_points"]):
                assert any("score" in mp for mp in doc["matched_points"]) <= bool(mask & 2)
    print(name, "bodies:", len(bods), "bytes:", sum(map(len, bods)), "scored:", scored, "null margins:", nulls)
