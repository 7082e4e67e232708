"""Rule 7f without a device: the restatement of the matched
shape (tests/shape_ref.py) applied to the float64 route reference's records
(tests/traversals_ref.py on the oracle's stage arrays), and pinned by things it
did not compute itself:

 * every polyline decodes with the oracle's polyline6 decoder (itself pinned
   to tests/golden/decode_cases.json) to its vertices / 1e6;
 * every polyline is byte-equal to reporter_amd.tracegen.encode of the
   unquantised vertices;
 * every vertex lies within 0.5e-6 deg * 111319.4954833 m * sqrt(2) = 0.079 m
   (the quantisation's half step on both axes, nothing else) of its record's
   edge polyline (specref.foot_on_edge), and as close to the part of it between
   the record's two offsets;
 * the span invariants; on every TO_END record the last vertex is the quantised
   last shape point of the edge;
 * for a one-chain trace, tracegen.synthesize_gps(edges made of the spans, the
   polyline) returns the decoded vertices at the span ends;
 * the structs' sizes, the dtypes and the NULL-engine OTM_EINVAL of the five
   calls.

tests/test_gpu_shape.py compares k_shape with the same restatement on the
engine's own records, exactly.
"""
import ctypes as C
import math

import numpy as np
import pytest

import shape_cases
import shape_ref
import specref as sr
import specref_cases
import specref_checks as ck
import traversals_cases
import traversals_ref as tr
from reporter_amd import _lib, synth, tracegen

BOUND_M = 0.5e-6 * sr.MPD * math.sqrt(2.0)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("shape")
    out = specref_cases.build(d, synth)
    out.update(traversals_cases.build(d))
    out.update(shape_cases.build(d))
    return out


@pytest.fixture(scope="module")
def run(cases, oracle):
    """name -> (Graph, record arrays (edge, b, z, flags, trav_off), the shape), once per case."""
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
            recs = [r for rs in res.by_trace for r in rs]
            edge = np.array([r.edge for r in recs], np.int64)
            b = np.array([r.off0 for r in recs], np.float32)
            z = np.array([r.off1 for r in recs], np.float32)
            flags = np.array([r.flags for r in recs], np.uint32)
            toff = np.cumsum([0] + [len(rs) for rs in res.by_trace]).astype(np.int64)
            memo[name] = (G, (edge, b, z, flags, toff), shape_ref.reference(G, edge, b, z, flags, toff))
        return memo[name]
    return get


def _dist_to_part(G, e, b, z, lat, lon):
    """Metres from (lat, lon) to the part of edge e's polyline between offsets b and z."""
    s0 = int(G.eshape[e])
    ls = sr.MPD * math.cos(math.radians(lat))
    best = float("inf")
    for s in range(s0, int(G.eshape[e + 1]) - 1):
        c0, c1 = float(G.scum[s]), float(G.scum[s + 1])
        lo, hi = max(b, c0), min(z, c1)
        if lo > hi:
            continue
        t0, t1 = ((lo - c0) / (c1 - c0), (hi - c0) / (c1 - c0)) if c1 > c0 else (0.0, 0.0)
        pts = []
        for t in (t0, t1):
            pts.append(((G.slon[s] + t * (G.slon[s + 1] - G.slon[s]) - lon) * ls,
                        (G.slat[s] + t * (G.slat[s + 1] - G.slat[s]) - lat) * sr.MPD))
        (ax, ay), (bx, by) = pts
        vx, vy = bx - ax, by - ay
        l2 = vx * vx + vy * vy
        u = min(max(-(ax * vx + ay * vy) / l2, 0.0), 1.0) if l2 > 0 else 0.0
        best = min(best, math.hypot(ax + u * vx, ay + u * vy))
    return best


@pytest.mark.parametrize("name", shape_cases.ALL)
def test_reference_is_pinned(run, oracle, name):
    G, (edge, b, z, flags, toff), sh = run(name)
    shape_cases.assert_reached(name, G, edge, b, z, flags, toff, sh.spans, sh.vtx_off, sh.polylines)
    assert sh.vtx_off[-1] == len(sh.vertices) and len(sh.spans) == len(edge)
    worst = 0.0
    for t in range(len(toff) - 1):
        at = "%s trace %d" % (name, t)
        v = sh.vertices[sh.vtx_off[t]:sh.vtx_off[t + 1]]
        raw = sh.raw[sh.vtx_off[t]:sh.vtx_off[t + 1]]
        poly = sh.polylines[t]
        assert len(poly) == sh.poly_off[t + 1] - sh.poly_off[t] <= 12 * len(v), at
        # ---- the two decoders and the other encoder
        if len(v) == 0:
            assert poly == b"" and toff[t] == toff[t + 1], at
            continue
        dec = oracle.decode_polyline6(poly.decode("ascii"))              # [lon, lat]
        assert len(dec) == len(v), at
        assert [[lo, la] for la, lo in (v / 1e6).tolist()] == dec, at + " oracle decode"
        assert tracegen.encode([[lo, la] for la, lo in raw.tolist()]).encode("ascii") == poly, at + " tracegen.encode"
        # ---- the spans
        sp = sh.spans[toff[t]:toff[t + 1]]
        fl = flags[toff[t]:toff[t + 1]]
        assert (sp[:, 1] > sp[:, 0]).all() and sp[0, 0] == 0 and fl[0] & tr.CHAIN_START and sp[-1, 1] == len(v) - 1, at
        for k in range(1, len(sp)):
            assert sp[k, 0] == sp[k - 1, 1] + (1 if fl[k] & tr.CHAIN_START else 0), at + " span %d" % k
        # ---- every vertex on its record's edge, between the record's offsets
        for k in range(len(sp)):
            r = int(toff[t]) + k
            e, lo, hi = int(edge[r]), float(b[r]), float(z[r])
            for i in range(int(sp[k, 0]), int(sp[k, 1]) + 1):
                la, lon = v[i, 0] / 1e6, v[i, 1] / 1e6
                d = math.sqrt(sr.foot_on_edge(G, e, la, lon).sqd)
                dp = _dist_to_part(G, e, lo, hi, la, lon)
                worst = max(worst, d, dp)
                assert d <= BOUND_M and dp <= BOUND_M, "%s vertex %d: %.4f m / %.4f m from its edge" % (at, i, d, dp)
            if fl[k] & tr.TO_END:
                last = int(G.eshape[e + 1]) - 1
                assert (v[sp[k, 1]] == [shape_ref.quantise(G.slat[last]), shape_ref.quantise(G.slon[last])]).all(), at
    print("%s: %d vertices, %d bytes, farthest vertex %.4f m (bound %.4f)" % (
        name, len(sh.vertices), sh.poly_off[-1], worst, BOUND_M))


@pytest.mark.parametrize("name", ["hand_shape", "hand_shape_sw", "hand_long_edge", "city_5s"])
def test_spans_and_polyline_feed_synthesize_gps(run, name):
    """A batch's (spans, polyline) is an (edges, shape) argument of the reference's trace synthesis."""
    G, (edge, b, z, flags, toff), sh = run(name)
    done = 0
    for t in range(len(toff) - 1):
        fl = flags[toff[t]:toff[t + 1]]
        if len(fl) == 0 or ((fl & tr.CHAIN_START) != 0).sum() != 1:
            continue
        sp = sh.spans[toff[t]:toff[t + 1]]
        edges = [dict(length=float(z[r] - b[r]) / 1000.0, speed=40.0, begin_shape_index=int(sp[k, 0]),
                      end_shape_index=int(sp[k, 1])) for k, r in enumerate(range(int(toff[t]), int(toff[t + 1])))]
        got = tracegen.synthesize_gps(edges, sh.polylines[t].decode("ascii"), now=1507000000.0)
        dec = tracegen.decode(sh.polylines[t].decode("ascii"))          # [lon, lat]
        want = [dec[int(sp[0, 0])]] + [dec[int(e)] for e in sp[:, 1]]
        assert [[p["lon"], p["lat"]] for p in got["trace"]] == want
        v = sh.vertices[sh.vtx_off[t]:sh.vtx_off[t + 1]]
        assert [[float("%.6f" % (lo * 1e-6)), float("%.6f" % (la * 1e-6))] for la, lo in v.tolist()] == dec
        done += 1
    assert done >= 1


# ------------------------------------------------------------------ the structs and the calls that need no device
def test_struct_layout():
    assert _lib.SHAPE_VERTEX_DTYPE.itemsize == 8 and _lib.SHAPE_SPAN_DTYPE.itemsize == 8
    assert _lib.SHAPE_VERTEX_DTYPE.names == ("lat_e6", "lon_e6") and _lib.SHAPE_SPAN_DTYPE.names == (
        "begin_vertex", "end_vertex")
    assert all(_lib.SHAPE_VERTEX_DTYPE.fields[n][0] == np.dtype("<i4") for n in _lib.SHAPE_VERTEX_DTYPE.names)
    assert all(_lib.SHAPE_SPAN_DTYPE.fields[n][0] == np.dtype("<i4") for n in _lib.SHAPE_SPAN_DTYPE.names)
    assert C.sizeof(_lib.ShapeSizes) == 32 and C.sizeof(_lib.ShapeOut) == 72
    assert [n for n, _ in _lib.ShapeSizes._fields_] == ["n_traces", "n_traversals", "n_vertices", "n_bytes"]
    assert [getattr(_lib.ShapeOut, n).offset for n, _ in _lib.ShapeOut._fields_] == list(range(0, 72, 8))
    hdr = open(_lib.os.path.join(_lib._HERE, "..", "include", "otmatch.h")).read()
    for name in ("otm_shape_vertex", "otm_shape_span", "otm_shape_sizes", "otm_shape_out"):
        assert "typedef struct %s {" % name in hdr


def test_null_engine_is_einval():
    L = _lib.lib()
    on, z, dst = C.c_int(7), _lib.ShapeSizes(7, 7, 7, 7), _lib.ShapeOut()
    for rc in (L.otm_set_shape(None, 1), L.otm_shape_info(None, C.byref(on)), L.otm_shape_size(None, C.byref(z)),
               L.otm_fetch_shape(None, C.byref(dst)), L.otm_shape_device(None, C.byref(dst), C.byref(z))):
        assert rc == -1                                     # OTM_EINVAL
        assert "NULL" in _lib.last_error()
    assert on.value == 7 and (z.n_traces, z.n_traversals, z.n_vertices, z.n_bytes) == (7, 7, 7, 7)
    assert all(not getattr(dst, n) for n, _ in _lib.ShapeOut._fields_)
