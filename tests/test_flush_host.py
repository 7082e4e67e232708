"""The datastore flush body written by libotmatch's host writer
(otm_flush_body_host, reporter_amd/csrc/flush_host.cpp), byte for byte against
datastore.serialize(datastore.flush_records(...)) on the same numbers.  No GPU:
the writer has no HIP call, and a stand-alone program built from it
(tests/native/flush_host_main.c) runs under ASan + UBSan, their runtimes linked
into the program."""
import ctypes as C
import json
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import flush_cases as fc
from reporter_amd import _lib, datastore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reporter_amd", "csrc")

N_SEGMENTS = (1, 63, 64, 65, 257)
NBINS = (1, 4, 16, 17, 40)
WORLDS = (1, 2, 3, 7)
BIN_KPH = (10.0, 2.5, 0.1)
KINDS = ("random", "row0", "last", "dense", "empty", "padding", "special")


def test_bin_kph_is_the_float32_value():
    c, s = fc.window("row0", 1, 1, 1)
    body, _ = datastore.flush_body_host(c, s, fc.make_ids(1), 0, 1, 1, 0.1)
    assert body.startswith(b'{"mode":"auto","bin_kph":0.10000000149011612,"rank":0,"world":1,"segments":[{"id":0,')


@pytest.mark.parametrize("nbins", NBINS)
@pytest.mark.parametrize("world", WORLDS)
def test_host_writer_matrix(nbins, world):
    n = 0
    for nseg in N_SEGMENTS:
        ids = fc.make_ids(nseg)
        for ki, kind in enumerate(KINDS):
            c, s = fc.window(kind, nseg, nbins, world, seed=ki)
            bin_kph = BIN_KPH[(ki + nseg) % 3]
            for rank in range(world):
                cr, sr = fc.slice_of(c, s, rank, world)
                want, nrec = fc.reference(cr, sr, ids, rank, world, nbins, bin_kph)
                got, got_n = datastore.flush_body_host(cr, sr, ids, rank, world, nbins, bin_kph)
                assert got == want, (nseg, kind, rank)
                assert got_n == nrec
                n += nrec
    assert n > 0


@pytest.mark.parametrize("bin_kph", BIN_KPH)
def test_every_bin_width_over_a_dense_window(bin_kph):
    ids = fc.make_ids(65)
    for kind in ("dense", "special", "empty"):
        c, s = fc.window(kind, 65, 16, 2)
        for rank in range(2):
            cr, sr = fc.slice_of(c, s, rank, 2)
            want, nrec = fc.reference(cr, sr, ids, rank, 2, 16, bin_kph)
            assert datastore.flush_body_host(cr, sr, ids, rank, 2, 16, bin_kph) == (want, nrec)


def test_special_values_appear_as_written():
    """What the special rows are there for, checked on the reference itself
    too: 0.0, the count past 2^32, ids at both ends of u64."""
    ids = fc.make_ids(257)
    c, s = fc.window("special", 257, 16, 1)
    body, nrec = datastore.flush_body_host(c, s, ids, 0, 1, 16, 10.0)
    assert (body, nrec) == fc.reference(c, s, ids, 0, 1, 16, 10.0)
    segs = json.loads(body)["segments"]
    assert len(segs) == nrec > 20
    assert {0, 2 ** 63 - 1, 2 ** 63 + 12345} <= {int(i) for i in ids}
    assert b'"speed_sum_kph":0.0,' in body and b'"speed_sum_kph":0.001,' in body
    assert b'"speed_sum_kph":123456.789,' in body and b'"speed_sum_kph":4611686018427388.0,' in body
    assert max(g["count"] for g in segs) == 3 * fc.BIG_BIN > 2 ** 32
    assert [g["id"] for g in segs] == [int(ids[r]) for r in range(257) if c[r].sum() > 0]


def _one_row(v):
    c = np.zeros((1, 4), np.int64)
    c[0, 2] = 3
    ids = np.array([2 ** 64 - 1], np.uint64)
    got, nrec = datastore.flush_body_host(c, np.array([v], np.uint64), ids, 0, 1, 4, 2.5)
    rec = datastore.flush_records(c.reshape(-1), np.zeros(1, np.int64), ids, 0, 1, 4, 2.5)
    rec["segments"][0]["speed_sum_kph"] = v / 1000.0  # (flush_records' int64 cast stops at 2^63 - 1)
    return got, nrec, datastore.serialize(rec)


@pytest.mark.parametrize("v", [2 ** 64 - 1000, 2 ** 64 - 1, 2 ** 63, 10 ** 19, 10 ** 19 - 1, 2 ** 53 + 1])
def test_sums_past_int64_against_repr(v):
    got, nrec, want = _one_row(v)
    assert got == want and nrec == 1
    assert ('"speed_sum_kph":%s,' % repr(v / 1000.0)).encode() in got
    if v == 2 ** 64 - 1000:
        # repr's exponent form from 1e16 up: the double is 2^64 / 1000 =
        # 18446744073709552.0, whose shortest digits that read back are these 16
        assert repr(v / 1000.0) == "1.844674407370955e+16" and float("1.844674407370955e+16") == 18446744073709552.0
        assert b'"speed_sum_kph":1.844674407370955e+16,' in got


def test_n_records_and_nul_terminator():
    ids = fc.make_ids(65)
    c, s = fc.window("dense", 65, 4, 1)
    c32 = np.ascontiguousarray(c.reshape(-1).astype(np.uint32))
    out, n, nrec = C.c_void_p(), C.c_size_t(), C.c_int64()
    L = _lib.lib()
    assert L.otm_flush_body_host(c32.ctypes.data, s.ctypes.data, ids.ctypes.data, 65, 65, 4, 10.0, 0, 1, C.byref(out),
                                 C.byref(n), C.byref(nrec)) == 0
    raw = C.string_at(out, n.value + 1)
    L.otm_free(out)
    assert nrec.value == 65 and raw[-1:] == b"\0" and b"\0" not in raw[:-1]
    assert raw[:-1] == fc.reference(c, s, ids, 0, 1, 4, 10.0)[0]
    # n_records may be NULL
    assert L.otm_flush_body_host(c32.ctypes.data, s.ctypes.data, ids.ctypes.data, 65, 65, 4, 10.0, 0, 1, C.byref(out),
                                 C.byref(n), None) == 0
    L.otm_free(out)


def test_argument_errors():
    L = _lib.lib()
    ids = fc.make_ids(4)
    c = np.ones(16, np.uint32)
    s = np.ones(4, np.uint64)
    out, n, nrec = C.c_void_p(), C.c_size_t(), C.c_int64()

    def call(counts=c.ctypes.data, sums=s.ctypes.data, idp=ids.ctypes.data, nbins=4, kph=10.0, rank=0, world=1,
             body=C.byref(out), blen=C.byref(n)):
        rc = L.otm_flush_body_host(counts, sums, idp, 4, 4 // world if world > 0 else 4, nbins, kph, rank, world, body,
                                   blen, C.byref(nrec))
        return rc, _lib.last_error()

    assert call()[0] == 0
    L.otm_free(out)
    for kw in (dict(counts=None), dict(sums=None), dict(idp=None), dict(body=None), dict(blen=None), dict(nbins=0),
               dict(world=0), dict(rank=1, world=1), dict(rank=2, world=2), dict(rank=-1), dict(kph=0.0)):
        L.otm_flush_body_host(c.ctypes.data, s.ctypes.data, ids.ctypes.data, 4, 4, 4, 10.0, 0, 1, C.byref(out),
                              C.byref(n), None)  # (a success in between: the message below is this call's)
        L.otm_free(out)
        rc, msg = call(**kw)
        assert rc == -1, kw  # OTM_EINVAL
        assert msg and ("NULL" in msg or "nbins" in msg or "world" in msg), (kw, msg)


def _compiler():
    """A C++ compiler with the ASan and UBSan runtimes: g++, or the clang that
    builds the library."""
    for cxx in (shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and os.path.exists(cxx):
            return cxx
    return None


def _write_case(path, c, s, ids, nseg, rank, world, nbins, bin_kph):
    rows = len(s)
    with open(path, "wb") as f:
        f.write(struct.pack("<5q", nseg, rows, nbins, rank, world))
        f.write(struct.pack("<2f", bin_kph, 0.0))
        f.write(np.asarray(ids, np.uint64).tobytes())
        f.write(np.asarray(c, np.int64).reshape(-1).astype(np.uint32).tobytes())
        f.write(np.asarray(s, np.uint64).tobytes())


def test_standalone_program_under_asan_and_ubsan(tmp_path):
    cxx = _compiler()
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path / "flush_host_main")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    inc = ["-I", CSRC, "-I", os.path.join(ROOT, "include")]
    objs = []
    for src, lang in ((os.path.join(CSRC, "flush_host.cpp"), ["-std=c++17"]), (os.path.join(CSRC, "json.cpp"), ["-std=c++17"]),
                      (os.path.join(ROOT, "tests", "native", "flush_host_main.c"), ["-x", "c"])):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        subprocess.check_call([cxx] + lang + san + inc + ["-c", src, "-o", obj])
        objs.append(obj)
    # the sanitizer runtimes linked into the program itself (g++'s default is
    # the shared one): the program runs as it stands, in the environment the
    # test inherits, with only the sanitizers' options added
    static = ["-static-libsan"] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    subprocess.check_call([cxx] + san + static + objs + ["-o", exe])
    syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
    assert "__asan_" in syms and "__ubsan_" in syms
    assert not re.search(r"\ship[A-Z_]", syms)  # nothing of HIP is linked
    needed = subprocess.run(["readelf", "-d", exe], capture_output=True, text=True).stdout
    assert "asan" not in needed and "ubsan" not in needed, needed
    env = dict(os.environ)
    env.update(ASAN_OPTIONS="halt_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    cases = []
    ids = fc.make_ids(257)
    for kind, nbins, world in (("empty", 16, 1), ("dense", 16, 1), ("dense", 17, 3), ("special", 40, 7), ("padding", 4, 7)):
        c, s = fc.window(kind, 257, nbins, world)
        for rank in sorted({0, world - 1}):
            cr, sr = fc.slice_of(c, s, rank, world)
            cases.append((cr, sr, ids, 257, rank, world, nbins, 0.1, fc.reference(cr, sr, ids, rank, world, nbins, 0.1)))
    # the exponent-form sum (repr(v / 1000.0) directly: past flush_records' int64)
    got, nrec, want = _one_row(2 ** 64 - 1000)
    c1 = np.zeros((1, 4), np.int64)
    c1[0, 2] = 3
    cases.append((c1, np.array([2 ** 64 - 1000], np.uint64), np.array([2 ** 64 - 1], np.uint64), 1, 0, 1, 4, 2.5,
                  (want, 1)))
    for k, (cr, sr, idv, nseg, rank, world, nbins, kph, (want, nrec)) in enumerate(cases):
        case, out = str(tmp_path / ("case%d" % k)), str(tmp_path / ("out%d" % k))
        _write_case(case, cr, sr, idv, nseg, rank, world, nbins, kph)
        r = subprocess.run([exe, case, out], capture_output=True, text=True, env=env, timeout=60)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
        assert r.stdout.split() == ["0", str(nrec), str(len(want)), "0"], (k, r.stdout)
        assert open(out, "rb").read() == want, k
