"""The pair window's definition (datastore.pair_records) on a hand-written
report array against a body written out as a literal, and the parts of its
C ABI that need no device: otm_pairs_cfg_check and the refusals without an
engine.  The GPU side is tests/test_gpu_pairs.py."""
import ctypes as C

import numpy as np
import pytest

from reporter_amd import _lib, datastore

IDS = np.array([100, 200, 300], np.uint64)  # rows 0, 1, 2
BUCKET, ORIGIN = 60, 600
T1_INT = 1  # OTM_REP_T1_INT

# (id, next_id, t0, t1, length, queue_length, flags)
RECORDS = [
    (100, 200, 600.0, 610.0, 100, 5, 0),        # two reports on one key ...
    (100, 200, 659.9, 670.5, 100, 7, 0),        # ... (the second just below the bucket's end)
    (100, 200, 660.0, 672.0, 100, 0, 0),        # the same pair, t0 exactly on the bucket edge: the next bucket
    (100, -1, 605.0, 615.0, 100, 1, 0),         # no next_id: its own key, first in its bucket
    (200, 300, 719.999, 730.0, 50, 0, 0),       # just below an edge: still bucket 660
    (100, 200, 600.0, -1.0, 100, 0, T1_INT),    # rejected: t1 the int -1 of a partial next segment
    (100, 200, 620.0, 610.0, 100, 0, 0),        # rejected: a negative speed
    (100, 200, 620.0, 620.0, 0, 0, 0),          # rejected: 0 / 0 is NaN
    (999, 200, 600.0, 610.0, 100, 0, 0),        # rejected: the id has no row
    (100, 200, 599.9, 610.0, 100, 0, 0),        # out of range: bucket -1
    (100, 200, 600.0 + 4096 * 60, 600.0 + 4096 * 60 + 10, 100, 0, 0),  # out of range: bucket 4096
    (300, 999, 600.0 + 4095 * 60, 600.0 + 4095 * 60 + 10, 30, 2, 0),   # the last bucket; a next_id with no row
]

HEAD = b'{"mode":"auto","bucket_s":60,"origin":600,"privacy":%d,"pairs":['
R_NONEXT = b'{"id":100,"bucket":600,"count":1,"duration_ms":10000,"length":100,"queue_length":1,"t_min":605,"t_max":615}'
R_TWO = (b'{"id":100,"next_id":200,"bucket":600,"count":2,"duration_ms":20600,"length":100,"queue_length":12,'
         b'"t_min":600,"t_max":670}')
R_EDGE = (b'{"id":100,"next_id":200,"bucket":660,"count":1,"duration_ms":12000,"length":100,"queue_length":0,'
          b'"t_min":660,"t_max":672}')
R_BELOW = (b'{"id":200,"next_id":300,"bucket":660,"count":1,"duration_ms":10001,"length":50,"queue_length":0,'
           b'"t_min":719,"t_max":730}')
R_LAST = (b'{"id":300,"bucket":246300,"count":1,"duration_ms":10000,"length":30,"queue_length":2,"t_min":246300,'
          b'"t_max":246310}')


def reports(rows=RECORDS):
    r = np.zeros(len(rows), _lib.REPORT_DTYPE)
    for i, (a, b, t0, t1, ln, q, f) in enumerate(rows):
        r[i] = (a, b, t0, t1, ln, q, f, 0)
    return r


def test_definition_against_a_literal_body():
    d, st = datastore.pair_records(reports(), IDS, BUCKET, ORIGIN, 1)
    assert datastore.serialize(d) == HEAD % 1 + b",".join([R_NONEXT, R_TWO, R_EDGE, R_BELOW, R_LAST]) + b"]}"
    assert st == dict(reports=6, keys=5, records=5, suppressed_keys=0, suppressed_reports=0, out_of_range=2, dropped=0)
    assert tuple(st) == _lib.PAIRS_STATS == datastore.PAIR_STATS


def test_definition_privacy_floor():
    d, st = datastore.pair_records(reports(), IDS, BUCKET, ORIGIN, 2)
    assert datastore.serialize(d) == HEAD % 2 + R_TWO + b"]}"
    assert st == dict(reports=6, keys=5, records=1, suppressed_keys=4, suppressed_reports=4, out_of_range=2, dropped=0)
    d, st = datastore.pair_records(reports(), IDS, BUCKET, ORIGIN, 3)
    assert datastore.serialize(d) == HEAD % 3 + b"]}"
    assert (st["records"], st["suppressed_keys"], st["suppressed_reports"]) == (0, 5, 6)


def test_definition_is_order_free_and_checks_its_arguments():
    want = datastore.pair_records(reports(), IDS, BUCKET, ORIGIN, 1)
    assert datastore.pair_records(reports(RECORDS[::-1]), IDS, BUCKET, ORIGIN, 1) == want
    assert datastore.pair_records(reports([]), IDS, BUCKET, ORIGIN, 1)[0]["pairs"] == []
    for bucket, origin, privacy in ((0, 0, 1), (60, 600, 0), (60, -60, 1), (60, 601, 1)):
        with pytest.raises(ValueError):
            datastore.pair_records(reports(), IDS, bucket, origin, privacy)


def _last_error():
    return _lib.lib().otm_last_error(None).decode()


@pytest.mark.parametrize("cfg,word", [
    (None, "NULL"),
    ((0, 1, 0, 0), "bucket_s"),
    ((-5, 1, 0, 0), "bucket_s"),
    ((60, 0, 0, 0), "privacy"),
    ((60, 1, -60, 0), "origin"),
    ((60, 1, 601, 0), "multiple"),
    ((60, 1, 600, -1), "max_keys"),
])
def test_cfg_check_refusals(cfg, word):
    L = _lib.lib()
    c = None if cfg is None else C.byref(_lib.PairsCfg(*cfg))
    assert L.otm_pairs_cfg_check(c) == -1  # OTM_EINVAL
    assert word in _last_error()


def test_cfg_check_accepts():
    L = _lib.lib()
    for cfg in ((60, 1, 600, 0), (1, 1, 0, 1), (3600, 3, 1499997600, 100000)):
        assert L.otm_pairs_cfg_check(C.byref(_lib.PairsCfg(*cfg))) == 0


def test_every_call_is_refused_without_an_engine():
    L = _lib.lib()
    cfg, st, body, n, slots = _lib.PairsCfg(60, 1, 600, 0), _lib.PairsStats(), C.c_void_p(), C.c_size_t(), C.c_int64()
    r = reports()
    calls = [lambda: L.otm_pairs_begin(None, C.byref(cfg)),
             lambda: L.otm_pairs_add_reports(None, len(r), r.ctypes.data),
             lambda: L.otm_pairs_flush(None, C.byref(body), C.byref(n), C.byref(st)),
             lambda: L.otm_pairs_end(None),
             lambda: L.otm_pairs_info(None, C.byref(cfg), C.byref(slots))]
    for call in calls:
        assert call() == -1
        assert "NULL" in _last_error()
    assert body.value is None and n.value == 0


def test_structs_match_the_header():
    assert C.sizeof(_lib.PairsCfg) == 24 and C.sizeof(_lib.PairsStats) == 56
    assert _lib.PairsCfg.origin.offset == 8 and _lib.PairsCfg.max_keys.offset == 16
