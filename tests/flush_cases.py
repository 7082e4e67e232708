"""Windows for the flush writers' tests (test_flush_host.py, test_gpu_flush.py)
and the reference they are compared with, byte for byte:
datastore.serialize(datastore.flush_records(...)) on the same numbers."""
import numpy as np

from reporter_amd import datastore

BIG_BIN = 2 ** 31 - 1
# speed sums (1/1000 km/h) of the special rows: 0 with a count ("0.0"), small
# and round values, and values past 2^53 (the integer is rounded to a double
# before the division) up to the int64 limit of flush_records' own cast
SPECIAL_SUMS = [0, 1, 999, 1000, 123456789, 2 ** 53 + 1, 2 ** 62, 2 ** 63 - 1]
# at or above 2^52 x 1000: past the GPU float writer's range (the decline path)
DECLINE_SUM = 2 ** 52 * 1000 + 12345


def padded(n_segments, world):
    return (n_segments + world - 1) // world * world


def make_ids(n_segments, seed=5):
    """u64 ids with 0, 2^63 - 1 and a value at or above 2^63 among them."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(1, 2 ** 62, size=n_segments, dtype=np.uint64)
    for k, v in enumerate((0, 2 ** 63 - 1, 2 ** 63 + 12345)):
        if k < n_segments:
            ids[(k * 7) % n_segments if n_segments > 2 else k] = np.uint64(v)
    return ids


def window(kind, n_segments, nbins, world, seed=0, rows_at=()):
    """(counts int64 [S_pad, nbins], sums uint64 [S_pad]) of one window over
    the padded rows.  kind: random | row0 | last | dense | empty | padding |
    special | rows (nonzero exactly at rows_at, padding rows included)."""
    sp = padded(n_segments, world)
    rng = np.random.default_rng(seed * 1000003 + n_segments * 131 + nbins * 7 + world)
    c = np.zeros((sp, nbins), np.int64)
    s = np.zeros(sp, np.uint64)

    def fill(rows):
        for r in rows:
            c[r] = rng.integers(0, 50, size=nbins)
            c[r, rng.integers(0, nbins)] += 1  # (never all zero)
            s[r] = np.uint64(int(rng.integers(0, 2 ** 40)))

    if kind == "random":
        fill(np.nonzero(rng.random(sp) < 0.3)[0])
    elif kind == "row0":
        fill([0])
    elif kind == "last":
        fill([n_segments - 1])
    elif kind == "dense":
        fill(range(sp))
    elif kind == "padding":
        fill(range(n_segments, sp))
    elif kind == "rows":
        fill([r for r in rows_at if 0 <= r < sp])
    elif kind == "special":
        for k, r in enumerate(range(0, n_segments, max(1, n_segments // 24))):
            c[r, k % nbins] = 1 + k
            s[r] = np.uint64(SPECIAL_SUMS[k % len(SPECIAL_SUMS)])
            if k % 5 == 4:  # bins of 2^31 - 1 in three bins: the count passes 2^32
                c[r, :] = 0
                c[r, [0, nbins // 2, nbins - 1]] = BIG_BIN
    elif kind != "empty":
        raise ValueError(kind)
    # rows past n_segments may hold anything: they never appear
    if kind in ("random", "special", "dense"):
        fill(range(n_segments, sp))
    return c, s


def slice_of(c, s, rank, world):
    rows = c.shape[0] // world
    return c[rank * rows:(rank + 1) * rows], s[rank * rows:(rank + 1) * rows]


def reference(c, s, ids, rank, world, nbins, bin_kph):
    """The reference body of a slice and its record count.  bin_kph is the
    float the ABI carries; sums reach flush_records as the same integers (its
    int64 cast holds everything below 2^63)."""
    assert int(np.asarray(s).max(initial=0)) < 2 ** 63
    rec = datastore.flush_records(np.asarray(c, np.int64).reshape(-1), np.asarray(s).astype(np.int64), ids, rank, world,
                                  nbins, float(np.float32(bin_kph)))
    return datastore.serialize(rec), len(rec["segments"])
