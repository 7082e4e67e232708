"""queue_length by the written rule (DESIGN.md §3 rule 7b), in plain Python
and float64: an independent restatement that shares no code with
reporter_amd/.  The kernel walks each segment backwards and stops early; this
reference lists every interval of a trace forwards, once, then cuts each
segment's share out of the list.

Inputs are a batch's times, the stage arrays (state / columns, route_dist,
ipos, chain starts: `Engine.debug` on the GPU, the oracle's keep_stages arrays
on the CPU) and the segment records; the output is queue_length per segment.
A segment is *on a boundary* when the answer hangs on the last bits of a
comparison: an interval the walk tested lies within 1e-9 (relative) of the
threshold, or the unrounded sum lies within 1e-6 of k + 0.5 or of length +
0.5.  Those segments are excluded from exact comparison.
"""
import math

import numpy as np

KMAX = 32


def trace_intervals(a, n, time, state, is_col, chain_start, route_dist, ipos):
    """The intervals of the trace at [a, a + n) in index order, as (first
    anchor's trace-local index, d, t_prev, t_next).  Anchors: the chain's
    states, and inside a step q -> p the interpolated points whose ipos is not
    behind an earlier anchor of the step; q at 0, p at route_dist[p]."""
    out = []
    q = None
    for pl in range(n):
        p = a + pl
        if not (is_col[p] and state[p] >= 0):
            continue
        if q is not None and not chain_start[p]:
            anchors = [(q, 0.0)]
            run = 0.0
            for k in range(q + 1, pl):
                x = float(ipos[a + k])
                if x >= run:
                    anchors.append((k, x))
                    run = x
            anchors.append((pl, float(route_dist[p])))
            for (i0, x0), (i1, x1) in zip(anchors, anchors[1:]):
                out.append((i0, max(x1 - x0, 0.0), float(time[a + i0]), float(time[a + i1])))
        q = pl
    return out


def segment_queue(intervals, seg, v):
    """-> (queue_length, on a boundary, took the discharge branch) of one
    segment record over its trace's intervals, at the threshold v km/h."""
    length = int(seg["length"])
    if int(seg["segment_id"]) < 0 or length < 0:
        return 0, False, False
    T0, T1 = float(seg["start_time"]), float(seg["end_time"])
    lo, hi = int(seg["begin_shape_index"]), int(seg["end_shape_index"])
    rem = []  # (slow, piece, near the threshold)
    for i0, d, tp, tn in intervals:
        if not lo <= i0 <= hi:
            continue
        c = (tn if tn < T1 else T1) - (tp if tp > T0 else T0)
        if not c > 0.0:
            continue
        dt = tn - tp
        slow = dt > 0.0 and d * 3.6 < v * dt
        near = abs(d * 3.6 - v * dt) <= 1e-9 * v * dt
        rem.append((slow, d * (c / dt), near))
    if not rem:
        return 0, False, False
    j = len(rem) - 1
    near = rem[j][2]
    discharge = False
    total = 0.0
    if not rem[j][0]:
        if j == 0:
            return 0, near, False
        near = near or rem[j - 1][2]
        if not rem[j - 1][0]:
            return 0, near, False
        discharge = True
        total = rem[j][1]
        j -= 1
    while j >= 0:
        near = near or rem[j][2]
        if not rem[j][0]:
            break
        total = total + rem[j][1]
        j -= 1
    frac = total - math.floor(total)
    edge = abs(frac - 0.5) <= 1e-6 or abs(total - (length + 0.5)) <= 1e-6
    return min(int(math.floor(total + 0.5)), length), near or edge, discharge


def queue_lengths(batch, stages, traces, segments, v):
    """queue_length of every segment of a batch's results.  stages: dict with
    state, route_dist, ipos, chain_start and (optionally) is_col, per point;
    traces / segments: the result records (dense offsets).  v: the threshold
    in km/h as the engine holds it (a float32).
    -> (int32 [S], on-boundary bool [S], discharge bool [S])"""
    v = float(np.float32(v))
    off = np.asarray(batch["trace_off"], np.int64)
    time = np.asarray(batch["time"], np.float64)
    state = stages["state"]
    is_col = stages.get("is_col")
    if is_col is None:
        is_col = state >= 0
    S = len(segments)
    out = np.zeros(S, np.int32)
    bnd = np.zeros(S, bool)
    dis = np.zeros(S, bool)
    if v <= 0.0:
        return out, bnd, dis
    for t in range(len(off) - 1):
        s0, ns = int(traces["seg_off"][t]), int(traces["seg_cnt"][t])
        if ns == 0:
            continue
        a, n = int(off[t]), int(off[t + 1] - off[t])
        iv = trace_intervals(a, n, time, state, is_col, stages["chain_start"], stages["route_dist"], stages["ipos"])
        for s in range(s0, s0 + ns):
            out[s], bnd[s], dis[s] = segment_queue(iv, segments[s], v)
    return out, bnd, dis


def chain_starts(trace_off, st):
    """The chain-start flags of the oracle's stage arrays (which do not carry
    them): the Viterbi forward pass of DESIGN.md §3 rule 5 in float32, as far
    as it decides where a chain starts -- at a column with candidates whose
    previous column is not linked to it, or from which every transition is
    infinite.  Points without candidates are no columns of a chain (a column
    without candidates unlinks the next one: its col_prev is -1)."""
    ncand, col_prev = st["ncand"], st["col_prev"]
    emis, toff, trans = st["cand_emis"], st["trans_off"], st["trans"]
    cs = np.zeros(len(ncand), np.uint8)
    for t in range(len(trace_off) - 1):
        last, prev = -1, None
        for p in range(int(trace_off[t]), int(trace_off[t + 1])):
            K = int(ncand[p])
            if K == 0:
                continue
            em = emis[p * KMAX:p * KMAX + K].astype(np.float32)
            cur = None
            if prev is not None and int(col_prev[p]) == last:
                T = trans[int(toff[p]):int(toff[p]) + len(prev) * K].reshape(len(prev), K)
                with np.errstate(invalid="ignore"):
                    best = (prev[:, None] + T).astype(np.float32).min(axis=0)
                if (best < np.inf).any():
                    cur = np.where(best < np.inf, best + em, np.float32(np.inf)).astype(np.float32)
            if cur is None:
                cs[p] = 1
                cur = em
            prev, last = cur, p
    return cs


def oracle_stages(batch, r):
    """The stage arrays queue_lengths reads, from an oracle result made with keep_stages."""
    return dict(state=r["state"], route_dist=r["route_dist"], ipos=r["ipos"],
                chain_start=chain_starts(np.asarray(batch["trace_off"], np.int64), r))
