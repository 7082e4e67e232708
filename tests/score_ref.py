"""Match scores by the written rule (DESIGN.md §3 rule 7e) in ordered numpy
float32: one record per input point, restated from the text and sharing no
code with reporter_amd/.  This is the exact reference: every sum below is the
one the rule writes, in f32, and a minimum is exact in any order, so an
implementation of the rule agrees with it bit for bit.

Stage-isolated, like tests/points_ref.py: the inputs are the batch and an
implementation's own stage arrays (`Engine.debug` on the GPU, the oracle's
keep_stages arrays through points_ref.oracle_stages on the CPU): ncand,
cand_emis, cand_edge, cand_off, trans_off, trans, state, col_prev,
chain_start, is_col.

`viterbi64` runs tests/specref.py's float64 Viterbi (Chain.m, Chain.margin)
on the same arrays, and `check_f64` compares records with it inside bounds
derived from the roundings, not measured.
"""
import numpy as np

import specref as sr

KMAX = sr.KMAX
SCORED, CHAIN_START, CHAIN_END, ALONE, TIE = 1, 2, 4, 8, 16
DTYPE = np.dtype([("cost", "<f4"), ("margin", "<f4"), ("chain_cost", "<f4"), ("emission", "<f4"),
                  ("transition", "<f4"), ("alt_edge", "<i4"), ("alt_offset", "<f4"), ("flags", "u1"),
                  ("ncand", "u1"), ("state", "i1"), ("alt", "i1")])
STAGES = ("ncand", "cand_emis", "cand_edge", "cand_off", "trans_off", "trans", "state", "col_prev", "chain_start",
          "is_col")
F32 = np.float32
INF32 = F32(np.inf)


def stages_of(batch, st):
    """Stage arrays cut to the batch's points, and chain_start / is_col made
    from an oracle result when it carries none (points_ref.oracle_stages)."""
    if "chain_start" not in st or "is_col" not in st:
        import points_ref
        st = dict(st, **points_ref.oracle_stages(batch, st))
    return st


def block(st, p):
    """Column p's transition block T (Kq x Kp, f32), read as T[i * Kp + j]."""
    q = int(st["col_prev"][p])
    Kq, Kp = int(st["ncand"][q]), int(st["ncand"][p])
    o = int(st["trans_off"][p])
    return np.asarray(st["trans"][o:o + Kq * Kp], F32).reshape(Kq, Kp)


def chains_of(batch, st, codes=None):
    """The chains K5 decoded, per trace: lists of columns with a state, cut
    where chain_start is set.  A trace answered 500 (codes: the traces' result
    codes) has none, whatever states it was left with: route recovery can fail
    a trace after its columns got their states."""
    off = np.asarray(batch["trace_off"], np.int64)
    out = []
    for t in range(len(off) - 1):
        cur = None
        if codes is not None and int(codes[t]) != 200:
            continue
        for p in range(int(off[t]), int(off[t + 1])):
            if not st["is_col"][p] or st["state"][p] < 0:
                continue
            if cur is None or st["chain_start"][p]:
                cur = []
                out.append(cur)
            else:
                assert int(st["col_prev"][p]) == cur[-1], "a linked column follows its col_prev"
            cur.append(p)
    return out


def scores(batch, st, codes=None):
    """-> records (DTYPE), one per input point, by rule 7e in ordered f32.
    codes: the traces' result codes (any point of a trace answered 500 has the
    all-zero record); None: every trace with states is scored."""
    st = stages_of(batch, st)
    n = len(batch["lat"])
    rec = np.zeros(n, DTYPE)
    rec["alt"] = -1
    rec["alt_edge"] = -1
    em_all = np.asarray(st["cand_emis"], F32)
    for cols in chains_of(batch, st, codes):
        nc = len(cols)
        K = [int(st["ncand"][p]) for p in cols]
        em = [em_all[p * KMAX:p * KMAX + k] for p, k in zip(cols, K)]
        T = [None] + [block(st, p) for p in cols[1:]]
        # forward: K5's own values
        alpha = [em[0].copy()]
        for k in range(1, nc):
            v = alpha[k - 1][:, None] + T[k]                    # f32 + f32, Kq x Kp
            alpha.append((v.min(axis=0) + em[k]).astype(F32))
        # backward, over all states, dead ones included
        beta = [None] * nc
        beta[nc - 1] = np.zeros(K[-1], F32)
        for k in range(nc - 2, -1, -1):
            g = em[k + 1] + beta[k + 1]
            beta[k] = (T[k + 1] + g[None, :]).min(axis=1).astype(F32)
        chain_cost = alpha[-1].min()
        for k, p in enumerate(cols):
            m = alpha[k] + beta[k]
            assert m.dtype == F32
            s = int(st["state"][p])
            assert np.isfinite(m[s]), "the chosen state's through-cost is finite"
            others = m.copy()
            others[s] = INF32
            fl = SCORED | (CHAIN_START if k == 0 else 0) | (CHAIN_END if k == nc - 1 else 0)
            r = rec[p]
            if K[k] < 2 or not np.isfinite(others.min()):
                margin, alt = INF32, -1
                fl |= ALONE
            else:
                alt = int(np.argmin(others))                   # the lowest index that attains the minimum
                d = F32(others[alt] - m[s])
                margin = d if d > 0 else F32(0.0)
                r["alt_edge"] = st["cand_edge"][p * KMAX + alt]
                r["alt_offset"] = st["cand_off"][p * KMAX + alt]
                if margin == 0:
                    fl |= TIE
            r["cost"], r["margin"], r["chain_cost"] = m[s], margin, chain_cost
            r["emission"] = em[k][s]
            r["transition"] = T[k][int(st["state"][cols[k - 1]]), s] if k else F32(0.0)
            r["flags"], r["ncand"], r["state"], r["alt"] = fl, K[k], s, alt
    return rec


def fold_chain_costs(rec):
    """Both exact consequences of the rule, from records alone: per chain, the
    f32 fold ((em0 + tr1) + em1) + tr2 ... and the last column's cost, each
    bit-equal to chain_cost.  -> the number of chains checked."""
    acc, chains = None, 0
    for r in rec[(rec["flags"] & SCORED) != 0]:
        if r["flags"] & CHAIN_START:
            assert acc is None, "a chain starts inside another"
            assert r["transition"] == 0
            acc = F32(r["emission"])
        else:
            assert acc is not None, "a scored record outside a chain"
            acc = F32(F32(acc + r["transition"]) + r["emission"])
        if r["flags"] & CHAIN_END:
            assert acc.view(np.uint32) == r["chain_cost"].view(np.uint32), (acc, r["chain_cost"])
            assert r["cost"].view(np.uint32) == r["chain_cost"].view(np.uint32), (r["cost"], r["chain_cost"])
            acc, chains = None, chains + 1
    assert acc is None, "the last chain has no end"
    return chains


# ------------------------------------------------------------------ the float64 side
def viterbi64(batch, st):
    """specref.viterbi in float64 on the same stage arrays -> {column: (Chain, k)}."""
    st = stages_of(batch, st)
    trans = {}
    for p in np.nonzero(np.asarray(st["col_prev"]) >= 0)[0]:
        p = int(p)
        if st["is_col"][p] and st["ncand"][p] > 0 and st["ncand"][int(st["col_prev"][p])] > 0:
            trans[p] = block(st, p).astype(np.float64)
    where = {}
    for chains in sr.viterbi(batch, st["is_col"], st["ncand"], st["cand_emis"], st["col_prev"], trans):
        for ch in chains:
            for k, p in enumerate(ch.cols):
                where[p] = (ch, k)
    return where


def tol_m(ncols, m):
    """Bound on |f32 through-cost - float64 through-cost| for a chain of ncols
    columns: the forward and backward sweeps together make two additions per
    column on partial sums <= m, forming m one more: specref.tol_viterbi over
    ncols + 1 columns."""
    return sr.tol_viterbi(ncols + 1, m)


CAP = 0.01      # excluded columns: at most 1 % of a case's scored columns


def check_f64(batch, st, rec, what="", max_excl=None):
    """Records against the float64 reference, inside the derived bounds.
    First the caps, before anything is compared: no scored column whose chosen
    state differs from the float64 optimum, and at most max_excl (None: CAP of
    the scored columns) columns whose runner-up the float64 reference cannot
    adjudicate -- its own runner-up and the record's lie within twice the
    margin's bound.  -> dict(scored, excluded, state_diff, worst): worst is
    the largest error / bound ratio seen."""
    st = stages_of(batch, st)
    where = viterbi64(batch, st)
    scored = [int(p) for p in np.nonzero((rec["flags"] & SCORED) != 0)[0]]
    out = dict(scored=len(scored), excluded=0, state_diff=0, worst=0.0)
    todo = []
    for p in scored:
        r = rec[p]
        assert p in where, "%s point %d: scored, in no float64 chain" % (what, p)
        ch, k = where[p]
        s = int(r["state"])
        if ch.state[k] != s:
            out["state_diff"] += 1
            continue
        n, m64 = len(ch.cols), ch.m[k]
        others = np.array(m64, np.float64)
        others[s] = np.inf
        alt64 = int(np.argmin(others)) if np.isfinite(others).any() else -1
        bound = tol_m(n, float(m64[s])) + (tol_m(n, float(m64[alt64])) if alt64 >= 0 else 0.0)
        alt = int(r["alt"])
        excl = alt64 >= 0 and 0 <= alt < len(m64) and alt != s and alt != alt64 and \
            abs(float(m64[alt]) - float(m64[alt64])) <= 2 * bound
        out["excluded"] += bool(excl)
        todo.append((p, ch, k, s, alt64, bound, excl))
    assert out["state_diff"] == 0, "%s: %d columns whose chosen state differs" % (what, out["state_diff"])
    cap = CAP * len(scored) if max_excl is None else max_excl
    assert out["excluded"] <= cap, "%s: %d of %d scored columns excluded" % (what, out["excluded"], len(scored))

    def ratio(err, bound):
        q = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        out["worst"] = max(out["worst"], q)
        return q
    for p, ch, k, s, alt64, bound, excl in todo:
        r = rec[p]
        n, m64 = len(ch.cols), ch.m[k]
        t_s = tol_m(n, float(m64[s]))
        assert ratio(abs(float(r["cost"]) - float(m64[s])), t_s) <= 1.0, \
            "%s point %d: cost %r, float64 %r, bound %g" % (what, p, r["cost"], m64[s], t_s)
        assert ratio(abs(float(r["chain_cost"]) - ch.cost), tol_m(n, ch.cost)) <= 1.0, \
            "%s point %d: chain cost %r, float64 %r" % (what, p, r["chain_cost"], ch.cost)
        margin64 = ch.margin[k]
        # infinite exactly where the reference's is
        assert bool(np.isinf(r["margin"])) == bool(np.isinf(margin64)) == (alt64 < 0), \
            "%s point %d: margin %r, float64 %r" % (what, p, r["margin"], margin64)
        assert bool(r["flags"] & ALONE) == bool(np.isinf(margin64)), (what, p)
        if alt64 < 0:
            assert r["alt"] == -1 and r["alt_edge"] == -1, (what, p)
            continue
        assert ratio(abs(float(r["margin"]) - max(margin64, 0.0)), bound) <= 1.0, \
            "%s point %d: margin %r, float64 %r, bound %g" % (what, p, r["margin"], margin64, bound)
        assert excl or int(r["alt"]) == alt64, "%s point %d: runner-up %d, float64 %d" % (what, p, r["alt"], alt64)
    return out
