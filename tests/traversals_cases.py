"""Two hand cases for rule 7d's kernel (tests/test_traversals.py on the
reference, tests/test_gpu_traversals.py on k_traversals), in the form of
tests/specref_cases.py: (graph path, batch, meili overrides, max_excl).

hand_long_edge   a (60 m) -> L (800 m) -> c (60 m), one way east.  Both traces
                 enter L from a and put 70 states on it, 11 m apart (columns:
                 more than interpolation_distance), so the traversal of L is
                 opened more than one 64-point chunk before it is closed.
                 Trace 0 leaves L for c; trace 1 ends its chain on L after a
                 backward stay of 11 m, so the last end_offset is the largest
                 offset reached (764 m), not the last state's (753 m).
hand_many_short  a (60 m), 100 edges of 3 m, b (60 m), one way east.  Trace 0
                 goes from a to b in one step whose path has 100 edges; trace 1
                 does the same from a state 8 m before a's end with three
                 interpolated points behind it, the last on the first short
                 edge.  The short edges come in fours: an OSMLR segment of four
                 edges, then four edges without one (plain, internal, internal,
                 plain), so the step's records form 1 + 3 groups per eight.
The search radius is 4 m and 3 m, so no probe sees a second edge or a node.
"""
import os

import handgraph
from handgraph import EDGE_INTERNAL, SEG_BEGIN, SEG_END
from specref_cases import _xy

LONG_STATES, LONG_GAP = 70, 11.0
N_SHORT = 100
IDS = {}    # case -> {edge name: id in the file}, filled by build()


def _chain_graph(path, xs, names, attrs):
    from specref_cases import _pt
    nodes = [_pt(x, 0.0) for x in xs]
    edges, segs = [], []
    for k, nm in enumerate(names):
        kind = attrs(k, nm)
        e = dict(**{"from": k, "to": k + 1}, way=7000 + k, level=0)
        if kind[0] == "own":
            e.update(seg=len(segs), seg_pos=0, flags=SEG_BEGIN | SEG_END)
            segs.append(((len(segs) + 1) << 3, None))
        elif kind[0] == "part":       # position kind[1] of a segment of kind[2] edges
            if kind[1] == 0:
                segs.append(((len(segs) + 1) << 3, None))
            e.update(seg=len(segs) - 1, seg_pos=kind[1],
                     flags=(SEG_BEGIN if kind[1] == 0 else 0) | (SEG_END if kind[1] == kind[2] - 1 else 0))
        else:
            e.update(seg=-1, flags=EDGE_INTERNAL if kind[1] else 0)
        edges.append(e)
    ids = handgraph.write(path, nodes, edges, segs)
    return {nm: ids[k] for k, nm in enumerate(names)}


def build(tmpdir):
    """-> {name: (graph, batch, meili, max_excl)}."""
    d = str(tmpdir)
    cases = {}
    long_ = os.path.join(d, "trav_long_edge.otmg")
    IDS["hand_long_edge"] = _chain_graph(long_, [0.0, 60.0, 860.0, 920.0], ["a", "L", "c"], lambda k, nm: ("own",))
    on_l = [(65.0 + LONG_GAP * i, 1.5) for i in range(LONG_STATES)]
    back = (on_l[-1][0] - LONG_GAP, 1.5)
    cases["hand_long_edge"] = (long_, _xy([[(30.0, 1.5)] + on_l + [(890.0, 1.5)], [(30.0, 1.5)] + on_l + [back]],
                                          dt=2.0, acc=4.0),
                               dict(search_radius=4.0, max_search_radius=4.0, gps_accuracy=4.0), 0)

    many = os.path.join(d, "trav_many_short.otmg")
    xs = [0.0] + [60.0 + 3.0 * k for k in range(N_SHORT + 1)] + [60.0 + 3.0 * N_SHORT + 60.0]
    names = ["a"] + ["s%d" % k for k in range(N_SHORT)] + ["b"]

    def attrs(k, nm):
        if nm in ("a", "b"):
            return ("own",)
        i = k - 1
        if (i // 4) % 2 == 0:
            return ("part", i % 4, 4)
        return ("none", i % 4 in (1, 2))
    IDS["hand_many_short"] = _chain_graph(many, xs, names, attrs)
    xb = xs[-2] + 30.0
    second = [(30.0, 1.0), (52.0, 1.0), (55.0, 1.0), (58.0, 1.0), (61.5, 1.0), (xb, 1.0)]
    cases["hand_many_short"] = (many, _xy([[(30.0, 1.0), (xb, 1.0)], second], dt=2.0, acc=3.0),
                                dict(search_radius=3.0, max_search_radius=3.0, gps_accuracy=3.0), 0)
    return cases
