"""The hand case of rule 7g's tests beside tests/shape_cases.py's, in the same
form: (graph path, batch, meili overrides, max_excl).

hand_attr_zero   shape_cases.FIRST_ROAD with its traces 0-2 in a frame at
                 (lat 0.0001, lon -0.0003): the road crosses both the equator
                 (y = 0 .. -20 m is lat 0.0001 .. -0.00008) and the prime
                 meridian (x = 0 .. 490 m is lon -0.0003 .. 0.0041), so matched
                 lat and lon take values in (-1, 0) whose text has the integer
                 part "-0", and values on both sides of 0.
"""
import os
import re

import shape_cases

ALL = shape_cases.ALL + ["hand_attr_zero"]


def build(tmpdir):
    """-> {name: (graph, batch, meili, max_excl)}."""
    pt = shape_cases._frame(0.0001, -0.0003)
    path = os.path.join(str(tmpdir), "attr_zero.otmg")
    shape_cases._write(path, [(pt, shape_cases.FIRST_ROAD)])
    return {"hand_attr_zero": (path, shape_cases._batch(pt, shape_cases.FIRST_TRACES), dict(shape_cases.MEILI), 0)}


def assert_zero_reached(bodies):
    """hand_attr_zero: text with the integer part -0 on both axes, and both signs on both."""
    text = "".join(bodies)
    for key in ("lat", "lon"):
        vals = re.findall(r'"%s":(-?\d+\.\d{6})' % key, text)
        assert any(v.startswith("-0.") and float(v) < 0 for v in vals), key
        assert any(float(v) > 0 for v in vals), key
        assert all(-1 < float(v) < 1 for v in vals), key
