"""The DEVICE build of the group law (ec.cuh over G1Cfg and G2Cfg, glv.cuh, the lane-group conversions of quad.cuh and
fq2.cuh), operation by operation, against oracle.bn254 on exact integers (tests/native/groupcheck.hip,
tests/grouparith.py).

hostcheck.cpp reaches these functions through chains of canonical wire inputs, and the MSM, EC-FFT, points_* and codec
tests through whole kernels, where an exceptional branch is taken only with the representatives the pipeline happened
to produce.  Here every entry point runs alone, one case per lane, on operands in every representative its types
admit: coordinates plus any multiple of p below their bound, infinity at every multiple of p, P == +-Q under
different Z (grouparith.py lists the kinds; test_group_ops_cpu.py asserts their shares).  Every output limb, value
bound (as the harness reports it from the C++ type) and point is checked.  The case set is tiled over 2^16 lanes:
every copy must agree bit for bit.  The lane-group conversions hold one case per quad / octet, and every lane of the
group must return the whole result."""
import collections

import pytest

import grouparith as ga

pytestmark = pytest.mark.gpu

COUNTS = collections.OrderedDict()
_LOAD_ERROR = []


def _ops():
    try:
        return ga.ops(ga.load_device())
    except Exception as e:  # noqa: BLE001 (reported by the tests)
        _LOAD_ERROR.append("%s: %s" % (type(e).__name__, e))
        return [None]


OPS = _ops()


def _ids(op):
    return op.id if op is not None else "harness-unavailable"


def _need(op):
    if op is None:
        pytest.fail("tests/native/groupcheck.hip did not build or load: " + "; ".join(_LOAD_ERROR))


@pytest.fixture(scope="module")
def gc():
    _need(OPS[0])
    yield ga.load_device()
    if COUNTS:
        print("\ngroup-law cases (distinct cases x lanes):")
        for k, v in COUNTS.items():
            print("  %-36s %6d x %d" % (k, v[0], v[1]))


@pytest.mark.parametrize("op", OPS, ids=_ids)
def test_group_op_on_the_device(gc, op):
    _need(op)
    cols, wants = ga.cases_for(op, OPS)           # the builder and seeds of test_group_ops_cpu.py
    assert ga.distinct(cols) == len(wants) == ga.size_of(op)
    out, n = ga.run_device(gc, op, cols)
    COUNTS[op.id] = (len(wants), n)
    ga.check(op, cols, wants, out)
