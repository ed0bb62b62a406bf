"""The DEVICE build of the pairing tower (fq12.cuh, gt_pow of batch_verify.cuh), operation by operation, against
pairing_ref.py (tests/native/towercheck.hip, tests/towerarith.py).

On the device every large tower function is a __noinline__ call that passes its operands and result through the
private stack, at about 250 VGPRs and up to 7 KB of scratch per lane: a different program from the host build that
test_tower_ops_cpu.py and test_pairing_cpu.py check, and one the pairing tests see only through whole pairings of
canonical inputs.  Here every operation runs alone, 64 lanes per workgroup, on operands at the edges of the < 2p
representation (towerarith.py lists them), and every output limb, value bound and value is checked.  The case set
is tiled over 4096 lanes (1024 for the exponentiations): every copy must agree bit for bit.  The storage round
trip runs at 193 lanes, which is no multiple of the workgroup."""
import collections

import pytest

import towerarith as ta

pytestmark = pytest.mark.gpu

COUNTS = collections.OrderedDict()
_LOAD_ERROR = []


def _ops():
    try:
        return ta.ops(ta.load_device())
    except Exception as e:  # noqa: BLE001 (reported by the tests)
        _LOAD_ERROR.append("%s: %s" % (type(e).__name__, e))
        return [None]


OPS = _ops()


def _ids(op):
    return op.id if op is not None else "harness-unavailable"


def _need(op):
    if op is None:
        pytest.fail("tests/native/towercheck.hip did not build or load: " + "; ".join(_LOAD_ERROR))


@pytest.fixture(scope="module")
def tc():
    _need(OPS[0])
    yield ta.load_device()
    if COUNTS:
        print("\ntower cases (distinct cases x lanes):")
        for k, v in COUNTS.items():
            print("  %-28s %6d x %d" % (k, v[0], v[1]))


@pytest.mark.parametrize("op", OPS, ids=_ids)
def test_tower_op_on_the_device(tc, op):
    _need(op)
    cols, wants = ta.cases_for(op)
    out, n = ta.run_device(tc, op, cols, ta.lanes_for(op))
    COUNTS[op.id] = (ta.distinct(cols), n)
    ta.check(op, cols, wants, out)


def test_cyclotomic_sqr_is_sqr_on_the_subgroup(tc):
    by = {op.id: op for op in OPS}
    cols = ta._cols(ta.cyclotomic_elements())
    a, _ = ta.run_device(tc, by["f12_cyclotomic_sqr"], cols, ta.LANES_CHEAP)
    b, _ = ta.run_device(tc, by["f12_sqr"], cols, ta.LANES_CHEAP)
    assert ta.canonical(a) == ta.canonical(b)
