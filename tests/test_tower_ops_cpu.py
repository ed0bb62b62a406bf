"""The pairing tower (fq12.cuh, gt_pow of batch_verify.cuh) operation by operation, on the host build of
tests/native/tower_ops.h (towercheck_host.cpp), against pairing_ref.py: the cases, the expectations and the host
branch of the headers are checked here without a GPU, and the device harness (towercheck.hip) is cross-compiled so
that test_tower_ops_gpu.py finds it built.  Cases and checks are tests/towerarith.py's."""
import ctypes

import pytest

import devarith as da
import towerarith as ta

_LOAD_ERROR = []


def _ops():
    """the operation table (read at collection); a harness that does not build fails this module's tests, one each,
    instead of aborting the collection of the whole session"""
    try:
        return ta.ops(ta.load_host())
    except Exception as e:  # noqa: BLE001 (reported by the tests)
        _LOAD_ERROR.append("%s: %s" % (type(e).__name__, e))
        return [None]


OPS = _ops()


def _ids(op):
    return op.id if op is not None else "harness-unavailable"


def _need(op):
    if op is None:
        pytest.fail("tests/native/towercheck_host.cpp did not build or load: " + "; ".join(_LOAD_ERROR))


def test_device_harness_cross_compiles_with_the_same_table():
    """towercheck.hip builds for gfx950 without a GPU and reports the same operations, bounds and scratch needs as the
    host build (its tc_count / tc_info are host code)"""
    _need(OPS[0])
    dev = ta._proto(ctypes.CDLL(ta.build_device()))
    assert dev.tc_is_device() == 1 and ta.load_host().tc_is_device() == 0
    got = [(op.id, op.ins, op.outs, op.scratch) for op in ta.ops(dev)]
    assert got == [(op.id, op.ins, op.outs, op.scratch) for op in OPS]


def test_the_table_covers_the_tower():
    _need(OPS[0])
    ids = [op.id for op in OPS]
    assert len(set(ids)) == len(ids)
    assert {op.name for op in OPS} == set(ta.OPS)
    for B in (49, 80, 96, 112, 128, 144, 176, 288):
        assert "f2n<%d>" % B in ids
    for k in (1, 2, 3):
        assert "f6_frobenius<%d>" % k in ids and "f12_frobenius<%d>" % k in ids
    assert "gt_pow<4>" in ids and "gt_pow<8>" in ids
    for op in OPS:                                       # every tower value is claimed below 2p, normalised
        assert all(b == (32, 2) or b[0] in (0, -1) for b in op.outs), op.id


@pytest.mark.parametrize("op", OPS, ids=_ids)
def test_cases_meet_the_type_invariants_and_the_size(op):
    _need(op)
    cols, wants = ta.cases_for(op)
    C = len(wants)
    assert all(len(c) == C for c in cols)
    want_n = ta.N_STORE if op.name == "store_load_f12" else ta.N_SLOW if op.name in ta.SLOW else ta.N_CHEAP
    assert C == want_n
    assert ta.distinct(cols) == C, (op.id, ta.distinct(cols))
    for (B, LU), col in zip(op.ins, cols):
        if B > 0:
            assert all(da.check_limbs(r, B, LU, ta.Q) for r in col), op.id
        else:
            assert all(0 <= int(w) < 1 << 32 for r in col for w in r), op.id


def test_the_named_cases_are_there():
    """the inputs the operations are known to be delicate at, by what the reference says about them"""
    _need(OPS[0])
    by = {op.id: op for op in OPS}
    Q, RQ = ta.Q, da.RQ

    def vals(op_id):
        cols, wants = ta.cases_for(by[op_id])
        return [[da.from_limbs(c[i]) for c in cols] for i in range(len(wants))], wants

    for name in ("f6_is_zero", "f12_is_zero"):                   # zero in every spelling, and one slot off zero
        ins, wants = vals(name)
        m = len(ins[0])
        assert {tuple([0] * m), tuple([Q] * m), tuple([0, Q] * (m // 2))} <= {tuple(v) for v in ins}
        assert sum(w[0] for w in wants) >= 4
        near = [v for v, w in zip(ins, wants) if not w[0] and sum(x % Q != 0 for x in v) == 1]
        assert {x % Q for v in near for x in v} >= {0, 1} and len(near) >= 4 * m
    for name in ("f6_inv", "f12_inv", "final_exp_first_chunk", "final_exponentiation"):   # zero gives zero
        ins, wants = vals(name)
        zero = [w for v, w in zip(ins, wants) if all(x % Q == 0 for x in v)]
        assert len(zero) >= 3 and all(w == [0] * len(w) for w in zero), name
    ins, wants = vals("f12_eq")                                  # equal in another representation; unequal
    assert sum(w[0] for v, w in zip(ins, wants) if v[:12] != v[12:]) >= 100 and sum(not w[0] for w in wants) >= 100
    # Z = 0 in every spelling: H = 2 Y Z and with it ellVW vanish; ell0 = xi (3 b' Z^2 - Y^2) vanishes with Y as well
    ins, wants = vals("doubling_step")
    z0 = [(v, w) for v, w in zip(ins, wants) if v[4] % Q == 0 and v[5] % Q == 0 and any(x % Q for x in v[:2])]
    assert {(v[4], v[5]) for v, _ in z0} >= {(0, 0), (Q, Q), (0, Q), (Q, 0)}
    assert all(w[2:4] == [0, 0] for _, w in z0)
    yz0 = [w for v, w in z0 if v[2] % Q == 0 and v[3] % Q == 0]
    assert len(yz0) >= 4 and all(w[:4] == [0, 0, 0, 0] for w in yz0) and any(w[:2] != [0, 0] for _, w in z0)
    ins, wants = vals("mixed_addition_step")                     # the current point is the base: D = E = 0
    same = [w for v, w in zip(ins, wants) if w[2:6] == [0, 0, 0, 0] and any(x % Q for x in v[:4])]
    assert len(same) >= 32
    ins, _ = vals("apply_line")                                  # (px, py) = (0, 1)
    assert {(v[18], v[19]) for v in ins} >= {(0, RQ), (Q, RQ), (0, RQ + Q), (Q, RQ + Q)}
    for words in (4, 8):
        ins, _ = vals("gt_pow<%d>" % words)
        es = {v[12] for v in ins}                                # (an exponent record reads as 29-bit limbs here)
        lim = lambda e: da.from_limbs([(e >> (32 * i)) & 0xffffffff for i in range(8)] + [0])  # noqa: E731
        want = [0, 1, 2, (1 << 128) - 1] + ([ta.R_ORDER - 1, ta.R_ORDER, (1 << 256) - 1] if words == 8 else [])
        assert {lim(e) for e in want} <= es
    ins, wants = vals("f12_cyclotomic_sqr")                      # true cyclotomic elements among the operands
    assert sum(w == [c * RQ % Q for c in ta.flat(ta.pr.f12_sqr(ta.nest("f12", [x * da.RQI % Q for x in v])))]
               for v, w in zip(ins, wants)) >= 24


@pytest.mark.parametrize("op", OPS, ids=_ids)
def test_tower_op_on_the_host(op):
    _need(op)
    cols, wants = ta.cases_for(op)
    ta.check(op, cols, wants, ta.run_host(ta.load_host(), op, cols))


def test_cyclotomic_sqr_is_sqr_on_the_subgroup():
    _need(OPS[0])
    by = {op.id: op for op in OPS}
    cols = ta._cols(ta.cyclotomic_elements())
    lib = ta.load_host()
    a = ta.canonical(ta.run_host(lib, by["f12_cyclotomic_sqr"], cols))
    b = ta.canonical(ta.run_host(lib, by["f12_sqr"], cols))
    assert a == b
