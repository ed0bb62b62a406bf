"""tests/native/devcheck.hip cross-compiles for gfx950 without a GPU (so a compile error fails here, and the GPU run
finds _devcheck.so built), and the input builders of tests/devarith.py produce what they promise: every record
meets its type's invariant, the edge values are all there, and the maximal vectors sit at the limit."""
import random

import pytest

import devarith as da
from oracle import bn254 as o


@pytest.fixture(scope="module")
def dc():
    return da.load()


def test_harness_cross_compiles_and_reports_its_operations(dc):
    names = set()
    for field in (0, 1, 2):
        ops = da.ops(dc, field)
        assert ops
        for op in ops:
            names.add(op.name)
            assert op.group in (1, 2, 4, 8) and op.ins and op.outs
            for B, LU in op.ins + op.outs:
                assert B in (0, -1, -2) or (1 <= B <= 16 * dc.dc_const(1) and 2 <= LU <= 15)
    for n in ("mul", "sqr", "mul2", "mul4", "mulsub", "add", "dbl", "sub", "neg", "csub", "reduce_to", "reduce_q",
              "canonical", "canonical_q", "unpack", "pack", "inv", "is_zero", "eq", "normalise", "sub_sub2",
              "fq2_mul", "fq2_sqr", "fq2_mulsub", "fq2_sub_sub2", "fq2_scale", "fq2_inv", "fq2_is_zero",
              "fq2_reduce_to", "g1_xyzz_madd", "g1_jac_dbl", "g1_jac_add",
              "g2_jac_dbl", "g2_jac_add"):
        assert n in names, n


def test_extreme_products_sit_at_the_static_assert_limit(dc):
    """the extreme cases follow MONT_SLACK: B1 B2 (sum over the products) within a square root's rounding of
    MONT_SLACK x 256, so a change to the constant moves the cases with it"""
    E = dc.dc_const(0) * 256
    best = {}
    for op in da.ops(dc, 0):
        if op.name in ("mul", "sqr", "mul2", "mul4") and all(lu == 2 for _, lu in op.ins):
            b = [B for B, _ in op.ins] * (2 if op.name == "sqr" else 1)
            s = sum(b[i] * b[i + 1] for i in range(0, len(b), 2))
            assert s <= E
            best[op.name] = max(best.get(op.name, 0), s)
    for n, s in best.items():
        assert s == E or (n != "mul4" and s > E * 0.99), (n, s, E)


def test_the_tower_instantiations_of_fq2_are_listed(dc):
    """the Fq2 forms fq12.cuh instantiates beside those the group laws use, at their bounds"""
    have = {(op.name, tuple(B for B, _ in op.ins[::2])) for op in da.ops(dc, 2) if op.name.startswith("fq2_")}
    for want in (("fq2_mul", (32, 64)), ("fq2_mul", (32, 80)), ("fq2_mul", (64, 64)), ("fq2_scale", (32, 16)),
                 ("fq2_scale", (64, 16)), ("fq2_inv", (32,)), ("fq2_is_zero", (32,)), ("fq2_is_zero", (80,)),
                 ("fq2_reduce_to", (64,)), ("fq2_reduce_to", (112,))):
        assert want in have, want
    for op in da.ops(dc, 2):
        if op.name in ("fq2_scale", "fq2_inv", "fq2_reduce_to"):
            assert op.outs == [(32, 2), (32, 2)], op.id


def test_fq2_zero_reaches_inv_and_is_zero_in_every_spelling(dc):
    for op in da.ops(dc, 2):
        if op.name in ("fq2_inv", "fq2_is_zero"):
            cols = da.operand_sets(op, 4096, seed=100 + op.idx)          # as test_device_arith_gpu.py draws them
            rows = {(da.from_limbs(a), da.from_limbs(b)) for a, b in zip(*cols)}
            assert {(0, 0), (0, o.Q), (o.Q, 0), (o.Q, o.Q), (1, o.Q), (o.Q, o.Q + 1)} <= rows, op.id


def test_fq2_expectations_of_the_tower_forms():
    R = da.RQ
    a, k = (12345, 678), 91011
    am = [c * R % da.Q for c in a]
    assert da.fq2_expect("fq2_scale", am + [k * R % da.Q]) == tuple(c * k * R % da.Q for c in a)
    inv = da.fq2_expect("fq2_inv", [am[0] + da.Q, am[1]])
    assert da.demont(o.Fq2Ops.mul(inv, tuple(am)), o.Fq2Ops) == (R, 0)      # a^-1 R * a R / R = R, the Montgomery one
    assert da.fq2_expect("fq2_inv", [da.Q, 0]) == (0, 0)
    assert da.fq2_expect("fq2_is_zero", [da.Q, 0]) == [1] and da.fq2_expect("fq2_is_zero", [da.Q, 1]) == [0]
    assert da.fq2_expect("fq2_reduce_to", [am[0] + 3 * da.Q, am[1]]) == tuple(am)


@pytest.mark.parametrize("field,p", [(0, o.Q), (1, o.R)])
def test_builders_meet_the_type_invariant(dc, field, p):
    rng = random.Random(3)
    for op in da.ops(dc, field):
        cols = da.operand_sets(op, 600, seed=op.idx)
        for (B, LU), col in zip(op.ins, cols):
            assert len(col) == 600
            if B <= 0:
                continue
            for rec in col:
                assert da.check_limbs(rec, B, LU, p), (op.id, rec)
            vals = {da.from_limbs(r) for r in col}
            assert {0, 1, p - 1, da.vmax(B, p)} <= vals, op.id
            assert {k * p + d for k in range(1, (B + 15) // 16) for d in (-1, 0, 1)
                    if k * p + d <= da.vmax(B, p)} <= vals, op.id
            m = da.maximal(B, LU, p)
            if m is not None:
                assert m in col, op.id
            if LU > 2:
                assert any(max(r[:8]) >= (LU - 1) << 28 for r in col), op.id


def test_every_product_meets_its_corners(dc):
    """every multi-operand operation gets all operands at their maximal vectors and all at their largest values,
    and the first two in the mixed combinations (the asymmetric extremes too, e.g. mul(640, 67))"""
    for field, p in ((0, o.Q), (1, o.R), (2, o.Q)):
        for op in da.ops(dc, field):
            if len(op.ins) < 2 or not all(B > 0 for B, _ in op.ins):
                continue
            cols = da.operand_sets(op, 600, seed=op.idx)
            rows = {tuple(tuple(c[i]) for c in cols) for i in range(600)}
            M = [tuple(da.maximal(B, LU, p) or da.to_limbs(da.vmax(B, p))) for B, LU in op.ins]
            H = [tuple(da.to_limbs(da.vmax(B, p))) for B, _ in op.ins]
            for a, b in ((M, M), (H, H), (M, H), (H, M)):
                assert tuple([a[0], b[1]] + a[2:]) in rows, (op.id, a is M, b is M)


@pytest.mark.parametrize("B,LU", [(16, 2), (17, 2), (208, 2), (640, 2), (208, 12), (320, 10), (640, 15), (96, 4)])
def test_maximal_vector_is_at_the_limit(B, LU):
    for p in (o.Q, o.R):
        m = da.maximal(B, LU, p)
        assert da.check_limbs(m, B, LU, p)
        assert all(x == LU * (1 << 28) - 1 for x in m[:8])
        bumped = m[:8] + [m[8] + 1]                  # one more in limb 8 leaves the bound
        assert not da.check_limbs(bumped, B, LU, p)
        assert 16 * (da.vmax(B, p) + 1) >= B * p > 16 * da.vmax(B, p)


def test_spread_keeps_the_value():
    rng = random.Random(5)
    for _ in range(500):
        v = rng.randrange(40 * o.Q)
        LU = rng.randint(3, 15)
        l = da.spread(v, LU, rng)
        assert da.from_limbs(l) == v and max(l[:8]) < LU << 28


def test_expectations_match_the_montgomery_definitions(dc):
    """field_expect on values where the answer is known by construction"""
    p = o.Q
    R = (1 << da.RBITS) % p
    ops = {op.name + str(op.ins): op for op in da.ops(dc, 0)}
    mul = next(op for op in ops.values() if op.name == "mul")
    a, b = 12345, 67890
    assert da.field_expect(mul, [a * R % p, b * R % p])[0] == a * b * R % p
    inv = next(op for op in ops.values() if op.name == "inv")
    assert da.field_expect(inv, [a * R % p])[0] * a % p == R
    rq = next(op for op in ops.values() if op.name == "reduce_q")
    v = 5 * p + 17
    got, exact = da.field_expect(rq, [v])
    assert exact and got % p == v % p and 16 * got < 17 * p
