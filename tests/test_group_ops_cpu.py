"""The group law (ec.cuh over G1Cfg and G2Cfg, glv.cuh) operation by operation, on the host build of
tests/native/group_ops.h (groupcheck_host.cpp), against oracle.bn254 on exact integers: the cases, the expectations and
the host branch of the headers are checked here without a GPU, and the device harness (groupcheck.hip) is
cross-compiled so that test_group_ops_gpu.py finds it built.  Cases and checks are tests/grouparith.py's; this module
also asserts what the case sets promise about themselves (sizes, the share of every exceptional kind, every spelling
of infinity, the largest representatives), counted from the oracle's reading of the operand records alone."""
import ctypes
import itertools

import pytest

import devarith as da
import grouparith as ga
from oracle import bn254 as o

_LOAD_ERROR = []
Q = o.Q


def _ops():
    """the operation table (read at collection); a harness that does not build fails this module's tests, one each,
    instead of aborting the collection of the whole session"""
    try:
        return ga.ops(ga.load_host())
    except Exception as e:  # noqa: BLE001 (reported by the tests)
        _LOAD_ERROR.append("%s: %s" % (type(e).__name__, e))
        return [None]


OPS = _ops()
BIN = [op for op in OPS if op is not None and op.name in ga.BINARY] or [None]


def _ids(op):
    return op.id if op is not None else "harness-unavailable"


def _need(op):
    if op is None:
        pytest.fail("tests/native/groupcheck_host.cpp did not build or load: " + "; ".join(_LOAD_ERROR))


def _table(ops):
    return [(op.id, op.group, op.ins, op.outs) for op in ops]


@pytest.fixture(scope="module")
def dev_ops():
    _need(OPS[0])
    dev = ga._proto(ctypes.CDLL(ga.build_device()))
    assert dev.gc_is_device() == 1 and ga.load_host().gc_is_device() == 0
    return ga.ops(dev)


def test_device_harness_cross_compiles_with_the_same_table(dev_ops):
    """groupcheck.hip builds for gfx950 without a GPU and reports the same operations and bounds as the host build
    (its gc_count / gc_info are host code); the lane-group conversions are the device build's alone"""
    assert _table([op for op in dev_ops if op.list != 3]) == _table(OPS)
    assert ga.load_host().gc_count(3) == 0
    lane = [op for op in dev_ops if op.list == 3]
    assert {(op.name, op.group) for op in lane} == {("g1_pair_round_trip", 4), ("g1_pair_dbl", 4),
                                                    ("g2_pair_round_trip", 8), ("g2_pair_dbl", 8)}
    for op in lane:                                       # a Jacobian point of the per-lane configuration in and out
        per_lane = next(x for x in OPS if x.id == "%s:jac_dbl" % op.name[:2])
        assert op.ins == per_lane.ins and op.outs == per_lane.outs


def test_the_table_covers_the_group_law():
    """every per-lane entry point of ec.cuh and glv_image for both configurations; an operation is listed for one only
    if production instantiates it there: the lazily carried forms where CV::LAZY_MADD is set and jac_to_xyzz for the
    row / column window sums are G1's alone (grouparith.G1_ONLY), scalar_mul runs with 8 words everywhere and with 4
    for G1 (batch_verify.cuh bv_g1_mul_affine)"""
    _need(OPS[0])
    ids = [op.id for op in OPS]
    assert len(set(ids)) == len(ids)
    common = set(ga.SPEC) - set(ga.G1_ONLY)
    assert {op.name for op in OPS if op.list == 0} == set(ga.SPEC)
    assert {op.name for op in OPS if op.list == 1} == common
    assert [op.name for op in OPS if op.list == 2] == ["glv_decompose"]
    for lst, words in ga.SCALAR_WORDS.items():
        assert sorted(op.kp for op in OPS if op.list == lst and op.name == "scalar_mul") == sorted(words)
    for op in OPS:
        assert op.group == 1
        if op.list < 2:                                   # one record per coordinate over Fq, two over Fq2
            kinds, outk, _ = ga.SPEC[op.name]
            nc = op.list + 1
            assert len(op.ins) == sum(ga.NCOORD[k] * nc if k in ga.NCOORD else 1 for k in kinds), op.id
            assert len(op.outs) == {"jac": 3 * nc, "xyzz": 4 * nc, "aff": 2 * nc, "bool": 1}[outk], op.id
            assert all(lu == 2 for b, lu in op.ins + op.outs if b > 0), op.id
    split = next(op for op in OPS if op.list == 2)
    assert split.ins == [(-2, 0)] and split.outs == [(-1, 0), (0, 0), (0, 0)]


@pytest.mark.parametrize("op", OPS, ids=_ids)
def test_cases_meet_the_type_invariants_and_the_size(op):
    """no case is dropped after construction: the number of distinct cases is the size the operation is to have"""
    _need(op)
    cols, wants = ga.cases_for(op, OPS)
    C = len(wants)
    assert all(len(c) == C for c in cols)
    want_n = ga.N_GLV if op.list == 2 else (ga.N_SMUL if op.name == "scalar_mul" else ga.N_CHEAP)[op.list]
    assert C == want_n == ga.size_of(op)
    assert ga.distinct(cols) == C, (op.id, ga.distinct(cols))
    for (B, LU), col in zip(op.ins, cols):
        if B > 0:
            assert all(da.check_limbs(r, B, LU, Q) for r in col), op.id
        elif B == 0:
            assert all(r[0] in (0, 1) and not any(r[1:]) for r in col), op.id
        else:
            assert all(0 <= int(w) < 1 << 32 for r in col for w in r[:8]) and all(r[8] == 0 for r in col), op.id
            if B == -3:
                assert all(not any(r[LU:8]) for r in col), op.id


def test_lane_group_case_sets(dev_ops):
    for op in dev_ops:
        if op.list == 3:
            cols, wants = ga.cases_for(op, dev_ops)
            assert len(wants) == ga.distinct(cols) == ga.N_LANE[op.name[:2]]
            assert all(da.check_limbs(r, B, LU, Q) for (B, LU), col in zip(op.ins, cols) for r in col)
            assert sum(w is None for w in wants) >= len(wants) // 8


def _rows(op):
    cols, wants = ga.cases_for(op, OPS)
    return [[c[i] for c in cols] for i in range(len(wants))], wants


def _point_operands(sh, op, row):
    return [(k, recs) for k, recs in ga.split_operands(sh, ga.SPEC[op.name][0], row) if k in ga.NCOORD]


@pytest.mark.parametrize("op", BIN, ids=_ids)
def test_binary_case_mix(op):
    """from the oracle alone: the doubling result (2P, not infinity), the infinity result and each operand at infinity
    take an eighth of the cases at least; for the signed forms, an eighth of all cases under each value of negate"""
    _need(op)
    sh = ga.shape(op, OPS)
    C_ = sh.C
    kinds = ga.SPEC[op.name][0]
    rows, wants = _rows(op)
    n = len(rows)
    count = {}
    for row, want in zip(rows, wants):
        args = ga.read_args(sh, kinds, row)
        P, Qp = args[0], args[1]
        neg = args[2] if "f" in kinds else 0
        Qe = ga._signed(C_, Qp, neg)
        facts = {"left infinite": C_.is_zero(P), "right infinite": C_.is_zero(Qp), "infinity result": want is None,
                 "doubling result": not C_.is_zero(P) and not C_.is_zero(Qe) and C_.equals(P, Qe) and want is not None,
                 "P == -Q": not C_.is_zero(P) and not C_.is_zero(Qe) and C_.equals(P, C_.negate(Qe))}
        if facts["doubling result"]:
            assert want == da.oracle_affine(C_, C_.twice(P))
        for k, v in facts.items():
            count[(k, neg)] = count.get((k, neg), 0) + bool(v)
    for neg in ((0, 1) if "f" in kinds else (0,)):
        for k in ("left infinite", "right infinite", "infinity result", "doubling result"):
            assert 8 * count[(k, neg)] >= n, (op.id, k, neg, count[(k, neg)], n)
        # kind (c) is one case in eight; the signed forms share it between the two values of negate
        assert (16 if "f" in kinds else 8) * count[("P == -Q", neg)] >= n, (op.id, neg, count[("P == -Q", neg)])


@pytest.mark.parametrize("op", [x for x in OPS if x is not None and x.list < 2 and set(ga.SPEC[x.name][0]) & set("jxs")]
                         or [None], ids=_ids)
def test_infinity_takes_every_multiple_of_p(op):
    """every Jacobian / XYZZ operand is infinite as every tuple of multiples of p its Z / ZZ bound admits (over Fq2:
    every pair), and an infinite XYZZ operand has ZZZ = 0 mod p as well"""
    _need(op)
    sh = ga.shape(op, OPS)
    nc = sh.fld.nc
    rows, _ = _rows(op)
    seen = {}
    for row in rows:
        for pos, (k, recs) in enumerate(_point_operands(sh, op, row)):
            if k == "a":
                continue
            z = [da.from_limbs(r) for r in recs[2 * nc:3 * nc]]
            if all(v % Q == 0 for v in z):
                seen.setdefault(pos, set()).add(tuple(v // Q for v in z))
                if k != "j":
                    assert all(da.from_limbs(r) % Q == 0 for r in recs[3 * nc:]), op.id
    for pos, (k, _) in enumerate(_point_operands(sh, op, rows[0])):
        if k != "a":
            assert seen[pos] == set(ga.inf_multiples(ga.marker_bounds(sh, k))), (op.id, pos)
            assert len(seen[pos]) == ga.kcount(ga.marker_bounds(sh, k)[0]) ** nc >= 2


def _at_top(recs, bounds, which):
    """every component of a coordinate within 64 steps of the top of its bound (grouparith.top_values)"""
    for r, B in zip(recs, bounds):
        if which == "vmax":
            ok = 0 <= da.vmax(B, Q) - da.from_limbs(r) < 64
        else:
            m = da.maximal(B, 2, Q)
            ok = list(r[:8]) == m[:8] and 0 <= m[8] - int(r[8]) < 64
        if not ok:
            return False
    return True


@pytest.mark.parametrize("op", BIN, ids=_ids)
def test_the_largest_representatives_are_met(op):
    """counted from the records: the largest + k p a component's bound admits, with k >= 1, occurs on EVERY component
    of both operands, once at least in a case with no exception and once with P == Q.  The one exemption is ZZ and ZZZ
    of the affine + affine accumulator, which are the Montgomery one by contract and take no offset.  And every
    coordinate of both operands sits at the top of its bound in a case with no exception, once as the largest value
    below the bound and once as the all-limbs-maximal record (every component of it at once; within the 64 steps the
    search for a root may take)"""
    _need(op)
    sh = ga.shape(op, OPS)
    C_, nc = sh.C, sh.fld.nc
    kinds = ga.SPEC[op.name][0]
    rows, wants = _rows(op)
    hit = {}
    tops = set()
    for row, want in zip(rows, wants):
        args = ga.read_args(sh, kinds, row)
        P, Qe = args[0], ga._signed(C_, args[1], args[2] if "f" in kinds else 0)
        if C_.is_zero(P) or C_.is_zero(Qe) or want is None:
            continue
        cls = "P == Q" if C_.equals(P, Qe) else "plain"
        for pos, (k, recs) in enumerate(_point_operands(sh, op, row)):
            by_coord = sh.a + sh.x[2:] if k == "s" else sh.bounds(k)
            for j, (r, B) in enumerate(zip(recs, [b for co in by_coord for b in co])):
                v = da.from_limbs(r)
                if v // Q >= 1 and v // Q == ga.kmax(v % Q, B):
                    hit.setdefault((pos, j), set()).add(cls)
            if cls == "plain":
                for co, bounds in enumerate(by_coord):
                    for which in ("vmax", "maximal"):
                        if _at_top(recs[co * nc:(co + 1) * nc], bounds, which):
                            tops.add((pos, co, which))
    want_hit, want_tops = set(), set()
    for pos, (k, recs) in enumerate(_point_operands(sh, op, rows[0])):
        fixed = 2 * nc if k == "s" else len(recs)         # the accumulator's ZZ = ZZZ = one
        want_hit |= {(pos, j) for j in range(fixed)}
        want_tops |= {(pos, co, which) for co in range(fixed // nc) for which in ("vmax", "maximal")}
    assert want_tops == set(ga.top_forms(kinds[:2])[1:])
    assert set(hit) == want_hit and all(v == {"plain", "P == Q"} for v in hit.values()), (op.id, hit)
    assert tops >= want_tops, (op.id, want_tops - tops)


def test_the_accumulator_of_the_affine_plus_affine_form_is_in_contract():
    """xyzz_add_affine2_lazy takes what xyzz_from_affine_signed returns: ZZ = ZZZ = the Montgomery one and X, Y within
    the AFFINE bound, or infinity; so that is all the cases hold (the XYZZ type alone would admit more)"""
    _need(OPS[0])
    op = next(x for x in OPS if x.id == "g1:xyzz_add_affine2_lazy")
    sh = ga.shape(op, OPS)
    rows, _ = _rows(op)
    for row in rows:
        X, Y, ZZ, ZZZ = (da.from_limbs(r) for r in row[:4])
        assert da.check_limbs(row[0], sh.a[0][0], 2, Q) and da.check_limbs(row[1], sh.a[1][0], 2, Q)
        assert (ZZ, ZZZ) == (da.RQ, da.RQ) or (ZZ % Q == 0 and ZZZ % Q == 0)
    assert any(row[:2] == [da.to_limbs(0)] * 2 and da.from_limbs(row[2]) % Q == 0 for row in rows)


def test_the_named_cases_are_there():
    _need(OPS[0])
    by = {op.id: op for op in OPS}
    lim = lambda e: [(e >> (32 * i)) & 0xffffffff for i in range(8)] + [0]  # noqa: E731
    for op_id, words in (("g1:scalar_mul<8>", 8), ("g1:scalar_mul<4>", 4), ("g2:scalar_mul<8>", 8)):
        rows, wants = _rows(by[op_id])
        es = [r[-1] for r in rows]
        named = [0, 1, 2, (1 << 128) - 1, 1 << 127]
        named += [o.R - 1, o.R, o.R + 1, (1 << 256) - 1, 1 << 255] if words == 8 else []
        for e in named:
            assert es.count(lim(e)) >= 2, (op_id, hex(e))
    # the subgroup check: [r] P is infinity on the subgroup and is not on the twist outside it
    op = by["g2:scalar_mul<8>"]
    sh = ga.shape(op, OPS)
    rows, wants = _rows(op)
    inside = outside = 0
    for row, want in zip(rows, wants):
        P, e = ga.read_args(sh, "ae", row)
        if e == o.R and not o.G2.is_zero(P):
            on_sub = o.G2.is_zero(o.G2.mul(P, o.R))
            assert (want is None) == on_sub
            inside += on_sub
            outside += not on_sub
    assert inside >= 3 and outside >= 3
    for name in ("jac_dbl", "jac_madd", "jac_add", "xyzz_madd", "xyzz_add"):   # twist points outside the subgroup
        op = by["g2:" + name]
        rows, _ = _rows(op)
        far = 0
        for row in rows[2:64:3]:
            P = ga.read_args(sh, ga.SPEC[name][0], row)[0]
            far += (not o.G2.is_zero(P)) and o.G2.on_curve(P) and not o.G2.is_zero(o.G2.mul(P, o.R))
        assert far >= 4, name
    rows, wants = _rows(by["misc:glv_decompose"])
    from test_glv_split import EDGE, UNREDUCED
    have = {sum(int(w) << (32 * j) for j, w in enumerate(r[0][:8])) for r in rows}
    assert set(EDGE) | set(UNREDUCED) <= have
    # (the split rounds both quotients down, so k1 is never negative and k2 nearly always: both values of its flag occur)
    assert sum(w[2] for w in wants) > 100 and sum(not w[2] for w in wants) >= 10
    for cv in ("g1", "g2"):                              # every spelling of the affine zero, and one slot off each
        rows, wants = _rows(by[cv + ":is_inf_aff"])
        nc = 1 if cv == "g1" else 2
        vals = {tuple(da.from_limbs(r) for r in row) for row in rows}
        assert set(itertools.product((0, Q), repeat=2 * nc)) <= vals
        assert sum(w[0] for w in wants) == 4 ** nc
        assert sum(1 for v in vals if sum(x % Q != 0 for x in v) == 1) >= 4 * nc


@pytest.mark.parametrize("op", OPS, ids=_ids)
def test_group_op_on_the_host(op):
    _need(op)
    cols, wants = ga.cases_for(op, OPS)
    ga.check(op, cols, wants, ga.run_host(ga.load_host(), op, cols))
