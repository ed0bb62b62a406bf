"""The DEVICE branch of the arithmetic headers against exact integers (tests/native/devcheck.hip, tests/devarith.py).

Every field operation runs on 2^16 lanes (4096 distinct cases, each repeated 16 times over 256 blocks: a fault that
shows on some waves or some launches only makes the copies disagree) at the bounds its production call sites
instantiate and at the extreme its static_assert admits.  Every output must be congruent to the exact result,
have limbs 0..7 below the limit of its type and a value below the bound its type claims (reported by the harness
from the C++ type).  The lane-group code (lane-pair Fq2, lane-quad G1, lane-octet G2) holds one case per group;
neighbouring groups hold different cases, and every lane of a group must return the whole result."""
import collections

import numpy as np
import pytest

import devarith as da
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

LANES = 1 << 16
COUNTS = collections.OrderedDict()


@pytest.fixture(scope="module")
def dc():
    lib = da.load()
    yield lib
    if COUNTS:
        print("\ndevice arithmetic cases (distinct cases x lanes):")
        for k, v in COUNTS.items():
            print("  %-40s %6d x %d" % (k, v[0], v[1]))


def _run(lib, op, cols, group):
    """cols: per operand element a list of C records; each case on `group` adjacent lanes, the whole repeated up to
    LANES lanes.  Returns the outputs of the first copy, shape (C, NOUT, 9), after checking every copy agrees."""
    import torch
    C = len(cols[0])
    nin, nout = len(op.ins), len(op.outs)
    a = np.asarray(cols, dtype=np.uint32).reshape(nin, C, 9)
    a = np.repeat(a, group, axis=1)                    # (nin, C * group, 9)
    rep = max(1, LANES // (C * group))
    a = np.tile(a, (1, rep, 1))
    n = a.shape[1]
    d_in = torch.from_numpy(a.view(np.int32).copy()).cuda()
    d_out = torch.zeros((n, nout, 9), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream()
    rc = lib.dc_run(op.field, op.idx, d_in.data_ptr(), d_out.data_ptr(), n, s.cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint32).reshape(rep, C, group, nout, 9)
    bad = np.nonzero((out != out[0:1, :, 0:1]).any(axis=(3, 4)))
    assert bad[0].size == 0, "%s: copies disagree (copy, case, lane): %s" % (
        op.id, list(zip(*[b[:5].tolist() for b in bad])))
    COUNTS[op.id] = (C, n)
    return out[0, :, 0]


def _check_element(op, what, rec, B, LU, p, want=None, exact=False):
    """one output element: limbs and value within its type's claim, and (if given) the expected value"""
    v = da.from_limbs(rec)
    assert all(int(x) < LU << 28 for x in rec[:8]), "%s %s: limbs %s above LU %d" % (op.id, what, list(rec), LU)
    assert 16 * v < B * p, "%s %s: value %d/16 p above its bound %d/16 p" % (op.id, what, 16 * v // p, B)
    if want is not None:
        ok = v == want if exact else (v - want) % p == 0
        assert ok, "%s %s: got %#x, want %#x%s" % (op.id, what, v, want, "" if exact else " (mod p)")
    return v


_LOAD_ERROR = []


def _ops(fields):
    """the harness's operation lists (read at collection); a harness that fails to build or load fails the tests of
    this module, one each, instead of aborting the collection of the whole session"""
    try:
        lib = da.load()
        return [op for f in fields for op in da.ops(lib, f)]
    except Exception as e:  # noqa: BLE001 (reported by the test below)
        _LOAD_ERROR.append("%s: %s" % (type(e).__name__, e))
        return [None]


def _ids(op):
    return op.id if op is not None else "harness-unavailable"


def _need(op):
    if op is None:
        pytest.fail("tests/native/devcheck.hip did not build or load: " + "; ".join(_LOAD_ERROR))


@pytest.mark.parametrize("op", _ops((0, 1)), ids=_ids)
def test_field_op_at_its_bounds(dc, op):
    _need(op)
    p = da.FIELDS[op.field]
    C = 4096
    cols = da.operand_sets(op, C, seed=op.idx * 7 + op.field)
    out = _run(dc, op, cols, 1)
    (BO, LO), = op.outs
    for i in range(C):
        if op.ins[0][0] == -2:
            vals = [sum(int(w) << (32 * j) for j, w in enumerate(cols[0][i][:8]))]
        else:
            vals = [da.from_limbs(c[i]) for c in cols]
        want, exact = da.field_expect(op, vals)
        rec = out[i, 0]
        what = "case %d in %s" % (i, [hex(v) for v in vals])
        if BO == 0:                                   # bool
            assert int(rec[0]) == want and not rec[1:].any(), "%s %s: got %d want %d" % (op.id, what, rec[0], want)
        elif BO == -1:                                # packed words
            got = sum(int(w) << (32 * j) for j, w in enumerate(rec[:8]))
            assert got == want, "%s %s: packed %#x" % (op.id, what, got)
        else:
            _check_element(op, what, rec, BO, LO, p, want, exact)


def _check_fq2(dc, op):
    C = 4096
    cols = da.operand_sets(op, C, seed=100 + op.idx)
    out = _run(dc, op, cols, op.group)
    for i in range(C):
        vals = [da.from_limbs(c[i]) for c in cols]
        want = da.fq2_expect(op.name, vals)
        for j, (B, LU) in enumerate(op.outs):
            if B == 0:                                    # bool (fq2_is_zero)
                assert int(out[i, j][0]) == want[j] and not out[i, j][1:].any(), "%s case %d in %s: got %d want %d" % (
                    op.id, i, [hex(v) for v in vals], out[i, j][0], want[j])
                continue
            _check_element(op, "case %d c%d" % (i, j), out[i, j], B, LU, o.Q, want[j])


# ---- points: Montgomery coordinates, any representative the coordinate's bound admits
def _coord_recs(x, F, k, rng):
    """records of coordinate x (Montgomery, canonical) plus k p on every component"""
    return [da.to_limbs(c + k * o.Q) for c in da.comps(x, F)]


def _jac_recs(C, A, z, ks, rng):
    """affine A under Z = z (oracle values) -> Montgomery X | Y | Z records, plus ks[i] p"""
    F = C.F
    if A is None:                                   # infinity: Z = ks[2] p, X and Y some point's
        X, Y, Z = F.one, F.one, F.zero
    else:
        z2 = F.sqr(z)
        X, Y, Z = F.mul(A[0], z2), F.mul(A[1], F.mul(z2, z)), z
    out = []
    for c, k in zip((X, Y, Z), ks):
        out += _coord_recs(da.tomont(c, F), F, k, rng)
    return out


def _rand_el(F, rng):
    return rng.randrange(1, o.Q) if F is o.FqOps else (rng.randrange(o.Q), rng.randrange(1, o.Q))


def _point_cases(C, op, n, seed):
    """(operand records, expected affine or None) for jac_dbl / jac_add: random points, P + P under different Z,
    P + (-P), infinity as Z = 0 and Z = k p on either side, coordinates up to their bounds (X + k p)"""
    import random
    rng = random.Random(seed)
    F = C.F
    nc = len(da.comps(F.one, F))
    bx, by, bz = op.ins[0][0], op.ins[nc][0], op.ins[2 * nc][0]
    kmax = [max(0, b // 16 - 1) for b in (bx, by, bz)]
    pts = da.random_points(C, n, seed)
    cases = []
    for i in range(n):
        A = (pts[i][0], pts[i][1])
        kind = i % 8
        ks = [rng.randint(0, k) for k in kmax]
        z = _rand_el(F, rng)
        if op.name.endswith("dbl"):
            if kind == 7:
                recs, want = _jac_recs(C, None, z, [0, 0, rng.randint(0, kmax[2])], rng), None
            else:
                recs = _jac_recs(C, A, z, ks, rng)
                want = da.oracle_affine(C, C.twice((A[0], A[1], F.one)))
            cases.append((recs, want))
            continue
        B = (pts[(i + 1) % n][0], pts[(i + 1) % n][1])
        ks2 = [rng.randint(0, k) for k in kmax]
        z2 = _rand_el(F, rng)
        if kind == 1:
            B = A                                           # P + P under another Z
        elif kind == 2:
            B = (A[0], F.neg(A[1]))                         # P + (-P)
        if kind == 3:
            P_, Q_ = None, B
        elif kind == 4:
            P_, Q_ = A, None
        elif kind == 5:
            P_, Q_ = None, None
        else:
            P_, Q_ = A, B
        kz = [0, 0, rng.randint(0, kmax[2])]
        r1 = _jac_recs(C, P_, z, ks if P_ is not None else kz, rng)
        r2 = _jac_recs(C, Q_, z2, ks2 if Q_ is not None else kz, rng)
        J = lambda X: (X[0], X[1], F.one) if X is not None else C.zero
        want = da.oracle_affine(C, C.add(J(P_), J(Q_)))
        cases.append((r1 + r2, want))
    return cases


def _check_points(dc, op, C, n, seed):
    F = C.F
    cases = _point_cases(C, op, n, seed)
    cols = [list(c) for c in zip(*[r for r, _ in cases])]
    out = _run(dc, op, cols, op.group)
    nc = len(da.comps(F.one, F))
    for i, (_, want) in enumerate(cases):
        coords = []
        for c in range(3):
            v = []
            for j in range(nc):
                B, LU = op.outs[c * nc + j]
                v.append(_check_element(op, "case %d coord %d.%d" % (i, c, j), out[i, c * nc + j], B, LU, o.Q))
            coords.append(v[0] if nc == 1 else (v[0] % o.Q, v[1] % o.Q))
        got = da.affine_of_jac(C, *[x % o.Q if nc == 1 else x for x in coords])
        assert got == want, "%s case %d (kind %d): got %s want %s" % (op.id, i, i % 8, got, want)


def _check_madd(dc, op, n=1024, seed=7):
    """G1 xyzz_madd_lazy (the bucket accumulation's hot loop), both signs: random, P = +-Q (doubling / infinity
    through either sign), Q at infinity, the accumulator at infinity as ZZ = 0 and as ZZ = p"""
    import random
    rng = random.Random(seed)
    C, F = o.G1, o.FqOps
    pts = da.random_points(C, n + 1, seed)
    bX, bY = op.ins[0][0], op.ins[1][0]
    cols_cases, wants = [], []
    for i in range(n):
        A, Bq = pts[i][:2], pts[i + 1][:2]
        kind = i % 8
        neg = rng.randrange(2)
        if kind == 1:
            Bq = A
        elif kind == 2:
            Bq = (A[0], F.neg(A[1]))
        z = _rand_el(F, rng)
        z2 = F.sqr(z)
        acc_inf = kind in (4, 5)
        X, Y, ZZ, ZZZ = F.mul(A[0], z2), F.mul(A[1], F.mul(z2, z)), z2, F.mul(z2, z)
        recs = [da.to_limbs(da.tomont(X, F) + rng.randint(0, bX // 16 - 1) * o.Q),
                da.to_limbs(da.tomont(Y, F) + rng.randint(0, bY // 16 - 1) * o.Q)]
        if acc_inf:
            recs += [da.to_limbs(0 if kind == 4 else o.Q)] * 2
        else:
            recs += [da.to_limbs(da.tomont(ZZ, F)), da.to_limbs(da.tomont(ZZZ, F))]
        q_inf = kind == 3
        recs += [da.to_limbs(0), da.to_limbs(0)] if q_inf else [da.to_limbs(da.tomont(Bq[0], F)),
                                                                 da.to_limbs(da.tomont(Bq[1], F))]
        recs.append([neg] + [0] * 8)
        P_ = C.zero if acc_inf else (A[0], A[1], F.one)
        Q_ = C.zero if q_inf else (Bq[0], Bq[1] if not neg else F.neg(Bq[1]), F.one)
        cols_cases.append(recs)
        wants.append(da.oracle_affine(C, C.add(P_, Q_)))
    cols = [list(c) for c in zip(*cols_cases)]
    out = _run(dc, op, cols, 1)
    for i, want in enumerate(wants):
        v = [_check_element(op, "case %d coord %d" % (i, j), out[i, j], B, LU, o.Q) for j, (B, LU) in enumerate(op.outs)]
        got = da.affine_of_xyzz(C, *[x % o.Q for x in v])
        assert got == want, "%s case %d (kind %d): got %s want %s" % (op.id, i, i % 8, got, want)


@pytest.mark.parametrize("op", _ops((2,)), ids=_ids)
def test_ext_op_at_its_bounds(dc, op):
    _need(op)
    if op.name.startswith("fq2_"):
        _check_fq2(dc, op)
    elif op.name == "g1_xyzz_madd":
        _check_madd(dc, op)
    elif op.name.startswith("g1_jac"):
        _check_points(dc, op, o.G1, 1024, seed=11 + op.idx)
    elif op.name.startswith("g2_jac"):
        _check_points(dc, op, o.G2, 256, seed=13 + op.idx)
    else:
        raise AssertionError("no check for " + op.id)
