"""The BN254a pairing without a GPU: the Python restatement (tests/pairing_ref.py) against the properties the
reference's own tests pin, the generated constants against values derived here, and the device tower and pairing
(fq12.cuh, compiled for the host by g++ from tests/native/pairing_hostcheck.cpp) against the restatement."""
import ctypes
import importlib.util
import os
import random
import subprocess

import pytest

import pairing_ref as pr
from oracle import bn254 as o
from oracle import groth16 as g
from oracle.javarand import fp_random

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "pairing_hostcheck.cpp")
LIB = os.path.join(HERE, "native", "_pairing_hostcheck.so")
Q = pr.Q


def rand_f12(rng):
    return pr.fq12_from_flat(rng.randrange(Q) for _ in range(12))


# ---------------------------------------------------------------------------- oracle pins
def test_final_exponentiation_is_the_power_map():
    """BNFinalExponentiationTest.java:43-66: the chunked final exponentiation equals
    f^((q^12 - 1)/r * 2z(6z^2 + 3z + 1)) for a random f (the hard part is the Fuentes-Castaneda multiple)."""
    f = rand_f12(random.Random(7))
    z = pr.FINAL_EXPONENT_Z
    e = (Q ** 12 - 1) // pr.R
    assert e * pr.R == Q ** 12 - 1
    assert pr.final_exponentiation(f) == pr.f12_pow(f, e * 2 * z * (6 * z * z + 3 * z + 1))


def test_bilinearity():
    """BilinearityTest.java:50-80 with P = g1 random(5), Q = g2 random(6)."""
    a, b = fp_random(5, o.R), fp_random(6, o.R)
    P, Qp = o.G1.mul(o.G1.one, a), o.G2.mul(o.G2.one, b)
    ePQ = pr.reduced_pairing(P, Qp)
    e1 = pr.reduced_pairing(o.G1.one, o.G2.one)
    assert pr.reduced_pairing(o.G1.mul(P, 3), Qp) == pr.f12_pow(ePQ, 3)
    assert pr.reduced_pairing(P, o.G2.mul(Qp, 3)) == pr.f12_pow(ePQ, 3)
    assert ePQ == pr.f12_pow(e1, a * b % o.R)


def test_non_degenerate_and_order_r():
    e1 = pr.reduced_pairing(o.G1.one, o.G2.one)
    assert e1 != pr.F12_ONE
    assert pr.f12_pow(e1, o.R) == pr.F12_ONE


def test_cyclotomic_squaring_after_the_first_chunk():
    f = pr.ate_miller(o.G1.mul(o.G1.one, 9), o.G2.one)
    x = pr.final_exp_first_chunk(f)
    assert pr.f12_cyclotomic_sqr(x) == pr.f12_sqr(x)


def _gen():
    spec = importlib.util.spec_from_file_location("gen_pairing_consts", os.path.join(ROOT, "tools", "gen_pairing_consts.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_generated_constants():
    m = _gen()
    c = m.derive()
    u = 4965661367192848881
    assert c["ate_loop_count"] == 6 * u + 2 == 29793968203157093288
    assert (c["ate_loop_count"].bit_length(), bin(c["ate_loop_count"]).count("1")) == (65, 37)
    assert c["final_exponent_z"] == u and (u.bit_length(), bin(u).count("1")) == (63, 28)
    assert c["fq2_frob_c1"] == [1, Q - 1]
    assert c["fq6_frob_c1"] == pr.FQ6_FROB_C1 and c["fq6_frob_c2"] == pr.FQ6_FROB_C2
    assert c["fq12_frob_c1"] == pr.FQ12_FROB_C1
    # the defining identities, independently of how the powers were taken
    assert o.Fq2Ops.mul(c["twist_b"], (9, 1)) == (3, 0)
    assert pr.f2_pow(c["fq6_frob_c1"][1], 3) == pr.f2_pow((9, 1), Q - 1)
    assert pr.f2_pow(c["fq12_frob_c1"][1], 6) == pr.f2_pow((9, 1), Q - 1)
    assert c["q_x_mul_twist"] == c["fq6_frob_c1"][1]
    assert pr.f2_pow(c["q_y_mul_twist"], 2) == pr.f2_pow((9, 1), Q - 1)
    # the untwist-Frobenius-twist map keeps a G2 point on the curve
    x, y, _ = pr.mul_by_q(o.G2.to_affine(o.G2.mul(o.G2.one, 77)))
    assert o.G2.on_curve((x, y, (1, 0)))
    # the committed header is the generator's output
    with open(m.PATH) as f:
        assert f.read() == m.render()
    assert m.ate_steps(c["ate_loop_count"]).count(0) == 64 and len(m.ate_steps(c["ate_loop_count"])) == 102


# ---------------------------------------------------------------------------- oracle verifier
@pytest.fixture(scope="module")
def proof_2p10():
    r1cs, primary, auxiliary = g.serial_construct(1 << 10, 15)
    crs = g.serial_setup(r1cs)
    (A, B, C), _ = g.serial_prove(crs, primary, auxiliary)
    ab = pr.reduced_pairing(crs.alpha_g1, crs.beta_g2)
    return crs, ab, primary, (A, B, C)


def _verify(crs, ab, primary, proof):
    return pr.verify(ab, crs.gamma_g2, crs.delta_g2, crs.gamma_abc_g1, primary, proof)


def tamperings(primary, proof):
    """the five tampered (primary, proof) pairs every verifier test rejects"""
    A, B, C = proof
    bad_primary = list(primary)
    bad_primary[1] = (bad_primary[1] + 1) % o.R
    return [
        ("A+g1", primary, (o.G1.add(A, o.G1.one), B, C)),
        ("B+g2", primary, (A, o.G2.add(B, o.G2.one), C)),
        ("C+g1", primary, (A, B, o.G1.add(C, o.G1.one))),
        ("primary", bad_primary, (A, B, C)),
        ("A<->C", primary, (C, B, A)),
    ]


def test_oracle_verifier_accepts_and_rejects(proof_2p10):
    crs, ab, primary, proof = proof_2p10
    assert _verify(crs, ab, primary, proof)
    for name, pri, prf in tamperings(primary, proof):
        assert not _verify(crs, ab, pri, prf), name


# ---------------------------------------------------------------------------- device headers on the host
@pytest.fixture(scope="module")
def hc():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(
            os.path.getmtime(p) for p in [SRC] + [os.path.join(ROOT, "octopuszk_amd", "csrc", h)
                                                  for h in ("fq12.cuh", "fq2.cuh", "fp29.cuh", "pairing_consts_gen.h")]):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-maybe-uninitialized", "-shared", "-fPIC",
                               "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


def _w(vals):
    b = b"".join(int(v).to_bytes(32, "little") for v in vals)
    return ctypes.create_string_buffer(b, len(b))


def _out(words):
    return ctypes.create_string_buffer(4 * words)


def _vals(buf, n):
    return [int.from_bytes(buf.raw[32 * i:32 * i + 32], "little") for i in range(n)]


def f6_flat(a):
    return [a[j][k] for j in range(3) for k in range(2)]


def f6_from_flat(v):
    return tuple((v[2 * j], v[2 * j + 1]) for j in range(3))


def edge_f12s(rng):
    """operands at the edges: 0, 1, p - 1 in every slot, single non-zero slots, and random values"""
    out = [pr.fq12_from_flat([Q - 1] * 12), pr.fq12_from_flat([1] * 12), pr.F12_ONE]
    for i in range(12):
        v = [0] * 12
        v[i] = Q - 1
        out.append(pr.fq12_from_flat(v))
    out += [rand_f12(rng) for _ in range(6)]
    return out


F6_OPS = {0: lambda a, b: pr.f6_mul(a, b), 1: lambda a, b: pr.f6_sqr(a), 2: lambda a, b: pr.f6_inv(a),
          3: lambda a, b: pr.f6_frob(a, 1), 4: lambda a, b: pr.f6_frob(a, 2), 5: lambda a, b: pr.f6_frob(a, 3),
          6: lambda a, b: pr.f6_mul_by_v(a)}
F12_OPS = {0: lambda a, b: pr.f12_mul(a, b), 1: lambda a, b: pr.f12_sqr(a), 2: lambda a, b: pr.f12_inv(a),
           3: lambda a, b: pr.f12_frob(a, 1), 4: lambda a, b: pr.f12_frob(a, 2), 5: lambda a, b: pr.f12_frob(a, 3),
           6: lambda a, b: pr.f12_cyclotomic_sqr(a), 7: lambda a, b: pr.f12_conj(a)}


@pytest.mark.parametrize("hi", [0, 1])
def test_fq6_ops(hc, hi):
    rng = random.Random(61 + hi)
    vals = [f6_from_flat(pr.fq12_flat(x)[:6]) for x in edge_f12s(rng)]
    for a in vals:
        b = vals[rng.randrange(len(vals))]
        for op, fn in F6_OPS.items():
            if op == 2 and a == pr.F6_ZERO:
                continue
            out = _out(48)
            hc.pc_f6_op(op, hi, _w(f6_flat(a)), _w(f6_flat(b)), out)
            assert f6_from_flat(_vals(out, 6)) == fn(a, b), (op, a, b)


@pytest.mark.parametrize("hi", [0, 1])
def test_fq12_ops(hc, hi):
    rng = random.Random(71 + hi)
    vals = edge_f12s(rng)
    for a in vals:
        b = vals[rng.randrange(len(vals))]
        for op, fn in F12_OPS.items():
            out = _out(96)
            hc.pc_f12_op(op, hi, _w(pr.fq12_flat(a)), _w(pr.fq12_flat(b)), out)
            assert pr.fq12_from_flat(_vals(out, 12)) == fn(a, b), (op, a, b)
        out = _out(96)
        ell = [vals[rng.randrange(len(vals))][0][j] for j in range(3)]
        hc.pc_mul_by_024(hi, _w(pr.fq12_flat(a)), _w([c for e in ell for c in e]), out)
        assert pr.fq12_from_flat(_vals(out, 12)) == pr.f12_mul_by_024(a, ell[0], ell[1], ell[2])


def test_final_exponentiation_parts(hc):
    rng = random.Random(3)
    for a in [rand_f12(rng) for _ in range(2)]:
        for op, fn in ((9, pr.final_exp_first_chunk), (10, pr.exp_by_neg_z), (8, pr.final_exponentiation)):
            out = _out(96)
            hc.pc_f12_op(op, 0, _w(pr.fq12_flat(a)), _w(pr.fq12_flat(a)), out)
            assert pr.fq12_from_flat(_vals(out, 12)) == fn(a), op


def _jac_g1(rng, P):
    """P in Jacobian coordinates with a random Z != 1 (the pairing normalises any Z)"""
    if o.G1.is_zero(P):
        return (0, 1, 0)
    x, y, _ = o.G1.to_affine(P)
    z = rng.randrange(2, Q)
    return (x * z * z % Q, y * z * z * z % Q, z)


def _jac_g2(rng, P):
    F = o.Fq2Ops
    if o.G2.is_zero(P):
        return ((0, 0), (1, 0), (0, 0))
    x, y, _ = o.G2.to_affine(P)
    z = (rng.randrange(Q), rng.randrange(Q))
    z2 = F.sqr(z)
    return (F.mul(x, z2), F.mul(y, F.mul(z2, z)), z)


def pairing_cases(seed, n):
    """n random pairs (Z != 1 on both sides) plus P, Q and both at infinity"""
    rng = random.Random(seed)
    cases = []
    for _ in range(n):
        P = o.G1.mul(o.G1.one, rng.randrange(1, o.R))
        Qp = o.G2.mul(o.G2.one, rng.randrange(1, o.R))
        cases.append((_jac_g1(rng, P), _jac_g2(rng, Qp)))
    P0, Q0 = cases[0]
    cases += [((0, 1, 0), Q0), (P0, ((0, 0), (1, 0), (0, 0))), ((0, 1, 0), ((0, 0), (1, 0), (0, 0)))]
    return cases


def g2_flat(Qp):
    return [c for x in Qp for c in x]


def test_miller_loop_and_reduced_pairing(hc):
    for P, Qp in pairing_cases(17, 8):
        out = _out(96)
        hc.pc_pairing(0, _w(P), _w(g2_flat(Qp)), out)
        assert pr.fq12_from_flat(_vals(out, 12)) == pr.ate_miller(P, Qp)
        hc.pc_pairing(1, _w(P), _w(g2_flat(Qp)), out)
        assert out.raw == pr.reduced_pairing_bytes(P, Qp)


def test_infinity_runs_the_java_arithmetic(hc):
    """an input at infinity runs the Java's arithmetic on (0, 1, 0).  P at infinity: the Java's value (which here is
    the GT identity, although the Miller value is not one).  Q at infinity: the Miller value is zero, so the Java's final exponentiation throws (it inverts
    zero); the device's inversion maps 0 to 0 and the bytes are all zero."""
    P = o.G1.mul(o.G1.one, 11)
    want = pr.reduced_pairing((0, 1, 0), o.G2.one)
    assert pr.ate_miller((0, 1, 0), o.G2.one) != pr.F12_ONE
    out = _out(96)
    hc.pc_pairing(1, _w((0, 1, 0)), _w(g2_flat(o.G2.one)), out)
    assert out.raw == pr.gt_bytes(want)
    for p in (P, (0, 1, 0)):
        assert pr.ate_miller(p, o.G2.zero) == pr.F12_ZERO
        with pytest.raises(ValueError):
            pr.final_exponentiation(pr.F12_ZERO)
        hc.pc_pairing(1, _w(p), _w(g2_flat(((0, 0), (1, 0), (0, 0)))), out)
        assert out.raw == bytes(384)


def test_prepared_coefficients(hc):
    Qp = o.G2.mul(o.G2.one, 1234567)
    out = _out(102 * 48)
    hc.pc_prepare(_w(g2_flat(Qp)), out)
    v = _vals(out, 102 * 6)
    got = [((v[6 * s], v[6 * s + 1]), (v[6 * s + 2], v[6 * s + 3]), (v[6 * s + 4], v[6 * s + 5])) for s in range(102)]
    assert got == pr.precompute_g2(Qp)
