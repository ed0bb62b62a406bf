"""Pure-Python (exact `int`) restatement of the reference's BN254a optimal-ate pairing and Groth16 verifier.

TEST INFRASTRUCTURE ONLY: the oracle of tests/test_pairing_*.py and tests/test_groth16_verify_gpu.py.  Built on
oracle.bn254's field and curve classes (imported, not modified).  Paths are relative to the reference's
src/main/java/:

    algebra/fields/Fp6_3Over2.java                       Fq6 = Fq2[v]/(v^3 - xi), xi = 9 + u
    algebra/fields/Fp12_2Over3Over2.java                 Fq12 = Fq6[w]/(w^2 - v)
    algebra/curves/barreto_naehrig/BNPairing.java        precomputeG2, millerLoop, finalExponentiation
    algebra/curves/barreto_naehrig/bn254a/BN254aPublicParameters.java:25-41   twist, loop count, z
    zk_proof_systems/zkSNARK/Verifier.java:24-59         verify

The constants are derived here from their definitions (powers of xi), not copied.  Elements: Fq2 = (c0, c1),
Fq6 = (c0, c1, c2) of Fq2, Fq12 = (c0, c1) of Fq6.
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import bn254 as o  # noqa: E402

Q = o.Q
R = o.R
F2 = o.Fq2Ops

XI = (9, 1)                                   # BN254aFq6Parameters.java:35 / BN254aFq12Parameters.java:37
U = 4965661367192848881                       # the BN parameter u; finalExponentZ = u, positive
ATE_LOOP_COUNT = 6 * U + 2                    # 29793968203157093288
FINAL_EXPONENT_Z = U
IS_ATE_LOOP_COUNT_NEGATIVE = False
IS_FINAL_EXPONENT_Z_NEGATIVE = False


def f2_pow(a, e):
    r = F2.one
    while e:
        if e & 1:
            r = F2.mul(r, a)
        a = F2.sqr(a)
        e >>= 1
    return r


def f2_frob(a, k):  # Fp2.java FrobeniusMap: c1 * nonresidue^((q^k - 1)/2) = (-1)^k
    return (a[0], a[1] if k % 2 == 0 else (-a[1]) % Q)


def f2_scale(a, c):
    return ((a[0] * c) % Q, (a[1] * c) % Q)


TWIST_B = F2.mul((3, 0), F2.inv(XI))                          # BN254aPublicParameters.java:26
FQ6_FROB_C1 = [f2_pow(XI, (Q ** k - 1) // 3) for k in range(6)]
FQ6_FROB_C2 = [f2_pow(XI, 2 * (Q ** k - 1) // 3) for k in range(6)]
FQ12_FROB_C1 = [f2_pow(XI, (Q ** k - 1) // 6) for k in range(12)]
Q_X_MUL_TWIST = FQ6_FROB_C1[1]                                # xi^((q-1)/3)
Q_Y_MUL_TWIST = f2_pow(XI, (Q - 1) // 2)                      # xi^((q-1)/2)


def mul_xi(a):  # Fp6_3Over2.java:32-34 mulByNonResidue
    return F2.mul(XI, a)


# ---------------------------------------------------------------------------- Fq6 (Fp6_3Over2.java)
F6_ZERO = (F2.zero, F2.zero, F2.zero)
F6_ONE = (F2.one, F2.zero, F2.zero)


def f6_add(a, b):
    return tuple(F2.add(x, y) for x, y in zip(a, b))


def f6_sub(a, b):
    return tuple(F2.sub(x, y) for x, y in zip(a, b))


def f6_neg(a):
    return tuple(F2.neg(x) for x in a)


def f6_mul(a, b):  # Fp6_3Over2.java:35-49 (Karatsuba)
    c0C0, c1C1, c2C2 = F2.mul(a[0], b[0]), F2.mul(a[1], b[1]), F2.mul(a[2], b[2])
    c0F = F2.sub(F2.sub(F2.mul(F2.add(a[1], a[2]), F2.add(b[1], b[2])), c1C1), c2C2)
    c1F = F2.sub(F2.sub(F2.mul(F2.add(a[0], a[1]), F2.add(b[0], b[1])), c0C0), c1C1)
    c2F = F2.sub(F2.add(F2.sub(F2.mul(F2.add(a[0], a[2]), F2.add(b[0], b[2])), c0C0), c1C1), c2C2)
    return (F2.add(c0C0, mul_xi(c0F)), F2.add(c1F, mul_xi(c2C2)), c2F)


def f6_sqr(a):  # Fp6_3Over2.java:72-87 (CH-SQR2)
    s0 = F2.sqr(a[0])
    c0c1 = F2.mul(a[0], a[1])
    s1 = F2.add(c0c1, c0c1)
    s2 = F2.sqr(F2.add(F2.sub(a[0], a[1]), a[2]))
    c1c2 = F2.mul(a[1], a[2])
    s3 = F2.add(c1c2, c1c2)
    s4 = F2.sqr(a[2])
    return (F2.add(s0, mul_xi(s3)), F2.add(s1, mul_xi(s4)),
            F2.sub(F2.sub(F2.add(F2.add(s1, s2), s3), s0), s4))


def f6_inv(a):  # Fp6_3Over2.java:88-103 (Algorithm 17)
    c0, c1, c2 = a
    t0, t1, t2 = F2.sqr(c0), F2.sqr(c1), F2.sqr(c2)
    t3, t4, t5 = F2.mul(c0, c1), F2.mul(c0, c2), F2.mul(c1, c2)
    s0 = F2.sub(t0, mul_xi(t5))
    s1 = F2.sub(mul_xi(t2), t3)
    s2 = F2.sub(t1, t4)
    t6 = F2.inv(F2.add(F2.mul(c0, s0), mul_xi(F2.add(F2.mul(c2, s1), F2.mul(c1, s2)))))
    return (F2.mul(t6, s0), F2.mul(t6, s1), F2.mul(t6, s2))


def f6_frob(a, k):  # Fp6_3Over2.java:104-109
    return (f2_frob(a[0], k), F2.mul(FQ6_FROB_C1[k % 6], f2_frob(a[1], k)),
            F2.mul(FQ6_FROB_C2[k % 6], f2_frob(a[2], k)))


def f6_mul_f2(a, c):
    return tuple(F2.mul(x, c) for x in a)


def f6_mul_by_v(a):  # Fp12_2Over3Over2.java:33-35 mulByNonResidue: (xi c2, c0, c1)
    return (mul_xi(a[2]), a[0], a[1])


# ---------------------------------------------------------------------------- Fq12 (Fp12_2Over3Over2.java)
F12_ONE = (F6_ONE, F6_ZERO)


def f12_mul(a, b):  # Fp12_2Over3Over2.java:36-45
    c0C0, c1C1 = f6_mul(a[0], b[0]), f6_mul(a[1], b[1])
    return (f6_add(c0C0, f6_mul_by_v(c1C1)),
            f6_sub(f6_sub(f6_mul(f6_add(a[0], a[1]), f6_add(b[0], b[1])), c0C0), c1C1))


def f12_sqr(a):  # Fp12_2Over3Over2.java:67-76 (complex squaring)
    c0c1 = f6_mul(a[0], a[1])
    factor = f6_mul(f6_add(a[0], a[1]), f6_add(a[0], f6_mul_by_v(a[1])))
    return (f6_sub(f6_sub(factor, c0c1), f6_mul_by_v(c0c1)), f6_add(c0c1, c0c1))


def f12_inv(a):  # Fp12_2Over3Over2.java:77-85 (Algorithm 8)
    t0, t1 = f6_sqr(a[0]), f6_sqr(a[1])
    t3 = f6_inv(f6_sub(t0, f6_mul_by_v(t1)))
    return (f6_mul(a[0], t3), f6_neg(f6_mul(a[1], t3)))


def f12_frob(a, k):  # Fp12_2Over3Over2.java:86-91
    return (f6_frob(a[0], k), f6_mul_f2(f6_frob(a[1], k), FQ12_FROB_C1[k % 12]))


def f12_conj(a):  # Fp12_2Over3Over2.java:92-94 unitaryInverse
    return (a[0], f6_neg(a[1]))


def _sq_pair(x, y):  # (x + y s)^2 over Fq2[s]/(s^2 - xi), as cyclotomicSquared writes it
    tmp = F2.mul(x, y)
    t0 = F2.sub(F2.sub(F2.mul(F2.add(x, y), F2.add(x, mul_xi(y))), tmp), mul_xi(tmp))
    return t0, F2.add(tmp, tmp)


def f12_cyclotomic_sqr(a):  # Fp12_2Over3Over2.java:95-151
    z0, z4, z3 = a[0]
    z2, z1, z5 = a[1]
    t0, t1 = _sq_pair(z0, z1)
    t2, t3 = _sq_pair(z2, z3)
    t4, t5 = _sq_pair(z4, z5)

    def three_minus_two(t, z):  # 3 t - 2 z, as (t - z) + (t - z) + t
        d = F2.sub(t, z)
        return F2.add(F2.add(d, d), t)

    def three_plus_two(t, z):   # 3 t + 2 z
        s = F2.add(t, z)
        return F2.add(F2.add(s, s), t)

    z0 = three_minus_two(t0, z0)
    z1 = three_plus_two(t1, z1)
    z2 = three_plus_two(mul_xi(t5), z2)
    z3 = three_minus_two(t4, z3)
    z4 = three_minus_two(t2, z4)
    z5 = three_plus_two(t3, z5)
    return ((z0, z4, z3), (z2, z1, z5))


def f12_mul_by_024(a, ell0, ellVW, ellVV):  # Fp12_2Over3Over2.java:152-216
    z0, z1, z2 = a[0]
    z3, z4, z5 = a[1]
    x0, x2, x4 = ell0, ellVV, ellVW
    D0, D2, D4 = F2.mul(z0, x0), F2.mul(z2, x2), F2.mul(z4, x4)
    t2 = F2.add(z0, z4)
    t1 = F2.add(z0, z2)
    s0 = F2.add(F2.add(z1, z3), z5)
    S1 = F2.mul(z1, x2)
    T3 = F2.add(S1, D4)
    n0 = F2.add(mul_xi(T3), D0)
    T3 = F2.mul(z5, x4)
    S1 = F2.add(S1, T3)
    T3 = F2.add(T3, D2)
    T4 = mul_xi(T3)
    T3 = F2.mul(z1, x0)
    S1 = F2.add(S1, T3)
    n1 = F2.add(T4, T3)
    t0 = F2.add(x0, x2)
    T3 = F2.sub(F2.sub(F2.mul(t1, t0), D0), D2)
    T4 = F2.mul(z3, x4)
    S1 = F2.add(S1, T4)
    n2 = F2.add(T3, T4)
    t0 = F2.add(z2, z4)
    t1 = F2.add(x2, x4)
    T3 = F2.sub(F2.sub(F2.mul(t0, t1), D2), D4)
    T4 = mul_xi(T3)
    T3 = F2.mul(z3, x0)
    S1 = F2.add(S1, T3)
    n3 = F2.add(T4, T3)
    T3 = F2.mul(z5, x2)
    S1 = F2.add(S1, T3)
    T4 = mul_xi(T3)
    t0 = F2.add(x0, x4)
    T3 = F2.sub(F2.sub(F2.mul(t2, t0), D0), D4)
    n4 = F2.add(T4, T3)
    t0 = F2.add(F2.add(x0, x2), x4)
    n5 = F2.sub(F2.mul(s0, t0), S1)
    return ((n0, n1, n2), (n3, n4, n5))


def f12_cyclotomic_exp(a, e):  # Fp12_2Over3Over2.java:217-230
    res = F12_ONE
    found = False
    for i in range(e.bit_length() - 1, -1, -1):
        if found:
            res = f12_cyclotomic_sqr(res)
        if (e >> i) & 1:
            found = True
            res = f12_mul(res, a)
    return res


def f12_pow(a, e):  # generic square-and-multiply (tests only)
    r = F12_ONE
    for i in range(e.bit_length() - 1, -1, -1):
        r = f12_sqr(r)
        if (e >> i) & 1:
            r = f12_mul(r, a)
    return r


# ---------------------------------------------------------------------------- pairing (BNPairing.java)
TWO_INV = pow(2, -1, Q)


def doubling_step(cur):  # BNPairing.java:84-110; returns (new current, (ell0, ellVW, ellVV))
    X, Y, Z = cur
    A = f2_scale(F2.mul(X, Y), TWO_INV)
    B = F2.sqr(Y)
    C = F2.sqr(Z)
    D = F2.add(F2.add(C, C), C)
    E = F2.mul(TWIST_B, D)
    Fv = F2.add(F2.add(E, E), E)
    G = f2_scale(F2.add(B, Fv), TWO_INV)
    H = F2.sub(F2.sqr(F2.add(Y, Z)), F2.add(B, C))
    I = F2.sub(E, B)
    J = F2.sqr(X)
    ESq = F2.sqr(E)
    new = (F2.mul(A, F2.sub(B, Fv)), F2.sub(F2.sqr(G), F2.add(F2.add(ESq, ESq), ESq)), F2.mul(B, H))
    return new, (mul_xi(I), F2.neg(H), F2.add(F2.add(J, J), J))


def mixed_addition_step(base, cur):  # BNPairing.java:112-136
    X1, Y1, Z1 = cur
    x2, y2 = base[0], base[1]
    D = F2.sub(X1, F2.mul(x2, Z1))
    E = F2.sub(Y1, F2.mul(y2, Z1))
    Fv = F2.sqr(D)
    G = F2.sqr(E)
    H = F2.mul(D, Fv)
    I = F2.mul(X1, Fv)
    J = F2.sub(F2.add(H, F2.mul(Z1, G)), F2.add(I, I))
    new = (F2.mul(D, J), F2.sub(F2.mul(E, F2.sub(I, J)), F2.mul(H, Y1)), F2.mul(Z1, H))
    return new, (mul_xi(F2.sub(F2.mul(E, x2), F2.mul(D, y2))), D, F2.neg(E))


def mul_by_q(P):  # BNPairing.java:138-143
    return (F2.mul(Q_X_MUL_TWIST, f2_frob(P[0], 1)), F2.mul(Q_Y_MUL_TWIST, f2_frob(P[1], 1)), f2_frob(P[2], 1))


def precompute_g1(P):  # BNPairing.java:278-282
    X, Y, _ = o.G1.to_affine(P)
    return X, Y


def precompute_g2(Qp):  # BNPairing.java:284-325: 102 (ell0, ellVW, ellVV) triples
    QA = o.G2.to_affine(Qp)
    cur = (QA[0], QA[1], F2.one)
    coeffs = []
    for i in range(ATE_LOOP_COUNT.bit_length() - 2, -1, -1):   # every bit below the MSB
        cur, c = doubling_step(cur)
        coeffs.append(c)
        if (ATE_LOOP_COUNT >> i) & 1:
            cur, c = mixed_addition_step(QA, cur)
            coeffs.append(c)
    Q1 = mul_by_q(QA)
    Q2 = mul_by_q(Q1)
    Q2 = (Q2[0], F2.neg(Q2[1]), Q2[2])
    cur, c = mixed_addition_step(Q1, cur)
    coeffs.append(c)
    cur, c = mixed_addition_step(Q2, cur)
    coeffs.append(c)
    return coeffs


def miller_loop(Pprec, coeffs):  # BNPairing.java:236-276
    PX, PY = Pprec
    f = F12_ONE
    idx = 0

    def line(f, c):
        return f12_mul_by_024(f, c[0], f2_scale(c[1], PY), f2_scale(c[2], PX))

    for i in range(ATE_LOOP_COUNT.bit_length() - 2, -1, -1):
        f = f12_sqr(f)
        f = line(f, coeffs[idx])
        idx += 1
        if (ATE_LOOP_COUNT >> i) & 1:
            f = line(f, coeffs[idx])
            idx += 1
    f = line(f, coeffs[idx])
    f = line(f, coeffs[idx + 1])
    return f


def exp_by_neg_z(f):  # BNPairing.java:145-151
    r = f12_cyclotomic_exp(f, FINAL_EXPONENT_Z)
    return r if IS_FINAL_EXPONENT_Z_NEGATIVE else f12_conj(r)


def final_exp_first_chunk(f):  # BNPairing.java:153-171
    C = f12_mul(f12_conj(f), f12_inv(f))
    return f12_mul(f12_frob(C, 2), C)


def final_exp_last_chunk(elt):  # BNPairing.java:173-234
    A = exp_by_neg_z(elt)
    B = f12_cyclotomic_sqr(A)
    C = f12_cyclotomic_sqr(B)
    D = f12_mul(C, B)
    E = exp_by_neg_z(D)
    F = f12_cyclotomic_sqr(E)
    G = exp_by_neg_z(F)
    H = f12_conj(D)
    I = f12_conj(G)
    J = f12_mul(I, E)
    K = f12_mul(J, H)
    L = f12_mul(K, B)
    M = f12_mul(K, E)
    N = f12_mul(M, elt)
    O = f12_frob(L, 1)
    P = f12_mul(O, N)
    Qv = f12_frob(K, 2)
    Rv = f12_mul(Qv, P)
    S = f12_conj(elt)
    T = f12_mul(S, L)
    Uv = f12_frob(T, 3)
    return f12_mul(Uv, Rv)


def final_exponentiation(f):  # BNPairing.java:333-336
    return final_exp_last_chunk(final_exp_first_chunk(f))


def ate_miller(P, Qp):
    return miller_loop(precompute_g1(P), precompute_g2(Qp))


def reduced_pairing(P, Qp):  # AbstractPairing.reducedPairing: finalExponentiation(atePairing(P, Q))
    return final_exponentiation(ate_miller(P, Qp))


# ---------------------------------------------------------------------------- wire formats
def fq12_flat(a):
    """the twelve Fq values in the Java's nesting order c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1"""
    return [a[i][j][k] for i in range(2) for j in range(3) for k in range(2)]


def fq12_from_flat(v):
    v = list(v)
    return tuple(tuple((v[6 * i + 2 * j], v[6 * i + 2 * j + 1]) for j in range(3)) for i in range(2))


def gt_bytes(a) -> bytes:
    return b"".join(int(x).to_bytes(32, "little") for x in fq12_flat(a))


F12_ZERO = (F6_ZERO, F6_ZERO)


def reduced_pairing_bytes(P, Qp) -> bytes:
    """the device's GT bytes for (P, Q): the Java's value, or 384 zero bytes where the Miller value is zero (Q at
    infinity: every line's ell0 and ellVW vanish there).  The Java has no value in that case — its final
    exponentiation inverts zero and BigInteger.modInverse throws — and the device's inversion maps 0 to 0."""
    f = ate_miller(P, Qp)
    if f == F12_ZERO:
        return bytes(384)
    return gt_bytes(final_exponentiation(f))


def gt_from_bytes(b: bytes):
    assert len(b) == 384
    return fq12_from_flat(int.from_bytes(b[32 * i:32 * i + 32], "little") for i in range(12))


# ---------------------------------------------------------------------------- Groth16 verify (Verifier.java:24-59)
def verify(alpha_g1_beta_g2, gamma_g2, delta_g2, gamma_abc_g1, primary, proof) -> bool:
    """proof = (A, B, C) as Jacobian triples; gamma_abc_g1 one G1 point per primary input."""
    assert primary[0] == 1
    A, B, C = proof
    AB = reduced_pairing(A, B)
    CDelta = reduced_pairing(C, delta_g2)
    abc = o.G1.zero
    for s, g in zip(primary, gamma_abc_g1):
        abc = o.G1.add(abc, o.G1.mul(g, s % R))
    rhs = f12_mul(f12_mul(alpha_g1_beta_g2, reduced_pairing(abc, gamma_g2)), CDelta)  # GT add = Fq12 product
    return AB == rhs
