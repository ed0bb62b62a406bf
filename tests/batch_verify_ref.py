"""The randomized batch check of Groth16 proofs restated on tests/pairing_ref.py (the oracle of
ozk_groth16_wellformed_dev and ozk_groth16_verify_rlc_dev).

    FE( prod_i ML(r_i A_i, B_i) * (ML(ABC*, gamma) ML(C*, delta))^-1 ) == alphaBeta^S
    ABC* = sum_j s_j gammaABC_j,  s_j = sum_i r_i x_ij mod r,  C* = sum_i r_i C_i,  S = sum_i r_i
"""
import pairing_ref as pr
from oracle import bn254 as o

Q, R = pr.Q, pr.R


def g1_on_curve_jac(P) -> bool:
    X, Y, Z = P
    if Z % Q == 0:
        return False
    z6 = pow(Z, 6, Q)
    return (Y * Y - X ** 3 - 3 * z6) % Q == 0


def g2_on_twist_jac(P) -> bool:
    F = o.Fq2Ops
    X, Y, Z = P
    if F.is_zero(Z):
        return False
    z2 = F.sqr(Z)
    z6 = F.mul(F.sqr(z2), z2)
    rhs = F.add(F.mul(F.sqr(X), X), F.mul(o.G2.b, z6))
    return F.eq(F.sqr(Y), rhs)


def g2_in_subgroup(P) -> bool:
    """[r]P = O: the definition of the order-r subgroup"""
    return o.G2.is_zero(o.G2.mul(P, R))


def point_wellformed(kind, P) -> bool:
    if kind == 1:
        return g1_on_curve_jac(P)
    return g2_on_twist_jac(P) and g2_in_subgroup(P)


def _coords(b: bytes):
    """64-byte LE wire-out values -> ints, None if one is not canonical (upper half non-zero or >= q)"""
    out = []
    for i in range(len(b) // 64):
        v = int.from_bytes(b[64 * i:64 * i + 64], "little")
        if v >= Q:
            return None
        out.append(v)
    return out


def record_wellformed(rec: bytes) -> bool:
    """the flag of one 768-byte record A | B | C"""
    a, b, c = _coords(rec[:192]), _coords(rec[192:576]), _coords(rec[576:])
    if a is None or b is None or c is None:
        return False
    B = ((b[0], b[1]), (b[2], b[3]), (b[4], b[5]))
    return g1_on_curve_jac(tuple(a)) and g1_on_curve_jac(tuple(c)) and point_wellformed(2, B)


def combination(primaries, rs):
    """(s_j for every input j, S)"""
    n = len(primaries[0])
    s = [sum(r * x for r, x in zip(rs, (p[j] for p in primaries))) % R for j in range(n)]
    return s, sum(rs)


def rlc_verify(alpha_g1_beta_g2, gamma_g2, delta_g2, gamma_abc_g1, primaries, proofs, rs) -> bool:
    """proofs as (A, B, C) Jacobian triples, all well-formed; rs the weights.  The batch equation as it stands."""
    s, S = combination(primaries, rs)
    abc = o.G1.zero
    for sj, g in zip(s, gamma_abc_g1):
        abc = o.G1.add(abc, o.G1.mul(g, sj))
    cs = o.G1.zero
    for r, (_, _, C) in zip(rs, proofs):
        cs = o.G1.add(cs, o.G1.mul(C, r))
    f = pr.F12_ONE
    for r, (A, B, _) in zip(rs, proofs):
        f = pr.f12_mul(f, pr.ate_miller(o.G1.mul(A, r), B))
    key = pr.f12_mul(pr.ate_miller(abc, gamma_g2), pr.ate_miller(cs, delta_g2))
    lhs = pr.final_exponentiation(pr.f12_mul(f, pr.f12_inv(key)))
    return lhs == pr.f12_cyclotomic_exp(alpha_g1_beta_g2, S)


def cancelling_pair(proof):
    """the same valid proof twice with A_1 + G and A_2 - G: the unweighted sum of the two equations still holds
    (e(A + G, B) e(A - G, B) = e(A, B)^2), so only the random weights catch it"""
    A, B, C = proof
    return [(o.G1.add(A, o.G1.one), B, C), (o.G1.add(A, o.G1.negate(o.G1.one)), B, C)]
