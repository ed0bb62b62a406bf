"""Exact-integer model of KZG set openings, on top of tests/kzg_ref.py: the vanishing polynomial
expanded and schoolbook long division by it, Lagrange interpolation, the evaluation-form quotient as the transform of
the coefficient-form quotient (so it shares no formula with the kernel), the set verifier over oracle.bn254 and the
model pairing, the byte formats and the gamma derivation.  Written from the protocol's description, not from
octopuszk_amd/kzg.py or csrc/kzg_set.cuh, which the tests compare with it."""
import hashlib

import codec_ref as ref
import kzg_ref as kr
from oracle import bn254 as o

R = o.R
GAMMA_TAG = b"OZK-kzg-set-gamma"
RHO_TAG = b"OZK-kzg-set-rho"


# ---------------------------------------------------------------------------- polynomials
def vanishing(points):
    """the t + 1 coefficients of prod (X - z_i), lowest first (monic)"""
    z = [1]
    for p in points:
        z = [((z[j - 1] if j else 0) - p * (z[j] if j < len(z) else 0)) % R for j in range(len(z) + 1)]
    return z


def long_division(p, d):
    """(quotient, remainder) of p by the monic d, schoolbook from the top; the remainder has len(d) - 1 entries"""
    t = len(d) - 1
    assert d[t] == 1
    rem = [c % R for c in p]
    quot = [0] * max(len(p) - t, 0)
    for j in range(len(p) - 1, t - 1, -1):
        c = rem[j]
        quot[j - t] = c
        for k in range(t + 1):
            rem[j - t + k] = (rem[j - t + k] - c * d[k]) % R
    return quot, (rem + [0] * t)[:t]


def interpolate(points, values):
    """the coefficients (len(points) of them) of the polynomial of degree < t through (z_i, y_i)"""
    t = len(points)
    out = [0] * t
    for i in range(t):
        others = [points[k] for k in range(t) if k != i]
        num = vanishing(others)
        den = 1
        for zk in others:
            den = den * (points[i] - zk) % R
        s = values[i] * pow(den, -1, R) % R
        for j in range(t):
            out[j] = (out[j] + s * num[j]) % R
    return out


def div_set(p, points):
    """(q, values): the quotient row of len(p) entries, q_0 .. q_{len-t-1} then zeros, and p(z_i)"""
    q, _ = long_division(p, vanishing(points))
    return (q + [0] * len(p))[:len(p)], [kr.horner(p, z) for z in points]


def open_set_evals(f, points, omega):
    """(q(omega^i), values) for the interpolant p of f on the domain of omega: through the coefficients"""
    q, values = div_set(kr.intt(f, omega), points)
    return kr.ntt(q, omega), values


# ---------------------------------------------------------------------------- group side
def g2_mul(P, k):
    k %= R
    return o.G2.to_affine(o.G2.mul(P, k)) if k and not o.G2.is_zero(P) else o.G2.to_affine(o.G2.zero)


def g2_commit(tau_g2, p):
    acc = o.G2.zero
    for P, c in zip(tau_g2, p):
        acc = o.G2.add(acc, g2_mul(P, c))
    return o.G2.to_affine(acc)


def string(t_max, tau):
    """(tau_g1[:t_max], tau_g2[:t_max + 1]) over the generators"""
    return ([kr.g1_mul(o.G1.one, pow(tau, i, R)) for i in range(t_max)],
            [g2_mul(o.G2.one, pow(tau, i, R)) for i in range(t_max + 1)])


def verify(tau_g1, tau_g2, C, points, values, pi) -> bool:
    """e(C - [I(tau)] g1, g2) e(-pi, [Z_S(tau)] g2) = 1; O on the left of a pairing gives 1, [Z_S(tau)] g2 = O fails"""
    import pairing_ref as pr
    if len(set(points)) != len(points):
        return False
    zs = g2_commit(tau_g2, vanishing(points))
    if o.G2.is_zero(zs):
        return False
    lhs = kr.g1_add(C, o.G1.to_affine(o.G1.negate(kr.commit(tau_g1, interpolate(points, values)))))
    acc = pr.F12_ONE
    for P, Qp in ((lhs, tau_g2[0]), (o.G1.to_affine(o.G1.negate(pi)), zs)):
        if not o.G1.is_zero(P):
            acc = pr.f12_mul(acc, pr.reduced_pairing(P, Qp))
    return acc == pr.F12_ONE


# ---------------------------------------------------------------------------- bytes and hashes
def opening_bytes(C, points, values, pi) -> bytes:
    return (ref.encode_g1(C) + len(points).to_bytes(4, "little") + b"".join(kr.le(z) for z in points)
            + b"".join(kr.le(y) for y in values) + ref.encode_g1(pi))


def vk_bytes(tau_g1, tau_g2) -> bytes:
    return (len(tau_g1).to_bytes(4, "little") + b"".join(ref.encode_g1(P) for P in tau_g1)
            + b"".join(ref.encode_g2(P) for P in tau_g2))


def gamma(points, commitments, values) -> int:
    """commitments: K compressed encodings; values: K rows of t"""
    h = hashlib.sha256(GAMMA_TAG + len(commitments).to_bytes(8, "little") + len(points).to_bytes(8, "little")
                       + b"".join(kr.le(z) for z in points) + b"".join(commitments)
                       + b"".join(kr.le(v) for row in values for v in row)).digest()
    return int.from_bytes(h[:16], "little") or 1


def rho(seed: bytes, n: int):
    out = []
    for j in range((n + 1) // 2):
        block = hashlib.sha256(RHO_TAG + seed + j.to_bytes(8, "little")).digest()
        out += [int.from_bytes(block[:16], "little") or 1, int.from_bytes(block[16:], "little") or 1]
    return out[:n]
