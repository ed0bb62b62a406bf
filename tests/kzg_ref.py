"""Exact-integer model of the KZG layer over oracle.bn254: division by X - z with the plain
recurrence, evaluation by Horner, a number-theoretic transform, the evaluation-form opening as the transform of the
coefficient-form quotient (and so independent of the formulas the kernel uses), the verification equation through
tests/pairing_ref.py, and the gamma and rho derivations.  Written from the protocol's description, not from
octopuszk_amd/kzg.py or csrc/kzg.cuh, which the tests compare with it."""
import hashlib

import codec_ref as ref
from oracle import bn254 as o

R = o.R
GAMMA_TAG = b"OZK-kzg-gamma"
RHO_TAG = b"OZK-kzg-rho"
OPENING_BYTES, VK_BYTES = 128, 160


def le(v: int) -> bytes:
    return (int(v) % (1 << 256)).to_bytes(32, "little")


def ints(b: bytes):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


# ---------------------------------------------------------------------------- polynomials
def horner(p, z):
    acc = 0
    for c in reversed(p):
        acc = (acc * z + c) % R
    return acc


def div_linear(p, z):
    """(q, y) with p(X) - y = q(X) (X - z): q has len(p) entries, the last one 0 (the layout of the quotient row)"""
    n = len(p)
    q = [0] * n
    for j in range(n - 1, 0, -1):
        q[j - 1] = (p[j] + z * q[j]) % R
    return q, (p[0] + z * q[0]) % R


def root(n: int) -> int:
    return o.fr_root_of_unity(n) if n > 1 else 1


def ntt(a, omega):
    """[sum_i a_i omega^(i j)]_j, by the definition for short inputs and radix 2 above"""
    n = len(a)
    if n <= 8:
        return [sum(a[i] * pow(omega, i * j, R) for i in range(n)) % R for j in range(n)]
    even, odd = ntt(a[0::2], omega * omega % R), ntt(a[1::2], omega * omega % R)
    out, w = [0] * n, 1
    for j in range(n // 2):
        t = w * odd[j] % R
        out[j], out[j + n // 2] = (even[j] + t) % R, (even[j] - t) % R
        w = w * omega % R
    return out


def intt(f, omega):
    n_inv = pow(len(f), -1, R)
    return [v * n_inv % R for v in ntt(f, pow(omega, -1, R))]


def open_evals(f, z, omega):
    """(q_i = q(omega^i), y) for the interpolant p of f on the domain of omega: through the coefficients"""
    q, y = div_linear(intt(f, omega), z)
    return ntt(q, omega), y


def combine(rows, weights):
    return [sum(w * row[j] for w, row in zip(weights, rows)) % R for j in range(len(rows[0]))]


# ---------------------------------------------------------------------------- group side
def g1_mul(P, k):
    k %= R
    return o.G1.to_affine(o.G1.mul(P, k)) if k and not o.G1.is_zero(P) else o.G1.to_affine(o.G1.zero)


def g1_add(P, Q):
    return o.G1.to_affine(o.G1.add(P, Q))


def commit(tau_g1, p):
    acc = o.G1.zero
    for P, c in zip(tau_g1, p):
        acc = o.G1.add(acc, g1_mul(P, c))
    return o.G1.to_affine(acc)


def string(n, tau, g1=o.G1.one, g2=o.G2.one):
    """(tau_g1[:n], (g2, [tau] g2))"""
    return [g1_mul(g1, pow(tau, i, R)) for i in range(n)], (o.G2.to_affine(g2), o.G2.to_affine(o.G2.mul(g2, tau % R)))


def verify(g1, g2, tau_g2, C, z, y, pi) -> bool:
    """e(C - [y] g1 + [z] pi, g2) e(-pi, tau_g2) = 1 with the model pairing; O on the left of a pairing gives 1"""
    import pairing_ref as pr
    lhs = g1_add(g1_add(C, g1_mul(g1, R - y % R)), g1_mul(pi, z))
    acc = pr.F12_ONE
    for P, Qp in ((lhs, g2), (o.G1.negate(pi), tau_g2)):
        if not o.G1.is_zero(P):
            acc = pr.f12_mul(acc, pr.reduced_pairing(P, Qp))
    return acc == pr.F12_ONE


# ---------------------------------------------------------------------------- bytes and hashes
def opening_bytes(C, z, y, pi) -> bytes:
    return ref.encode_g1(C) + le(z) + le(y) + ref.encode_g1(pi)


def vk_bytes(g1, g2, tau_g2) -> bytes:
    return ref.encode_g1(g1) + ref.encode_g2(g2) + ref.encode_g2(tau_g2)


def gamma(z, commitments, values) -> int:
    """commitments: compressed encodings"""
    h = hashlib.sha256(GAMMA_TAG + len(commitments).to_bytes(8, "little") + le(z) + b"".join(commitments)
                       + b"".join(le(v) for v in values)).digest()
    return int.from_bytes(h[:16], "little") or 1


def rho(seed: bytes, n: int):
    out = []
    for j in range((n + 1) // 2):
        block = hashlib.sha256(RHO_TAG + seed + j.to_bytes(8, "little")).digest()
        out += [int.from_bytes(block[:16], "little") or 1, int.from_bytes(block[16:], "little") or 1]
    return out[:n]
