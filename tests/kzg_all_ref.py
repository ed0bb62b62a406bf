"""Exact-integer model of KZG openings at every coset of the evaluation domain at once, on top of
tests/kzg_ref.py, over a string of KNOWN tau: a group element [a] g1 is the integer a modulo r, a transform "in the
exponent" is a number-theoretic transform of those integers.  Two routes to the same r = n / l proofs:

  definition   q_k = floor(p / (X^l - omega^(k l))) by long division, evaluated at tau;
  model        the five steps of the FK20 construction: transforms of the reversed, strided powers of tau (once per
               key), transforms of the strided coefficients, the products summed over the l residues, an inverse
               transform whose upper half is taken, and one transform of size r.

Written from the construction's description, not from octopuszk_amd/kzg.py, which the tests compare with it."""
import kzg_ref as kr
from oracle import bn254 as o

R = o.R
CHECKED_SHAPES = ((2, 1), (2, 2), (4, 1), (8, 4), (16, 1), (16, 4), (16, 16), (32, 2))


def coset(n, l, k):
    """S_k = (omega^(k + r j))_j, j < l, for the n-th root omega and r = n / l"""
    r, omega = n // l, kr.root(n)
    return [pow(omega, k + r * j, R) for j in range(l)]


def divide_by_binomial(p, l, a):
    """floor(p / (X^l - a)): q_j = p_{j + l} + a q_{j + l}, from the top"""
    n = len(p)
    q = [0] * max(n - l, 0)
    for j in range(n - l - 1, -1, -1):
        q[j] = (p[j + l] + a * (q[j + l] if j + l < len(q) else 0)) % R
    return q


def proofs_by_definition(p, l, tau):
    """[q_k(tau)]_k, k < r: the logarithm of every proof"""
    n = len(p)
    r, omega = n // l, kr.root(n)
    return [kr.horner(divide_by_binomial(p, l, pow(omega, k * l, R)), tau) for k in range(r)]


def key_tables(n, l, tau):
    """step 1: X_v = transform of (tau^(l (r - 1 - j) + v), j < r, then r zeros) with the 2r-th root, v < l"""
    r = n // l
    w2 = kr.root(2 * r)
    return [kr.ntt([pow(tau, l * (r - 1 - j) + v, R) for j in range(r)] + [0] * r, w2) for v in range(l)]


def model(p, l, tau):
    """(proofs, W): the logarithms of the r proofs by steps 1 to 5, and the 2r entries of the inverse transform of step 4
    (() for r = 1, where the one proof is O)"""
    n = len(p)
    r = n // l
    assert n >= 2 and n & (n - 1) == 0 and 1 <= l <= n and l & (l - 1) == 0
    if r == 1:
        return [0], ()
    w2 = kr.root(2 * r)
    X = key_tables(n, l, tau)
    c = [kr.ntt([p[l * i + v] % R for i in range(r)] + [0] * r, w2) for v in range(l)]
    U = [sum(c[v][i] * X[v][i] for v in range(l)) % R for i in range(2 * r)]
    W = kr.intt(U, w2)
    return kr.ntt(W[r:], pow(kr.root(n), l, R)), W


def values(p):
    """p(omega^i), i < n, by Horner"""
    omega = kr.root(len(p))
    return [kr.horner(p, pow(omega, i, R)) for i in range(len(p))]


def rows(n, rng):
    """the three checked row shapes: random, a lone top coefficient, a lone constant"""
    return [[rng.randrange(R) for _ in range(n)], [0] * (n - 1) + [rng.randrange(1, R)], [rng.randrange(1, R)] + [0] * (n - 1)]
