"""Exact-integer model of the KZG multi-opening, on top of tests/kzg_ref.py and
tests/kzg_set_ref.py: the grouped sum of rows and the values at every row's own points in host integers, the prover
with a known tau (every commitment and proof point is [p(tau)] g1), the two challenges, the opening's bytes and the
verifier over oracle.bn254 and the model pairing.  Written from the protocol's description (Boneh, Drake, Fisch,
Gabizon: the two-element scheme), not from octopuszk_amd/kzg.py or csrc/kzg_multi.cuh, which the tests compare with
it."""
import hashlib

import codec_ref as ref
import kzg_ref as kr
import kzg_set_ref as ks
from oracle import bn254 as o

R = o.R
GAMMA_TAG = b"OZK-kzg-multi-gamma"
Z_TAG = b"OZK-kzg-multi-z"
RHO_TAG = b"OZK-kzg-multi-rho"


# ---------------------------------------------------------------------------- the two kernels
def combine_groups(rows, weights, group_of, groups):
    """out[g][j] = sum_{i : group_of[i] = g} w_i rows[i][j]; a group with no row is a zero row"""
    n = len(rows[0])
    out = [[0] * n for _ in range(groups)]
    for row, w, g in zip(rows, weights, group_of):
        for j in range(n):
            out[g][j] = (out[g][j] + w * row[j]) % R
    return out


def values_at(rows, sets):
    """the values of row i at its own points (which may repeat)"""
    return [[kr.horner(p, z % R) for z in s] for p, s in zip(rows, sets)]


# ---------------------------------------------------------------------------- the protocol in the exponent
def group_rows(sets):
    """(the distinct sets as sorted tuples, in the order their first rows come; the group of every row)"""
    keys, group_of = [], []
    for s in sets:
        key = tuple(sorted(s))
        if key not in keys:
            keys.append(key)
        group_of.append(keys.index(key))
    return keys, group_of


def challenges(commitments, sets, values, w) -> tuple:
    """(gamma, z); commitments and w: compressed encodings"""
    body = len(sets).to_bytes(8, "little")
    for c, s, ys in zip(commitments, sets, values):
        body += len(s).to_bytes(8, "little") + b"".join(kr.le(z) for z in s) + c + b"".join(kr.le(y) for y in ys)
    d = hashlib.sha256(GAMMA_TAG + body).digest()
    return int.from_bytes(d[:16], "little") or 1, int.from_bytes(hashlib.sha256(Z_TAG + d + w).digest()[:16], "little") or 1


def _product(z, points):
    acc = 1
    for p in points:
        acc = acc * (z - p) % R
    return acc


def at_z(sets, values, gamma, z):
    """(gamma^i c_i per row for c_i = Z_{T \\ S_i}(z), sum_i gamma^i c_i r_i(z), Z_T(z)): T the union of the sets, r_i the
    interpolant of row i's values on its set"""
    union = sorted({p for s in sets for p in s})
    weights, total = [], 0
    for i, (s, ys) in enumerate(zip(sets, values)):
        w = pow(gamma, i, R) * _product(z, [p for p in union if p not in s]) % R
        weights.append(w)
        total = (total + w * kr.horner(ks.interpolate(list(s), list(ys)), z)) % R
    return weights, total, _product(z, union)


def prove(rows, sets, tau, commitments=None):
    """The prover with a known tau.  Returns a dict: the scalars of C_i, W and W' (their logarithms to g1), the values,
    the challenges, L(z) and the sum it must equal."""
    values = values_at(rows, sets)
    logs = [kr.horner(p, tau) for p in rows]
    if commitments is None:
        commitments = [ref.encode_g1(kr.g1_mul(o.G1.one, c)) for c in logs]
    keys, group_of = group_rows(sets)
    n = len(rows[0])
    gamma, _ = challenges(commitments, sets, values, bytes(32))
    f = combine_groups(rows, [pow(gamma, i, R) for i in range(len(rows))], group_of, len(keys))
    h = [0] * n
    for fg, key in zip(f, keys):
        q, _ = ks.div_set(fg, list(key))
        h = [(a + b) % R for a, b in zip(h, q)]
    w_log = kr.horner(h, tau)
    w = ref.encode_g1(kr.g1_mul(o.G1.one, w_log))
    gamma, z = challenges(commitments, sets, values, w)
    weights, total, z_t = at_z(sets, values, gamma, z)
    big_l = [(-z_t * hj) % R for hj in h]
    for g, (fg, key) in enumerate(zip(f, keys)):
        c_g = _product(z, [p for p in sorted({p for s in sets for p in s}) if p not in key])
        big_l = [(a + c_g * b) % R for a, b in zip(big_l, fg)]
    q2, l_at_z = kr.div_linear(big_l, z)
    return {"commitments": commitments, "logs": logs, "values": values, "gamma": gamma, "z": z, "w": w, "w_log": w_log,
            "w2_log": kr.horner(q2, tau), "w2": ref.encode_g1(kr.g1_mul(o.G1.one, kr.horner(q2, tau))),
            "l_at_z": l_at_z, "sum_at_z": total}


def opening_of(proof, sets) -> bytes:
    return opening_bytes(proof["commitments"], sets, proof["values"], proof["w"], proof["w2"])


# ---------------------------------------------------------------------------- bytes and the verifier
def opening_bytes(commitments, sets, values, w, w2) -> bytes:
    """commitments, w, w2: compressed encodings"""
    out = len(sets).to_bytes(4, "little")
    for c, s, ys in zip(commitments, sets, values):
        out += c + len(s).to_bytes(4, "little") + b"".join(kr.le(z) for z in s) + b"".join(kr.le(y) for y in ys)
    return out + w + w2


def parse_opening(b):
    """(commitments, sets, values, w, w2) of well-formed bytes"""
    k, at = int.from_bytes(b[:4], "little"), 4
    cs, sets, values = [], [], []
    for _ in range(k):
        t = int.from_bytes(b[at + 32:at + 36], "little")
        cs.append(b[at:at + 32])
        sets.append(kr.ints(b[at + 36:at + 36 + 32 * t]))
        values.append(kr.ints(b[at + 36 + 32 * t:at + 36 + 64 * t]))
        at += 36 + 64 * t
    assert len(b) == at + 64
    return cs, sets, values, b[at:at + 32], b[at + 32:]


def _point(enc):
    code, P = ref.decode_g1(enc)
    assert code == 0
    return o.G1.to_affine(P)


def verify(g1, g2, tau_g2, opening: bytes) -> bool:
    """e(F + [z] W', g2) e(-W', tau_g2) = 1 for F = sum_i gamma^i c_i C_i - [sum_i gamma^i c_i r_i(z)] g1 - [Z_T(z)] W,
    with the model pairing; O on the left of a pairing gives 1"""
    import pairing_ref as pr
    cs, sets, values, w, w2 = parse_opening(opening)
    if any(len(set(s)) != len(s) for s in sets):
        return False
    gamma, z = challenges(cs, sets, values, w)
    weights, total, z_t = at_z(sets, values, gamma, z)
    W, W2 = _point(w), _point(w2)
    lhs = kr.g1_add(kr.g1_mul(g1, R - total), kr.g1_mul(W, R - z_t))
    for c, wt in zip(cs, weights):
        lhs = kr.g1_add(lhs, kr.g1_mul(_point(c), wt))
    lhs = kr.g1_add(lhs, kr.g1_mul(W2, z))
    acc = pr.F12_ONE
    for P, Qp in ((lhs, g2), (o.G1.to_affine(o.G1.negate(W2)), tau_g2)):
        if not o.G1.is_zero(P):
            acc = pr.f12_mul(acc, pr.reduced_pairing(P, Qp))
    return acc == pr.F12_ONE


def rho(seed: bytes, n: int):
    out = []
    for j in range((n + 1) // 2):
        block = hashlib.sha256(RHO_TAG + seed + j.to_bytes(8, "little")).digest()
        out += [int.from_bytes(block[:16], "little") or 1, int.from_bytes(block[16:], "little") or 1]
    return out[:n]
