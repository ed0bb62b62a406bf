"""Seeded inputs for the codec tests: curve points (some Jacobian with Z != 1, some O) and compressed encodings with
malformed ones of every class mixed in.  Everything comes from oracle.bn254 and tests/codec_ref.py."""
import random

import codec_ref as ref
from oracle import bn254 as o

Q = o.Q
G1_CLASSES = ("x_eq_q", "x_all_ones", "inf_stray_bit", "inf_y_larger", "non_residue")
G2_CLASSES = G1_CLASSES + ("c1_ge_q",)


def curve(type_):
    return o.G1 if type_ == 1 else o.G2


def points(type_, n, seed):
    """n points start + i step of the group (cheap: one addition each), affine; every 7th rescaled to a Jacobian
    form with Z != 1 and every 29th replaced by O (from the second point on, so that n = 1 is a real point)"""
    C, rng = curve(type_), random.Random(seed)
    P = C.mul(C.one, rng.randrange(1, o.R))
    step = C.mul(C.one, rng.randrange(1, o.R))
    out = []
    for i in range(n):
        A = C.to_affine(P)
        if i % 29 == 28:
            A = C.zero
        elif i % 7 == 3:
            A = rescale(type_, A, rng.randrange(2, Q))
        out.append(A)
        P = C.add(P, step)
    return out


def rescale(type_, A, z):
    """the affine point A as the Jacobian (x z^2, y z^3, z)"""
    if type_ == 1:
        return (A[0] * z * z % Q, A[1] * z * z * z % Q, z)
    F = o.Fq2Ops
    zz = (z, (z * 7 + 1) % Q)
    z2 = F.sqr(zz)
    return (F.mul(A[0], z2), F.mul(A[1], F.mul(z2, zz)), zz)


def encode(type_, P):
    return ref.encode_g1(P) if type_ == 1 else ref.encode_g2(P)


def decode(type_, b):
    return ref.decode_g1(b) if type_ == 1 else ref.decode_g2(b)


def wire(type_, P, fmt):
    return ref.g1_wire(P, fmt) if type_ == 1 else ref.g2_wire(P, fmt)


def _le(v):
    return int(v).to_bytes(32, "little")


def _is_residue(v):
    return v % Q == 0 or pow(v, (Q - 1) // 2, Q) == 1


def non_residue_x(type_, rng):
    """an x < q (component-wise) that no curve point has"""
    F = o.Fq2Ops
    while True:
        if type_ == 1:
            x = rng.randrange(Q)
            if not _is_residue(x * x * x + 3):
                return _le(x)
        else:
            x = (rng.randrange(Q), rng.randrange(Q))
            rhs = F.add(F.mul(F.sqr(x), x), o.G2.b)
            if not _is_residue(rhs[0] * rhs[0] + rhs[1] * rhs[1]):
                return _le(x[0]) + _le(x[1])


def malformed(type_, cls, rng, valid):
    """(encoding, the code it must decode to); `valid` is a valid encoding of a finite point to start from"""
    size = 32 * type_
    pre = bytes(valid[:32]) if type_ == 2 else b""   # a valid c0 in front of a bad c1
    flags = rng.choice((0, ref.Y_LARGER))
    if cls == "x_eq_q":
        if type_ == 2:
            return _le(Q) + bytes(valid[32:]), ref.E_RANGE   # c0 = q in front of a valid c1
        b = bytearray(_le(Q))
        b[-1] |= flags
        return bytes(b), ref.E_RANGE
    if cls == "x_all_ones":
        return pre + _le((1 << 254) - 1), ref.E_RANGE
    if cls == "c1_ge_q":
        b = bytearray(pre + _le(rng.randrange(Q, 1 << 254)))
        b[-1] |= flags
        return bytes(b), ref.E_RANGE
    if cls == "inf_stray_bit":
        b = bytearray(size)
        b[-1] = ref.INFINITY
        bit = rng.randrange(8 * size - 2)
        b[bit >> 3] |= 1 << (bit & 7)
        return bytes(b), ref.E_INFINITY
    if cls == "inf_y_larger":
        return bytes(size - 1) + bytes([ref.INFINITY | ref.Y_LARGER]), ref.E_INFINITY
    if cls == "non_residue":
        b = bytearray(non_residue_x(type_, rng))
        b[-1] |= flags
        return bytes(b), ref.E_NO_POINT
    raise ValueError(cls)


def encodings(type_, n, seed):
    """n encodings: valid ones (both flag values, Jacobian sources, O) with about 5 % malformed ones mixed in at seeded
    positions, every class present from n = 63 on.  Returns (list of bytes, {position: (class, code)})."""
    rng = random.Random(seed * 1000003 + n)
    encs = [encode(type_, P) for P in points(type_, n, seed + n)]
    classes = G1_CLASSES if type_ == 1 else G2_CLASSES
    count = 0 if n < 8 else max(len(classes), round(0.05 * n))
    bad = {}
    finite = next(e for e in encs if not e[-1] & ref.INFINITY)
    for j, pos in enumerate(sorted(rng.sample(range(n), count))):
        cls = classes[j % len(classes)]
        encs[pos], code = malformed(type_, cls, rng, finite)
        bad[pos] = (cls, code)
    return encs, bad
