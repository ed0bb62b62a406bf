"""Integer model of the compressed point format: square roots in Fq and Fq2, encoding and
strict decoding with the four codes, and the byte forms of a proof and of a verification key.  Python ints and
oracle.bn254 only.

The Fq2 root is Algorithm 9 of Adj and Rodriguez-Henriquez ("Square root computation over even extension fields",
q = 3 mod 4): a^((q-3)/4), then (1 + alpha)^((q-1)/2).  The device header (octopuszk_amd/csrc/point_codec.cuh) uses
the norm method, so the two check each other.
"""
from oracle import bn254 as o

Q = o.Q
F2 = o.Fq2Ops
OK, E_RANGE, E_INFINITY, E_NO_POINT = 0, 1, 2, 3
Y_LARGER, INFINITY = 0x80, 0x40
VK_MAGIC = b"OZKVK\x00\x00\x01"   # five letters, two zero bytes, format version 1


def larger(y: int) -> bool:
    return y > Q - y


def larger2(y) -> bool:
    return larger(y[1]) if y[1] else larger(y[0])


def fq_sqrt(a: int):
    """the root a^((q+1)/4) of a, or None when a is not a square"""
    r = pow(a, (Q + 1) // 4, Q)
    return r if r * r % Q == a % Q else None


def fq2_pow(a, e: int):
    r = F2.one
    for i in range(e.bit_length() - 1, -1, -1):
        r = F2.sqr(r)
        if (e >> i) & 1:
            r = F2.mul(r, a)
    return r


def fq2_sqrt(a):
    """the root of a that is not `larger2`, or None when a is not a square"""
    a = (a[0] % Q, a[1] % Q)
    a1 = fq2_pow(a, (Q - 3) // 4)
    x0 = F2.mul(a1, a)
    alpha = F2.mul(a1, x0)
    a0 = F2.mul((alpha[0], (-alpha[1]) % Q), alpha)   # alpha^q alpha
    if a0 == (Q - 1, 0):
        return None
    if alpha == (Q - 1, 0):
        x = F2.mul((0, 1), x0)
    else:
        x = F2.mul(fq2_pow(F2.add(F2.one, alpha), (Q - 1) // 2), x0)
    assert F2.sqr(x) == a
    return F2.neg(x) if larger2(x) else x


# ---------------------------------------------------------------------------- points
def _le(v: int) -> bytes:
    return int(v).to_bytes(32, "little")


def encode_g1(P) -> bytes:
    """P: Jacobian (X, Y, Z), any Z, coordinates taken mod q"""
    if P[2] % Q == 0:
        return bytes(31) + bytes([INFINITY])
    x, y, _ = o.G1.to_affine(tuple(c % Q for c in P))
    b = bytearray(_le(x))
    b[31] |= Y_LARGER if larger(y) else 0
    return bytes(b)


def encode_g2(P) -> bytes:
    if P[2][0] % Q == 0 and P[2][1] % Q == 0:
        return bytes(63) + bytes([INFINITY])
    x, y, _ = o.G2.to_affine(tuple((c[0] % Q, c[1] % Q) for c in P))
    b = bytearray(_le(x[0]) + _le(x[1]))
    b[63] |= Y_LARGER if larger2(y) else 0
    return bytes(b)


def decode_g1(b: bytes):
    """(code, point): the affine point (x, y, 1), or O = (0, 1, 0) for infinity and for every failure"""
    assert len(b) == 32
    ylarger, infinity = bool(b[31] & Y_LARGER), bool(b[31] & INFINITY)
    x = int.from_bytes(b, "little") & ((1 << 254) - 1)
    if infinity:
        return (E_INFINITY if x or ylarger else OK), o.G1.zero_affine
    if x >= Q:
        return E_RANGE, o.G1.zero_affine
    y = fq_sqrt((x * x * x + 3) % Q)
    if y is None:
        return E_NO_POINT, o.G1.zero_affine
    if y == 0 and ylarger:
        return E_INFINITY, o.G1.zero_affine
    if larger(y) != ylarger:
        y = Q - y
    return OK, (x, y, 1)


def decode_g2(b: bytes):
    assert len(b) == 64
    ylarger, infinity = bool(b[63] & Y_LARGER), bool(b[63] & INFINITY)
    x0 = int.from_bytes(b[:32], "little")
    x1 = int.from_bytes(b[32:], "little") & ((1 << 254) - 1)
    if infinity:
        return (E_INFINITY if x0 or x1 or ylarger else OK), o.G2.zero_affine
    if x0 >= Q or x1 >= Q:
        return E_RANGE, o.G2.zero_affine
    x = (x0, x1)
    y = fq2_sqrt(F2.add(F2.mul(F2.sqr(x), x), o.G2.b))
    if y is None:
        return E_NO_POINT, o.G2.zero_affine
    if y == (0, 0) and ylarger:
        return E_INFINITY, o.G2.zero_affine
    if ylarger:
        y = F2.neg(y)
    return OK, (x, y, (1, 0))


# ---------------------------------------------------------------------------- wire forms of a decoded point
def g1_wire(P, fmt: int) -> bytes:
    """fmt 0: wire-in (32-byte coordinates), 1: wire-out (64-byte coordinates)"""
    return o.g1_to_wire(P) if fmt == 0 else o.g1_out_le(P)


def g2_wire(P, fmt: int) -> bytes:
    return o.g2_to_wire(P) if fmt == 0 else o.g2_out_le(P)


# ---------------------------------------------------------------------------- proofs and keys
def proof_to_bytes(A, B, C) -> bytes:
    return encode_g1(A) + encode_g2(B) + encode_g1(C)


def proof_from_bytes(b: bytes):
    """(code, (A, B, C)): the first non-zero code in the order A, B, C"""
    assert len(b) == 128
    ca, A = decode_g1(b[:32])
    cb, B = decode_g2(b[32:96])
    cc, C = decode_g1(b[96:])
    return (ca or cb or cc), (A, B, C)


def proof_record(b: bytes):
    """(code, the 768-byte wire-out record A | B | C that the device decoder writes)"""
    code, (A, B, C) = proof_from_bytes(b)
    return code, g1_wire(A, 1) + g2_wire(B, 1) + g1_wire(C, 1)


def vk_to_bytes(alpha_beta: bytes, gamma, delta, gamma_abc) -> bytes:
    """magic and version (8) | num_inputs u32 | 4 bytes of padding | alphaG1betaG2 (384) | gamma (64) | delta (64)
    | gammaABC (32 each)"""
    assert len(alpha_beta) == 384
    head = VK_MAGIC + len(gamma_abc).to_bytes(4, "little") + bytes(4)
    return head + alpha_beta + encode_g2(gamma) + encode_g2(delta) + b"".join(encode_g1(P) for P in gamma_abc)


def vk_from_bytes(b: bytes):
    if len(b) < 16 + 384 + 128 or b[:8] != VK_MAGIC or b[12:16] != bytes(4):
        raise ValueError("bad verification key header")
    n = int.from_bytes(b[8:12], "little")
    if n < 1 or len(b) != 16 + 384 + 128 + 32 * n:
        raise ValueError("bad verification key length")
    cg, gamma = decode_g2(b[400:464])
    cd, delta = decode_g2(b[464:528])
    abc = [decode_g1(b[528 + 32 * i:560 + 32 * i]) for i in range(n)]
    codes = [cg, cd] + [c for c, _ in abc]
    if any(codes):
        raise ValueError("verification key point %d does not decode (code %d)"
                         % next((i, c) for i, c in enumerate(codes) if c))
    return b[16:400], gamma, delta, [P for _, P in abc]
