"""Model of the proving-key file (OZKPK version 1) and of the prepared records a compressed
point decodes into, in plain Python integers over tests/codec_ref.py and oracle.bn254.  Written from the format's
description, not from octopuszk_amd/keyfile.py, which the tests compare with it."""
import hashlib
import struct

import codec_ref as ref
from oracle import bn254 as o

Q, R = o.Q, o.R
MAGIC = b"OZKPK\x00\x00\x01"
NAMES = ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2", "query_a", "query_b_g1", "query_b_g2",
         "delta_abc_g1", "query_h", "r1cs_a", "r1cs_b", "r1cs_c")
G2_NAMES = ("beta_g2", "delta_g2", "query_b_g2")
HEADER = 8 + 16 + 32 + 13 * 20

# ---------------------------------------------------------------------------- prepared records
# A record is what CurveIO::store_aff packs of a canonical Montgomery coordinate pair: per Fq value the integer
# v * 2^261 mod q (the library's Montgomery radix, fp29.cuh: nine 29-bit limbs) in 32 little-endian bytes; G1 x | y,
# G2 x.c0 | x.c1 | y.c0 | y.c1.  O is all zero.  The second record of a base is (beta x, y), beta the cube root of
# unity with (beta x, y) = [lambda] (x, y) on G1, its square on the twist (tools/gen_glv.py).
MONT = pow(2, 261, Q)
LAMBDA = 4407920970296243842393367215006156084916469457145843978461
BETA_G1 = 2203960485148121921418603742825762020974279258880205651966
BETA_G2 = BETA_G1 * BETA_G1 % Q


def _m(v):
    return (v * MONT % Q).to_bytes(32, "little")


def records(type_, P):
    """(record of P, record of phi(P)) for an affine point as codec_ref decodes it (O: zero_affine)"""
    C = o.G1 if type_ == 1 else o.G2
    if C.is_zero(P):
        return bytes(64 * type_), bytes(64 * type_)
    x, y = P[0], P[1]
    if type_ == 1:
        return _m(x) + _m(y), _m(BETA_G1 * x % Q) + _m(y)
    bx = (BETA_G2 * x[0] % Q, BETA_G2 * x[1] % Q)
    return _m(x[0]) + _m(x[1]) + _m(y[0]) + _m(y[1]), _m(bx[0]) + _m(bx[1]) + _m(y[0]) + _m(y[1])


def prepared(type_, encs):
    """(the 2 n records of the GLV plan: n of the points, then n of their images; the n codes)"""
    decoded = [(ref.decode_g1 if type_ == 1 else ref.decode_g2)(e) for e in encs]
    recs = [records(type_, P) for _, P in decoded]
    return b"".join(r[0] for r in recs) + b"".join(r[1] for r in recs), [c for c, _ in decoded]


def in_subgroup(P) -> bool:
    """[r]P = O for a point of the twist, in oracle integers"""
    return o.G2.is_zero(o.G2.mul(P, R))


# ---------------------------------------------------------------------------- the file
def domain(nc, ni):
    m = 1
    while m < nc + ni:
        m *= 2
    return m


def r1cs_section(ptr, index, value) -> bytes:
    b = struct.pack("<III", len(ptr) - 1, len(index), 0 if value is None else 1)
    b += b"".join(struct.pack("<I", int(p)) for p in ptr) + b"".join(struct.pack("<I", int(i)) for i in index)
    if value is not None:
        b += b"".join(int(v).to_bytes(32, "little") for v in value)
    return b


def write(ni, na, nc, sections) -> bytes:
    """sections: name -> bytes, every name of NAMES; laid out back to back after the header"""
    payload = b"".join(sections[n] for n in NAMES)
    table, off = b"", HEADER
    for i, n in enumerate(NAMES):
        table += struct.pack("<IQQ", i + 1, off, len(sections[n]))
        off += len(sections[n])
    return MAGIC + struct.pack("<IIII", ni, na, nc, domain(nc, ni)) + hashlib.sha256(payload).digest() + table + payload


def parse(b: bytes, verify_digest=True):
    """{"counts": (ni, na, nc, m), name: bytes for the point sections, r1cs_*: (ptr, index, value or None)}"""
    if len(b) < 8:
        raise ValueError("header: truncated")
    if b[:7] != MAGIC[:7]:
        raise ValueError("header: wrong magic")
    if b[7] != 1:
        raise ValueError("header: wrong version")
    if len(b) < HEADER:
        raise ValueError("header: truncated")
    ni, na, nc, m = struct.unpack_from("<IIII", b, 8)
    if m != domain(nc, ni):
        raise ValueError("header: domain size")
    nv = ni + na
    want = {"alpha_g1": 32, "beta_g1": 32, "delta_g1": 32, "beta_g2": 64, "delta_g2": 64, "query_a": 32 * nv,
            "query_b_g1": 32 * nv, "query_b_g2": 64 * nv, "delta_abc_g1": 32 * (nv - ni), "query_h": 32 * (m + 1)}
    spans, out = [], {"counts": (ni, na, nc, m)}
    for i, n in enumerate(NAMES):
        sid, off, length = struct.unpack_from("<IQQ", b, 56 + 20 * i)
        if sid != i + 1:
            raise ValueError("header: section id")
        if off < HEADER or off + length > len(b):
            raise ValueError("section %s: out of bounds" % n)
        if n in want and length != want[n]:
            raise ValueError("section %s: length" % n)
        spans.append((off, off + length, n))
    for (_, end, _), (start, _, n) in zip(sorted(spans), sorted(spans)[1:]):
        if start < end:
            raise ValueError("section %s: overlap" % n)
    if verify_digest and hashlib.sha256(b[HEADER:]).digest() != b[24:56]:
        raise ValueError("digest mismatch")
    for off, end, n in spans:
        s = b[off:end]
        if n in want:
            out[n] = s
            continue
        if len(s) < 12:
            raise ValueError("section %s: length" % n)
        rows, nnz, hv = struct.unpack_from("<III", s, 0)
        if hv > 1 or rows != nc or len(s) != 12 + 4 * (rows + 1) + 4 * nnz + 32 * nnz * hv:
            raise ValueError("section %s: length" % n)
        ptr = list(struct.unpack_from("<%dI" % (rows + 1), s, 12))
        idx = list(struct.unpack_from("<%dI" % nnz, s, 12 + 4 * (rows + 1)))
        if ptr[0] != 0 or any(a > c for a, c in zip(ptr, ptr[1:])) or ptr[-1] != nnz:
            raise ValueError("section %s: row offsets" % n)
        if any(i >= nv for i in idx):
            raise ValueError("section %s: index" % n)
        val = None
        if hv:
            base = 12 + 4 * (rows + 1) + 4 * nnz
            val = [int.from_bytes(s[base + 32 * k:base + 32 * k + 32], "little") for k in range(nnz)]
            if any(v >= R for v in val):
                raise ValueError("section %s: coefficient" % n)
        out[n] = (ptr, idx, val)
    return out
