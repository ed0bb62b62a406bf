"""Compressed BN254 points on the GPU, through the C ABI of libozk_hip.so (include/ozk.h).
There is no CPU path.

A compressed point is its affine x, little-endian, with two flags in the top bits of the last byte: bit 7 Y_LARGER
(the canonical y is the larger of y and q - y), bit 6 INFINITY.  G1 is 32 bytes; G2 is 64, x.c0 | x.c1, Y_LARGER
decided on y.c1 unless it is 0.  Decoding is strict and returns one int32 code per point: 0 ok, 1 a coordinate >= q,
2 bad infinity encoding, 3 no curve point has this x.  No subgroup check is made, except by decompress_prepared
(the points of a proving key) where it is asked for: code 4, a G2 point outside the order-r subgroup.

Every function takes and returns uint8 CUDA tensors and is asynchronous on the current stream.  `fmt` names the
uncompressed side: "wire_in" (X | Y | Z with 32-byte coordinates, what the MSMs and pairings take) or "wire_out"
(64-byte coordinates, what they return and what a proof record holds).

The last section is the same strict decoder in host integers (decode_code, require_points, receipt_head): what the
parsers of receipts, openings and keys run where there may be no GPU.
"""
import torch

from . import lib as _lib
from . import wire as _wire
from .device import _ptr, _stream

G1_COMPRESSED, G2_COMPRESSED, PROOF_COMPRESSED, PROOF_RECORD = 32, 64, 128, 768
OK, E_RANGE, E_INFINITY, E_NO_POINT, E_SUBGROUP = 0, 1, 2, 3, 4
CODE_NAMES = {OK: "ok", E_RANGE: "coordinate >= q", E_INFINITY: "bad infinity encoding",
              E_NO_POINT: "no curve point has this x", E_SUBGROUP: "not in the order-r subgroup"}
_FORMATS = {"wire_in": 0, "wire_out": 1}


def _format(fmt):
    if fmt not in _FORMATS:
        raise ValueError("fmt must be 'wire_in' or 'wire_out'")
    return _FORMATS[fmt]


def _decompress(enc, type_, fmt):
    L = _lib.load()
    n = _wire.count(enc, 32 * type_, "compressed points")
    enc = enc.contiguous()
    f = _format(fmt)
    out = torch.empty(n * 96 * type_ * (1 + f), dtype=torch.uint8, device=enc.device)
    codes = torch.empty(n, dtype=torch.int32, device=enc.device)
    _lib.check(L.ozk_points_decompress_dev(_ptr(enc), n, type_, f, _ptr(out), _ptr(codes), _stream()))
    return out, codes


def _compress(points, type_, fmt):
    L = _lib.load()
    f = _format(fmt)
    n = _wire.count(points, 96 * type_ * (1 + f), "points")
    points = points.contiguous()
    out = torch.empty(n * 32 * type_, dtype=torch.uint8, device=points.device)
    _lib.check(L.ozk_points_compress_dev(_ptr(points), n, type_, f, _ptr(out), _stream()))
    return out


def decompress_g1(enc, fmt="wire_in"):
    """n x 32 bytes -> (n points with Z = 1 in `fmt`, n int32 codes).  Infinity, and every point whose code is not
    0, is written as (0, 1, 0)."""
    return _decompress(enc, 1, fmt)


def decompress_g2(enc, fmt="wire_in"):
    """n x 64 bytes -> (n points in `fmt`, n int32 codes); O is ((0, 0), (1, 0), (0, 0))."""
    return _decompress(enc, 2, fmt)


def decompress_prepared(enc, type_, check_subgroup=False):
    """n compressed points of group `type_` (1: G1, 2: G2) -> (the prepared bases device.prepare_bases makes of the
    decoded points, n int32 codes), without the decoded points in between.  Infinity, and every point whose code is
    not 0, is the (0, 0) marker in both of its records.  check_subgroup (G2 only): code 4 for a point outside the
    order-r subgroup."""
    L = _lib.load()
    if type_ not in (1, 2):
        raise ValueError("type_ must be 1 (G1) or 2 (G2)")
    n = _wire.count(enc, 32 * type_, "compressed points")
    enc = enc.contiguous()
    nbytes = int(L.ozk_var_msm_prepared_bytes(n, type_))
    out = torch.empty(nbytes, dtype=torch.uint8, device=enc.device)
    codes = torch.empty(n, dtype=torch.int32, device=enc.device)
    _lib.check(L.ozk_points_decompress_prepared_dev(_ptr(enc), n, type_, _ptr(out), nbytes, _ptr(codes),
                                                    1 if check_subgroup else 0, _stream()))
    return out, codes


def compress_g1(points, fmt="wire_in"):
    """n G1 points in `fmt`, any Z (Z = 0 is infinity) -> n x 32 bytes"""
    return _compress(points, 1, fmt)


def compress_g2(points, fmt="wire_in"):
    """n G2 points in `fmt`, any Z -> n x 64 bytes"""
    return _compress(points, 2, fmt)


def decompress_proofs(buf):
    """K x 128 bytes (A | B | C compressed) -> (K x 768-byte wire-out records A | B | C, K int32 codes): code 0 when
    the three points decoded, else the first non-zero code in the order A, B, C."""
    L = _lib.load()
    k = _wire.count(buf, PROOF_COMPRESSED, "compressed proofs")
    buf = buf.contiguous()
    recs = torch.empty(k * PROOF_RECORD, dtype=torch.uint8, device=buf.device)
    codes = torch.empty(k, dtype=torch.int32, device=buf.device)
    _lib.check(L.ozk_groth16_proofs_decompress_dev(_ptr(buf), k, _ptr(recs), _ptr(codes), _stream()))
    return recs, codes


# ---------------------------------------------------------------------------- the strict decoder on the host
FQ = 21888242871839275222246405745257275088696311157297823662689037894645226208583
_INV82 = pow(82, -1, FQ)
_TWIST_B = (27 * _INV82 % FQ, -3 * _INV82 % FQ)   # 3 / (9 + u) = 3 (9 - u) / 82


def _is_square(v) -> bool:
    return v % FQ == 0 or pow(v, (FQ - 1) // 2, FQ) == 1


def decode_code(enc: bytes, type_) -> int:
    """The code the strict decoder of section 13 gives one compressed point (0 ok, 1 range, 2 infinity, 3 no point),
    in host integers: a receipt is five points, parsed where there may be no GPU.  Existence of y only: a square in
    Fq2 is an element whose norm is a square in Fq."""
    ylarger, infinity = bool(enc[-1] & 0x80), bool(enc[-1] & 0x40)
    xs = [int.from_bytes(enc[i:i + 32], "little") for i in range(0, len(enc), 32)]
    xs[-1] &= (1 << 254) - 1
    if infinity:
        return E_INFINITY if any(xs) or ylarger else OK
    if any(x >= FQ for x in xs):
        return E_RANGE
    if type_ == 1:
        rhs = (xs[0] ** 3 + 3) % FQ
        on, y_zero = _is_square(rhs), rhs == 0
    else:
        a, b = xs
        a2, b2 = (a * a - b * b) % FQ, 2 * a * b % FQ
        r0, r1 = (a2 * a - b2 * b + _TWIST_B[0]) % FQ, (a2 * b + b2 * a + _TWIST_B[1]) % FQ
        on, y_zero = _is_square(r0 * r0 + r1 * r1), r0 == 0 and r1 == 0
    if not on:
        return E_NO_POINT
    return E_INFINITY if y_zero and ylarger else OK


def require_points(fields, owner):
    """fields: (name, compressed encoding, type_) of the points of a receipt, an opening or a key (`owner`);
    ValueError naming the first that does not decode"""
    for name, enc, type_ in fields:
        code = decode_code(enc, type_)
        if code:
            raise ValueError("%s: %s does not decode: code %d (%s)" % (owner, name, code, CODE_NAMES.get(code, "?")))


def receipt_head(b, magic, size):
    """bytes of a receipt with the right length and magic, or ValueError"""
    b = bytes(b)
    if len(b) != size:
        raise ValueError("receipt: length %d, not %d" % (len(b), size))
    if b[:8] != magic:
        raise ValueError("receipt: wrong magic or version")
    return b
