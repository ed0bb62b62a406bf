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
"""
import torch

from . import lib as _lib
from .device import _ptr, _stream

G1_COMPRESSED, G2_COMPRESSED, PROOF_COMPRESSED, PROOF_RECORD = 32, 64, 128, 768
OK, E_RANGE, E_INFINITY, E_NO_POINT, E_SUBGROUP = 0, 1, 2, 3, 4
CODE_NAMES = {OK: "ok", E_RANGE: "coordinate >= q", E_INFINITY: "bad infinity encoding",
              E_NO_POINT: "no curve point has this x", E_SUBGROUP: "not in the order-r subgroup"}
_FORMATS = {"wire_in": 0, "wire_out": 1}


def _count(t, rec, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8):
        raise TypeError("%s must be a uint8 CUDA tensor" % what)
    if t.numel() == 0 or t.numel() % rec:
        raise ValueError("%s: %d bytes are not a whole number of %d-byte records" % (what, t.numel(), rec))
    return t.numel() // rec


def _format(fmt):
    if fmt not in _FORMATS:
        raise ValueError("fmt must be 'wire_in' or 'wire_out'")
    return _FORMATS[fmt]


def _decompress(enc, type_, fmt):
    L = _lib.load()
    n = _count(enc, 32 * type_, "compressed points")
    enc = enc.contiguous()
    f = _format(fmt)
    out = torch.empty(n * 96 * type_ * (1 + f), dtype=torch.uint8, device=enc.device)
    codes = torch.empty(n, dtype=torch.int32, device=enc.device)
    _lib.check(L.ozk_points_decompress_dev(_ptr(enc), n, type_, f, _ptr(out), _ptr(codes), _stream()))
    return out, codes


def _compress(points, type_, fmt):
    L = _lib.load()
    f = _format(fmt)
    n = _count(points, 96 * type_ * (1 + f), "points")
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
    n = _count(enc, 32 * type_, "compressed points")
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
    k = _count(buf, PROOF_COMPRESSED, "compressed proofs")
    buf = buf.contiguous()
    recs = torch.empty(k * PROOF_RECORD, dtype=torch.uint8, device=buf.device)
    codes = torch.empty(k, dtype=torch.int32, device=buf.device)
    _lib.check(L.ozk_groth16_proofs_decompress_dev(_ptr(buf), k, _ptr(recs), _ptr(codes), _stream()))
    return recs, codes
