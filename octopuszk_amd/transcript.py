"""The hashes of the ceremonies and of KZG: the weight stream of the batched checks, the 128-bit challenge and the seed
of a check.  Every caller passes its own tag; host only."""
import hashlib
import os


def weights(seed: bytes, n: int, tag: bytes) -> bytes:
    """n weights in [1, 2^128) as n x 32 bytes little-endian: block j of the stream is SHA-256(tag | seed | j as 8
    bytes little-endian), two weights per block"""
    out = bytearray(32 * n)
    pad = bytes(16)
    one = (1).to_bytes(16, "little")
    for j in range((n + 1) // 2):
        block = hashlib.sha256(tag + seed + j.to_bytes(8, "little")).digest()
        for half in (0, 1):
            i = 2 * j + half
            if i < n:
                w = block[16 * half:16 * half + 16]
                out[32 * i:32 * i + 32] = (w if w != pad else one) + pad
    return bytes(out)


def digest(tag: bytes, *parts) -> bytes:
    """SHA-256(tag | the parts): what a later challenge of the same transcript hashes in place of the parts"""
    return hashlib.sha256(tag + b"".join(parts)).digest()


def challenge128(tag: bytes, *parts) -> int:
    """the first 16 bytes, little-endian, of SHA-256(tag | the parts); 1 if they are zero"""
    return int.from_bytes(digest(tag, *parts)[:16], "little") or 1


def seed_bytes(seed) -> bytes:
    if seed is None:
        return os.urandom(32)
    if isinstance(seed, (bytes, bytearray)):
        return bytes(seed)
    return int(seed).to_bytes(32, "little")
