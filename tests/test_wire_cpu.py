"""wire.py and transcript.py where one function replaced several: the packer and its inverse at their bounds, the
infinity test of a wire-out point in both groups, and the branch of the 128-bit challenge that no digest reaches."""
import hashlib

import pytest
import torch

from oracle import bn254 as o

R = o.R


def test_le32_and_ints32_round_trip_at_the_bounds():
    from octopuszk_amd import wire
    values = [0, 1, R - 1, (1 << 256) - 1]
    raw = wire.le32(values)
    assert len(raw) == 128 and raw == b"".join(v.to_bytes(32, "little") for v in values)
    assert wire.ints32(raw) == values
    assert wire.le32([]) == b"" and wire.ints32(b"") == []
    assert wire.le32(v for v in values) == raw                    # any iterable
    with pytest.raises(OverflowError):
        wire.le32([1 << 256])
    with pytest.raises(OverflowError):
        wire.le32([-1])


@pytest.mark.parametrize("type_", (1, 2))
def test_is_inf_out_reads_all_of_z_and_nothing_else(type_):
    """a wire-out point is 3 (G1) or 6 (G2) words of 64 bytes, Z the last third of them"""
    from octopuszk_amd import wire
    words = 3 * type_
    z_words = range(2 * type_, words)
    zero = torch.zeros(64 * words, dtype=torch.uint8)
    assert wire.is_inf_out(zero, type_) is True
    if type_ == 1:
        assert wire.is_inf_out(zero) is True                      # the default is G1
    for w in z_words:
        for at in (0, 31, 32, 63):                                # the low and the high 32 bytes of the word
            p = zero.clone()
            p[64 * w + at] = 1
            assert wire.is_inf_out(p, type_) is False, (w, at)
    for w in range(2 * type_):                                    # X and Y do not count
        for at in (0, 63):
            p = zero.clone()
            p[64 * w + at] = 0xFF
            assert wire.is_inf_out(p, type_) is True, (w, at)
    full = torch.full((64 * words,), 0xFF, dtype=torch.uint8)
    full[64 * 2 * type_:] = 0
    assert wire.is_inf_out(full, type_) is True


def test_challenge128_is_never_zero(monkeypatch):
    from octopuszk_amd import transcript
    body = b"tag" + b"one" + b"two"
    want = int.from_bytes(hashlib.sha256(body).digest()[:16], "little")
    assert transcript.challenge128(b"tag", b"one", b"two") == want and 1 <= want < 1 << 128

    class _Digest:
        def __init__(self, data):
            assert data == body

        def digest(self):
            return bytes(16) + b"\xff" * 16

    monkeypatch.setattr(hashlib, "sha256", _Digest)
    assert transcript.challenge128(b"tag", b"one", b"two") == 1
