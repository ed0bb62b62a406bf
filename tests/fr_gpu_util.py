"""Shared by test_fr_vectors_gpu.py and test_fft_tables_gpu.py: 32-byte little-endian Fr values between Python
integers, host buffers and device tensors; device buffers filled with a poison byte so that a guard tail shows a
write past the end; tuning knobs set for the length of a block."""
import contextlib
import ctypes

import numpy as np
import torch

from oracle import bn254 as o

R = o.R
POISON = 0xA5
GUARD = 32      # bytes behind every output that the call must leave alone


def host32(v):
    """a 32-byte LE host buffer; the caller keeps it alive until the stream has been synchronised"""
    return ctypes.create_string_buffer(int(v).to_bytes(32, "little"), 32)


def vp(buf):
    return ctypes.cast(buf, ctypes.c_void_p)


def poisoned(nbytes):
    return torch.full((nbytes,), POISON, dtype=torch.uint8, device="cuda")


def zeroed(nbytes):
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")


def dev_from_ints(values, guard=0):
    """n x 32 B LE on the device, followed by `guard` poison bytes"""
    raw = b"".join(int(v).to_bytes(32, "little") for v in values) + bytes([POISON]) * guard
    return torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()


def ints(t, n):
    """the first n 32-byte elements of a device tensor as Python integers"""
    raw = bytes(t[:32 * n].cpu().numpy())
    return [int.from_bytes(raw[k:k + 32], "little") for k in range(0, 32 * n, 32)]


def tail_untouched(t, used):
    """everything behind the first `used` bytes still holds the poison"""
    tail = bytes(t[used:].cpu().numpy())
    return len(tail) > 0 and tail == bytes([POISON]) * len(tail)


def mismatches(got, want):
    """positions where two equally long lists differ (for the assertion message)"""
    assert len(got) == len(want)
    return [i for i, (x, y) in enumerate(zip(got, want)) if x != y]


@contextlib.contextmanager
def knobs_set(L, monkeypatch, knobs):
    """the environment knobs in force (ozk_tuning_reload) inside the block, gone again behind it"""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    L.ozk_tuning_reload()
    try:
        yield
    finally:
        for k in knobs:
            monkeypatch.delenv(k)
        L.ozk_tuning_reload()


def knob_id(knobs):
    return "_".join("%s%s" % (a[4:], b) for a, b in knobs.items()) or "default"
