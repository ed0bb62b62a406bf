"""Host bytes and device marshalling: the 32-byte little-endian element, wire-format points, and the way bytes reach
and leave the device.  Nothing here calls the library."""
import ctypes

import numpy as np
import torch

from .fft import FR


def le32(values) -> bytes:
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def ints32(b: bytes):
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def vp(b: bytes):
    return ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p)


def upload(a: np.ndarray) -> torch.Tensor:
    """A host TEMPORARY to the device.  Large ones go through pinned memory: handed a pageable range, the HIP runtime
    registers it with the kernel driver, and when the freed range is later recycled and unmapped the driver evicts all
    GPU queues of the process for 10-30 ms — a stall that would land in some later proof."""
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a if a.flags.writeable else a.copy())
    return (t.pin_memory() if t.numel() * t.element_size() >= (1 << 20) else t).cuda()


def dev_bytes(b: bytes) -> torch.Tensor:
    return upload(np.frombuffer(b, dtype=np.uint8))


def host_bytes(t) -> bytes:
    return bytes(t.cpu().numpy())


def g1_wire(P) -> bytes:
    return le32(P)


def g2_wire(P) -> bytes:
    return le32(P[i][j] for i in range(3) for j in range(2))


def wire_out_to_in(out: torch.Tensor, type_: int) -> torch.Tensor:
    """One point in the natives' return layout (64-byte LE coordinates, upper half zero) -> the 32-byte
    coordinates they take as input (VariableBaseMSM.java:221-228 vs :239-258)."""
    k = 3 if type_ == 1 else 6
    return out.view(k, 64)[:, :32].reshape(-1).contiguous()


def is_inf_out(p, type_=1) -> bool:
    """whether one wire-out point (192 bytes for type_ 1 = G1, 384 for 2 = G2) is O: Z = 0, whatever X and Y hold"""
    k = 3 if type_ == 1 else 6
    return not bool(p.view(k, 64)[2 * k // 3:].any().item())


def scalar_in_range(k, what, lo=0):
    k = int(k)
    if not lo <= k < FR:
        raise ValueError("%s must lie in [%d, r)" % (what, lo))
    return k


def count(t, rec, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8):
        raise TypeError("%s must be a uint8 CUDA tensor" % what)
    if t.numel() == 0 or t.numel() % rec:
        raise ValueError("%s: %d bytes are not a whole number of %d-byte records" % (what, t.numel(), rec))
    return t.numel() // rec
