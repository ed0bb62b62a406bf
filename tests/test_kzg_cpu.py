"""No-GPU checks of the KZG layer: the integer model against itself and against the model
pairing, the per-lane pieces of the two opening kernels built for the host (tests/native/kzg_hostcheck.cpp) against the
model, the byte formats, and every argument error raised before the library is touched."""
import ctypes
import os
import random
import subprocess

import pytest
import torch

import ceremony_ref as cref
import codec_ref as ref
import kzg_ref as kr
from oracle import bn254 as o

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "kzg_hostcheck.cpp")
LIB = os.path.join(HERE, "native", "_kzg_hostcheck.so")
CSRC = os.path.join(HERE, "..", "octopuszk_amd", "csrc")
R = o.R
rng = random.Random(22)


def _poly(n):
    return [rng.randrange(R) for _ in range(n)]


# ---------------------------------------------------------------------------- the model against itself
@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_model_quotient_identity(n):
    p = _poly(n)
    for z in (0, 1, R - 1, rng.randrange(R)):
        q, y = kr.div_linear(p, z)
        assert y == kr.horner(p, z) and q[n - 1] == 0
        # p(X) - y = q(X) (X - z), coefficient by coefficient: p_j - [j = 0] y = q_{j-1} - z q_j
        for j in range(n):
            assert (p[j] - (y if j == 0 else 0)) % R == ((q[j - 1] if j else 0) - z * q[j]) % R


@pytest.mark.parametrize("n", [2, 4, 8, 16])
def test_model_evaluation_form_equals_coefficient_form(n):
    """the formulas of the evaluation-form kernel, in integers, against the transform of the coefficient-form quotient"""
    omega = kr.root(n)
    f = _poly(n)
    assert kr.ntt(kr.intt(f, omega), omega) == f
    for z in [rng.randrange(R)] + [pow(omega, k, R) for k in (0, 1, n - 1)]:
        want_q, want_y = kr.open_evals(f, z, omega)
        w = [pow(omega, i, R) for i in range(n)]
        inv = [pow(wi - z, -1, R) if (wi - z) % R else 0 for wi in w]
        if z in w:
            k = w.index(z)
            y = f[k]
            q = [(f[i] - y) * inv[i] % R for i in range(n)]
            q[k] = -pow(omega, -k, R) * sum(q[i] * w[i] for i in range(n) if i != k) % R
        else:
            y = (pow(z, n, R) - 1) * pow(n, -1, R) * sum(f[i] * w[i] * -inv[i] for i in range(n)) % R
            q = [(f[i] - y) * inv[i] % R for i in range(n)]
        assert (q, y) == (want_q, want_y)


def test_model_verifier_accepts_and_rejects():
    tau = 0x1234567
    tau_g1, (g2, tau_g2) = kr.string(4, tau)
    g1 = tau_g1[0]
    p, z = _poly(4), rng.randrange(R)
    q, y = kr.div_linear(p, z)
    C, pi = kr.commit(tau_g1, p), kr.commit(tau_g1, q)
    assert C == kr.g1_mul(g1, kr.horner(p, tau))
    assert kr.verify(g1, g2, tau_g2, C, z, y, pi)
    assert not kr.verify(g1, g2, tau_g2, kr.g1_add(C, g1), z, y, pi)
    assert not kr.verify(g1, g2, tau_g2, C, (z + 1) % R, y, pi)
    assert not kr.verify(g1, g2, tau_g2, C, z, (y + 1) % R, pi)
    assert not kr.verify(g1, g2, tau_g2, C, z, y, kr.g1_add(pi, g1))
    # a constant: pi = O, C = [y] g1; the zero polynomial: C = O, y = 0
    zero = o.G1.to_affine(o.G1.zero)
    assert kr.verify(g1, g2, tau_g2, kr.g1_mul(g1, 7), z, 7, zero)
    assert kr.verify(g1, g2, tau_g2, zero, z, 0, zero)


# ---------------------------------------------------------------------------- the kernels' per-lane pieces
@pytest.fixture(scope="module")
def hc():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("kzg.cuh", "fp29.cuh", "consts_gen.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


def _words(b):
    return (ctypes.c_uint32 * (len(b) // 4)).from_buffer_copy(b)


def _out(n):
    return (ctypes.c_uint32 * (8 * n))()


@pytest.mark.parametrize("chunk", [1, 2, 7])
def test_pieces_recurrence_carries_and_application(hc, chunk):
    """pieces of `chunk` coefficients: their values, the carries composed from the top, the recurrence from each carry"""
    for n in (1, chunk, chunk + 1, 3 * chunk + 2, 23):
        p = _poly(n)
        p[0] += R if p[0] < (1 << 256) - R else 0            # a coefficient written as p + r
        for z in (0, 1, R - 1, rng.randrange(R)):
            quot, value = _out(n), _out(1)
            hc.kzghc_open(_words(b"".join(kr.le(c) for c in p)), n, chunk, _words(kr.le(z)), quot, value)
            q, y = kr.div_linear(p, z)
            assert (kr.ints(bytes(quot)), kr.ints(bytes(value))) == (q, [y]), (n, chunk, z)


def test_chunk_inversion_with_zeros(hc):
    batch = hc.kzghc_batch()
    assert batch >= 3
    mid = batch // 2
    for n in (batch, batch - 1, 1):
        for zeros in ((), (0,), (mid,), (n - 1,), tuple(range(n))):
            d = [0 if k in zeros else rng.randrange(1, R) for k in range(n)]
            out = _out(n)
            hc.kzghc_inverses(_words(b"".join(kr.le(v) for v in d)), n, out)
            assert kr.ints(bytes(out)) == [pow(v, -1, R) if v else 0 for v in d], (n, zeros)


# ---------------------------------------------------------------------------- bytes
def _opening_fields():
    tau_g1, _ = kr.string(2, 5)
    C, pi = kr.g1_mul(tau_g1[0], 11), kr.g1_mul(tau_g1[0], 13)
    return C, 3, 4, pi


def test_opening_bytes_round_trip_and_failures():
    from octopuszk_amd import kzg
    C, z, y, pi = _opening_fields()
    b = kr.opening_bytes(C, z, y, pi)
    op = kzg.Opening.from_bytes(b)
    assert (op.c, op.z, op.y, op.pi) == (ref.encode_g1(C), z, y, ref.encode_g1(pi))
    assert op.to_bytes() == b and len(b) == kzg.OPENING_BYTES == kr.OPENING_BYTES
    inf = kr.opening_bytes(o.G1.to_affine(o.G1.zero), z, 0, o.G1.to_affine(o.G1.zero))
    assert kzg.Opening.from_bytes(inf).to_bytes() == inf
    with pytest.raises(ValueError, match="length"):
        kzg.Opening.from_bytes(b[:-1])
    with pytest.raises(ValueError, match="opening: z"):
        kzg.Opening.from_bytes(b[:32] + kr.le(R) + b[64:])
    with pytest.raises(ValueError, match="opening: y"):
        kzg.Opening.from_bytes(b[:64] + kr.le(R + 1) + b[96:])
    no_point = next(kr.le(x) for x in range(2, 50) if ref.decode_g1(kr.le(x))[0] == 3)
    with pytest.raises(ValueError, match="opening: C does not decode"):
        kzg.Opening.from_bytes(no_point + b[32:])
    with pytest.raises(ValueError, match="opening: pi does not decode"):
        kzg.Opening.from_bytes(b[:96] + kr.le(o.Q))
    with pytest.raises(ValueError, match="opening: z"):
        kzg.Opening(b[:32], R, 0, b[96:])


def _subgroup_model(points, encodings):
    code, P = ref.decode_g2(encodings)
    return code == 0 and o.G2.is_zero(o.G2.mul(P, R))


def test_verify_key_bytes_round_trip_and_failures(monkeypatch):
    from octopuszk_amd import kzg
    tau_g1, (g2, tau_g2) = kr.string(1, 9)
    b = kr.vk_bytes(tau_g1[0], g2, tau_g2)
    assert len(b) == kzg.VK_BYTES == kr.VK_BYTES
    # the subgroup test runs on the device (vectors.in_subgroup_g2): here the model's stands in for it, fed by what
    # from_bytes hands it
    monkeypatch.setattr(kzg.VerifyKey, "points", lambda self: (None, bytes(384)))
    monkeypatch.setattr(kzg, "_g2_in_subgroup", _subgroup_model)
    vk = kzg.VerifyKey.from_bytes(b)
    assert (vk.g1, vk.g2, vk.tau_g2) == (b[:32], b[32:96], b[96:]) and vk.to_bytes() == b
    with pytest.raises(ValueError, match="length"):
        kzg.VerifyKey.from_bytes(b + b"\x00")
    no1 = next(kr.le(x) for x in range(2, 50) if ref.decode_g1(kr.le(x))[0] == 3)
    with pytest.raises(ValueError, match="verification key: g1 does not decode"):
        kzg.VerifyKey.from_bytes(no1 + b[32:])
    with pytest.raises(ValueError, match="verification key: g2 does not decode"):
        kzg.VerifyKey.from_bytes(b[:32] + kr.le(o.Q) + b[64:])
    with pytest.raises(ValueError, match="verification key: tau_g2 does not decode"):
        kzg.VerifyKey.from_bytes(b[:96] + kr.le(o.Q) + b[128:])
    inf1, inf2 = ref.encode_g1(o.G1.to_affine(o.G1.zero)), ref.encode_g2(o.G2.to_affine(o.G2.zero))
    with pytest.raises(ValueError, match="verification key: g1 is the point at infinity"):
        kzg.VerifyKey.from_bytes(inf1 + b[32:])
    with pytest.raises(ValueError, match="verification key: tau_g2 is the point at infinity"):
        kzg.VerifyKey.from_bytes(b[:96] + inf2)
    outside = ref.encode_g2(cref.twist_point_outside_the_subgroup())
    with pytest.raises(ValueError, match="verification key: tau_g2 is not in the order-r subgroup"):
        kzg.VerifyKey.from_bytes(b[:96] + outside)
    with pytest.raises(ValueError, match="verification key: g2 is not in the order-r subgroup"):
        kzg.VerifyKey.from_bytes(b[:32] + outside + b[96:])


def test_streams_match_the_model():
    from octopuszk_amd import kzg, transcript
    seed = bytes(range(32))
    assert kr.ints(transcript.weights(seed, 5, kzg._RHO_TAG)) == kr.rho(seed, 5)
    assert kr.rho(seed, 5) != cref.weights(seed, 5)
    cs = [kr.le(i + 1) for i in range(3)]
    assert kzg.combine_challenge(7, cs, [1, 2, 3]) == kr.gamma(7, cs, [1, 2, 3])
    assert 1 <= kr.gamma(7, cs, [1, 2, 3]) < 1 << 128


# ---------------------------------------------------------------------------- argument errors, the library absent
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was reached: %s" % name)


class _FakeSrs:
    m = 4
    tau_g1 = torch.zeros(96 * 9, dtype=torch.uint8)


def test_argument_errors_come_before_any_library_call(monkeypatch):
    from octopuszk_amd import kzg, lib
    monkeypatch.setattr(lib, "load", lambda: _NoLibrary())
    monkeypatch.setattr(kzg._lib, "load", lambda: _NoLibrary())
    for n in (0, 10, -1):
        with pytest.raises(ValueError, match="carries 9 powers"):
            kzg.CommitKey.from_srs(_FakeSrs(), n)
    ck = kzg.CommitKey.from_srs(_FakeSrs(), 5)
    assert (ck.n, ck.m) == (5, 4)
    cpu = torch.zeros(32 * 5, dtype=torch.uint8)
    for call in (ck.commit, ck.commit_evals, lambda t: ck.open(t, 1), lambda t: ck.open_evals(t, 1),
                 lambda t: ck.open_many_points(t, [1]), lambda t: ck.open_combined(t, 1)):
        with pytest.raises(TypeError, match="CUDA"):           # the device
            call(cpu)
        with pytest.raises(TypeError, match="uint8"):          # the dtype
            call(cpu.to(torch.int32))
    with pytest.raises(TypeError):
        ck.commit([1, 2, 3, 4, 5])
    # the sizes of an evaluation row
    for bad in (0, 1, 3, 6, 12):
        with pytest.raises(ValueError, match="power of two"):
            kzg._eval_size(bad, 8)
    with pytest.raises(ValueError, match="at most 2 m"):
        kzg._eval_size(32, 8)
    assert kzg._eval_size(16, 8) == 16
    with pytest.raises(ValueError, match="power of two"):
        ck.lagrange(6)
    with pytest.raises(ValueError, match="at most 2 m"):
        ck.lagrange(16)
    # points and values as ints
    for bad in (R, R + 5, -1):
        with pytest.raises(ValueError, match=r"\[0, r\)"):
            kzg._scalars([1, bad], 2, "points")
        with pytest.raises(ValueError, match=r"\[0, r\)"):
            kzg.verify_combined(None, [bytes(32)], bad, [0], bytes(32))
        with pytest.raises(ValueError, match=r"\[0, r\)"):
            kzg.verify_combined(None, [bytes(32)], 0, [bad], bytes(32))
    with pytest.raises(ValueError, match="1 points for 2 rows"):
        kzg._scalars([1], 2, "points")


class _Shaped:
    """what _rows reads of a tensor, with a CUDA tensor's answers: the layout checks run where there is no GPU"""

    def __init__(self, shape, stride, ptr=256):
        self.shape, self._stride, self._ptr, self.dtype, self.is_cuda = shape, stride, ptr, torch.uint8, True

    def dim(self):
        return len(self.shape)

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def stride(self, i):
        return self._stride[i]

    def data_ptr(self):
        return self._ptr

    def unsqueeze(self, _):
        return _Shaped((1,) + tuple(self.shape), (self.shape[0],) + tuple(self._stride), self._ptr)


def test_row_layout_errors(monkeypatch):
    from octopuszk_amd import kzg
    monkeypatch.setattr(kzg.torch, "Tensor", _Shaped)
    assert kzg._rows(_Shaped((64,), (1,)), "coeffs", 2) == (1, 2, 2)
    assert kzg._rows(_Shaped((3, 64), (160, 1)), "coeffs", 2) == (3, 2, 5)
    with pytest.raises(ValueError, match="16-byte aligned"):
        kzg._rows(_Shaped((64,), (1,), ptr=264), "coeffs")
    with pytest.raises(ValueError, match="multiple of 32"):
        kzg._rows(_Shaped((3, 64), (72, 1)), "coeffs")
    with pytest.raises(ValueError, match="whole 32-byte elements"):
        kzg._rows(_Shaped((65,), (1,)), "coeffs")
    with pytest.raises(ValueError, match="the key has n = 3"):
        kzg._rows(_Shaped((64,), (1,)), "coeffs", 3)
    with pytest.raises(ValueError, match="not 3-D"):
        kzg._rows(_Shaped((1, 1, 32), (32, 32, 1)), "coeffs")
