"""The compressed point format with exact integers: the Python model (tests/codec_ref.py)
against oracle.bn254, and the header the kernels compile (octopuszk_amd/csrc/point_codec.cuh, built for the host)
against the model, byte for byte and code for code."""
import ctypes
import os
import random
import subprocess

import pytest

import codec_cases as cases
import codec_ref as ref
from oracle import bn254 as o

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "codec_hostcheck.cpp")
LIB = os.path.join(HERE, "native", "_codec_hostcheck.so")
CSRC = os.path.join(HERE, "..", "octopuszk_amd", "csrc")
Q = o.Q
F2 = o.Fq2Ops


@pytest.fixture(scope="module")
def cdhc():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("point_codec.cuh", "fq12.cuh", "fq2.cuh", "fp29.cuh", "curve.cuh",
                                                    "pairing_consts_gen.h", "consts_gen.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


def _residue(v):
    return v % Q == 0 or pow(v, (Q - 1) // 2, Q) == 1


def _fq2_branch_cases():
    """the cases of section 13 "branches": 0, real squares, real non-squares (purely imaginary roots), purely
    imaginary elements, elements whose Algorithm 9 alpha is -1, and non-squares"""
    rng = random.Random(2)
    sq = [v for v in (rng.randrange(1, Q) for _ in range(40)) if _residue(v)][:6]
    nsq = [v for v in (rng.randrange(1, Q) for _ in range(40)) if not _residue(v)][:6]
    out = [(0, 0), (1, 0), (Q - 1, 0), (0, 1), (0, Q - 1), (4, 0), (3, 0)]
    out += [(n, 0) for n in sq + nsq] + [(0, n) for n in sq + nsq]
    # Algorithm 9's alpha = a^((q-1)/2) is -1 exactly for the real non-squares above; squares of purely imaginary
    # elements are such values built the other way round
    out += [F2.sqr((0, s)) for s in sq[:3]]
    nonsq = []
    while len(nonsq) < 6:
        a = (rng.randrange(Q), rng.randrange(Q))
        if not _residue(a[0] * a[0] + a[1] * a[1]):
            nonsq.append(a)
    return out + nonsq


# ---------------------------------------------------------------------------- the model against the oracle
def test_fq_sqrt_model():
    rng = random.Random(1)
    for a in [0, 1, 4, Q - 1, 3] + [rng.randrange(Q) for _ in range(300)]:
        r = ref.fq_sqrt(a)
        assert (r is None) == (not _residue(a)), a
        if r is not None:
            assert r * r % Q == a


def test_fq2_sqrt_model_branches_and_random():
    rng = random.Random(3)
    elems = _fq2_branch_cases() + [(rng.randrange(Q), rng.randrange(Q)) for _ in range(500)]
    none = 0
    for a in elems:
        r = ref.fq2_sqrt(a)
        is_square = _residue(a[0] * a[0] + a[1] * a[1])
        assert (r is None) == (not is_square), a
        if r is None:
            none += 1
        else:
            assert F2.sqr(r) == a and not ref.larger2(r), a
    assert 150 < none < 400   # about half of the random elements
    assert ref.fq2_sqrt((Q - 4, 0)) in ((0, 2), (0, Q - 2))   # a real non-square: purely imaginary root


@pytest.mark.parametrize("type_", [1, 2])
def test_round_trip_generators_infinity_and_random_multiples(type_):
    C = cases.curve(type_)
    rng = random.Random(10 + type_)
    pts = [C.one, C.zero, C.zero_affine] + [C.mul(C.one, rng.randrange(1, o.R)) for _ in range(200)]
    flags = set()
    for P in pts:
        enc = cases.encode(type_, P)
        assert len(enc) == 32 * type_
        code, back = cases.decode(type_, enc)
        assert code == ref.OK and back == C.to_affine(P)
        if C.is_zero(P):
            assert enc == bytes(32 * type_ - 1) + bytes([ref.INFINITY])
            continue
        flags.add(enc[-1] & ref.Y_LARGER)
        neg = cases.encode(type_, C.negate(P))
        assert neg[:-1] == enc[:-1] and neg[-1] ^ enc[-1] == ref.Y_LARGER
        assert cases.decode(type_, neg) == (ref.OK, C.to_affine(C.negate(P)))
    assert flags == {0, ref.Y_LARGER}


def test_g1_small_x_codes_follow_eulers_criterion():
    seen = set()
    for x in range(400):
        code, P = ref.decode_g1(x.to_bytes(32, "little"))
        assert code == (ref.OK if _residue(x * x * x + 3) else ref.E_NO_POINT), x
        seen.add(code)
        if code == ref.OK:
            assert o.G1.on_curve(P) and P[0] == x and not ref.larger(P[1])
        else:
            assert P == o.G1.zero_affine
    assert seen == {ref.OK, ref.E_NO_POINT}


@pytest.mark.parametrize("type_", [1, 2])
def test_model_malformed_classes(type_):
    rng = random.Random(20 + type_)
    C = cases.curve(type_)
    valid = cases.encode(type_, C.mul(C.one, 12345))
    for cls in (cases.G1_CLASSES if type_ == 1 else cases.G2_CLASSES):
        for _ in range(4):
            enc, code = cases.malformed(type_, cls, rng, valid)
            assert cases.decode(type_, enc) == (code, C.zero_affine), cls


def test_proof_and_key_model_round_trip():
    A, B, Cc = o.G1.mul(o.G1.one, 5), o.G2.mul(o.G2.one, 7), o.G1.mul(o.G1.one, 11)
    b = ref.proof_to_bytes(A, B, Cc)
    assert len(b) == 128
    code, pts = ref.proof_from_bytes(b)
    assert code == 0 and pts == (o.G1.to_affine(A), o.G2.to_affine(B), o.G1.to_affine(Cc))
    bad = bytearray(b)
    bad[96:128] = cases.non_residue_x(1, random.Random(4))
    assert ref.proof_from_bytes(bytes(bad))[0] == ref.E_NO_POINT
    bad[0:32] = Q.to_bytes(32, "little")
    assert ref.proof_from_bytes(bytes(bad))[0] == ref.E_RANGE   # A's code comes first
    abc = [o.G1.mul(o.G1.one, k) for k in (2, 3, 4)]
    gt = bytes(range(256)) + bytes(128)
    vk = ref.vk_to_bytes(gt, B, o.G2.one, abc)
    assert len(vk) == 16 + 384 + 128 + 96
    assert ref.vk_from_bytes(vk) == (gt, o.G2.to_affine(B), o.G2.to_affine(o.G2.one), [o.G1.to_affine(P) for P in abc])
    for broken in (vk[:-1], b"X" + vk[1:], vk[:528] + bytes(bad[96:128]) + vk[560:]):
        with pytest.raises(ValueError):
            ref.vk_from_bytes(broken)


# ---------------------------------------------------------------------------- the header against the model
def _words(b):
    return (ctypes.c_uint32 * (len(b) // 4)).from_buffer_copy(b)


def _le(v):
    return int(v).to_bytes(32, "little")


def test_header_fq_sqrt(cdhc):
    rng = random.Random(5)
    for a in [0, 1, 4, 3, Q - 1, Q - 4] + [rng.randrange(Q) for _ in range(300)]:
        out = (ctypes.c_uint32 * 8)()
        ok = cdhc.cdhc_fq_sqrt(_words(_le(a)), out)
        want = ref.fq_sqrt(a)
        assert bool(ok) == (want is not None), a
        if want is not None:
            assert bytes(out) == _le(want), a


def test_header_fq2_sqrt(cdhc):
    rng = random.Random(6)
    elems = _fq2_branch_cases() + [(rng.randrange(Q), rng.randrange(Q)) for _ in range(300)]
    for a in elems:
        out = (ctypes.c_uint32 * 16)()
        ok = cdhc.cdhc_fq2_sqrt(_words(_le(a[0]) + _le(a[1])), out)
        want = ref.fq2_sqrt(a)
        assert bool(ok) == (want is not None), a
        if want is not None:
            assert bytes(out) == _le(want[0]) + _le(want[1]), a


def _host_decode(cdhc, type_, enc, fmt):
    out = (ctypes.c_uint32 * (24 * type_ * (1 + fmt)))()
    fn = cdhc.cdhc_g1_decode if type_ == 1 else cdhc.cdhc_g2_decode
    code = fn(_words(enc), fmt, out)
    return code, bytes(out)


def _host_encode(cdhc, type_, P, fmt):
    out = (ctypes.c_uint32 * (8 * type_))()
    fn = cdhc.cdhc_g1_encode if type_ == 1 else cdhc.cdhc_g2_encode
    fn(_words(cases.wire(type_, P, fmt)), fmt, out)
    return bytes(out)


@pytest.mark.parametrize("type_", [1, 2])
def test_header_decode_matches_model(cdhc, type_):
    encs, bad = cases.encodings(type_, 160, seed=31)
    assert {cls for cls, _ in bad.values()} == set(cases.G1_CLASSES if type_ == 1 else cases.G2_CLASSES)
    C = cases.curve(type_)
    encs += [cases.encode(type_, C.one), cases.encode(type_, C.negate(C.one)), cases.encode(type_, C.zero)]
    if type_ == 1:
        encs += [x.to_bytes(32, "little") for x in range(40)]
    codes = set()
    for i, enc in enumerate(encs):
        code, P = cases.decode(type_, enc)
        if i in bad:
            assert code == bad[i][1] != 0, bad[i]
        codes.add(code)
        for fmt in (0, 1):
            got_code, got = _host_decode(cdhc, type_, enc, fmt)
            assert got_code == code, (i, enc.hex())
            assert got == cases.wire(type_, P, fmt), (i, fmt, enc.hex())
    assert codes == {0, 1, 2, 3}


@pytest.mark.parametrize("type_", [1, 2])
def test_header_encode_matches_model(cdhc, type_):
    pts = cases.points(type_, 90, seed=41)
    C = cases.curve(type_)
    assert any(C.is_zero(P) for P in pts)
    jac = [P for P in pts if not C.is_zero(P) and P[2] not in (1, (1, 0))]
    assert len(jac) >= 8                                   # Jacobian inputs with Z != 1
    pts += [C.one, C.negate(C.one), C.zero_affine]
    for P in pts:
        want = cases.encode(type_, P)
        for fmt in (0, 1):
            assert _host_encode(cdhc, type_, P, fmt) == want, (fmt, P)
        code, back = cases.decode(type_, want)
        assert code == 0 and back == C.to_affine(P)
