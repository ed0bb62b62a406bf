"""Phase-1 contributions to a powers-of-tau string without a GPU: the per-point function of the
points-times-scalars kernel (octopuszk_amd/csrc/points_mul.cuh, built for the host) against the integer model, the
model's verifier on honest and tampered contributions, the receipt's and the file's bytes and strict parsing, and the
errors raised before any library call."""
import ctypes
import functools
import hashlib
import os
import random
import subprocess

import pytest

import ceremony_ref as cref
import codec_cases as cases
import phase1_ref as p1
from oracle import bn254 as o

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "points_mul_hostcheck.cpp")
LIB = os.path.join(HERE, "native", "_points_mul_hostcheck.so")
CSRC = os.path.join(HERE, "..", "octopuszk_amd", "csrc")
Q, R = o.Q, o.R


@pytest.fixture(scope="module")
def pmhc():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("points_mul.cuh", "points_scale.cuh", "glv.cuh", "fq2.cuh",
                                                    "fp29.cuh", "ec.cuh", "curve.cuh", "consts_gen.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


def _words(b):
    return (ctypes.c_uint32 * (len(b) // 4)).from_buffer_copy(b)


def _le(v):
    return int(v).to_bytes(32, "little")


# ---------------------------------------------------------------------------- the kernel's per-point function
def _points(type_):
    C = cases.curve(type_)
    rng = random.Random(50 + type_)
    P = C.to_affine(C.mul(C.one, rng.randrange(1, R)))
    J = cases.rescale(type_, C.to_affine(C.mul(C.one, rng.randrange(1, R))), rng.randrange(2, Q))
    pts = [C.to_affine(C.one), P, J, C.zero]
    if type_ == 2:
        pts.append(cref.twist_point_outside_the_subgroup())
    return pts


@pytest.mark.parametrize("type_", [1, 2])
def test_per_point_function_matches_the_model(pmhc, type_):
    C = cases.curve(type_)
    pts = _points(type_)
    assert pts[2][2] not in (1, (1, 0)) and C.is_zero(pts[3])
    if type_ == 2:
        assert not o.G2.is_zero(o.G2.mul(pts[4], R))
    for k in p1.scalars():
        for P in pts:
            out = (ctypes.c_uint32 * (24 * type_))()
            assert pmhc.pmhc_mul(_words(cases.wire(type_, P, 0)), type_, _words(_le(k)), out) == 0
            want = cref.wire(type_, cref.scale(type_, P, k))
            assert bytes(out) == want, (k, P)
            buf = _words(cases.wire(type_, P, 0))
            assert pmhc.pmhc_mul_in_place(buf, type_, _words(_le(k))) == 0 and bytes(buf) == want


@pytest.mark.parametrize("type_", [1, 2])
def test_a_scalar_from_r_on_gives_infinity_and_code_1(pmhc, type_):
    C = cases.curve(type_)
    inf = cref.wire(type_, C.to_affine(C.zero))
    for k in (R, R + 1, 1 << 254, (1 << 256) - 1):
        out = (ctypes.c_uint32 * (24 * type_))(*([0xFFFFFFFF] * (24 * type_)))
        assert pmhc.pmhc_mul(_words(cases.wire(type_, C.to_affine(C.one), 0)), type_, _words(_le(k)), out) == 1
        assert bytes(out) == inf
    out = (ctypes.c_uint32 * (24 * type_))()
    assert pmhc.pmhc_mul(_words(cases.wire(type_, C.to_affine(C.one), 0)), type_, _words(_le(R - 1)), out) == 0
    assert bytes(out) != inf


# ---------------------------------------------------------------------------- the model's verifier
M = 4
T, AL, BE = 0x1111111122222222 % R, 0x3333333344444444 % R, 0x5555555566666666 % R
FACTORS = (0x1234567890ABCDEF1234567890ABCDEF % R, 0xFEDCBA0987654321 % R, 0xA5A5A5A55A5A5A5A % R)
NONCES = (77, 1 << 200, R - 5)


@functools.lru_cache(maxsize=None)
def _honest():
    before = p1.from_secrets_exp(M, T, AL, BE)
    after, receipt = p1.contribute_exp(before, FACTORS, NONCES)
    return before, after, receipt


def test_model_contribution_multiplies_the_secrets():
    before, after, receipt = _honest()
    assert after == dict(p1.from_secrets_exp(M, T * FACTORS[0] % R, AL * FACTORS[1] % R, BE * FACTORS[2] % R))
    assert p1.wellformed(before) and p1.wellformed(after)
    assert p1.initial_exp(M)["tau_g1"] == [1] * (2 * M + 1) and p1.wellformed(p1.initial_exp(M))


def test_model_accepts_the_honest_contribution_and_a_chain():
    before, after, receipt = _honest()
    assert p1.verify_contribution_exp(before, after, receipt) == (True, None)
    s0 = p1.initial_exp(M)
    s1, r1 = p1.contribute_exp(s0, FACTORS, NONCES)
    s2, r2 = p1.contribute_exp(s1, (5, 6, 7), NONCES, previous=r1)
    assert p1.verify_chain_exp([s0, s1, s2], [r1, r2]) == (True, None)
    assert s2 == p1.from_secrets_exp(M, FACTORS[0] * 5 % R, FACTORS[1] * 6 % R, FACTORS[2] * 7 % R)


TAMPERS = ("generator g1", "generator g2", "tau_g1 point", "tau_g2 point", "alpha_tau_g1 point", "beta_tau_g1 point",
           "beta_g2", "tau_g2 by other powers", "pok over the wrong base", "swapped h", "receipt m")


@functools.lru_cache(maxsize=None)
def _tampers():
    """label -> (before, after, receipt, the check that must fail)"""
    before, after, receipt = _honest()
    out = {}

    def case(label, why, aft=after, rec=None):
        out[label] = (before, aft, p1.receipt_exp(before, aft, FACTORS, NONCES) if rec is None else rec, why)

    def bump(name, i):
        t = dict(after)
        if name == "beta_g2":
            t[name] = (after[name] + 1) % R
        else:
            t[name] = list(after[name])
            t[name][i] = (t[name][i] + 12345) % R
        return t

    case("generator g1", "generators", bump("tau_g1", 0))
    case("generator g2", "generators", bump("tau_g2", 0))
    case("tau_g1 point", "wellformed", bump("tau_g1", 2 * M))
    case("tau_g2 point", "wellformed", bump("tau_g2", M - 1))
    case("alpha_tau_g1 point", "wellformed", bump("alpha_tau_g1", 2))
    case("beta_tau_g1 point", "wellformed", bump("beta_tau_g1", 1))
    case("beta_g2", "wellformed", bump("beta_g2", 0))
    other = dict(after, tau_g2=[x * pow(FACTORS[0] + 1, i, R) % R for i, x in enumerate(before["tau_g2"])])
    case("tau_g2 by other powers", "wellformed", other)
    case("pok over the wrong base", "pok", rec=p1.receipt_exp(before, after, FACTORS, NONCES, pok_over=(0, 0, 2)))
    case("swapped h", "pok", rec=receipt[:16] + hashlib.sha256(b"another").digest() + receipt[48:])
    case("receipt m", "receipt_points", rec=p1.receipt_exp(before, after, FACTORS, NONCES, m=2 * M))
    assert tuple(out) == TAMPERS
    return out


@pytest.mark.parametrize("label", TAMPERS)
def test_model_rejects_each_tamper_class(label):
    before, after, receipt, why = _tampers()[label]
    assert p1.verify_contribution_exp(before, after, receipt) == (False, why)


def test_model_chain_rejects_a_swapped_h():
    s0 = p1.initial_exp(M)
    s1, r1 = p1.contribute_exp(s0, FACTORS, NONCES)
    s2, r2 = p1.contribute_exp(s1, (5, 6, 7), NONCES, previous=b"not the receipt before")
    assert p1.verify_chain_exp([s0, s1, s2], [r1, r2]) == (False, "chain")


# ---------------------------------------------------------------------------- receipt
def test_receipt_round_trip_and_layout():
    from octopuszk_amd import srs
    before, after, receipt = _honest()
    assert len(receipt) == srs.RECEIPT_BYTES == 432 and receipt[:8] == srs.MAGIC == b"OZKC1\x00\x00\x01"
    rec = srs.Receipt.from_bytes(receipt)
    assert rec.to_bytes() == receipt
    model = p1.parse_receipt(receipt)
    assert rec.m == model["m"] == M and rec.h == model["h"] == hashlib.sha256(b"").digest()
    six = receipt[48:112] + receipt[176:240] + receipt[304:368]
    for j in range(3):
        off = 48 + 128 * j
        assert rec.blocks[j] == (receipt[off:off + 32], receipt[off + 32:off + 64], receipt[off + 64:off + 96],
                                 model["blocks"][j][3])
        c = p1.challenge(j, receipt[8:48], six, receipt[off + 64:off + 96])
        assert rec.challenge(j) == c < 1 << 128
        assert rec.blocks[j][3] == (NONCES[j] + c * FACTORS[j]) % R       # z = u + c k
    assert len({rec.challenge(j) for j in range(3)}) == 3


BAD_RECEIPTS = ("short", "long", "magic", "version", "m = 0", "m = 6", "tau_z = r", "beta_z all ones", "tau_before",
                "alpha_after", "beta_r")


@functools.lru_cache(maxsize=None)
def _bad_receipts():
    receipt = _honest()[2]
    no_g1 = cases.non_residue_x(1, random.Random(7))
    out = [("short", receipt[:-1], "length"), ("long", receipt + b"\0", "length"),
           ("magic", b"X" + receipt[1:], "magic"), ("version", receipt[:7] + b"\x02" + receipt[8:], "magic"),
           ("m = 0", receipt[:8] + bytes(8) + receipt[16:], "m"),
           ("m = 6", receipt[:8] + (6).to_bytes(8, "little") + receipt[16:], "m"),
           ("tau_z = r", receipt[:144] + R.to_bytes(32, "little") + receipt[176:], "tau_z"),
           ("beta_z all ones", receipt[:400] + b"\xff" * 32, "beta_z")]
    for name, off, bad in (("tau_before", 48, no_g1), ("alpha_after", 176 + 32, Q.to_bytes(32, "little")),
                           ("beta_r", 304 + 64, no_g1)):
        out.append((name, receipt[:off] + bad + receipt[off + 32:], name))
    assert tuple(c[0] for c in out) == BAD_RECEIPTS
    return {c[0]: c for c in out}


@pytest.mark.parametrize("label", BAD_RECEIPTS)
def test_receipt_parsing_is_strict(label):
    from octopuszk_amd import srs
    _, b, word = _bad_receipts()[label]
    with pytest.raises(ValueError) as e:
        p1.parse_receipt(b)                                  # the model rejects it too, for the same field
    assert str(e.value) == word
    with pytest.raises(ValueError) as e:
        srs.Receipt.from_bytes(b)
    assert word in str(e.value), str(e.value)


# ---------------------------------------------------------------------------- the file
@pytest.mark.parametrize("m", [2, 8, 1 << 21])
def test_file_size_formula(m):
    from octopuszk_amd import srs
    assert srs.string_file_size(m) == p1.file_size(m) == 48 + 32 * (4 * m + 1) + 64 * (m + 1)
    if m == 1 << 21:
        assert round(srs.string_file_size(m) / 1e6) == 403


@functools.lru_cache(maxsize=None)
def _file():
    s = p1.from_secrets_exp(2, T, AL, BE)
    sections = p1.sections_exp(s)
    return sections, p1.file_bytes(2, sections)


def test_file_round_trip_on_the_models_bytes():
    from octopuszk_amd import srs
    sections, b = _file()
    assert len(b) == p1.file_size(2) and b[:8] == srs.FILE_MAGIC == b"OZKSRS\x00\x01"
    assert srs.parse_string_file(b) == (2, sections) == p1.parse_file(b)
    assert srs.string_file_bytes(2, sections) == b
    assert tuple(name for name, _, _ in srs.FILE_SECTIONS) == p1.ARRAYS + ("beta_g2",)


BAD_FILES = ("magic", "version", "m = 0", "m = 3", "short", "long", "m of another length", "payload bit", "digest bit",
             "header only")


@functools.lru_cache(maxsize=None)
def _bad_files():
    _, b = _file()
    out = [("magic", b"X" + b[1:], "magic"), ("version", b[:7] + b"\x02" + b[8:], "magic"),
           ("m = 0", b[:8] + bytes(8) + b[16:], "m"), ("m = 3", b[:8] + (3).to_bytes(8, "little") + b[16:], "m"),
           ("short", b[:-1], "length"), ("long", b + b"\0", "length"),
           ("m of another length", b[:8] + (4).to_bytes(8, "little") + b[16:], "length"),
           ("payload bit", b[:100] + bytes([b[100] ^ 1]) + b[101:], "digest"),
           ("digest bit", b[:20] + bytes([b[20] ^ 1]) + b[21:], "digest"),
           ("header only", b[:40], "length")]
    assert tuple(c[0] for c in out) == BAD_FILES
    return {c[0]: c for c in out}


@pytest.mark.parametrize("label", BAD_FILES)
def test_file_parsing_is_strict(label):
    from octopuszk_amd import srs
    _, b, word = _bad_files()[label]
    if label != "header only":
        with pytest.raises(ValueError) as e:
            p1.parse_file(b)
        assert str(e.value) == word
    with pytest.raises(ValueError) as e:
        srs.parse_string_file(b)
    assert word in str(e.value), str(e.value)


def test_file_writer_refuses_wrong_lengths():
    from octopuszk_amd import srs
    sections, _ = _file()
    with pytest.raises(ValueError):
        srs.string_file_bytes(3, sections)
    with pytest.raises(ValueError):
        srs.string_file_bytes(4, sections)
    with pytest.raises(ValueError):
        srs.string_file_bytes(2, dict(sections, tau_g2=sections["tau_g2"][:-1]))


# ---------------------------------------------------------------------------- early errors
def test_bad_arguments_raise_before_any_library_call(monkeypatch):
    import torch

    from octopuszk_amd import lib
    from octopuszk_amd import srs

    def no_library():
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(lib, "load", no_library)
    string = srs.Srs(2, None, None, None, None, None)
    for bad in (0, R, -3, 1 << 256):
        for kw in ("tau", "alpha", "beta"):
            with pytest.raises(ValueError):
                string.contribute(**dict({"tau": 5, "alpha": 6, "beta": 7}, **{kw: bad}))
    for nonces in ((0, 1, 2), (1, 2, R), (1, 2), (1, 2, 3, 4)):
        with pytest.raises(ValueError):
            string.contribute(5, 6, 7, nonces=nonces)
    pts, sc = torch.zeros(96 * 3, dtype=torch.uint8), torch.zeros(32 * 3, dtype=torch.uint8)
    for p, s, type_ in ((pts, sc, 3), (pts, sc, 0), (pts, sc[:64], 1), (pts, sc, 2), (pts[:100], sc, 1),
                        (pts[:0], sc[:0], 1), (pts, torch.zeros(24, dtype=torch.int32), 1), (None, sc, 1)):
        with pytest.raises(ValueError):
            srs.mul_points(p, s, type_)
    with pytest.raises(ValueError):
        srs.verify_chain([string], [])
    with pytest.raises(ValueError):
        srs.Srs.initial(3)
