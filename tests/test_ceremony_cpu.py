"""Phase-2 key contributions without a GPU: the per-point function of the scaling kernel and the
host recoding of its scalar (octopuszk_amd/csrc/points_scale.cuh, built for the host) against the integer model
(tests/ceremony_ref.py), the model's own identities on a toy CRS, and the receipt's bytes and strict parsing."""
import copy
import ctypes
import functools
import os
import random
import subprocess

import pytest

import ceremony_ref as cref
import codec_cases as cases
from oracle import bn254 as o
from oracle import groth16 as g

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "ceremony_hostcheck.cpp")
LIB = os.path.join(HERE, "native", "_ceremony_hostcheck.so")
CSRC = os.path.join(HERE, "..", "octopuszk_amd", "csrc")
Q, R = o.Q, o.R


@pytest.fixture(scope="module")
def cmhc():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("points_scale.cuh", "glv.cuh", "fq2.cuh", "fp29.cuh", "ec.cuh",
                                                    "curve.cuh", "consts_gen.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


def _words(b):
    return (ctypes.c_uint32 * (len(b) // 4)).from_buffer_copy(b)


def _le(v):
    return int(v).to_bytes(32, "little")


# ---------------------------------------------------------------------------- the kernel's pieces on the host
def test_no_g1_point_has_x_zero():
    """what lets the ladder take P - phi(P) with an affine addition: (beta - 1) x is never 0"""
    assert pow(3, (Q - 1) // 2, Q) == Q - 1


def _points(type_):
    C = cases.curve(type_)
    rng = random.Random(40 + type_)
    P = C.to_affine(C.mul(C.one, rng.randrange(1, R)))
    J = cases.rescale(type_, C.to_affine(C.mul(C.one, rng.randrange(1, R))), rng.randrange(2, Q))
    return [C.to_affine(C.one), P, J, C.zero]


@pytest.mark.parametrize("type_", [1, 2])
def test_per_point_function_matches_the_model(cmhc, type_):
    C = cases.curve(type_)
    pts = _points(type_)
    assert pts[2][2] not in (1, (1, 0)) and C.is_zero(pts[3])
    for k in cref.scalars():
        for P in pts:
            out = (ctypes.c_uint32 * (24 * type_))()
            assert cmhc.cmhc_scale(_words(cases.wire(type_, P, 0)), type_, _words(_le(k)), out) == 0
            assert bytes(out) == cref.wire(type_, cref.scale(type_, P, k)), (k, P)


def test_g2_is_exact_outside_the_subgroup(cmhc):
    """[r - 1] P of a twist point whose order does not divide r is the oracle's, and is not -P: the subgroup test"""
    P = cref.twist_point_outside_the_subgroup()
    out = (ctypes.c_uint32 * 48)()
    assert cmhc.cmhc_scale(_words(cases.wire(2, P, 0)), 2, _words(_le(R - 1)), out) == 0
    want = cref.scale(2, P, R - 1)
    assert bytes(out) == cref.wire(2, want)
    assert want != o.G2.to_affine(o.G2.negate(P))


@pytest.mark.parametrize("type_", [1, 2])
def test_recoding_reconstructs_the_scalar(cmhc, type_):
    rng = random.Random(16)
    density = []
    for k in cref.scalars() + [rng.randrange(R) for _ in range(1000)]:
        steps = (ctypes.c_uint8 * 256)()
        n = cmhc.cmhc_recode(_words(_le(k)), type_, steps)
        assert 0 <= n <= (130 if type_ == 1 else 255), (k, n)
        assert cref.schedule_value(list(steps[:n]), type_) == k, k      # raises on a digit outside its range
        assert n == 0 or steps[n - 1] != 0                               # no leading zero step
        density.append((n, sum(1 for c in steps[:n] if c)))
    # the cost DESIGN.md counts: about 128 doublings and 64 additions for G1, 254 and 85 for G2
    steps_mean = sum(n for n, _ in density[-1000:]) / 1000
    adds_mean = sum(a for _, a in density[-1000:]) / 1000
    assert (steps_mean, adds_mean) < ((129, 68) if type_ == 1 else (255, 88))


def test_recoding_refuses_scalars_from_r_on(cmhc):
    steps = (ctypes.c_uint8 * 256)()
    out = (ctypes.c_uint32 * 24)()
    for k in (R, R + 1, (1 << 256) - 1):
        assert cmhc.cmhc_recode(_words(_le(k)), 1, steps) == -1
        assert cmhc.cmhc_scale(_words(cases.wire(1, o.G1.one, 0)), 1, _words(_le(k)), out) == -1
    assert cmhc.cmhc_recode(_words(_le(R - 1)), 1, steps) > 0


# ---------------------------------------------------------------------------- the model on a toy CRS
D, U, SEED = 0x1234567890ABCDEF1234567890ABCDEF % R, 0xFEDCBA0987654321 % R, b"seed of the cpu tests"


@functools.lru_cache(maxsize=None)
def _toy():
    """(crs, primary, auxiliary, key in the exponent) of the smallest CRS tests/test_groth16_cpu.py builds"""
    r1cs, primary, auxiliary = g.serial_construct(8, 3)
    crs = g.serial_setup(r1cs)
    sec, q = crs.secrets, crs.qap
    key = dict(alpha_g1=sec["alpha"], beta_g1=sec["beta"], beta_g2=sec["beta"], delta_g1=sec["delta"],
               delta_g2=sec["delta"], query_a=list(q.At), query_b_g1=list(q.Bt), query_b_g2=list(q.Bt),
               delta_abc_g1=list(crs.delta_abc_scalars), query_h=list(crs.ht_scalars), r1cs="the r1cs",
               gen_g1=crs.gen_g1, gen_g2=crs.gen_g2)
    return crs, primary, auxiliary, key


@functools.lru_cache(maxsize=None)
def _contributed():
    return cref.contribute_exp(_toy()[3], D, U)


def test_model_contribution_moves_the_groth16_equation_to_the_new_delta():
    crs, primary, auxiliary, key = _toy()
    new, _ = _contributed()
    assert new["delta_g1"] == key["delta_g1"] * D % R and all(new[n] is key[n] for n in cref.UNCHANGED)
    crs2 = copy.copy(crs)
    crs2.secrets = dict(crs.secrets, delta=new["delta_g1"])
    crs2.delta_abc_scalars, crs2.ht_scalars = new["delta_abc_g1"], new["query_h"]
    full, H, _, _ = g.r1cs_to_qap_witness(crs.r1cs, primary, auxiliary)
    abc = g.proof_scalars(crs2, full, H, 11, 13)
    assert g.verify_in_the_exponent(crs2, primary, abc)
    assert not g.verify_in_the_exponent(crs, primary, abc)              # the old equation fails for it
    assert g.verify_in_the_exponent(crs, primary, g.proof_scalars(crs, full, H, 11, 13))


def test_model_accepts_the_honest_contribution():
    key = _toy()[3]
    new, receipt = _contributed()
    vk_b, vk_a = dict(delta_g2=key["delta_g2"], rest="vk"), dict(delta_g2=new["delta_g2"], rest="vk")
    assert cref.verify_contribution_exp(key, new, receipt, SEED, vk_before=vk_b, vk_after=vk_a) == (True, None)
    assert cref.verify_contribution_exp(key, new, receipt, SEED, r_log=U * key["delta_g1"] % R) == (True, None)


TAMPERS = ("query_h[first]", "query_h[middle]", "query_h[last]", "delta_abc_g1 doubled", "query_h by another d",
           "delta_g2 by another factor", "query_a changed", "r1cs changed", "delta_g1 at infinity", "z + 1",
           "the deltas of another key", "vk_after with the old delta")


@functools.lru_cache(maxsize=None)
def _tampers():
    """label -> (before, after, receipt, vk_before, vk_after, the check that must fail)"""
    key = _toy()[3]
    new, receipt = _contributed()
    vk_b, vk_a = dict(delta_g2=key["delta_g2"], rest="vk"), dict(delta_g2=new["delta_g2"], rest="vk")
    out = {}

    def case(label, why, after=new, rec=receipt, before=key, vb=vk_b, va=vk_a):
        out[label] = (before, after, rec, vb, va, why)

    nh = len(new["query_h"])
    for i, where in ((0, "first"), (nh // 2, "middle"), (nh - 1, "last")):
        t = dict(new, query_h=list(new["query_h"]))
        t["query_h"][i] = (t["query_h"][i] + 12345) % R
        case("query_h[%s]" % where, "vectors", t)
    t = dict(new, delta_abc_g1=list(new["delta_abc_g1"]))
    t["delta_abc_g1"][1] = t["delta_abc_g1"][1] * 2 % R
    assert t["delta_abc_g1"][1] != new["delta_abc_g1"][1]
    case("delta_abc_g1 doubled", "vectors", t)
    other = pow(D + 1, -1, R)
    case("query_h by another d", "vectors", dict(new, query_h=[x * other % R for x in key["query_h"]]))
    t = dict(new, delta_g2=key["delta_g2"] * (D + 1) % R)
    case("delta_g2 by another factor", "delta_ratio", t, cref.receipt_exp(key, t, D, U), va=dict(vk_a, delta_g2=t["delta_g2"]))
    t = dict(new, query_a=[(new["query_a"][0] + 1) % R] + new["query_a"][1:])
    case("query_a changed", "unchanged", t)
    case("r1cs changed", "unchanged", dict(new, r1cs="another r1cs"))
    t = dict(new, delta_g1=0)
    case("delta_g1 at infinity", "delta_wellformed", t, cref.receipt_exp(key, t, D, U))
    z = int.from_bytes(receipt[264:], "little")
    case("z + 1", "pok", rec=receipt[:264] + ((z + 1) % R).to_bytes(32, "little"))
    elsewhere = dict(key, delta_g1=key["delta_g1"] * 7 % R, delta_g2=key["delta_g2"] * 7 % R)
    case("the deltas of another key", "receipt_deltas", rec=cref.contribute_exp(elsewhere, D, U)[1])
    case("vk_after with the old delta", "vk", va=vk_b)
    assert tuple(out) == TAMPERS
    return out


@pytest.mark.parametrize("label", TAMPERS)
def test_model_rejects_each_tamper_class(label):
    before, after, receipt, vk_b, vk_a, why = _tampers()[label]
    for seed in (SEED, os.urandom(32)):
        assert cref.verify_contribution_exp(before, after, receipt, seed, vk_before=vk_b, vk_after=vk_a) == (False, why)


# ---------------------------------------------------------------------------- receipt, weights, bad scalars
def test_receipt_round_trip_and_layout():
    from octopuszk_amd import ceremony
    _, receipt = _contributed()
    assert len(receipt) == ceremony.RECEIPT_BYTES == 296 and receipt[:8] == ceremony.MAGIC == b"OZKC2\x00\x00\x01"
    rec = ceremony.Receipt.from_bytes(receipt)
    assert rec.to_bytes() == receipt
    model = cref.parse_receipt(receipt)
    assert rec.h == model["h"] == cref.transcript_digest(b"") and rec.z == model["z"]
    assert (rec.delta_g1_before, rec.delta_g2_after, rec.r) == (receipt[40:72], receipt[168:232], receipt[232:264])
    assert rec.body() == receipt[8:232]
    assert ceremony._challenge(rec.body(), rec.r) == cref.challenge(receipt[8:232], receipt[232:264]) < 1 << 128
    # the response answers the challenge: z = u + c d
    assert rec.z == (U + cref.challenge(receipt[8:232], receipt[232:264]) * D) % R


BAD_RECEIPTS = ("short", "long", "magic", "version", "z = r", "z all ones", "delta_g1_before", "delta_g1_after",
                "delta_g2_before", "delta_g2_after", "r")


@functools.lru_cache(maxsize=None)
def _bad_receipts():
    _, receipt = _contributed()
    rng = random.Random(7)
    no_g1 = cases.non_residue_x(1, rng)
    no_g2 = cases.non_residue_x(2, rng)
    out = [("short", receipt[:-1], "length"), ("long", receipt + b"\0", "length"),
           ("magic", b"X" + receipt[1:], "magic"), ("version", receipt[:7] + b"\x02" + receipt[8:], "magic"),
           ("z = r", receipt[:264] + R.to_bytes(32, "little"), "z"),
           ("z all ones", receipt[:264] + b"\xff" * 32, "z")]
    for name, off, bad in (("delta_g1_before", 40, no_g1), ("delta_g1_after", 72, Q.to_bytes(32, "little")),
                           ("delta_g2_before", 104, no_g2), ("delta_g2_after", 168, bytes(63) + b"\xc0"),
                           ("r", 232, no_g1)):
        out.append((name, receipt[:off] + bad + receipt[off + len(bad):], name))
    assert tuple(c[0] for c in out) == BAD_RECEIPTS
    return {c[0]: c for c in out}


@pytest.mark.parametrize("label", BAD_RECEIPTS)
def test_receipt_parsing_is_strict(label):
    from octopuszk_amd import ceremony
    _, b, word = _bad_receipts()[label]
    with pytest.raises(ValueError):
        cref.parse_receipt(b)                                # the model rejects it too
    with pytest.raises(ValueError) as e:
        ceremony.Receipt.from_bytes(b)
    assert word in str(e.value), str(e.value)


def test_host_decode_codes_match_the_codec_model():
    """the receipt parser's own point check against tests/codec_ref.py, every malformed class"""
    from octopuszk_amd import codec
    for type_ in (1, 2):
        encs, bad = cases.encodings(type_, 80, seed=9)
        assert len({cls for cls, _ in bad.values()}) >= 5
        for e in encs:
            assert codec.decode_code(e, type_) == cases.decode(type_, e)[0], e.hex()


def test_weight_stream_matches_the_model():
    from octopuszk_amd import ceremony, transcript
    for n in (1, 2, 5, 64):
        raw = transcript.weights(SEED, n, ceremony._RHO_TAG)
        got = [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(n)]
        assert got == cref.weights(SEED, n) and all(1 <= w < 1 << 128 for w in got)
    assert cref.weights(SEED, 5) == cref.weights(SEED, 6)[:5] and cref.weights(SEED, 4) != cref.weights(b"other", 4)
    assert transcript.seed_bytes(5) == (5).to_bytes(32, "little") and len(transcript.seed_bytes(None)) == 32


def test_bad_scalars_raise_before_any_library_call(monkeypatch):
    from octopuszk_amd import ceremony
    from octopuszk_amd import lib

    def no_library():
        raise AssertionError("the library was asked for")

    monkeypatch.setattr(lib, "load", no_library)
    for k in (R, R + 5, 1 << 256, -1):
        with pytest.raises(ValueError):
            ceremony.scale_points(None, k, 1)
    for d in (0, R, -3):
        with pytest.raises(ValueError):
            ceremony.contribute(None, None, d)
    with pytest.raises(ValueError):
        ceremony.contribute(None, None, 5, nonce=0)
    with pytest.raises(ValueError):
        ceremony.scale_points(None, 1, 3)
