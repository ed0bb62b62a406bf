"""The proving-key file without a GPU: octopuszk_amd/keyfile.py against the model
(tests/keyfile_ref.py) — round trip, every rejection class, reads by offset — and the decoders that turn a compressed
point into prepared records (octopuszk_amd/csrc/point_codec.cuh, built for the host) against the model, byte for byte
and code for code."""
import ctypes
import functools
import hashlib
import os
import random
import struct
import subprocess

import pytest

import codec_cases as cases
import codec_ref as ref
import keyfile_ref as kref
from oracle import bn254 as o

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "keyfile_hostcheck.cpp")
LIB = os.path.join(HERE, "native", "_keyfile_hostcheck.so")
CSRC = os.path.join(HERE, "..", "octopuszk_amd", "csrc")
Q = o.Q

NI, NA, NC = 2, 7, 5          # a 5-constraint R1CS with coefficients: nv = 9, m = 8
NV, M = NI + NA, 8


@functools.lru_cache(maxsize=None)
def _small_key():
    """(the sections of a small key: name -> bytes; the R1CS sides as (ptr, index, value))"""
    rng = random.Random(14)
    sections = {}
    for k, name in enumerate(kref.NAMES[:10]):
        type_ = 2 if name in kref.G2_NAMES else 1
        n = {"query_a": NV, "query_b_g1": NV, "query_b_g2": NV, "delta_abc_g1": NV - NI, "query_h": M + 1}.get(name, 1)
        pts = [P for P in cases.points(type_, 40, seed=60 + k) if not cases.curve(type_).is_zero(P)][:n]
        if n > 1:
            pts[1] = cases.curve(type_).zero        # the queries of a real key hold O
        sections[name] = b"".join(cases.encode(type_, P) for P in pts)
    sides = []
    for name in kref.NAMES[10:]:
        counts = [rng.randrange(0, 4) for _ in range(NC)]
        ptr = [0]
        for c in counts:
            ptr.append(ptr[-1] + c)
        idx = [rng.randrange(NV) for _ in range(ptr[-1])]
        val = [rng.choice((1, o.R - 1, rng.randrange(o.R))) for _ in range(ptr[-1])] if name != "r1cs_c" else None
        sides.append((ptr, idx, val))
        sections[name] = kref.r1cs_section(ptr, idx, val)
    return sections, sides


def _file():
    sections, _ = _small_key()
    return kref.write(NI, NA, NC, sections)


def _redigest(b):
    """b with the digest of its present payload (for corruptions that are to reach the check after the digest)"""
    return b[:24] + hashlib.sha256(b[kref.HEADER:]).digest() + b[56:]


def _entry(b, name):
    return struct.unpack_from("<IQQ", b, 56 + 20 * kref.NAMES.index(name))


def _set_entry(b, name, off, length):
    i = kref.NAMES.index(name)
    return b[:56 + 20 * i] + struct.pack("<IQQ", i + 1, off, length) + b[56 + 20 * (i + 1):]


# ---------------------------------------------------------------------------- format
def test_round_trip_of_a_small_key():
    from octopuszk_amd import keyfile
    sections, sides = _small_key()
    want = _file()
    assert keyfile.HEADER_BYTES == kref.HEADER and keyfile.NAMES == kref.NAMES
    got = keyfile.build(NI, NA, NC, {n: (sections[n] if i < 10 else keyfile.r1cs_section(*sides[i - 10]))
                                     for i, n in enumerate(kref.NAMES)})
    assert got == want                                      # the writer against the model's writer
    kf = keyfile.KeyFile(want)
    kf.verify_digest()
    h = kf.header
    assert (h.num_inputs, h.num_auxiliary, h.num_constraints, h.m, h.nv) == (NI, NA, NC, M, NV)
    model = kref.parse(want)
    assert model["counts"] == (NI, NA, NC, M)
    for name in kref.NAMES[:10]:
        assert kf.read(name) == sections[name] == model[name]
    for (ptr, idx, val), (mp, mi, mv), (wp, wi, wv) in zip(kf.r1cs(), (model[n] for n in kref.NAMES[10:]), sides):
        assert list(ptr) == mp == wp and list(idx) == mi == wi
        assert (val is None) == (mv is None) == (wv is None)
        if wv is not None:
            assert [int(v) for v in val] == mv == wv


def _corruptions():
    """(label, corrupted file, the section its error must name, a word its error must hold)"""
    b = _file()
    out = []
    out.append(("magic", b"X" + b[1:], "header", "magic"))
    out.append(("version", b[:7] + b"\x02" + b[8:], "header", "version"))
    out.append(("truncated header", b[:100], "header", "truncated"))
    out.append(("truncated file", b[:-5], "r1cs_c", "truncated"))
    _, off, length = _entry(b, "query_h")
    out.append(("out of bounds", _set_entry(b, "query_h", len(b) - 8, length), "query_h", "out of bounds"))
    out.append(("inside the header", _set_entry(b, "alpha_g1", 16, 32), "alpha_g1", "out of bounds"))
    _, a_off, _ = _entry(b, "alpha_g1")
    out.append(("overlap", _set_entry(b, "beta_g1", a_off + 16, 32), "beta_g1", "overlaps"))
    out.append(("length against the counts", _set_entry(b, "query_a", _entry(b, "query_a")[1], 32 * (NV - 1)), "query_a",
                "counts"))
    # the R1CS of side A rewritten in place (same length), the digest renewed so that the parser reaches the section
    _, r_off, r_len = _entry(b, "r1cs_a")
    sec = bytearray(b[r_off:r_off + r_len])
    rows, nnz, _ = struct.unpack_from("<III", sec, 0)

    def with_section(s):
        return _redigest(b[:r_off] + bytes(s) + b[r_off + r_len:])

    s = bytearray(sec)
    struct.pack_into("<I", s, 12 + 4 * 2, struct.unpack_from("<I", s, 12 + 4 * 3)[0] + 1)   # offset 2 above offset 3
    out.append(("decreasing row offsets", with_section(s), "r1cs_a", "non-decreasing"))
    s = bytearray(sec)
    struct.pack_into("<I", s, 12 + 4 * rows, nnz - 1 if nnz else 1)
    out.append(("row offsets do not end at nnz", with_section(s), "r1cs_a", "nnz"))
    s = bytearray(sec)
    struct.pack_into("<I", s, 12 + 4 * (rows + 1), NV)
    out.append(("index >= nv", with_section(s), "r1cs_a", "index"))
    s = bytearray(sec)
    base = 12 + 4 * (rows + 1) + 4 * nnz
    s[base + 32:base + 64] = o.R.to_bytes(32, "little")
    out.append(("coefficient >= r", with_section(s), "r1cs_a", "coefficient 1"))
    s = bytearray(sec)
    struct.pack_into("<I", s, 4, nnz + 1)
    out.append(("r1cs length against its counts", with_section(s), "r1cs_a", "counts"))
    _, q_off, _ = _entry(b, "query_b_g2")
    flipped = bytearray(b)
    flipped[q_off + 70] ^= 4
    out.append(("digest", bytes(flipped), "digest", "mismatch"))
    return out


@pytest.mark.parametrize("case", _corruptions(), ids=lambda c: c[0])
def test_rejections(case):
    from octopuszk_amd import keyfile
    label, b, section, word = case
    with pytest.raises(ValueError):
        kref.parse(b)                                        # the model rejects it too
    with pytest.raises(ValueError) as e:
        kf = keyfile.KeyFile(b)
        kf.verify_digest()
        kf.r1cs()
    assert section in str(e.value) and word in str(e.value), str(e.value)


def test_the_r1cs_assert_of_the_small_key_has_what_the_corruptions_need():
    _, sides = _small_key()
    ptr, idx, val = sides[0]
    assert len(idx) >= 2 and val is not None and ptr[3] >= 1


@pytest.mark.parametrize("world", [1, 2, 3])
def test_rank_slices_read_by_offset_join_to_the_whole(world):
    from octopuszk_amd import keyfile
    from octopuszk_amd.zksnark import ShardedProver, shard_plan
    sections, _ = _small_key()
    kf = keyfile.KeyFile(_file())
    for attr, key, names, type_ in ShardedProver._MSMS:
        whole = b"".join(sections[n] for n in names)
        joined, rows = b"", 0
        for rank in range(world):
            lo, hi = shard_plan(NV, M, NV - NI, rank, world)[key]
            part, parts = kf.read_joined(names, lo, hi)
            assert len(part) == 32 * type_ * (hi - lo) and sum(c for _, _, c in parts) == hi - lo
            for j in range(hi - lo):
                name, i = keyfile.locate(parts, j)
                assert part[32 * type_ * j:32 * type_ * (j + 1)] == sections[name][32 * type_ * i:32 * type_ * (i + 1)]
            joined += part
            rows += hi - lo
        assert joined == whole and rows == len(whole) // (32 * type_)


# ---------------------------------------------------------------------------- the decoders, built for the host
@pytest.fixture(scope="module")
def kfhc():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("point_codec.cuh", "glv.cuh",
                                                    "fq2.cuh", "fp29.cuh", "ec.cuh", "curve.cuh",
                                                    "pairing_consts_gen.h", "consts_gen.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


def _words(b):
    return (ctypes.c_uint32 * (len(b) // 4)).from_buffer_copy(b)


def test_model_constants():
    assert (kref.BETA_G1 ** 2 + kref.BETA_G1 + 1) % Q == 0 and (kref.LAMBDA ** 2 + kref.LAMBDA + 1) % o.R == 0
    P = o.G1.to_affine(o.G1.mul(o.G1.one, 31337))
    assert o.G1.equals((kref.BETA_G1 * P[0] % Q, P[1], 1), o.G1.mul(P, kref.LAMBDA))
    T = o.G2.to_affine(o.G2.mul(o.G2.one, 271828))
    assert o.G2.equals(((kref.BETA_G2 * T[0][0] % Q, kref.BETA_G2 * T[0][1] % Q), T[1], (1, 0)), o.G2.mul(T, kref.LAMBDA))


@pytest.mark.parametrize("type_", [1, 2])
def test_record_statement_against_the_conversion_of_wire_points(kfhc, type_):
    """what the model calls a record is what the steps of the conversion kernel write (from_wire, normalisation,
    canonical, glv_image, store_aff, compiled for the host): ten points, some Jacobian with Z != 1, one O"""
    C = cases.curve(type_)
    pts = cases.points(type_, 9, seed=77) + [C.zero]
    assert sum(1 for P in pts if not C.is_zero(P) and P[2] not in (1, (1, 0))) >= 1
    fn = kfhc.kfhc_g1_convert if type_ == 1 else kfhc.kfhc_g2_convert
    for P in pts:
        out = (ctypes.c_uint32 * (32 * type_))()
        fn(_words(cases.wire(type_, P, 0)), out)
        a, b = kref.records(type_, C.zero_affine if C.is_zero(P) else C.to_affine(P))
        assert bytes(out) == a + b, P


@pytest.mark.parametrize("type_", [1, 2])
def test_decode_to_prepared_matches_model(kfhc, type_):
    encs, bad = cases.encodings(type_, 160, seed=31)
    assert {cls for cls, _ in bad.values()} == set(cases.G1_CLASSES if type_ == 1 else cases.G2_CLASSES)
    C = cases.curve(type_)
    inf = cases.encode(type_, C.zero)
    encs += [cases.encode(type_, C.one), cases.encode(type_, C.negate(C.one)), inf, inf]
    if type_ == 1:
        encs += [x.to_bytes(32, "little") for x in range(40)]
    want, codes = kref.prepared(type_, encs)
    assert set(codes) == {0, 1, 2, 3}
    n, rec = len(encs), 64 * type_
    fn = kfhc.kfhc_g1_decode_prepared if type_ == 1 else kfhc.kfhc_g2_decode_prepared
    for i, enc in enumerate(encs):
        out = (ctypes.c_uint32 * (32 * type_))()
        code = fn(_words(enc), out)
        assert code == codes[i], (i, enc.hex())
        assert bytes(out)[:rec] == want[rec * i:rec * (i + 1)], (i, enc.hex())
        assert bytes(out)[rec:] == want[rec * (n + i):rec * (n + i + 1)], (i, enc.hex())
        if codes[i] or enc == inf:
            assert bytes(out) == bytes(2 * rec)


def test_subgroup_function_on_the_host(kfhc):
    """[r]P = O through scalar_mul on stored records, as the subgroup kernel runs it: multiples of the generator
    pass, twist points from random x do not (the model multiplies by r in oracle integers)"""
    rng = random.Random(5)
    inside = [o.G2.to_affine(o.G2.mul(o.G2.one, rng.randrange(1, o.R))) for _ in range(3)]
    outside = []
    while len(outside) < 3:
        code, P = ref.decode_g2(cases._le(rng.randrange(Q)) + cases._le(rng.randrange(Q)))
        if code == 0:
            outside.append(P)
    for P, want in [(P, True) for P in inside] + [(P, False) for P in outside] + [(o.G2.zero_affine, True)]:
        assert kref.in_subgroup(P) == want
        assert bool(kfhc.kfhc_g2_in_subgroup(_words(kref.records(2, P)[0]))) == want
