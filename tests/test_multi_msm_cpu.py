"""The shared-base batched MSM's table plan and recoding, with exact integers: the Python model
(tests/multi_msm_ref.py) against oracle.bn254's naive MSM, and the header the kernels compile
(octopuszk_amd/csrc/msm_multi.cuh, built for the host) against the model."""
import ctypes
import os
import random
import subprocess

import pytest

import multi_msm_ref as ref
from oracle import bn254 as o

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "multi_msm_hostcheck.cpp")
LIB = os.path.join(HERE, "native", "_multi_msm_hostcheck.so")
CSRC = os.path.join(HERE, "..", "octopuszk_amd", "csrc")


@pytest.fixture(scope="module")
def mmhc():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("msm_multi.cuh", "glv.cuh", "fp29.cuh", "ec.cuh", "curve.cuh")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


def _bases(n, seed):
    rng = random.Random(seed)
    return [o.G1.to_affine(o.G1.mul(o.G1.one, rng.randrange(1, o.R))) for _ in range(n)]


def _naive(row, bases):
    return o.G1.to_affine(o.naive_msm(o.G1, [s % o.R for s in row], bases))


def test_plan_rule():
    assert [ref.window_bits(n) for n in (1, 15, 1023, 1024, 1280)] == [8] * 5
    assert ref.window_bits(1281) == 7 and ref.window_bits(2155) == 7 and ref.window_bits(2156) == 6
    assert ref.window_bits(3723) == 6 and ref.window_bits(3724) == 5 and ref.window_bits(4096) == 5
    for ws in range(ref.WS_MIN, ref.WS_MAX + 1):
        assert ref.windows(ws) * ws >= 128
    assert ref.records_per_base(8) * 64 == 128 << 10            # 128 KiB per base at ws = 8
    assert 4096 * ref.records_per_base(ref.window_bits(4096)) * 64 <= ref.TABLE_BUDGET


def test_edge_scalars_are_what_they_claim():
    k = int("5f" + "c1" * 15, 16)
    s = ref.edge_scalars()[-2]
    assert ref.glv_split(s) == (k, -k)                            # opposite signs
    for ws in (8, 7):
        digits, carry = ref.recode(k, ws)
        assert carry == 0
    digits, _ = ref.recode(k, 8)
    assert all(d < 0 for d in digits[:-1]) and digits[-1] == 0x5f + 1   # a carry out of every window below the top
    assert all(s < o.R for s in ref.edge_scalars())


@pytest.mark.parametrize("ws", [4, 5, 6, 7, 8])
def test_recode_exact(ws):
    rng = random.Random(ws)
    half = 1 << (ws - 1)
    mags = [0, 1, half, half + 1, (1 << 127) - 1, 1 << 126, int("5f" + "c1" * 15, 16), int(2 ** 126.96)]
    mags += [sum(half << (ws * w) for w in range(120 // ws))]   # raw == half everywhere: never carries
    mags += [sum((half + 1) << (ws * w) for w in range(120 // ws))]   # raw == half + 1: always carries
    mags += [rng.randrange(1 << 127) for _ in range(500)]
    for m in mags:
        digits, carry = ref.recode(m, ws)
        assert carry == 0, hex(m)
        assert all(-(half - 1) <= d <= half for d in digits)
        assert sum(d << (ws * w) for w, d in enumerate(digits)) == m


@pytest.mark.parametrize("ws", [4, 5, 6, 7, 8])
def test_carry_patterns_come_back_from_the_split(ws):
    """the scalars test_multi_msm_windows_gpu.py builds from the never-carries / always-carries magnitudes: the split
    gives back exactly those halves, and the model agrees with the naive MSM on them"""
    ref.assert_carry_patterns_realised(ws)
    bases = _bases(2, 13)
    rows = [[s, 0] for s, _, _ in ref.carry_pattern_scalars(ws)][:2] + [[s for s, _, _ in ref.carry_pattern_scalars(ws)][2:]]
    for row, g in zip(rows, ref.model_msm(rows, bases, ws)):
        assert g == _naive(row, bases), (ws, row)


@pytest.mark.parametrize("ws", [8, 7, 5])
def test_model_matches_naive_msm_on_edge_scalars(ws):
    bases = _bases(3, 11)
    edges = ref.edge_scalars()
    rows = [[e, 0, 0] for e in edges] + [[0, 0, e] for e in edges]
    rows += [[edges[i], edges[-1 - i], edges[(i + 5) % len(edges)]] for i in range(len(edges))]
    if ws != 8:
        rows = rows[::3]
    got = ref.model_msm(rows, bases, ws)
    for row, g in zip(rows, got):
        assert g == _naive(row, bases), (ws, row)


def test_model_random_rows_and_special_bases():
    rng = random.Random(3)
    P = _bases(1, 5)[0]
    bases = [P, o.G1.negate(P), o.G1.zero, P, o.G1.mul(P, 7)]     # repeated, negated, infinity, Z != 1
    rows = [[rng.randrange(o.R) for _ in bases] for _ in range(4)]
    rows += [[0] * len(bases), [5, 5, 9, 0, 0], [1, 0, 0, o.R - 1, 0], [3, 1, 1, o.R - 2, 0]]
    got = ref.model_msm(rows, bases)
    for row, g in zip(rows, got):
        assert g == _naive(row, bases), row
    assert got[4] == (0, 1, 0) and got[5] == (0, 1, 0) and got[6] == (0, 1, 0) and got[7] == (0, 1, 0)


def test_model_reduces_unreduced_scalars():
    bases = _bases(2, 8)
    rows = [[o.R, (1 << 256) - 1], [(1 << 254) - 1, o.R + 5]]
    for row, g in zip(rows, ref.model_msm(rows, bases)):
        assert g == _naive(row, bases)


def test_header_matches_model(mmhc):
    for n in (1, 15, 1023, 1280, 1281, 2155, 2156, 3723, 3724, 4096):
        assert mmhc.mmhc_window_bits(n) == ref.window_bits(n)
    rng = random.Random(17)
    scalars = ref.edge_scalars() + [o.R, (1 << 254) - 1, (1 << 256) - 1]
    scalars += [rng.randrange(o.R) for _ in range(2000)] + [rng.randrange(1 << 256) for _ in range(500)]
    for ws in range(ref.WS_MIN, ref.WS_MAX + 1):
        oc = ref.windows(ws)
        assert mmhc.mmhc_windows(ws) == oc
        for s in scalars:
            words = (ctypes.c_uint32 * 8)(*[(s >> (32 * i)) & 0xffffffff for i in range(8)])
            digits = (ctypes.c_int * (2 * oc))()
            neg = (ctypes.c_int * 2)()
            assert mmhc.mmhc_recode(words, ws, digits, neg) == 0, (ws, hex(s))
            for h, kh in enumerate(ref.glv_split(s)):
                want, carry = ref.recode(abs(kh), ws)
                assert carry == 0
                assert list(digits[h * oc:(h + 1) * oc]) == want, (ws, hex(s), h)
                assert bool(neg[h]) == (kh < 0) or kh == 0


def _host_eval(mmhc, bases, rows, ws, T):
    n, k = len(bases), len(rows)
    wire = b"".join(o.g1_to_wire(tuple(c % o.Q for c in P)) for P in bases)
    sc = b"".join(int(s).to_bytes(32, "little") for row in rows for s in row)
    out = ctypes.create_string_buffer(192 * k)
    assert mmhc.mmhc_eval(wire, n, sc, k, ws, T, out) == 0
    return [o.g1_from_out_le(out.raw[192 * i:192 * (i + 1)]) for i in range(k)]


@pytest.mark.parametrize("ws,T", [(8, 2), (8, 8), (8, 64), (8, 256), (7, 4), (5, 16)])
def test_pipeline_with_device_arithmetic_on_the_host(mmhc, ws, T):
    """chain / level table build, record round trip, lane split, phi on the half sums, shuffle tree, partial sums and
    normalisation, compiled for the host from the kernels' own headers, against the oracle's naive MSM"""
    rng = random.Random(ws * 100 + T)
    P = _bases(1, 4)[0]
    z = 0xabcdef0123456789
    R = _bases(2, 6)
    bases = [P, o.G1.negate(P), (0, 1, 0), P, (R[0][0] * z * z % o.Q, R[0][1] * z * z * z % o.Q, z), R[1], P]
    n = len(bases)
    edges = ref.edge_scalars() + [o.R, (1 << 256) - 1]
    rows = [[rng.randrange(o.R) for _ in range(n)] for _ in range(2)]
    rows += [[edges[(t + j) % len(edges)] for j in range(n)] for t in range(0, len(edges), 2 if ws == 8 else 5)]
    rows += [[0] * n, [5, 5, 9, 0, 0, 0, 0], [1, 0, 0, o.R - 1, 0, 0, 0], [2, 1, 0, 0, 0, 0, o.R - 1]]
    got = _host_eval(mmhc, bases, rows, ws, T)
    for row, g in zip(rows, got):
        assert tuple(g) == tuple(_naive(row, bases)), (ws, T, row)
    assert all(tuple(g) == (0, 1, 0) for g in got[-4:])
