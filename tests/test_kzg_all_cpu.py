"""KZG openings at every coset at once without a GPU: the integer model of the FK20 construction
against the direct definition (tests/kzg_all_ref.py), the per-lane functions of the multiply-accumulate kernel over
points (octopuszk_amd/csrc/points_mac.cuh, built for the host) against products of logarithms, the argument errors of
OpenAllKey raised before any library call, and the new names in the binding and the header.

The kernel streams its schedules from the workspace, so it has no term-group size G: the term counts below are 1, 2, 3,
both sides of 8 and of 16, 31 and 32 (every count runs the same loop)."""
import ctypes
import functools
import os
import random
import subprocess

import pytest

import ceremony_ref as cref
import codec_cases as cases
import kzg_all_ref as ka
import kzg_ref as kr
from oracle import bn254 as o

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "points_mac_hostcheck.cpp")
LIB = os.path.join(HERE, "native", "_points_mac_hostcheck.so")
CSRC = os.path.join(HERE, "..", "octopuszk_amd", "csrc")
R, Q = o.R, o.Q
TAU = 0x5eed0123456789abcdef0123456789abcdef0123456789abcdef % R
TERMS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32)


# ---------------------------------------------------------------------------- the model against the definition
@pytest.mark.parametrize("n,l", ka.CHECKED_SHAPES + ((4, 2), (4, 4), (64, 1), (64, 8), (64, 32)))
def test_model_equals_the_definition(n, l):
    rng = random.Random(100 * n + l)
    for p in ka.rows(n, rng) + [[0] * n]:
        proofs, W = ka.model(p, l, TAU)
        assert proofs == ka.proofs_by_definition(p, l, TAU), (n, l)
        assert len(proofs) == n // l
        if n // l > 1:
            assert len(W) == 2 * n // l and W[-1] == 0
    assert ka.model([0] * n, l, TAU)[0] == [0] * (n // l)


def test_the_definition_is_the_quotient_of_a_set_opening():
    """q_k of the definition is the quotient kzg_set_ref.div_set gives for the coset's points, in any order"""
    import kzg_set_ref as ks
    rng = random.Random(5)
    for n, l in ((8, 4), (16, 1), (16, 16), (32, 2)):
        p = [rng.randrange(R) for _ in range(n)]
        for k in range(n // l):
            S = ka.coset(n, l, k)
            assert ks.vanishing(S) == [-pow(kr.root(n), k * l, R) % R] + [0] * (l - 1) + [1]
            q, values = ks.div_set(p, S)
            assert q[:n - l] == ka.divide_by_binomial(p, l, pow(kr.root(n), k * l, R))
            assert values == [ka.values(p)[k + (n // l) * j] for j in range(l)]


def test_one_coset_and_two_cosets():
    rng = random.Random(9)
    for n in (2, 4, 32):
        p = [rng.randrange(R) for _ in range(n)]
        assert ka.model(p, n, TAU) == ([0], ())                         # l = n: the one quotient is the zero polynomial
        proofs, W = ka.model(p, n // 2, TAU)                             # r = 2
        assert proofs == ka.proofs_by_definition(p, n // 2, TAU) and len(W) == 4 and W[3] == 0


# ---------------------------------------------------------------------------- the kernel's per-lane functions
@pytest.fixture(scope="module")
def pmac():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("points_mac.cuh", "points_mul.cuh", "points_scale.cuh", "glv.cuh",
                                                    "fq2.cuh", "fp29.cuh", "ec.cuh", "curve.cuh", "consts_gen.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


def _words(b):
    return (ctypes.c_uint32 * (len(b) // 4)).from_buffer_copy(b)


def _le(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def _g(a):
    """[a] g1 as an affine point of the oracle (O for a = 0)"""
    return cref.scale(1, o.G1.to_affine(o.G1.one), a % R)


@functools.lru_cache(maxsize=None)
def _logs():
    rng = random.Random(77)
    return tuple(rng.randrange(1, R) for _ in range(32))


@functools.lru_cache(maxsize=None)
def _wires():
    """the 32 points [a_v] g1 as wire-in records; every third written with Z != 1"""
    rng = random.Random(78)
    out = []
    for v, a in enumerate(_logs()):
        P = _g(a)
        out.append(cases.wire(1, cases.rescale(1, P, rng.randrange(2, Q)) if v % 3 == 1 else P, 0))
    return tuple(out)


INF_WIRE = cases.wire(1, o.G1.zero, 0)


def _run(pmac, wires, scalars, code=0):
    out = (ctypes.c_uint32 * 24)(*([0xFFFFFFFF] * 24))
    assert pmac.pmac_run(_words(b"".join(wires)), _words(_le(scalars)), len(scalars), out) == code
    return bytes(out)


def _want(logs, scalars):
    return cref.wire(1, _g(sum(a * k for a, k in zip(logs, scalars))))


@pytest.mark.parametrize("terms", TERMS)
def test_lane_matches_the_sum_of_the_products_of_logarithms(pmac, terms):
    rng = random.Random(terms)
    logs, wires = _logs()[:terms], _wires()[:terms]
    special = [0, 1, R - 1, cref.LAMBDA, R - cref.LAMBDA, (1 << 127) + 1, 1 << 128, R - 2]
    rows = [[rng.randrange(R) for _ in range(terms)],
            [special[(v + terms) % len(special)] for v in range(terms)],
            [0] * terms,
            [R - 1] * terms,
            [1] * terms]
    for ks in rows:
        assert _run(pmac, wires, ks) == _want(logs, ks), (terms, ks)
    assert _run(pmac, wires, [0] * terms) == cref.wire(1, o.G1.to_affine(o.G1.zero))


@pytest.mark.parametrize("terms", TERMS)
def test_a_scalar_from_r_on_refuses_the_lane(pmac, terms):
    rng = random.Random(50 + terms)
    inf = cref.wire(1, o.G1.to_affine(o.G1.zero))
    for bad in (R, R + 1, 1 << 254, (1 << 256) - 1):
        ks = [rng.randrange(R) for _ in range(terms)]
        ks[rng.randrange(terms)] = bad
        assert _run(pmac, _wires()[:terms], ks, code=1) == inf
        assert pmac.pmac_steps(_words(_le(ks)), terms) == -1


@pytest.mark.parametrize("terms", [2, 3, 9, 32])
def test_equal_points_with_equal_and_opposite_scalars(pmac, terms):
    """the same point in every term: equal scalars meet the doubling case of the mixed addition at the first non-zero
    column, k and r - k its P == -Q case; both must be exact, with other terms around them and alone"""
    rng = random.Random(60 + terms)
    a = _logs()[0]
    same = [_wires()[0]] * terms
    for k in (1, 2, cref.LAMBDA, rng.randrange(R)):
        assert _run(pmac, same, [k] * terms) == _want([a] * terms, [k] * terms)
    k = rng.randrange(1, R)
    pair = [k, R - k] + [0] * (terms - 2)
    assert _run(pmac, same, pair) == cref.wire(1, o.G1.to_affine(o.G1.zero))
    assert _run(pmac, same, [1, R - 1] + [0] * (terms - 2)) == cref.wire(1, o.G1.to_affine(o.G1.zero))
    if terms > 2:
        ks = [k, R - k] + [rng.randrange(R) for _ in range(terms - 2)]
        wires = [_wires()[0], _wires()[0]] + list(_wires()[2:terms])
        assert _run(pmac, wires, ks) == _want((a, a) + _logs()[2:terms], ks)
    # P and -P as two different terms with the same scalar
    neg = cases.wire(1, o.G1.to_affine(o.G1.negate(_g(a))), 0)
    assert _run(pmac, [_wires()[0], neg] + [INF_WIRE] * (terms - 2), [k] * terms) == cref.wire(1, o.G1.to_affine(o.G1.zero))


@pytest.mark.parametrize("terms", TERMS)
def test_infinity_among_the_terms_and_as_all_terms(pmac, terms):
    rng = random.Random(70 + terms)
    ks = [rng.randrange(R) for _ in range(terms)]
    assert _run(pmac, [INF_WIRE] * terms, ks) == cref.wire(1, o.G1.to_affine(o.G1.zero))
    hole = rng.randrange(terms)
    wires = [INF_WIRE if v == hole else w for v, w in enumerate(_wires()[:terms])]
    logs = [0 if v == hole else a for v, a in enumerate(_logs()[:terms])]
    assert _run(pmac, wires, ks) == _want(logs, ks)


def test_schedules_fit_the_streamed_words(pmac):
    """the GLV halves are below 2^127, so no schedule is longer than 128 columns: the 16 words the kernel streams"""
    rng = random.Random(3)
    for k in [0, 1, R - 1, R - 2, cref.LAMBDA, cref.LAMBDA + 1, R - cref.LAMBDA, (1 << 253), (1 << 127) - 1] + \
             [rng.randrange(R) for _ in range(2000)]:
        steps = pmac.pmac_steps(_words(_le([k])), 1)
        assert 0 <= steps <= 128, k
    assert pmac.pmac_steps(_words(_le([0])), 1) == 0


# ---------------------------------------------------------------------------- argument errors, no device
class _FakeSrs:
    def __init__(self, m):
        self.m = m

    @property
    def tau_g1(self):
        raise AssertionError("the string was touched before the arguments were checked")


@pytest.mark.parametrize("n,coset,match", [
    (0, 1, "power of two"), (1, 1, "power of two"), (3, 1, "power of two"), (48, 1, "power of two"),
    (2048, 1, "carries"), (64, 0, "coset"), (64, 3, "coset"), (64, 64, "coset"), (16, 32, "coset"), (2, 4, "coset"),
    (64, -1, "coset"),
])
def test_key_arguments_are_checked_before_the_string_is_read(n, coset, match):
    from octopuszk_amd import kzg
    with pytest.raises(ValueError, match=match):
        kzg.OpenAllKey.from_srs(_FakeSrs(512), n, coset)


def test_the_group_fft_limit_is_an_argument_error():
    from octopuszk_amd import kzg
    with pytest.raises(ValueError, match="2\\^22"):
        kzg.OpenAllKey.from_srs(_FakeSrs(1 << 22), 1 << 22, 1)
    with pytest.raises(ValueError, match="2\\^22"):
        kzg.OpenAllKey.from_srs(_FakeSrs(1 << 23), 1 << 23, 2)


def test_open_all_refuses_rows_that_are_not_the_keys():
    import torch
    from octopuszk_amd import kzg
    key = kzg.OpenAllKey(None, 16, 4, None)
    assert (key.n, key.coset, key.cosets) == (16, 4, 4)
    with pytest.raises(TypeError):
        key.open_all(torch.zeros(16 * 32, dtype=torch.uint8))               # not on the device
    with pytest.raises(TypeError):
        key.open_all([0] * 16)
    with pytest.raises(TypeError):
        key.open_all(torch.zeros(16 * 8, dtype=torch.int32))


def test_all_openings_refuses_a_coset_that_is_not_there():
    from octopuszk_amd import kzg
    a = kzg.AllOpenings(bytes(32), None, None, 16, 4)
    assert a.cosets == 4
    for k in (-1, 4):
        with pytest.raises(ValueError):
            a.opening(k)
    with pytest.raises(ValueError):
        kzg.AllOpenings(bytes(31), None, None, 16, 4)


def test_new_names_are_bound_and_declared():
    from octopuszk_amd import kzg, lib
    names = ("ozk_points_mac_prepared_bytes", "ozk_points_mac_prepare_dev", "ozk_points_mac_workspace_bytes",
             "ozk_points_mac_dev")
    header = open(os.path.join(HERE, "..", "include", "ozk.h")).read()
    for name in names:
        assert name in lib.exported_symbols() and name + "(" in header
    assert "whole-coset" not in kzg.__doc__.split("Out of scope")[1]
