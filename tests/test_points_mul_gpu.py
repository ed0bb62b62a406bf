"""n points times n scalars on hardware (ozk_points_mul_dev): inputs [a_i] g of known a_i,
expected [a_i k_i] g, compared as compressed encodings.  The kernel has one path per group and no size threshold; the
sizes cover one lane, a wave that is not full, exactly full, one lane into a second workgroup, and several workgroups."""
import functools
import random

import numpy as np
import pytest
import torch

import ceremony_ref as cref
import codec_cases as cases
import phase1_ref as p1
import srs_gpu_util as u
from oracle import bn254 as o

pytestmark = pytest.mark.gpu
R = o.R
INVALID = -1
SIZES = {1: (1, 2, 63, 64, 65, 200), 2: (1, 3, 65)}
CASES = [(t, n) for t in (1, 2) for n in SIZES[t]]


def _inf(type_):
    """O as the point kernels write it: (0, 1, 0) / ((0, 0), (1, 0), (0, 0)), what ozk_points_scale_dev writes"""
    C = cases.curve(type_)
    return cref.wire(type_, C.to_affine(C.zero))


def _le(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


@functools.lru_cache(maxsize=None)
def _logs(type_, n):
    """the logarithms of the inputs: O at every seventh place from the third on, a repeated point next to its twin"""
    rng = random.Random(2000 * type_ + n)
    a = [rng.randrange(1, R) for _ in range(n)]
    for i in range(2, n, 7):
        a[i] = 0
    if n > 5:
        a[5] = a[4]
    return tuple(a)


@functools.lru_cache(maxsize=None)
def _scalars(type_, n):
    """the special list first (neighbouring lanes of the first wave hold different entries of it), random ones behind;
    from 64 lanes on the list runs again, shifted, against other points"""
    rng = random.Random(3000 * type_ + n)
    special = p1.scalars()[:13]
    k = [special[i % 13] if i < 13 or 64 <= i < 77 else rng.randrange(R) for i in range(n)]
    if n == 1:
        k = [R - 1]
    return tuple(k)


@functools.lru_cache(maxsize=None)
def _input(type_, n):
    return u.points(type_, _logs(type_, n))


@functools.lru_cache(maxsize=None)
def _expected(type_, n):
    return u.expected(type_, [a * k % R for a, k in zip(_logs(type_, n), _scalars(type_, n))])


def _mul(points, scalars, type_, codes=False):
    from octopuszk_amd import srs
    return srs.mul_points(points, u.dev(_le(scalars)), type_, codes)


@pytest.mark.parametrize("type_,n", CASES)
def test_matches_the_products_of_the_logarithms(type_, n):
    out, codes = _mul(_input(type_, n), _scalars(type_, n), type_, codes=True)
    assert u.compress(out, type_) == _expected(type_, n)
    assert not codes.any().item()
    raw, w = u.host(out), 96 * type_
    inf = _inf(type_)
    for i in range(n):                                                   # Z = 1, and O as the codec writes it
        rec = raw[w * i:w * (i + 1)]
        if _logs(type_, n)[i] * _scalars(type_, n)[i] % R:
            assert rec[64 * type_:64 * type_ + 32] == (1).to_bytes(32, "little") and not any(rec[64 * type_ + 32:])
        else:
            assert rec == inf
    # in place
    buf = _input(type_, n).clone()
    from octopuszk_amd import lib
    from octopuszk_amd.device import _ptr
    sc = u.dev(_le(_scalars(type_, n)))
    assert lib.load().ozk_points_mul_dev(_ptr(buf), _ptr(sc), n, type_, _ptr(buf), None, None) == 0
    assert u.host(buf) == raw


def test_inputs_with_z_not_one():
    n = 65
    rng = random.Random(n)
    raw = u.host(_input(1, n))
    raw = b"".join(u.rescale_g1(raw[96 * i:96 * i + 96], rng.randrange(2, u.Q)) if i % 3 == 1 and _logs(1, n)[i]
                   else raw[96 * i:96 * i + 96] for i in range(n))
    assert raw != u.host(_input(1, n))
    assert u.compress(_mul(u.dev(raw), _scalars(1, n), 1), 1) == _expected(1, n)


def test_g2_is_exact_outside_the_subgroup():
    P = cref.twist_point_outside_the_subgroup()
    ks = [R - 1, p1.LAMBDA, 0x123456789ABCDEF0123456789ABCDEF0123456789 % R]
    out = _mul(u.dev(cases.wire(2, P, 0) * 3), ks, 2)
    want = [cref.scale(2, P, k) for k in ks]
    assert u.host(out) == b"".join(cref.wire(2, W) for W in want)
    assert want[0] != o.G2.to_affine(o.G2.negate(P))                     # [r - 1] P is not -P: P is outside


@pytest.mark.parametrize("type_,n", [(1, 65), (1, 200), (2, 3)])
def test_a_scalar_from_r_on_gives_infinity_for_its_point_alone(type_, n):
    bad = {0: R, n - 1: (1 << 256) - 1}
    if n > 64:
        bad.update({31: R + 1, 63: 1 << 254, 64: R})
    ks = [bad.get(i, k) for i, k in enumerate(_scalars(type_, n))]
    out, codes = _mul(_input(type_, n), ks, type_, codes=True)
    assert codes.cpu().tolist() == [1 if i in bad else 0 for i in range(n)]
    raw, w, e = u.host(out), 96 * type_, 32 * type_
    got, want = u.compress(out, type_), _expected(type_, n)
    zero = u.expected(type_, [0])
    for i in range(n):
        if i in bad:
            assert raw[w * i:w * (i + 1)] == _inf(type_) and got[e * i:e * (i + 1)] == zero
        else:
            assert got[e * i:e * (i + 1)] == want[e * i:e * (i + 1)], i
    assert u.host(_mul(_input(type_, n), ks, type_)) == raw              # d_codes = NULL is accepted


@pytest.mark.parametrize("type_,n", [(1, 65), (2, 3)])
def test_equal_scalars_give_the_bytes_of_scale_points(type_, n):
    from octopuszk_amd import ceremony
    for k in (p1.LAMBDA + 1, R - 1, _scalars(type_, 65)[20]):
        assert u.host(_mul(_input(type_, n), [k] * n, type_)) == u.host(ceremony.scale_points(_input(type_, n), k, type_))


def test_equals_the_diagonal_sparse_product():
    from octopuszk_amd import srs
    from octopuszk_amd import zksnark as z
    n = 200
    ks = _scalars(1, n)
    mat = z._CsrDevice(np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int64), np.array(ks, dtype=object))
    assert u.host(srs.sparse_mat_points(mat, _input(1, n), 1)) == u.host(_mul(_input(1, n), ks, 1))


def test_bad_arguments_are_refused_and_nothing_is_written():
    from octopuszk_amd import lib
    from octopuszk_amd.device import _ptr
    L = lib.load()
    n = 64
    pts, sc = _input(1, n), u.dev(_le(_scalars(1, n)))
    out = torch.zeros_like(pts)
    codes = torch.zeros(n, dtype=torch.int32, device="cuda")

    def raw(p, s, n_, type_, o_, c=None):
        rc = L.ozk_points_mul_dev(p, s, n_, type_, o_, c, None)
        torch.cuda.synchronize()
        return rc

    assert raw(_ptr(pts), _ptr(sc), n, 1, _ptr(out), _ptr(codes)) == 0 and out.any().item()
    out.zero_()
    codes.fill_(7)
    for n_ in (0, -1, (1 << 24) + 1):
        assert raw(_ptr(pts), _ptr(sc), n_, 1, _ptr(out), _ptr(codes)) == INVALID
    assert raw(None, _ptr(sc), n, 1, _ptr(out), _ptr(codes)) == INVALID
    assert raw(_ptr(pts), None, n, 1, _ptr(out), _ptr(codes)) == INVALID
    assert raw(_ptr(pts), _ptr(sc), n, 1, None, _ptr(codes)) == INVALID
    for type_ in (0, 3):
        assert raw(_ptr(pts), _ptr(sc), n, type_, _ptr(out), _ptr(codes)) == INVALID
    for which in range(4):                                               # each buffer one byte off
        args = [_ptr(pts), _ptr(sc), _ptr(out), _ptr(codes)]
        args[which] += 1
        assert raw(args[0], args[1], n - 1, 1, args[2], args[3]) == INVALID
    assert not out.any().item() and codes.cpu().tolist() == [7] * n
    assert b"aligned" in L.ozk_last_error()
