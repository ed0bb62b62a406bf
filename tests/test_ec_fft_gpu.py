"""The transform over curve points on hardware (ozk_ec_fft_dev): inputs [s_i] g of known s_i,
expected [DFT(s)_j] g, compared as compressed encodings.  The implementation has ONE butterfly kernel and no size
threshold of its own beyond the B >= 64 boundary of the issue (a wave shares its twiddle in a pass of at least 64
blocks): 128 has one such pass, 256 two, 64 none."""
import ctypes
import functools
import random

import pytest
import torch

import srs_gpu_util as u
import srs_setup_ref as sref
from oracle import bn254 as o

pytestmark = pytest.mark.gpu
R = o.R
INVALID = -1
SIZES = {1: (1, 2, 4, 64, 128, 256), 2: (2, 4, 128)}
CASES = [(t, n) for t in (1, 2) for n in SIZES[t]]


@functools.lru_cache(maxsize=None)
def _scalars(type_, n):
    rng = random.Random(1000 * type_ + n)
    return tuple(rng.randrange(1, R) for _ in range(n))


@functools.lru_cache(maxsize=None)
def _input(type_, n):
    return u.points(type_, _scalars(type_, n))


def _omega(n):
    return o.fr_root_of_unity(n) if n > 1 else 1


def _fft(points, type_, n, inverse=False, omega=None):
    from octopuszk_amd import srs
    return srs.ec_fft(points, type_, _omega(n) if omega is None else omega, inverse)


@pytest.mark.parametrize("type_,n", CASES)
def test_forward_matches_the_transform_of_the_logarithms(type_, n):
    out = _fft(_input(type_, n), type_, n)
    assert u.compress(out, type_) == u.expected(type_, sref.dft(list(_scalars(type_, n)), _omega(n)))
    assert u.host(out)[64 * type_:64 * type_ + 32] == (1).to_bytes(32, "little")        # affine-normalised


@pytest.mark.parametrize("type_,n", CASES)
def test_inverse_matches_and_undoes_the_forward(type_, n):
    back = _fft(_input(type_, n), type_, n, inverse=True)
    assert u.compress(back, type_) == u.expected(type_, sref.inverse_dft(list(_scalars(type_, n)), _omega(n)))
    again = _fft(_fft(_input(type_, n), type_, n), type_, n, inverse=True)
    assert u.compress(again, type_) == u.compress(_input(type_, n), type_)


@pytest.mark.parametrize("n", [2, 64, 256])
@pytest.mark.parametrize("inverse", [False, True])
def test_exceptional_inputs(n, inverse):
    rng = random.Random(n)
    s = rng.randrange(1, R)
    zz = [rng.randrange(2, u.Q) if i % 3 == 1 else 1 for i in range(n)]
    lone = [0] * n
    lone[n // 2] = s
    cases = {
        "all equal: a == w b and a == -w b in every pass": [s] * n,
        "all O": [0] * n,
        "O scattered": [0 if i % 5 in (0, 3) else v for i, v in enumerate(_scalars(1, n))],
        "one point among O": lone,
        "pairs P, -P": [v if i % 2 == 0 else R - _scalars(1, n)[i - 1] for i, v in enumerate(_scalars(1, n))],
    }
    tr = sref.inverse_dft if inverse else sref.dft
    for name, scalars in cases.items():
        out = _fft(u.points(1, scalars), 1, n, inverse)
        assert u.compress(out, 1) == u.expected(1, tr(list(scalars), _omega(n))), name
    # Z != 1 on a third of the inputs
    raw = u.host(_input(1, n))
    raw = b"".join(u.rescale_g1(raw[96 * i:96 * i + 96], zz[i]) for i in range(n))
    out = _fft(u.dev(raw), 1, n, inverse)
    assert u.compress(out, 1) == u.expected(1, tr(list(_scalars(1, n)), _omega(n)))
    if not inverse:
        want = u.expected(1, sref.dft([s] * n, _omega(n)))
        assert want[32:] == u.expected(1, [0]) * (n - 1) and not want[31] & 0x40    # a single non-zero point


def test_exceptional_inputs_g2():
    n, rng = 2, random.Random(9)
    s = rng.randrange(1, R)
    for scalars in ([s, s], [0, 0], [0, s], [s, R - s]):
        for inverse, tr in ((False, sref.dft), (True, sref.inverse_dft)):
            out = _fft(u.points(2, scalars), 2, n, inverse)
            assert u.compress(out, 2) == u.expected(2, tr(list(scalars), _omega(n)))


def _raw(points, n, type_, omega, out, inverse=0):
    from octopuszk_amd import lib
    from octopuszk_amd.device import _ptr
    L = lib.load()
    wsb = int(L.ozk_ec_fft_workspace_bytes(n, type_))
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device="cuda")
    ob = (ctypes.c_uint8 * 32).from_buffer_copy(int(omega).to_bytes(32, "little"))
    rc = L.ozk_ec_fft_dev(_ptr(points), n, type_, ctypes.cast(ob, ctypes.c_void_p), inverse, _ptr(out), _ptr(ws),
                          wsb, None)
    torch.cuda.synchronize()
    return rc


def test_bad_arguments_are_refused_and_nothing_runs():
    from octopuszk_amd import lib
    n = 64
    pts = _input(1, n)
    out = torch.zeros_like(pts)
    assert _raw(pts, n, 1, _omega(n), out) == 0 and out.any().item()
    out.zero_()
    for omega in (o.fr_root_of_unity(2 * n), o.fr_root_of_unity(n // 2), 1, 0, R, R + _omega(n)):
        assert _raw(pts, n, 1, omega, out) == INVALID, omega
    assert _raw(pts, 1, 1, 5, out) == INVALID                       # n = 1 takes omega = 1 only
    assert _raw(pts, n, 1, _omega(n), pts) == INVALID                # in place is not allowed
    assert _raw(pts, 48, 1, _omega(n), out) == INVALID
    assert _raw(pts, n, 3, _omega(n), out) == INVALID
    assert not out.any().item()
    L = lib.load()
    assert L.ozk_ec_fft_workspace_bytes(48, 1) == 0 and L.ozk_ec_fft_workspace_bytes(1 << 23, 1) == 0
    assert L.ozk_ec_fft_workspace_bytes(1 << 20, 1) >= 132 * 3 * (1 << 18)
