"""The sparse matrix times a vector of points and the pointwise sum on hardware (ozk_sparse_mat_points_dev,
ozk_points_add_dev): a hand-made CSR over 200 points of known logarithm, the expected rows
computed in the exponent, compared as compressed encodings."""
import functools
import random

import numpy as np
import pytest

import ceremony_ref as cref
import codec_cases as cases
import srs_gpu_util as u
from oracle import bn254 as o

pytestmark = pytest.mark.gpu
R = o.R
NP = 200


@functools.lru_cache(maxsize=None)
def _logs():
    """the logarithms of the 200 points: O at 7 and 150, a point and its negative at (20, 21), a repeat at (30, 31)"""
    rng = random.Random(61)
    s = [rng.randrange(1, R) for _ in range(NP)]
    s[7] = s[150] = 0
    s[21] = R - s[20]
    s[31] = s[30]
    return tuple(s)


@functools.lru_cache(maxsize=None)
def _rows():
    rng = random.Random(62)
    big = rng.randrange(1 << 253, R)
    rows = [[], [(3, 0)], [(3, 1)], [(3, R - 1)], [(3, 2)], [(3, big)], [(7, big)], [(7, 1)],
            [(5, 1), (5, 1)], [(5, 1), (5, R - 1)], [(5, big), (5, R - big)], [(20, 1), (21, 1)], [(20, 2), (21, 2)],
            [(30, 1), (31, R - 1)], [(7, 1), (9, 1), (150, R - 1)], []]
    for count in (64, 65, 64 * 64 + 1, 130):
        rows.append([(rng.randrange(NP), rng.choice((1, 1, 1, R - 1, 2, big))) for _ in range(count)])
    for _ in range(140):                                     # more than 128 rows, short
        rows.append([(rng.randrange(NP), rng.choice((1, R - 1, 0, rng.randrange(R)))) for _ in range(rng.randrange(4))])
    rows.append([(NP - 1, 1)])
    return rows


def _matrix(with_coeff):
    from octopuszk_amd import zksnark as z
    rows = _rows()
    ptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int64)
    idx = np.array([i for r in rows for i, _ in r], dtype=np.int64)
    val = np.array([c for r in rows for _, c in r], dtype=object) if with_coeff else None
    mat = z._CsrDevice(ptr, idx, val)
    assert mat.n_long == 3 and mat.rows > 128
    return mat


@pytest.mark.parametrize("type_", [1, 2])
@pytest.mark.parametrize("with_coeff", [False, True])
def test_sparse_product_matches_the_exponents(type_, with_coeff):
    from octopuszk_amd import srs
    s = _logs()
    out = srs.sparse_mat_points(_matrix(with_coeff), u.points(type_, s), type_)
    want = [sum((c if with_coeff else 1) * s[i] for i, c in row) % R for row in _rows()]
    assert want[0] == 0 and want[9 if with_coeff else 11] == 0                  # rows that must come out as O
    got, exp = u.compress(out, type_), u.expected(type_, want)
    n = 32 * type_
    bad = [r for r in range(len(want)) if got[n * r:n * r + n] != exp[n * r:n * r + n]]
    assert not bad, bad
    raw = u.host(out)
    C = cases.curve(type_)
    assert raw[:96 * type_] == cref.wire(type_, C.to_affine(C.zero))              # the empty row: O as the codec writes it
    assert raw[96 * type_ * 2 + 64 * type_:96 * type_ * 2 + 64 * type_ + 32] == (1).to_bytes(32, "little")   # Z = 1


def test_sparse_product_refuses_bad_arguments():
    import torch
    from octopuszk_amd import lib
    from octopuszk_amd.device import _ptr
    L = lib.load()
    mat = _matrix(False)
    pts = u.points(1, _logs())
    out = torch.zeros(mat.rows * 96, dtype=torch.uint8, device="cuda")
    ws = torch.empty(256, dtype=torch.uint8, device="cuda")
    args = (_ptr(mat.ptr), _ptr(mat.idx), None, _ptr(pts))
    assert L.ozk_sparse_mat_points_dev(*args, mat.rows, 1, _ptr(mat.long), mat.n_long, _ptr(out), _ptr(ws), 256, None) == -1
    assert L.ozk_sparse_mat_points_dev(*args, mat.rows, 3, _ptr(mat.long), mat.n_long, _ptr(out), _ptr(ws), 1 << 40, None) == -1
    assert L.ozk_sparse_mat_points_dev(*args, 0, 1, None, 0, _ptr(out), None, 0, None) == -1
    assert L.ozk_sparse_mat_points_dev(*args, mat.rows, 1, None, mat.n_long, _ptr(out), _ptr(ws), 1 << 40, None) == -1
    assert L.ozk_sparse_mat_points_workspace_bytes(0, 1) == 0
    assert L.ozk_sparse_mat_points_workspace_bytes(3, 2) >= 3 * 4096 * 192
    torch.cuda.synchronize()
    assert not out.any().item()


@pytest.mark.parametrize("type_", [1, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_points_add(type_, n):
    from octopuszk_amd import srs
    rng = random.Random(10 * n + type_)
    a = [rng.randrange(1, R) for _ in range(n)]
    b = [rng.randrange(1, R) for _ in range(n)]
    b[0] = a[0]                                               # P + P, P - P
    if n > 4:
        a[1], b[2], a[3], b[3], b[4] = 0, 0, 0, 0, R - a[4]   # O + P, P + O, O + O, P + (-P)
    pa, pb = u.points(type_, a), u.points(type_, b)
    for negate in (False, True):
        out = srs.points_add(pa, pb, type_, negate)
        want = [(x - y if negate else x + y) % R for x, y in zip(a, b)]
        assert u.compress(out, type_) == u.expected(type_, want), negate
    if type_ == 1:
        zz = random.Random(3).randrange(2, u.Q)
        raw = u.host(pb)
        pz = u.dev(b"".join(u.rescale_g1(raw[96 * i:96 * i + 96], zz) if b[i] else raw[96 * i:96 * i + 96] for i in range(n)))
        assert u.compress(srs.points_add(pz, pa, 1), 1) == u.expected(1, [(x + y) % R for x, y in zip(a, b)])
