"""Sums of products of points and scalars on hardware (ozk_points_mac_dev): inputs [a_v[i]] g of
known a, expected [sum_v a_v[i] k_v[i]] g, compared as compressed encodings (srs_gpu_util.expected), and byte for byte
with the chain of ozk_points_mul_dev and ozk_points_add_dev calls it replaces.

The kernel streams its schedules from the workspace and has no term-group size and no size threshold: one path.  The
sizes cover one lane, a wave that is not full, exactly full, one lane into a second workgroup and three workgroups; the
term counts 1, 2, 3 and 32 at every size and 7, 16, 17 and 31 at one."""
import ctypes
import functools
import random

import pytest
import torch

import ceremony_ref as cref
import codec_cases as cases
import srs_gpu_util as u
from oracle import bn254 as o

pytestmark = pytest.mark.gpu
R = o.R
INVALID = -1
N_MAX, T_MAX = 130, 32
CASES = [(t, n) for n in (1, 63, 64, 65, 130) for t in (1, 2, 3, 32)] + [(t, 65) for t in (7, 16, 17, 31)]
INF = cref.wire(1, o.G1.to_affine(o.G1.zero))
SENTINEL = 0xA5


def _le(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def _ptr(t):
    return ctypes.c_void_p(int(t.data_ptr()))


@functools.lru_cache(maxsize=None)
def _logs():
    """a[v][i] for 32 terms x 130 lanes.  Lane 3: terms 0 and 1 hold the same point; lane 4: the same again (its scalars
    are opposite); lane 5: every term is O; lane 7: term 1 is O; lane 9 (and 70): term 0 and the last term are O"""
    rng = random.Random(4000)
    a = [[rng.randrange(1, R) for _ in range(N_MAX)] for _ in range(T_MAX)]
    a[1][3], a[1][4] = a[0][3], a[0][4]
    for v in range(T_MAX):
        a[v][5] = 0
    a[1][7] = 0
    for i in (9, 70):
        a[0][i] = a[T_MAX - 1][i] = 0
    return tuple(tuple(row) for row in a)


@functools.lru_cache(maxsize=None)
def _scalars():
    """k[v][i]: the special values in the first lanes of every term (shifted per term), random ones behind.  Lane 3:
    equal scalars on the equal points; lane 4: k and r - k on them"""
    rng = random.Random(4001)
    special = [0, 1, R - 1, cref.LAMBDA, cref.LAMBDA + 1, R - cref.LAMBDA, (1 << 127) + 1, 1 << 128, R - 2, 2, 3]
    k = [[special[(i + v) % len(special)] if i < 11 and i not in (3, 4) else rng.randrange(R) for i in range(N_MAX)]
         for v in range(T_MAX)]
    k[1][3] = k[0][3]
    k[1][4] = R - k[0][4]
    return tuple(tuple(row) for row in k)


@functools.lru_cache(maxsize=None)
def _pool():
    """the 32 x 130 points as host bytes, term-major"""
    flat = [a for row in _logs() for a in row]
    return u.host(u.points(1, flat))


def _points(terms, n, rescaled=False):
    raw = _pool()
    rng = random.Random(n)
    out = []
    for v in range(terms):
        for i in range(n):
            rec = raw[96 * (v * N_MAX + i):96 * (v * N_MAX + i + 1)]
            if rescaled and (i + v) % 3 == 1 and _logs()[v][i]:
                rec = u.rescale_g1(rec, rng.randrange(2, u.Q))
            out.append(rec)
    return u.dev(b"".join(out))


def _k(terms, n):
    return [[_scalars()[v][i] for i in range(n)] for v in range(terms)]


def _flat(rows):
    return u.dev(_le([k for row in rows for k in row]))


@functools.lru_cache(maxsize=None)
def _expected(terms, n):
    return u.expected(1, [sum(_logs()[v][i] * _scalars()[v][i] for v in range(terms)) % R for i in range(n)])


def _mac(points, ks, terms, n, codes=False):
    from octopuszk_amd import kzg
    table = kzg.points_mac_prepare(points, terms, n)
    return kzg.points_mac(table, _flat(ks), terms, n, codes=codes)


@pytest.mark.parametrize("terms,n", CASES)
def test_matches_the_sums_of_the_products_of_the_logarithms(terms, n):
    out, codes = _mac(_points(terms, n), _k(terms, n), terms, n, codes=True)
    assert u.compress(out, 1) == _expected(terms, n)
    assert not codes.any().item()
    raw = u.host(out)
    zero = u.expected(1, [0])
    for i in range(n):                                                   # Z = 1, and O as the codec writes it
        rec = raw[96 * i:96 * (i + 1)]
        if _expected(terms, n)[32 * i:32 * (i + 1)] == zero:
            assert rec == INF
        else:
            assert rec[64:] == (1).to_bytes(32, "little")
    if n > 5:
        assert raw[96 * 5:96 * 6] == INF                                 # every term O
    if n > 4 and terms == 2:
        assert raw[96 * 4:96 * 5] == INF                                 # [k] P + [r - k] P


@pytest.mark.parametrize("terms,n", [(3, 65), (32, 64)])
def test_inputs_with_z_not_one(terms, n):
    pts = _points(terms, n, rescaled=True)
    assert u.host(pts) != u.host(_points(terms, n))
    assert u.compress(_mac(pts, _k(terms, n), terms, n), 1) == _expected(terms, n)


@pytest.mark.parametrize("terms,n", [(1, 65), (3, 130), (32, 65)])
def test_a_scalar_from_r_on_refuses_its_lane_alone(terms, n):
    bad = {0: R, n - 1: (1 << 256) - 1, 31: R + 1, 63: 1 << 254, 64: R}
    ks = _k(terms, n)
    for j, (i, k) in enumerate(bad.items()):
        ks[j % terms][i] = k                                             # in different terms
    out, codes = _mac(_points(terms, n), ks, terms, n, codes=True)
    assert codes.cpu().tolist() == [1 if i in bad else 0 for i in range(n)]
    raw, got, want = u.host(out), u.compress(out, 1), _expected(terms, n)
    for i in range(n):
        if i in bad:
            assert raw[96 * i:96 * (i + 1)] == INF
        else:
            assert got[32 * i:32 * (i + 1)] == want[32 * i:32 * (i + 1)], i
    assert u.host(_mac(_points(terms, n), ks, terms, n)) == raw          # d_codes = NULL is accepted


@pytest.mark.parametrize("n", [1, 65, 130])
def test_one_term_gives_the_bytes_of_points_mul(n):
    from octopuszk_amd import srs
    want = srs.mul_points(_points(1, n), _flat(_k(1, n)), 1)
    assert u.host(_mac(_points(1, n), _k(1, n), 1, n)) == u.host(want)


@pytest.mark.parametrize("terms,n", [(2, 65), (3, 130), (17, 65), (32, 63)])
def test_any_terms_give_the_bytes_of_the_mul_and_add_chain(terms, n):
    from octopuszk_amd import srs
    pts, ks = _points(terms, n), _k(terms, n)
    acc = None
    for v in range(terms):
        prod = srs.mul_points(pts[96 * n * v:96 * n * (v + 1)], u.dev(_le(ks[v])), 1)
        acc = prod if acc is None else srs.points_add(acc, prod, 1)
    assert u.host(_mac(pts, ks, terms, n)) == u.host(acc)


def test_bad_arguments_are_refused_and_nothing_is_written():
    from octopuszk_amd import lib
    L = lib.load()
    terms, n = 3, 64
    pts, sc = _points(terms, n), _flat(_k(terms, n))
    pb, wb = L.ozk_points_mac_prepared_bytes(terms, n, 1), L.ozk_points_mac_workspace_bytes(terms, n, 1)
    assert (pb, wb) == (192 * terms * n, 68 * terms * n)
    for bad in ((0, n, 1), (33, n, 1), (terms, 0, 1), (terms, (1 << 24) + 1, 1), (terms, n, 2), (terms, n, 0), (terms, n, 3)):
        assert L.ozk_points_mac_prepared_bytes(*bad) == 0 and L.ozk_points_mac_workspace_bytes(*bad) == 0
    table = torch.full((pb + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    ws = torch.full((wb + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = torch.full((96 * n + 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    codes = torch.full((n + 4,), 7, dtype=torch.int32, device="cuda")

    def prepare(p, terms_, n_, type_, t, tbytes):
        rc = L.ozk_points_mac_prepare_dev(p, terms_, n_, type_, t, tbytes, None)
        torch.cuda.synchronize()
        return rc

    def mac(t, s, terms_, n_, type_, o_, c, w, wbytes):
        rc = L.ozk_points_mac_dev(t, s, terms_, n_, type_, o_, c, w, wbytes, None)
        torch.cuda.synchronize()
        return rc

    # ---- prepare
    for terms_, n_ in ((0, n), (33, n), (-1, n), (terms, 0), (terms, -1), (terms, (1 << 24) + 1)):
        assert prepare(_ptr(pts), terms_, n_, 1, _ptr(table), pb) == INVALID
    for type_ in (0, 2, 3):
        assert prepare(_ptr(pts), terms, n, type_, _ptr(table), pb) == INVALID
    assert b"G1 only" in L.ozk_last_error()
    assert prepare(None, terms, n, 1, _ptr(table), pb) == INVALID
    assert prepare(_ptr(pts), terms, n, 1, None, pb) == INVALID
    assert prepare(_ptr(pts), terms, n, 1, _ptr(table), pb - 1) == INVALID
    assert prepare(ctypes.c_void_p(pts.data_ptr() + 1), terms, n - 1, 1, _ptr(table), pb) == INVALID
    assert prepare(_ptr(pts), terms, n, 1, ctypes.c_void_p(table.data_ptr() + 1), pb) == INVALID
    assert b"aligned" in L.ozk_last_error()
    assert u.host(table) == bytes([SENTINEL]) * table.numel()
    assert prepare(_ptr(pts), terms, n, 1, _ptr(table), pb) == 0
    assert u.host(table[pb:]) == bytes([SENTINEL]) * 16                  # and the good call stays inside its bytes
    # ---- mac
    good = [_ptr(table), _ptr(sc), terms, n, 1, _ptr(out), _ptr(codes), _ptr(ws), wb]
    for terms_, n_ in ((0, n), (33, n), (terms, 0), (terms, (1 << 24) + 1)):
        assert mac(*(good[:2] + [terms_, n_] + good[4:])) == INVALID
    for type_ in (0, 2, 3):
        assert mac(*(good[:4] + [type_] + good[5:])) == INVALID
    for which in (0, 1, 5, 7):                                           # a null pointer (d_codes may be NULL)
        args = list(good)
        args[which] = None
        assert mac(*args) == INVALID
    for which in (0, 1, 5, 6, 7):                                        # each buffer one byte off
        args = list(good)
        args[which] = ctypes.c_void_p(args[which].value + 1)
        assert mac(*args) == INVALID
        assert b"aligned" in L.ozk_last_error()
    assert mac(*(good[:8] + [wb - 1])) == INVALID
    assert b"workspace" in L.ozk_last_error()
    assert u.host(out) == bytes([SENTINEL]) * out.numel() and codes.cpu().tolist() == [7] * (n + 4)
    assert u.host(ws) == bytes([SENTINEL]) * ws.numel()
    assert mac(*good) == 0
    assert u.compress(out[:96 * n], 1) == _expected(terms, n) and not codes[:n].any().item()
    assert u.host(out[96 * n:]) == bytes([SENTINEL]) * 16 and codes[n:].cpu().tolist() == [7] * 4
    assert u.host(ws[wb:]) == bytes([SENTINEL]) * 16
