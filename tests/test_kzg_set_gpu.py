"""GPU tests of KZG set openings: the two Fr entry points of csrc/kzg_set.cuh against the integer
model (tests/kzg_set_ref.py), byte for byte, and the protocol of octopuszk_amd/kzg.py over a string of known tau, where
every commitment and proof is [p(tau)] g1 (srs_gpu_util.expected)."""
import ctypes
import random

import pytest
import torch

import kzg_ref as kr
import kzg_set_ref as ks
import srs_gpu_util as u
from fr_gpu_util import evals_open_set as _evals_open_set
from fr_gpu_util import poly_open_set as _poly_open_set
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

R = o.R
T = 1024                       # KZG_TILE: the coefficients one workgroup handles
E_INVALID = -1
TAU = 0x5eed0123456789abcdef0123456789abcdef0123456789abcdef % R
M = 512                        # 2 M + 1 = T + 1 powers in G1, M powers in G2
SENTINEL = 0xA5
SENTINEL_INT = int.from_bytes(bytes([SENTINEL]) * 32, "little")


def _lib():
    from octopuszk_amd import lib
    return lib.load()


def _ptr(t):
    return ctypes.c_void_p(int(t.data_ptr()))


def _stream():
    return ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))


def _dev_ints(values):
    return u.dev(b"".join(kr.le(v) for v in values))


def _host_ints(values):
    buf = ctypes.create_string_buffer(b"".join(kr.le(v) for v in values), 32 * len(values))
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")


def _points(rng, t, special=()):
    """t distinct points, the special ones first"""
    out = list(special)[:t]
    while len(out) < t:
        z = rng.randrange(R)
        if z not in out:
            out.append(z)
    return out


def _poly_open(coeffs, length, z):
    """ozk_fr_poly_open_dev on one row: the bytes of the quotient row and of the value"""
    L = _lib()
    d_c, d_p = _dev_ints(coeffs), _dev_ints([z])
    quot = torch.full((length * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    vals = torch.full((32,), SENTINEL, dtype=torch.uint8, device="cuda")
    wsb = L.ozk_fr_poly_open_workspace_bytes(1, length)
    ws = _ws(wsb)
    assert L.ozk_fr_poly_open_dev(_ptr(d_c), 1, length, length, _ptr(d_p), _ptr(quot), length, _ptr(vals), _ptr(ws), wsb,
                                  _stream()) == 0
    return u.host(quot), u.host(vals)


@pytest.mark.parametrize("t", [1, 2, 3, 8, 32])
def test_poly_open_set_matches_the_model(t):
    rng = random.Random(t)
    for length in sorted({1, 2, t, t + 1, T - 1, T, T + 1, T + t, 2 * T + 1, 3 * T + 5}):
        rows = [[rng.randrange(R) for _ in range(length)] for _ in range(3)]
        rows[1][0] += R                                  # one coefficient written as p + r
        sets = [_points(rng, t, (0, 1, R - 1)), _points(rng, t), _points(rng, t)]
        rng.shuffle(sets[0])
        written = [list(s) for s in sets]
        written[2][0] += R                               # one point written as z + r
        cases = [  # (npolys, poly_stride, quot_stride)
            (3, length + 3, length + 2),
            (3, 0, length),                              # one polynomial at three sets
            (1, length, length),
        ]
        for npolys, stride, qs in cases:
            flat = []
            for y in range(npolys if stride else 1):
                flat += rows[y] + [7] * (max(stride, length) - length)
            pts = [z for y in range(npolys) for z in written[y]]
            got_q, got_y, gaps, quot, vals = _poly_open_set(flat, npolys, length, stride, t, pts, qs)
            for y in range(npolys):
                q, values = ks.div_set([c % R for c in rows[y if stride else 0]], sets[y])
                assert got_y[t * y:t * (y + 1)] == values, (length, npolys, stride, y)
                assert got_q[y] == q, (length, npolys, stride, y)
                assert got_q[y][max(length - t, 0):] == [0] * min(t, length)
            assert all(v == SENTINEL_INT for v in gaps)
        if t == 1:
            # the bytes of the single-point entry on the same inputs
            want_q, want_y = _poly_open(rows[0], length, sets[0][0])
            assert (u.host(quot), u.host(vals)) == (want_q, want_y)


def test_poly_open_set_across_the_chunk_of_tile_carries():
    """more than 256 tiles: the scan of the tiles' tails takes a second chunk"""
    length = 257 * T + 3
    rng = random.Random(7)
    p = [rng.randrange(R) for _ in range(length)]
    pts = _points(rng, 2)
    got_q, got_y, _, _, _ = _poly_open_set(p, 1, length, length, 2, pts, length)
    q, values = ks.div_set(p, pts)
    assert got_y == values and got_q[0] == q


@pytest.mark.parametrize("n", [2, 4, 64, T, 2 * T, 4 * T])
def test_evals_open_set_matches_the_model(n):
    rng = random.Random(n)
    omega = kr.root(n)
    rows = [[rng.randrange(R) for _ in range(n)] for _ in range(2)]
    coeffs = [kr.intt(row, omega) for row in rows]
    rows[0][1] += R
    flat = []
    for row in rows:
        flat += row + [9]
    for t in (1, 2, 3, 8):
        sets = [_points(rng, t, (0,)), _points(rng, t)]          # (1 and r - 1 lie in every domain)
        assert all(pow(z, n, R) != 1 for s in sets for z in s)
        written = [list(s) for s in sets]
        written[1][t - 1] += R
        pts = [z for s in written for z in s]
        got_q, got_y, quot, vals = _evals_open_set(flat, 2, n, n + 1, omega, t, pts, n + 2)
        for y in range(2):
            q, values = ks.div_set(coeffs[y], sets[y])
            assert got_y[t * y:t * (y + 1)] == values, (n, t, y)
            assert got_q[y] == kr.ntt(q, omega), (n, t, y)
        if t == 1:
            # the bytes of the single-point entry on the same inputs
            L = _lib()
            d_f, d_p = _dev_ints(flat), _dev_ints(pts)
            quot1 = torch.full_like(quot, SENTINEL)
            vals1 = torch.full_like(vals, SENTINEL)
            wsb = L.ozk_fr_evals_open_workspace_bytes(2, n)
            ws = _ws(wsb)
            om = ctypes.create_string_buffer(kr.le(omega), 32)
            assert L.ozk_fr_evals_open_dev(_ptr(d_f), 2, n, n + 1, ctypes.cast(om, ctypes.c_void_p), _ptr(d_p), _ptr(quot1),
                                           n + 2, _ptr(vals1), _ptr(ws), wsb, _stream()) == 0
            assert (u.host(quot), u.host(vals)) == (u.host(quot1), u.host(vals1))


def test_rejected_shapes_launch_nothing():
    L = _lib()
    n = 8
    buf = torch.full((4 * n * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    vals = torch.full((2 * 33 * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    ws = _ws(1 << 20)
    coeffs, quot = buf[:2 * n * 32], buf[2 * n * 32:]
    null = ctypes.c_void_p(0)
    omega = kr.root(n)
    good = [3, 5, 7, 11]                                              # two rows of two points, none in the domain
    keep_g, p_good = _host_ints(good)
    keep_b, p_many = _host_ints(list(range(2, 2 + 2 * 33)))

    def poly(c, npolys, length, stride, t, pts, q, qs, wbytes=1 << 20):
        return L.ozk_fr_poly_open_set_dev(c, npolys, length, stride, t, pts, q, qs, _ptr(vals), _ptr(ws), wbytes, _stream())

    assert poly(_ptr(coeffs), 2, n, n, 2, p_good, _ptr(quot), n) == 0  # (the shape itself is fine)
    torch.cuda.synchronize()
    buf.fill_(SENTINEL)
    vals.fill_(SENTINEL)
    wsb = L.ozk_fr_poly_open_set_workspace_bytes(2, n, 2)
    overlapping = buf[(2 * n - 1) * 32:]                              # its first element is the coefficients' last
    assert poly(_ptr(coeffs), 2, n, n, 0, p_good, _ptr(quot), n) == E_INVALID
    assert poly(_ptr(coeffs), 2, n, n, 33, p_many, _ptr(quot), n) == E_INVALID
    for repeated in ([3, 3, 7, 11], [3, 5, 7, 7 + R]):                # the second row's: equal mod r
        keep_r, p_rep = _host_ints(repeated)
        assert poly(_ptr(coeffs), 2, n, n, 2, p_rep, _ptr(quot), n) == E_INVALID
        assert b"distinct" in L.ozk_last_error()
    assert poly(_ptr(coeffs), 2, n, n, 2, p_good, _ptr(overlapping), n) == E_INVALID
    assert b"overlap" in L.ozk_last_error()
    assert poly(_ptr(coeffs), 2, n, n, 2, p_good, _ptr(coeffs), n) == E_INVALID
    assert poly(_ptr(coeffs), 2, n, n, 2, p_good, _ptr(quot), n, wbytes=wsb - 1) == E_INVALID
    assert poly(_ptr(coeffs), 2, 0, n, 2, p_good, _ptr(quot), n) == E_INVALID
    assert poly(_ptr(coeffs), 0, n, n, 2, p_good, _ptr(quot), n) == E_INVALID
    assert poly(_ptr(coeffs), 2, n, n - 1, 2, p_good, _ptr(quot), n) == E_INVALID
    assert poly(_ptr(coeffs), 2, n, n, 2, p_good, _ptr(quot), n - 1) == E_INVALID
    # beyond the cap, and a bad t: refused on the shape alone, before any pointer is looked at
    assert poly(null, 2, (1 << 27) + 1, (1 << 27) + 1, 2, null, null, (1 << 27) + 1, wbytes=0) == E_INVALID
    assert poly(null, 2, n, n, 33, null, null, n, wbytes=0) == E_INVALID
    for bad in ((2, (1 << 27) + 1, 2), (1, 0, 1), (0, 4, 1), (2, n, 0), (2, n, 33)):
        assert L.ozk_fr_poly_open_set_workspace_bytes(*bad) == 0
    om = ctypes.create_string_buffer(kr.le(omega), 32)

    def evals(f, npolys, size, t, pts, q, wbytes=1 << 20):
        return L.ozk_fr_evals_open_set_dev(f, npolys, size, size, ctypes.cast(om, ctypes.c_void_p), t, pts, q, size,
                                           _ptr(vals), _ptr(ws), wbytes, _stream())

    assert evals(_ptr(coeffs), 2, n, 2, p_good, _ptr(quot)) == 0
    torch.cuda.synchronize()
    buf.fill_(SENTINEL)
    vals.fill_(SENTINEL)
    assert evals(_ptr(coeffs), 2, n, 0, p_good, _ptr(quot)) == E_INVALID
    assert evals(_ptr(coeffs), 2, n, 9, p_many, _ptr(quot)) == E_INVALID
    keep_r, p_rep = _host_ints([3, 5, 7, 7])
    assert evals(_ptr(coeffs), 2, n, 2, p_rep, _ptr(quot)) == E_INVALID
    for inside in (1, omega, pow(omega, n - 1, R) + R):
        keep_i, p_in = _host_ints([3, 5, inside, 11])
        assert evals(_ptr(coeffs), 2, n, 2, p_in, _ptr(quot)) == E_INVALID
        assert b"domain" in L.ozk_last_error()
    good_om = om
    for bad_om in (1, kr.root(2 * n), omega * omega % R):            # an omega of another order
        om = ctypes.create_string_buffer(kr.le(bad_om), 32)
        assert evals(_ptr(coeffs), 2, n, 2, p_good, _ptr(quot)) == E_INVALID
        assert b"order" in L.ozk_last_error()
    om = good_om
    assert evals(_ptr(coeffs), 2, n, 2, p_good, _ptr(overlapping)) == E_INVALID
    assert evals(_ptr(coeffs), 2, n, 2, p_good, _ptr(quot),
                 wbytes=L.ozk_fr_evals_open_set_workspace_bytes(2, n, 2) - 1) == E_INVALID
    assert evals(_ptr(coeffs), 2, 6, 2, p_good, _ptr(quot)) == E_INVALID
    assert evals(_ptr(coeffs), 2, 1, 2, p_good, _ptr(quot)) == E_INVALID
    assert evals(null, 2, 1 << 28, 2, null, null, wbytes=0) == E_INVALID
    for bad in ((2, 6, 2), (2, 1, 2), (2, 1 << 28, 2), (0, 8, 2), (2, 8, 0), (2, 8, 9)):
        assert L.ozk_fr_evals_open_set_workspace_bytes(*bad) == 0
    torch.cuda.synchronize()
    assert u.host(buf) == bytes([SENTINEL]) * buf.numel() and u.host(vals) == bytes([SENTINEL]) * vals.numel()


# ---------------------------------------------------------------------------- the protocol
@pytest.fixture(scope="module")
def string():
    from octopuszk_amd import kzg, srs
    s = srs.Srs.from_secrets(M, TAU, 1, 1, generator=1)
    return s, kzg.SetVerifyKey.from_srs(s, 4)


def _at_tau(p):
    return kr.horner(p, TAU)


def _dev_rows(rows):
    return _dev_ints([v for row in rows for v in row]).view(len(rows), -1)


@pytest.mark.parametrize("n", [1, 2, 65, T + 1])
def test_protocol(string, n):
    from octopuszk_amd import kzg
    s, vk = string
    rng = random.Random(200 + n)
    ck = kzg.CommitKey.from_srs(s, n)
    rows = [[rng.randrange(R) for _ in range(n)], [5] + [0] * (n - 1)]              # random, constant
    d_rows = _dev_rows(rows)
    other = u.expected(1, [12345])
    for t in (1, 2, 4):
        sets = [_points(rng, t), _points(rng, t, (0, 1, R - 1))]
        ops = ck.open_set(d_rows, sets)
        for p, pts, op in zip(rows, sets, ops):
            q, values = ks.div_set(p, pts)
            assert (op.c, op.points, op.values, op.pi) == (u.expected(1, [_at_tau(p)]), tuple(pts), tuple(values),
                                                           u.expected(1, [_at_tau(q)]))
            assert kzg.verify_set(vk, op)
        assert ops[1].pi == kzg._G1_INF and (ops[0].pi == kzg._G1_INF) == (n <= t)
        shared = ck.open_set(d_rows, sets[0])                    # one list for all rows
        assert shared[0].to_bytes() == ops[0].to_bytes() and shared[1].points == tuple(sets[0])
        # each field changed (a constant opens to the same values at every set, so there a changed z still verifies)
        op = ops[0]
        moved = ((op.points[0] + 1) % R,) + op.points[1:]
        assert kzg.verify_set(vk, kzg.SetOpening(op.c, moved, op.values, op.pi)) == (n == 1)
        bumped = op.values[:-1] + ((op.values[-1] + 1) % R,)
        for bad in (kzg.SetOpening(other, op.points, op.values, op.pi), kzg.SetOpening(op.c, op.points, bumped, op.pi),
                    kzg.SetOpening(op.c, op.points, op.values, other)):
            assert not kzg.verify_set(vk, bad)
        if n > t:
            assert not kzg.verify_set(vk, kzg.SetOpening(op.c, op.points, op.values, kzg._G1_INF))
        assert kzg.verify_set(vk, kzg.SetOpening.from_bytes(op.to_bytes())) and len(op.to_bytes()) == 68 + 64 * t
    # the key's bytes read back verify the same opening; a key too small for the opening is an argument error
    vk2 = kzg.SetVerifyKey.from_bytes(vk.to_bytes())
    assert vk2.to_bytes() == vk.to_bytes() and len(vk.to_bytes()) == 4 + 32 * 4 + 64 * 5
    assert kzg.verify_set(vk2, op)
    small = kzg.SetVerifyKey.from_srs(s, 2)
    with pytest.raises(ValueError, match="t_max = 2"):
        kzg.verify_set(small, op)
    # a set through tau itself: the opening is honest, but [Z_S(tau)] g2 = O and nothing could be checked against it
    through_tau = ck.open_set(d_rows[0], [TAU, 5])[0]
    assert through_tau.values[0] == _at_tau(rows[0]) and not kzg.verify_set(vk, through_tau)
    # the evaluation form, on the largest domain the key covers
    ne = 1 << (n.bit_length() - 1)
    if ne < 2:
        return
    omega = kr.root(ne)
    f = [[rng.randrange(R) for _ in range(ne)], [9] * ne]
    d_f = _dev_rows(f)
    interp = [kr.intt(row, omega) + [0] * (n - ne) for row in f]
    for t in (1, 2, 4):
        pts = _points(rng, t)
        got, want = ck.open_set_evals(d_f, pts), ck.open_set(_dev_rows(interp), pts)
        assert [g.to_bytes() for g in got] == [w.to_bytes() for w in want]
        assert all(kzg.verify_set(vk, g) for g in got)


def test_verify_set_all_and_each(string):
    from octopuszk_amd import kzg
    s, vk = string
    n, k = 65, 5
    rng = random.Random(6)
    ck = kzg.CommitKey.from_srs(s, n)
    rows = [[rng.randrange(R) for _ in range(n)] for _ in range(k)]
    rows[3] = [4] + [0] * (n - 1)                     # a constant among them: pi = O
    d_rows = _dev_rows(rows)
    set_a, set_b = _points(rng, 2), _points(rng, 3)
    ops = ck.open_set(d_rows[:3], set_a) + ck.open_set(d_rows[3:], set_b)
    seed = bytes(range(32))
    assert kzg.verify_set_all(vk, ops, seed) and kzg.verify_set_all(vk, ops) and kzg.verify_set_all(vk, [])
    assert kzg.verify_set_each(vk, ops, seed) == [True] * k
    bad = list(ops)
    bad[4] = kzg.SetOpening(ops[4].c, ops[4].points, ((ops[4].values[0] + 1) % R,) + ops[4].values[1:], ops[4].pi)
    assert not kzg.verify_set_all(vk, bad, seed)
    assert kzg.verify_set_each(vk, bad, seed) == [True, True, True, True, False]
    assert kzg.verify_set_all(vk, [b.to_bytes() for b in ops], seed)


@pytest.mark.parametrize("k", [1, 3])
def test_open_set_combined(string, k):
    from octopuszk_amd import kzg
    s, vk = string
    n = 65
    rng = random.Random(40 + k)
    ck = kzg.CommitKey.from_srs(s, n)
    rows = [[rng.randrange(R) for _ in range(n)] for _ in range(k)]
    pts = _points(rng, 3)
    cs, ys, pi = ck.open_set_combined(_dev_rows(rows), pts)
    assert cs == [u.expected(1, [_at_tau(p)]) for p in rows] and ys == [[kr.horner(p, z) for z in pts] for p in rows]
    gamma = ks.gamma(pts, cs, ys)
    q, _ = ks.div_set(kr.combine(rows, [pow(gamma, i, R) for i in range(k)]), pts)
    assert pi == u.expected(1, [_at_tau(q)])
    assert kzg.verify_set_combined(vk, cs, pts, ys, pi)
    assert not kzg.verify_set_combined(vk, cs, pts, [[(ys[0][0] + 1) % R] + ys[0][1:]] + ys[1:], pi)
    assert not kzg.verify_set_combined(vk, cs, [(pts[0] + 1) % R] + pts[1:], ys, pi)
    if k > 1:
        assert not kzg.verify_set_combined(vk, [cs[1], cs[0]] + cs[2:], pts, ys, pi)
