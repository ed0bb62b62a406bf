"""GPU tests of the KZG layer: the three Fr entry points of csrc/kzg.cuh against the integer
model (tests/kzg_ref.py), byte for byte, and the protocol of octopuszk_amd/kzg.py over a string of known tau, where
every commitment and proof is [p(tau)] g1 (srs_gpu_util.expected)."""
import ctypes
import random

import pytest
import torch

import kzg_ref as kr
import srs_gpu_util as u
from fr_gpu_util import evals_open as _evals_open
from fr_gpu_util import poly_open as _poly_open
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

R = o.R
T = 1024                       # KZG_TILE: the coefficients one workgroup handles
E_INVALID = -1
TAU = 0x5eed0123456789abcdef0123456789abcdef0123456789abcdef % R
M = 512                        # 2 M + 1 = T + 1 powers in G1
SENTINEL = 0xA5


def _lib():
    from octopuszk_amd import lib
    return lib.load()


def _ptr(t):
    return ctypes.c_void_p(int(t.data_ptr()))


def _stream():
    return ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))


def _dev_ints(values):
    return u.dev(b"".join(kr.le(v) for v in values))


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")


LENGTHS = [1, 2, 3, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5]


@pytest.mark.parametrize("length", LENGTHS)
def test_poly_open_matches_the_model(length):
    rng = random.Random(length)
    root = rng.randrange(R)
    # row 0 has `root` as a root: (X - root) times a random polynomial (the zero polynomial at length 1)
    g = [rng.randrange(R) for _ in range(length - 1)]
    row0 = [(-root * g[0]) % R] + [(g[j - 1] - root * g[j]) % R for j in range(1, length - 1)] + [g[-1]] if g else [0]
    rows = [row0] + [[rng.randrange(R) for _ in range(length)] for _ in range(2)]
    rows[1][0] += R                                  # one coefficient written as p + r
    zr = rng.randrange(R)
    sentinel = int.from_bytes(bytes([SENTINEL]) * 32, "little")
    cases = [  # (npolys, poly_stride, quot_stride, points)
        (3, length + 3, length + 2, [root, R - 1, zr]),
        (3, 0, length, [1, root, zr + R]),           # one polynomial at three points, one of them written as z + r
        (3, length, length + 1, [0, 1, R - 1]),
        (1, length, length, [zr]),
    ]
    for npolys, stride, qs, points in cases:
        flat = []
        for y in range(npolys if stride else 1):
            flat += rows[y] + [7] * (max(stride, length) - length)
        got_q, got_y, gaps = _poly_open(flat, npolys, length, stride, points, qs)
        for y in range(npolys):
            q, val = kr.div_linear(rows[y if stride else 0], points[y] % R)
            assert got_y[y] == val, (length, npolys, stride, y)
            assert got_q[y] == q, (length, npolys, stride, y)
            assert got_q[y][length - 1] == 0
        assert all(v == sentinel for v in gaps)
        if root in points:
            assert got_y[points.index(root)] == 0


def test_poly_open_across_the_chunk_of_tile_carries():
    """more than 256 tiles: the scan of the tiles' carries takes a second chunk"""
    length = 256 * T + 5
    rng = random.Random(7)
    p = [rng.randrange(R) for _ in range(length)]
    z = rng.randrange(R)
    got_q, got_y, _ = _poly_open(p, 1, length, length, [z], length)
    q, y = kr.div_linear(p, z)
    assert got_y == [y] and got_q[0] == q


@pytest.mark.parametrize("n", [2, 4, 64, T, 2 * T, 4 * T])
def test_evals_open_matches_the_model(n):
    rng = random.Random(n)
    omega = kr.root(n)
    points = [rng.randrange(R)] + [pow(omega, k, R) for k in (0, 1, n // 2, n - 1)]
    points[2] += R                                   # omega written as omega + r
    rows = [[rng.randrange(R) for _ in range(n)] for _ in points]
    rows[0][1] += R
    stride = n + 1
    flat = []
    for row in rows:
        flat += row + [9]
    got_q, got_y, _, _ = _evals_open(flat, len(rows), n, stride, omega, points, n + 2)
    for y, row in enumerate(rows):
        q, val = kr.open_evals([v % R for v in row], points[y] % R, omega)
        assert got_y[y] == val, (n, y)
        assert got_q[y] == q, (n, y)
    # equal evaluations: the interpolant is a constant and the quotient is zero, outside the domain and inside
    const = [rng.randrange(R)] * n
    got_q, got_y, _, _ = _evals_open(const, 2, n, 0, omega, [points[0], omega], n)
    assert got_y == [const[0]] * 2 and got_q == [[0] * n] * 2
    # an omega of another order
    sentinel = bytes([SENTINEL]) * 32
    for bad in (1, kr.root(2 * n), omega * omega % R if n > 2 else 1):
        _, _, quot, vals = _evals_open(const, 1, n, n, bad, [points[0]], n, expect=E_INVALID)
        assert u.host(vals) == sentinel and u.host(quot) == sentinel * n


@pytest.mark.parametrize("k", [1, 2, 5])
def test_rows_combine(k):
    L = _lib()
    rng = random.Random(k)
    for length in (1, 300):
        stride = length + 1
        rows = [[rng.randrange(R) for _ in range(length)] for _ in range(k)]
        weights = ([0, R - 1, rng.randrange(R), 1, rng.randrange(R) + R])[:k] if k > 1 else [R - 1]
        flat = []
        for row in rows:
            flat += row + [3]
        want = kr.combine(rows, weights)
        d_rows, d_w = _dev_ints(flat), _dev_ints(weights)
        out = torch.full((length * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
        assert L.ozk_fr_rows_combine_dev(_ptr(d_rows), k, length, stride, _ptr(d_w), _ptr(out), _stream()) == 0
        assert kr.ints(u.host(out)) == want
        # in place: the output is the first row
        assert L.ozk_fr_rows_combine_dev(_ptr(d_rows), k, length, stride, _ptr(d_w), _ptr(d_rows), _stream()) == 0
        after = kr.ints(u.host(d_rows))
        assert after[:length] == want and after[length:] == flat[length:]
    zero_w = _dev_ints([0] * k)
    assert L.ozk_fr_rows_combine_dev(_ptr(d_rows), k, length, stride, _ptr(zero_w), _ptr(out), _stream()) == 0
    assert kr.ints(u.host(out)) == [0] * length


def test_rejected_shapes_launch_nothing():
    L = _lib()
    n = 8
    buf = torch.full((4 * n * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    vals = torch.full((64,), SENTINEL, dtype=torch.uint8, device="cuda")
    pts = _dev_ints([1, 2])
    ws = _ws(1 << 16)
    wsb = L.ozk_fr_poly_open_workspace_bytes(2, n)
    coeffs, quot = buf[:2 * n * 32], buf[2 * n * 32:]
    null = ctypes.c_void_p(0)

    def poly(c, npolys, length, stride, q, qs, w=ws, wbytes=1 << 16):
        return L.ozk_fr_poly_open_dev(c, npolys, length, stride, _ptr(pts), q, qs, _ptr(vals), _ptr(w), wbytes,
                                      _stream())

    assert poly(_ptr(coeffs), 2, n, n, _ptr(quot), n) == 0            # (the shape itself is fine)
    torch.cuda.synchronize()
    buf.fill_(SENTINEL)
    vals.fill_(SENTINEL)
    overlapping = buf[(2 * n - 1) * 32:]                              # its first element is the coefficients' last
    assert poly(_ptr(coeffs), 2, n, n, _ptr(overlapping), n) == E_INVALID
    assert b"overlap" in L.ozk_last_error()
    assert poly(_ptr(coeffs), 2, n, n, _ptr(coeffs), n) == E_INVALID
    assert poly(_ptr(coeffs), 2, n, n, _ptr(quot), n, wbytes=wsb - 1) == E_INVALID
    assert poly(_ptr(coeffs), 2, 0, n, _ptr(quot), n) == E_INVALID
    assert poly(_ptr(coeffs), 0, n, n, _ptr(quot), n) == E_INVALID
    assert poly(_ptr(coeffs), 2, n, n - 1, _ptr(quot), n) == E_INVALID
    assert poly(_ptr(coeffs), 2, n, n, _ptr(quot), n - 1) == E_INVALID
    # beyond the cap: refused on the shape alone, before any pointer is looked at
    assert poly(null, 2, (1 << 27) + 1, (1 << 27) + 1, null, (1 << 27) + 1, wbytes=0) == E_INVALID
    assert L.ozk_fr_poly_open_workspace_bytes(2, (1 << 27) + 1) == 0
    assert L.ozk_fr_poly_open_workspace_bytes(1, 0) == 0 and L.ozk_fr_poly_open_workspace_bytes(0, 4) == 0
    om = ctypes.create_string_buffer(kr.le(kr.root(n)), 32)

    def evals(f, npolys, size, q, wbytes=1 << 16):
        return L.ozk_fr_evals_open_dev(f, npolys, size, size, ctypes.cast(om, ctypes.c_void_p), _ptr(pts), q, size,
                                       _ptr(vals), _ptr(ws), wbytes, _stream())

    assert evals(_ptr(coeffs), 2, n, _ptr(overlapping)) == E_INVALID
    assert evals(_ptr(coeffs), 2, n, _ptr(quot), wbytes=L.ozk_fr_evals_open_workspace_bytes(2, n) - 1) == E_INVALID
    assert evals(_ptr(coeffs), 2, 6, _ptr(quot)) == E_INVALID
    assert evals(_ptr(coeffs), 2, 1, _ptr(quot)) == E_INVALID
    assert evals(null, 2, 1 << 28, null, wbytes=0) == E_INVALID
    for bad in ((2, 6), (2, 1), (2, 1 << 28), (0, 8)):
        assert L.ozk_fr_evals_open_workspace_bytes(*bad) == 0
    combine = L.ozk_fr_rows_combine_dev
    assert combine(_ptr(coeffs), 2, n, n, _ptr(pts), _ptr(buf[32:]), _stream()) == E_INVALID      # overlap, not row 0
    assert combine(_ptr(coeffs), 2, 0, n, _ptr(pts), _ptr(quot), _stream()) == E_INVALID
    assert combine(_ptr(coeffs), 0, n, n, _ptr(pts), _ptr(quot), _stream()) == E_INVALID
    assert combine(null, 2, (1 << 27) + 1, (1 << 27) + 1, null, null, _stream()) == E_INVALID
    torch.cuda.synchronize()
    assert u.host(buf) == bytes([SENTINEL]) * buf.numel() and u.host(vals) == bytes([SENTINEL]) * 64


# ---------------------------------------------------------------------------- the protocol
@pytest.fixture(scope="module")
def string():
    from octopuszk_amd import kzg, srs
    s = srs.Srs.from_secrets(M, TAU, 1, 1, generator=1)
    return s, kzg.VerifyKey.from_srs(s)


def _at_tau(p):
    return kr.horner(p, TAU)


def _dev_rows(rows):
    return _dev_ints([v for row in rows for v in row]).view(len(rows), -1)


@pytest.mark.parametrize("n", [1, 2, 65, T + 1])
def test_protocol(string, n):
    from octopuszk_amd import kzg
    s, vk = string
    rng = random.Random(100 + n)
    ck = kzg.CommitKey.from_srs(s, n)
    rows = [[rng.randrange(R) for _ in range(n)], [5] + [0] * (n - 1), [0] * n]     # random, constant, zero
    zs = [rng.randrange(R) for _ in rows]
    d_rows = _dev_rows(rows)
    want_c = [u.expected(1, [_at_tau(p)]) for p in rows]
    assert ck.commit(d_rows) == want_c
    ops = ck.open(d_rows, zs)
    for p, z, op in zip(rows, zs, ops):
        q, y = kr.div_linear(p, z)
        assert (op.c, op.z, op.y, op.pi) == (u.expected(1, [_at_tau(p)]), z, y, u.expected(1, [_at_tau(q)]))
        assert kzg.verify(vk, op)
    assert ops[1].pi == ops[2].pi == ops[2].c == kzg._G1_INF and ops[2].y == 0
    # each of the four fields changed (a polynomial of one coefficient is a constant: pi = O, and it opens to the
    # same value at every z, so there the changed z must still verify)
    op = ops[0]
    other = u.expected(1, [12345])
    assert (op.pi == kzg._G1_INF) == (n == 1)
    assert kzg.verify(vk, kzg.Opening(op.c, (op.z + 1) % R, op.y, op.pi)) == (n == 1)
    for bad in (kzg.Opening(other, op.z, op.y, op.pi), kzg.Opening(op.c, op.z, (op.y + 1) % R, op.pi),
                kzg.Opening(op.c, op.z, op.y, other), kzg.Opening(kzg._G1_INF, op.z, op.y, op.pi)):
        assert not kzg.verify(vk, bad)
    if n > 1:
        assert not kzg.verify(vk, kzg.Opening(op.c, op.z, op.y, kzg._G1_INF))
    # bytes: the key and the opening read back verify the same opening
    vk2 = kzg.VerifyKey.from_bytes(vk.to_bytes())
    assert vk2.to_bytes() == vk.to_bytes() and len(vk.to_bytes()) == 160
    assert kzg.verify(vk2, kzg.Opening.from_bytes(op.to_bytes())) and len(op.to_bytes()) == 128
    # one polynomial at several points
    many = ck.open_many_points(d_rows[0], zs)
    assert [m.to_bytes() for m in many] == [o_.to_bytes() for o_ in ck.open(_dev_rows([rows[0]] * 3), zs)]
    # the evaluation form, on the largest domain the key covers
    ne = 1 << (n.bit_length() - 1)
    if ne < 2:
        return
    omega = kr.root(ne)
    f = [[rng.randrange(R) for _ in range(ne)], [9] * ne]
    ze = [rng.randrange(R), pow(omega, ne - 1, R)]
    d_f = _dev_rows(f)
    interp = [kr.intt(row, omega) + [0] * (n - ne) for row in f]
    assert ck.commit_evals(d_f) == ck.commit(_dev_rows(interp))
    assert ck.commit_evals(d_f[0]) == [u.expected(1, [_at_tau(interp[0])])]
    got, want = ck.open_evals(d_f, ze), ck.open(_dev_rows(interp), ze)
    assert [g.to_bytes() for g in got] == [w.to_bytes() for w in want]
    assert all(kzg.verify(vk, g) for g in got)


def test_verify_all_and_each(string):
    from octopuszk_amd import kzg
    s, vk = string
    n, k = 65, 5
    rng = random.Random(5)
    ck = kzg.CommitKey.from_srs(s, n)
    rows = [[rng.randrange(R) for _ in range(n)] for _ in range(k)]
    rows[3] = [4] + [0] * (n - 1)                     # a constant among them: pi = O
    ops = ck.open(_dev_rows(rows), [rng.randrange(R) for _ in range(k)])
    seed = bytes(range(32))
    assert kzg.verify_all(vk, ops, seed) and kzg.verify_all(vk, ops) and kzg.verify_all(vk, [])
    assert kzg.verify_each(vk, ops, seed) == [True] * k
    bad = list(ops)
    bad[2] = kzg.Opening(ops[2].c, ops[2].z, (ops[2].y + 1) % R, ops[2].pi)
    assert not kzg.verify_all(vk, bad, seed)
    assert kzg.verify_each(vk, bad, seed) == [True, True, False, True, True]
    assert kzg.verify_all(vk, [b.to_bytes() for b in ops], seed)


@pytest.mark.parametrize("k", [1, 3])
def test_open_combined(string, k):
    from octopuszk_amd import kzg
    s, vk = string
    n = 65
    rng = random.Random(30 + k)
    ck = kzg.CommitKey.from_srs(s, n)
    rows = [[rng.randrange(R) for _ in range(n)] for _ in range(k)]
    z = rng.randrange(R)
    cs, ys, pi = ck.open_combined(_dev_rows(rows), z)
    assert cs == [u.expected(1, [_at_tau(p)]) for p in rows] and ys == [kr.horner(p, z) for p in rows]
    gamma = kr.gamma(z, cs, ys)
    q, _ = kr.div_linear(kr.combine(rows, [pow(gamma, i, R) for i in range(k)]), z)
    assert pi == u.expected(1, [_at_tau(q)])
    assert kzg.verify_combined(vk, cs, z, ys, pi)
    assert not kzg.verify_combined(vk, cs, z, [(ys[0] + 1) % R] + ys[1:], pi)
    assert not kzg.verify_combined(vk, cs, (z + 1) % R, ys, pi)
    if k > 1:
        assert not kzg.verify_combined(vk, [cs[1], cs[0]] + cs[2:], z, ys, pi)
