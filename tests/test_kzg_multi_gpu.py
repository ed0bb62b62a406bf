"""GPU tests of the KZG multi-opening: the two Fr entry points of csrc/kzg_multi.cuh against the
integer model (tests/kzg_multi_ref.py), byte for byte, and the protocol of octopuszk_amd/kzg.py over a string of known
tau, where every commitment and proof point is [p(tau)] g1."""
import ctypes
import random

import pytest
import torch

import kzg_multi_ref as km
import kzg_ref as kr
import srs_gpu_util as u
from fr_gpu_util import poly_eval_set as _eval_set
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

R = o.R
T = 1024                       # KZG_TILE: the coefficients one workgroup handles
E_INVALID = -1
TAU = 0x5eed0123456789abcdef0123456789abcdef0123456789abcdef % R
M = 512                        # 2 M + 1 = T + 1 powers in G1
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


def _ids(group_of):
    arr = (ctypes.c_int32 * len(group_of))(*group_of)
    return arr, ctypes.cast(arr, ctypes.c_void_p)


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


# ---------------------------------------------------------------------------- the grouped combine
def _combine_groups(flat, k, length, stride, weights, group_of, groups, out_stride):
    """the entry point on host ints -> (the output rows, the elements of the gaps between them, the output's bytes)"""
    L = _lib()
    d_r, d_w = _dev_ints(flat), _dev_ints(weights)
    keep, ids = _ids(group_of)
    out = torch.full((groups * out_stride * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    rc = L.ozk_fr_rows_combine_groups_dev(_ptr(d_r), k, length, stride, _ptr(d_w), ids, groups, _ptr(out), out_stride,
                                          _stream())
    assert rc == 0, L.ozk_last_error()
    got = kr.ints(u.host(out))
    rows = [got[g * out_stride:g * out_stride + length] for g in range(groups)]
    gaps = [v for g in range(groups) for v in got[g * out_stride + length:(g + 1) * out_stride]]
    return rows, gaps, u.host(out)


def _grouping(k, groups):
    """interleaved: rows 0, groups, 2 groups, .. in group 0; with three groups or more the last one is left empty"""
    ids = [i % groups for i in range(k)]
    return [0 if groups >= 3 and g == groups - 1 else g for g in ids]


@pytest.mark.parametrize("k,groups", [(1, 1), (3, 2), (17, 3), (17, 17), (256, 32)])
def test_rows_combine_groups_matches_the_model(k, groups):
    rng = random.Random(1000 * k + groups)
    for length in ((257,) if k == 256 else (1, 255, 256, 257, 1000)):
        rows = [[rng.randrange(R) for _ in range(length)] for _ in range(k)]
        weights = [rng.randrange(R) for _ in range(k)]
        written_r, written_w = [list(row) for row in rows], list(weights)
        written_r[k // 2][length // 2] += R                    # one element and one weight written as x + r
        written_w[k - 1] += R
        group_of = _grouping(k, groups)
        stride, out_stride = length + 3, length + 2
        flat = []
        for row in written_r:
            flat += row + [7] * (stride - length)
        got, gaps, _ = _combine_groups(flat, k, length, stride, written_w, group_of, groups, out_stride)
        assert got == km.combine_groups(rows, weights, group_of, groups), (length, k, groups)
        if groups >= 3:
            assert got[groups - 1] == [0] * length               # the empty group
        assert all(v == SENTINEL_INT for v in gaps)


@pytest.mark.parametrize("length", [1, 257, 1000])
def test_rows_combine_groups_of_one_group_is_rows_combine(length):
    L = _lib()
    rng = random.Random(length)
    k = 5
    flat = [rng.randrange(1 << 256) for _ in range(k * length)]            # any 256-bit words
    weights = [rng.randrange(1 << 256) for _ in range(k)]
    _, _, got = _combine_groups(flat, k, length, length, weights, [0] * k, 1, length)
    d_r, d_w = _dev_ints(flat), _dev_ints(weights)
    want = torch.full((length * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    assert L.ozk_fr_rows_combine_dev(_ptr(d_r), k, length, length, _ptr(d_w), _ptr(want), _stream()) == 0
    assert got == u.host(want)


# ---------------------------------------------------------------------------- the values at a set
def _open_set_values(flat, npolys, length, stride, t, points):
    """the value bytes ozk_fr_poly_open_set_dev writes on the same inputs"""
    L = _lib()
    d_c = _dev_ints(flat)
    keep, p_host = _host_ints(points)
    quot = torch.empty((npolys * length * 32,), dtype=torch.uint8, device="cuda")
    vals = torch.full((npolys * t * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    wsb = L.ozk_fr_poly_open_set_workspace_bytes(npolys, length, t)
    ws = _ws(wsb)
    assert L.ozk_fr_poly_open_set_dev(_ptr(d_c), npolys, length, stride, t, p_host, _ptr(quot), length, _ptr(vals), _ptr(ws),
                                      wsb, _stream()) == 0
    return u.host(vals)


@pytest.mark.parametrize("t", [1, 2, 3, 8, 32])
def test_poly_eval_set_matches_the_model(t):
    rng = random.Random(50 + t)
    for length in sorted({1, 2, t, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5}):
        rows = [[rng.randrange(R) for _ in range(length)] for _ in range(3)]
        written_rows = [list(row) for row in rows]
        written_rows[1][0] += R                          # one coefficient written as p + r
        sets = [_points(rng, t, (0, 1, R - 1)), _points(rng, t), _points(rng, t)]
        rng.shuffle(sets[0])
        distinct = [list(s) for s in sets]
        if t > 1:
            sets[2][t - 1] = sets[2][0]                  # a row with a repeated point
        written = [list(s) for s in sets]
        written[1][0] += R                               # one point written as z + r
        for npolys, stride in ((3, length + 3), (3, 0), (1, length)):     # stride 0: one polynomial at three sets
            flat = []
            for y in range(npolys if stride else 1):
                flat += written_rows[y] + [7] * (max(stride, length) - length)
            pts = [z for y in range(npolys) for z in written[y]]
            got, _ = _eval_set(flat, npolys, length, stride, t, pts)
            used = [rows[y if stride else 0] for y in range(npolys)]
            assert got == [v for row in km.values_at(used, sets[:npolys]) for v in row], (length, npolys, stride)
            if t > 1 and npolys == 3:
                assert got[2 * t + t - 1] == got[2 * t]
            # pairwise distinct points: the bytes of the set opening's values
            pts = [z for y in range(npolys) for z in distinct[y]]
            assert _eval_set(flat, npolys, length, stride, t, pts)[1] == _open_set_values(flat, npolys, length, stride, t, pts)


def test_poly_eval_set_across_the_chunk_of_tile_carries():
    """more than 256 tiles: the scan of the tiles' tails takes a second chunk"""
    length = 257 * T + 3
    rng = random.Random(7)
    p = [rng.randrange(R) for _ in range(length)]
    pts = _points(rng, 2)
    got, _ = _eval_set(p, 1, length, length, 2, pts)
    assert got == km.values_at([p], [pts])[0]


# ---------------------------------------------------------------------------- rejections
def test_rejected_shapes_launch_nothing():
    L = _lib()
    n = 8
    buf = torch.full((8 * n * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    vals = torch.full((2 * 33 * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    ws = _ws(1 << 20)
    rows, out = buf[:4 * n * 32], buf[4 * n * 32:]
    weights = _dev_ints([1, 2, 3, 4])
    null = ctypes.c_void_p(0)
    keep_i, ids = _ids([0, 1, 0, 1])
    stream = _stream()

    def combine(r, k, length, stride, w, g, groups, o_, ostride):
        return L.ozk_fr_rows_combine_groups_dev(r, k, length, stride, w, g, groups, o_, ostride, stream)

    assert combine(_ptr(rows), 4, n, n, _ptr(weights), ids, 2, _ptr(out), n) == 0       # (the shape itself is fine)
    torch.cuda.synchronize()
    buf.fill_(SENTINEL)
    big_w = _dev_ints([1] * 257)
    keep_b, big_ids = _ids([0] * 257)
    assert combine(_ptr(rows), 0, n, n, _ptr(weights), ids, 2, _ptr(out), n) == E_INVALID
    assert combine(_ptr(rows), 257, 1, 1, _ptr(big_w), big_ids, 1, _ptr(out), 1) == E_INVALID
    assert combine(_ptr(rows), 4, 0, n, _ptr(weights), ids, 2, _ptr(out), n) == E_INVALID
    assert combine(_ptr(rows), 4, n, n, _ptr(weights), ids, 0, _ptr(out), n) == E_INVALID
    assert combine(_ptr(rows), 4, 1, 1, _ptr(weights), ids, 33, _ptr(out), 1) == E_INVALID
    for bad_ids in ([0, 1, 2, 1], [0, -1, 0, 1], [0, 1, 0, 1 << 8]):
        keep_x, x = _ids(bad_ids)
        assert combine(_ptr(rows), 4, n, n, _ptr(weights), x, 2, _ptr(out), n) == E_INVALID
        assert b"group" in L.ozk_last_error()
    assert combine(_ptr(rows), 4, n, n - 1, _ptr(weights), ids, 2, _ptr(out), n) == E_INVALID
    assert combine(_ptr(rows), 4, n, n, _ptr(weights), ids, 2, _ptr(out), n - 1) == E_INVALID
    overlapping = buf[(4 * n - 1) * 32:]                                  # its first element is the rows' last
    assert combine(_ptr(rows), 4, n, n, _ptr(weights), ids, 2, _ptr(overlapping), n) == E_INVALID
    assert b"overlap" in L.ozk_last_error()
    assert combine(_ptr(rows), 4, n, n, _ptr(weights), ids, 2, _ptr(rows), n) == E_INVALID      # not even the first row
    for off in (buf[8:], ):                                               # 8 bytes off a 16-byte boundary
        assert combine(_ptr(off), 4, n, n, _ptr(weights), ids, 2, _ptr(out), n) == E_INVALID
        assert combine(_ptr(rows), 4, n, n, _ptr(off), ids, 2, _ptr(out), n) == E_INVALID
        assert combine(_ptr(rows), 4, n, n, _ptr(weights), ids, 2, _ptr(out[8:]), n) == E_INVALID
        assert b"aligned" in L.ozk_last_error()
    for args in ((null, _ptr(weights), ids, _ptr(out)), (_ptr(rows), null, ids, _ptr(out)),
                 (_ptr(rows), _ptr(weights), null, _ptr(out)), (_ptr(rows), _ptr(weights), ids, null)):
        assert combine(args[0], 4, n, n, args[1], args[2], 2, args[3], n) == E_INVALID
    # beyond the cap, bad k and groups: refused on the shape alone, before any pointer is looked at
    assert combine(null, 256, (1 << 20) + 1, (1 << 20) + 1, null, null, 1, null, (1 << 20) + 1) == E_INVALID
    assert combine(null, 257, n, n, null, null, 1, null, n) == E_INVALID
    assert combine(null, 4, n, n, null, null, 33, null, n) == E_INVALID

    keep_g, p_good = _host_ints([3, 5, 7, 7])                             # two rows of two points; repeats are fine
    keep_m, p_many = _host_ints(list(range(2, 2 + 2 * 33)))
    coeffs = rows[:2 * n * 32]

    def evals(c, npolys, length, stride, t, pts, v, w=_ptr(ws), wbytes=1 << 20):
        return L.ozk_fr_poly_eval_set_dev(c, npolys, length, stride, t, pts, v, w, wbytes, stream)

    assert evals(_ptr(coeffs), 2, n, n, 2, p_good, _ptr(vals)) == 0      # (the shape itself is fine)
    torch.cuda.synchronize()
    vals.fill_(SENTINEL)
    wsb = L.ozk_fr_poly_eval_set_workspace_bytes(2, n, 2)
    assert evals(_ptr(coeffs), 2, n, n, 0, p_good, _ptr(vals)) == E_INVALID
    assert evals(_ptr(coeffs), 2, n, n, 33, p_many, _ptr(vals)) == E_INVALID
    assert evals(_ptr(coeffs), 2, 0, n, 2, p_good, _ptr(vals)) == E_INVALID
    assert evals(_ptr(coeffs), 0, n, n, 2, p_good, _ptr(vals)) == E_INVALID
    assert evals(_ptr(coeffs), 2, n, n - 1, 2, p_good, _ptr(vals)) == E_INVALID
    assert evals(_ptr(coeffs), 2, n, n, 2, p_good, _ptr(vals), wbytes=wsb - 1) == E_INVALID
    assert b"workspace" in L.ozk_last_error()
    assert evals(_ptr(coeffs), 2, n, n, 2, p_good, _ptr(coeffs[(2 * n - 1) * 32:])) == E_INVALID
    assert b"overlap" in L.ozk_last_error()
    assert evals(_ptr(buf[8:]), 2, n, n, 2, p_good, _ptr(vals)) == E_INVALID
    assert evals(_ptr(coeffs), 2, n, n, 2, p_good, _ptr(vals[8:])) == E_INVALID
    assert b"aligned" in L.ozk_last_error()
    for args in ((null, p_good, _ptr(vals), _ptr(ws)), (_ptr(coeffs), null, _ptr(vals), _ptr(ws)),
                 (_ptr(coeffs), p_good, null, _ptr(ws)), (_ptr(coeffs), p_good, _ptr(vals), null)):
        assert evals(args[0], 2, n, n, 2, args[1], args[2], w=args[3]) == E_INVALID
    assert evals(null, 2, (1 << 27) + 1, (1 << 27) + 1, 2, null, null, w=null, wbytes=0) == E_INVALID
    assert evals(null, 2, n, n, 33, null, null, w=null, wbytes=0) == E_INVALID
    for bad in ((2, (1 << 27) + 1, 2), (1, 0, 1), (0, 4, 1), (2, n, 0), (2, n, 33)):
        assert L.ozk_fr_poly_eval_set_workspace_bytes(*bad) == 0
    torch.cuda.synchronize()
    assert u.host(buf) == bytes([SENTINEL]) * buf.numel() and u.host(vals) == bytes([SENTINEL]) * vals.numel()


# ---------------------------------------------------------------------------- the protocol
@pytest.fixture(scope="module")
def string():
    from octopuszk_amd import kzg, srs
    s = srs.Srs.from_secrets(M, TAU, 1, 1, generator=1)
    return s, kzg.VerifyKey.from_srs(s)


def _model_string():
    _, (g2, tau_g2) = kr.string(1, TAU)
    return o.G1.to_affine(o.G1.one), g2, tau_g2


def _dev_rows(rows):
    return _dev_ints([v for row in rows for v in row]).view(len(rows), -1)


def _open_and_check(ck, vk, rows, sets, **kw):
    """open_multi against the model: the bytes, the library's verifier, the model's verifier on the library's bytes"""
    from octopuszk_amd import kzg
    op = ck.open_multi(_dev_rows(rows), sets, **kw)
    proof = km.prove(rows, sets, TAU)
    assert op.to_bytes() == km.opening_of(proof, sets)
    assert kzg.verify_multi(vk, op) and kzg.verify_multi(vk, op.to_bytes())
    assert km.verify(*_model_string(), op.to_bytes())
    return op, proof


@pytest.mark.parametrize("n", [1, 2, 65, T + 1])
def test_protocol(string, n):
    from octopuszk_amd import kzg
    s, vk = string
    rng = random.Random(280 + n)
    ck = kzg.CommitKey.from_srs(s, n)
    a, b, c = _points(rng, 3, (0,))
    sets = [[a], [a, b], [c], [b, a], [a]]                      # three groups, one written in two orders
    rows = [[rng.randrange(R) for _ in range(n)] for _ in sets]
    op, proof = _open_and_check(ck, vk, rows, sets)
    assert [list(s_) for s_ in op.point_sets] == sets and [list(v) for v in op.values] == km.values_at(rows, sets)
    assert (op.w == kzg._G1_INF) == (n == 1) and (op.w2 == kzg._G1_INF) == (n == 1)
    assert kzg.multi_challenges(op.commitments, op.point_sets, op.values, op.w) == (proof["gamma"], proof["z"])
    assert len(op.to_bytes()) == 4 + 5 * 36 + 64 * 7 + 64


def test_protocol_edge_shapes(string, monkeypatch):
    from octopuszk_amd import kzg
    s, vk = string
    rng = random.Random(281)
    # every set larger than the polynomial: no quotient, W = O
    ck = kzg.CommitKey.from_srs(s, 2)
    sets = [_points(rng, 3), _points(rng, 3)]
    op, _ = _open_and_check(ck, vk, [[rng.randrange(R) for _ in range(2)] for _ in sets], sets)
    assert op.w == kzg._G1_INF and op.w2 != kzg._G1_INF
    # one row at one point
    ck = kzg.CommitKey.from_srs(s, 65)
    _open_and_check(ck, vk, [[rng.randrange(R) for _ in range(65)]], [[5]])
    # every set inside the largest (z and z omega): the values come from one pass per point over all rows; with nine
    # points from the set kernel again
    a, b = _points(rng, 2)
    nine = _points(rng, 9)
    for sets in ([[a], [b, a], [a], [b]], [[nine[3]], nine, nine[::-1]]):
        _open_and_check(ck, vk, [[rng.randrange(R) for _ in range(65)] for _ in sets], sets)
    # sets of three sizes, two distinct sets of a size, and the largest set there is
    sets = [_points(rng, 4), [7], _points(rng, 4), [8], _points(rng, 32), [7]]
    rows = [[rng.randrange(R) for _ in range(65)] for _ in sets]
    op, proof = _open_and_check(ck, vk, rows, sets)
    # the caller's commitments: no commitment MSM is run
    monkeypatch.setattr(ck, "commit", lambda coeffs: pytest.fail("commit was called"))
    given = ck.open_multi(_dev_rows(rows), sets, commitments=proof["commitments"])
    assert given.to_bytes() == op.to_bytes()


def test_rejections(string):
    from octopuszk_amd import kzg
    s, vk = string
    rng = random.Random(282)
    n = 65
    ck = kzg.CommitKey.from_srs(s, n)
    a, b, c = _points(rng, 3)
    sets = [[a], [a, b], [c]]
    rows = [[rng.randrange(R) for _ in range(n)] for _ in sets]
    op = ck.open_multi(_dev_rows(rows), sets)
    assert kzg.verify_multi(vk, op)
    cs, zs, ys = list(op.commitments), [list(r) for r in op.point_sets], [list(r) for r in op.values]
    other = u.expected(1, [12345])

    def changed(rows_, i, j):
        out = [list(r) for r in rows_]
        out[i][j] = (out[i][j] + 1) % R
        return out

    bad = {
        "a value": kzg.MultiOpening(cs, zs, changed(ys, 1, 1), op.w, op.w2),
        "a commitment": kzg.MultiOpening([cs[0], other, cs[2]], zs, ys, op.w, op.w2),
        "W": kzg.MultiOpening(cs, zs, ys, other, op.w2),
        "W'": kzg.MultiOpening(cs, zs, ys, op.w, other),
        "a point": kzg.MultiOpening(cs, changed(zs, 2, 0), ys, op.w, op.w2),
        "two rows' sets swapped": kzg.MultiOpening(cs, [zs[2], zs[1], zs[0]], [ys[2], ys[1], ys[0]], op.w, op.w2),
        "W and W' swapped": kzg.MultiOpening(cs, zs, ys, op.w2, op.w),
        "W' = O": kzg.MultiOpening(cs, zs, ys, op.w, kzg._G1_INF),
    }
    for what, o_ in bad.items():
        assert not kzg.verify_multi(vk, o_), what


def test_verify_multi_all_and_each(string):
    from octopuszk_amd import kzg
    s, vk = string
    n = 65
    rng = random.Random(283)
    ck = kzg.CommitKey.from_srs(s, n)
    a, b = _points(rng, 2)
    shapes = [[[a]], [[a], [a, b]], [[b, a], [a, b], [b]], [[5]], [[a, b], [6]]]
    ops = []
    for sets in shapes:
        rows = [[rng.randrange(R) for _ in range(n)] for _ in sets]
        ops.append(ck.open_multi(_dev_rows(rows), sets))
    ops[3] = ck.open_multi(_dev_rows([[4] + [0] * (n - 1)]), [[5]])          # a constant among them: W = W' = O
    assert ops[3].w == ops[3].w2 == kzg._G1_INF
    seed = bytes(range(32))
    assert kzg.verify_multi_all(vk, ops, seed) and kzg.verify_multi_all(vk, ops) and kzg.verify_multi_all(vk, [])
    assert kzg.verify_multi_each(vk, ops, seed) == [True] * 5 and kzg.verify_multi_each(vk, []) == []
    o2 = ops[2]
    ys = [list(r) for r in o2.values]
    ys[1][0] = (ys[1][0] + 1) % R
    bad = list(ops)
    bad[2] = kzg.MultiOpening(o2.commitments, o2.point_sets, ys, o2.w, o2.w2)
    assert not kzg.verify_multi_all(vk, bad, seed)
    assert kzg.verify_multi_each(vk, bad, seed) == [True, True, False, True, True]
    assert kzg.verify_multi_all(vk, [op.to_bytes() for op in ops], seed)
