"""ozk_fr_poly_eval_dev (k_fr_poly_eval and k_fr_sum_partials of csrc/fr_tables.cuh) through the C ABI, against plain
Horner in Python integers (kzg_ref.horner), byte for byte.  The kernel runs nb = min(ceil(len / 8192), 256) workgroups a
polynomial, S = 256 nb lanes, lane g over the coefficients g, g + S, ..: the lengths below take one workgroup with idle
lanes (len < 256), the first split (8193: nb = 2, 17 trips of the lane loop), nb = 4, and the cap (len > 2^21).  Every
case runs on canonical coefficients, on coefficients written as x + k r, and on rows of 2^256 - 1: the coefficients are
reduced mod r on load.  Then the three callers in octopuszk_amd/kzg.py that hand it the caller's rows unreduced."""
import ctypes
import random

import numpy as np
import pytest
import torch

import fr_gpu_util as fu
import kzg_ref as kr
import kzg_set_ref as ks
import srs_gpu_util as u
from fr_gpu_util import ALL_ONES, GUARD, R
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

E_INVALID = -1
CHUNK = 8192                    # the coefficients of one workgroup (256 lanes x 32) before the cap
LENGTHS = [1, 2, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
PAST_THE_CAP = 256 * CHUNK + CHUNK + 3
FORMS = ["canonical", "wide", "ones"]
SENTINEL_INT = int.from_bytes(bytes([fu.POISON]) * 32, "little")
TAU = 0x5eed0123456789abcdef0123456789abcdef0123456789abcdef % R
M = 512


def _eval(d_coeffs, npolys, length, stride, z):
    """one call on device coefficients -> the npolys values as bytes; the workspace has exactly the size asked for, and
    the GUARD bytes behind the output keep their poison"""
    L = fu.lib()
    out = fu.poisoned(32 * npolys + GUARD)
    wsb = int(L.ozk_fr_poly_eval_workspace_bytes(npolys))
    assert wsb > 0
    ws = fu.poisoned(wsb)
    keep, p_z = fu.host_ints([z])
    rc = L.ozk_fr_poly_eval_dev(fu.ptr(d_coeffs), npolys, length, stride, p_z, fu.ptr(out), fu.ptr(ws), wsb, fu.stream())
    assert rc == 0, L.ozk_last_error()
    raw = fu.host_bytes(out)
    assert fu.tail_untouched(out, 32 * npolys)
    return raw[:32 * npolys]


def _rows(form, npolys, length, seed):
    rng = random.Random(seed)
    if form == "ones":
        return [[ALL_ONES] * length for _ in range(npolys)]
    if form == "wide":
        rows = [fu.wide_row(rng, length, phase=y) for y in range(npolys)]
        if length >= 6:
            fu.assert_wide(rows)
        return rows
    return [[rng.randrange(R) for _ in range(length)] for _ in range(npolys)]


def _points(length, seed):
    """0 (the value is c_0: lane 0 needs r^0 = 1), 1 (the sum), r - 1, a random point, and for a power of two a root of
    unity of that order"""
    pts = [0, 1, R - 1, random.Random(seed).randrange(R)]
    if length > 1 and length & (length - 1) == 0:
        pts.append(kr.root(length))
    return pts


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("length", LENGTHS)
def test_poly_eval_matches_horner(length, form):
    rows = _rows(form, 3, length, 4100 + length)
    points = _points(length, 4200 + length)
    want = {z: [kr.le(kr.horner(row, z)) for row in rows] for z in points}      # Horner mod r reduces as it goes
    # (npolys, poly_stride): back to back, with gaps that hold a sentinel, and one polynomial at stride 0
    for npolys, stride in ((1, length), (3, length), (1, length + 3), (3, length + 3), (1, 0)):
        d_c = fu.dev_from_ints(fu.flat(rows[:npolys], max(stride, length), fill=SENTINEL_INT))
        for z in points:
            assert _eval(d_c, npolys, length, stride, z) == b"".join(want[z][:npolys]), (length, form, npolys, stride, z)


@pytest.fixture(scope="module")
def past_the_cap():
    """(the bytes of PAST_THE_CAP random 256-bit words, the point): dense, so that every lane of every workgroup
    contributes; the same words serve the canonical case with the top three bits cleared (< 2^253 < r)"""
    raw = np.random.default_rng(4300).integers(0, 256, size=(PAST_THE_CAP, 32), dtype=np.uint8)
    return raw, random.Random(4301).randrange(R)


def _ints_of(raw):
    b = raw.tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


@pytest.mark.parametrize("form", FORMS)
def test_poly_eval_past_the_cap_of_workgroups(past_the_cap, form):
    """len > 2^21: nb stays 256, S = 65536, and a lane makes 33 trips"""
    raw, z = past_the_cap
    raw = raw.copy()
    if form == "canonical":
        raw[:, 31] &= 0x1F
    elif form == "ones":
        raw[:] = 0xFF
    coeffs = _ints_of(raw)
    if form == "wide":
        assert 2 * sum(1 for v in coeffs if v >= 2 * R) >= len(coeffs)
    d_c = torch.from_numpy(raw.reshape(-1)).cuda()
    assert _eval(d_c, 1, PAST_THE_CAP, PAST_THE_CAP, z) == kr.le(kr.horner(coeffs, z))


def test_rejected_shapes_launch_nothing():
    L = fu.lib()
    n = 8
    coeffs = fu.poisoned(3 * n * 32)
    out = fu.poisoned(3 * 32)
    wsb = int(L.ozk_fr_poly_eval_workspace_bytes(3))
    ws = fu.poisoned(wsb)
    keep, z = fu.host_ints([5])
    null = ctypes.c_void_p(0)

    def call(c=None, npolys=3, length=n, stride=n, r=z, o_=None, w=None, wbytes=wsb):
        args = [fu.ptr(t) if p is None else p for p, t in ((c, coeffs), (o_, out), (w, ws))]   # (a null pointer is falsy)
        return L.ozk_fr_poly_eval_dev(args[0], npolys, length, stride, r, args[1], args[2], wbytes, fu.stream())

    assert call() == 0                                                   # (the shape itself is fine)
    torch.cuda.synchronize()
    out.fill_(fu.POISON)
    ws.fill_(fu.POISON)
    for kw in (dict(c=null), dict(r=null), dict(o_=null), dict(w=null), dict(npolys=0), dict(npolys=65536), dict(length=0),
               dict(stride=-1), dict(stride=n - 1), dict(wbytes=wsb - 1)):
        assert call(**kw) == E_INVALID, kw
    assert call(npolys=1, stride=0, wbytes=int(L.ozk_fr_poly_eval_workspace_bytes(1)) - 1) == E_INVALID
    assert L.ozk_fr_poly_eval_workspace_bytes(0) == 0 and L.ozk_fr_poly_eval_workspace_bytes(-1) == 0
    torch.cuda.synchronize()
    assert fu.tail_untouched(out, 0) and fu.tail_untouched(ws, 0) and fu.tail_untouched(coeffs, 0)


# ---------------------------------------------------------------------------- the callers in octopuszk_amd/kzg.py
@pytest.fixture(scope="module")
def string():
    from octopuszk_amd import kzg, srs
    s = srs.Srs.from_secrets(M, TAU, 1, 1, generator=1)
    return s, kzg.CommitKey.from_srs(s, 65)


def _dev_rows(rows):
    return fu.dev_from_ints([v for row in rows for v in row]).view(len(rows), -1)


def _point(enc):
    import codec_ref
    code, P = codec_ref.decode_g1(enc)
    assert code == 0
    return o.G1.to_affine(P)


def _combined(cs, gamma):
    acc = o.G1.to_affine(o.G1.zero)
    for i, c in enumerate(cs):
        acc = kr.g1_add(acc, kr.g1_mul(_point(c), pow(gamma, i, R)))
    return acc


def _written_rows(form, k, n, seed):
    rows = _rows(form, k, n, seed)
    return rows, fu.reduced(rows)


@pytest.mark.parametrize("form", ["wide", "ones"])
def test_open_combined_of_unreduced_rows(string, form):
    """the values, the commitments and the proof are those of the rows mod r, byte for byte, and the opening verifies
    under the model's pairing check"""
    s, ck = string
    k, n = 3, 65
    written, rows = _written_rows(form, k, n, 4400)
    z = random.Random(4401).randrange(R)
    cs, ys, pi = ck.open_combined(_dev_rows(written), z)
    assert ys == [kr.horner(p, z) for p in rows]
    assert cs == [u.expected(1, [kr.horner(p, TAU)]) for p in rows]
    gamma = kr.gamma(z, cs, ys)
    weights = [pow(gamma, i, R) for i in range(k)]
    q, _ = kr.div_linear(kr.combine(rows, weights), z)
    assert pi == u.expected(1, [kr.horner(q, TAU)])
    assert (cs, ys, pi) == ck.open_combined(_dev_rows(rows), z)
    _, (g2, tau_g2) = kr.string(1, TAU)
    g1 = o.G1.to_affine(o.G1.one)
    assert kr.verify(g1, g2, tau_g2, _combined(cs, gamma), z, sum(w * y for w, y in zip(weights, ys)) % R, _point(pi))


@pytest.mark.parametrize("form", ["wide", "ones"])
def test_open_set_combined_of_unreduced_rows(string, form):
    s, ck = string
    k, n, t = 3, 65, 3
    written, rows = _written_rows(form, k, n, 4410)
    rng = random.Random(4411)
    pts = [rng.randrange(R) for _ in range(t)]
    cs, ys, pi = ck.open_set_combined(_dev_rows(written), pts)
    assert ys == [[kr.horner(p, z) for z in pts] for p in rows]
    assert cs == [u.expected(1, [kr.horner(p, TAU)]) for p in rows]
    gamma = ks.gamma(pts, cs, ys)
    weights = [pow(gamma, i, R) for i in range(k)]
    q, _ = ks.div_set(kr.combine(rows, weights), pts)
    assert pi == u.expected(1, [kr.horner(q, TAU)])
    assert (cs, ys, pi) == ck.open_set_combined(_dev_rows(rows), pts)
    tau_g1, tau_g2 = ks.string(t, TAU)
    values = [sum(w * row[i] for w, row in zip(weights, ys)) % R for i in range(t)]
    assert ks.verify(tau_g1, tau_g2, _combined(cs, gamma), pts, values, _point(pi))


@pytest.mark.parametrize("form", ["wide", "ones"])
def test_poly_eval_points_of_unreduced_rows(form):
    from octopuszk_amd import kzg
    k, n = 3, 65
    written, rows = _written_rows(form, k, n, 4420)
    points = _points(64, 4421)
    got = kzg.poly_eval_points(_dev_rows(written), k, n, n, points)
    assert got == [[kr.horner(p, z) for p in rows] for z in points]
    assert got == kzg.poly_eval_points(_dev_rows(rows), k, n, n, points)
