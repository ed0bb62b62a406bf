"""No-GPU checks of KZG set openings: the integer model against itself and against the model
pairing, the per-lane pieces of the set kernels built for the host (tests/native/kzg_set_hostcheck.cpp) against the
model, the byte formats, the challenge and weight streams, and every argument error raised before the library is
touched."""
import ctypes
import hashlib
import os
import random
import subprocess

import pytest
import torch

import ceremony_ref as cref
import codec_ref as ref
import kzg_ref as kr
import kzg_set_ref as ks
from oracle import bn254 as o

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "kzg_set_hostcheck.cpp")
LIB = os.path.join(HERE, "native", "_kzg_set_hostcheck.so")
CSRC = os.path.join(HERE, "..", "octopuszk_amd", "csrc")
R = o.R
rng = random.Random(23)


def _poly(n):
    return [rng.randrange(R) for _ in range(n)]


def _points(t, special=(0, 1, R - 1)):
    out = list(special)[:t]
    while len(out) < t:
        z = rng.randrange(R)
        if z not in out:
            out.append(z)
    rng.shuffle(out)
    return out


# ---------------------------------------------------------------------------- the model against itself
@pytest.mark.parametrize("t", [1, 2, 3, 8])
def test_model_quotient_identity(t):
    for n in (1, t, t + 1, 2 * t + 3, 23):
        p, pts = _poly(n), _points(t)
        q, values = ks.div_set(p, pts)
        z_s, interp = ks.vanishing(pts), ks.interpolate(pts, values)
        assert len(q) == n and q[max(n - t, 0):] == [0] * min(t, n) and z_s[t] == 1
        assert [kr.horner(interp, z) for z in pts] == values == [kr.horner(p, z) for z in pts]
        assert all(kr.horner(z_s, z) == 0 for z in pts)
        # p = q Z_S + I, coefficient by coefficient
        for j in range(max(n, t)):
            conv = sum(q[j - k] * z_s[k] for k in range(t + 1) if 0 <= j - k < n)
            assert (p[j] if j < n else 0) == (conv + (interp[j] if j < t else 0)) % R, (n, t, j)
        # t chained divisions by the linear factors: the same quotient, t places up
        chained = list(p)
        for z in pts:
            chained = kr.div_linear(chained, z)[0]
        assert chained == q
    p, z = _poly(9), rng.randrange(R)
    assert ks.div_set(p, [z]) == (kr.div_linear(p, z)[0], [kr.div_linear(p, z)[1]])


@pytest.mark.parametrize("n", [2, 4, 8, 16])
def test_model_evaluation_form_formulas(n):
    """the formulas of the evaluation-form kernel, in integers, against the transform of the coefficient-form quotient"""
    omega = kr.root(n)
    f = _poly(n)
    w = [pow(omega, i, R) for i in range(n)]
    for t in (1, 2, 3, 8):
        pts = _points(t, (0,))
        want_q, want_y = ks.open_set_evals(f, pts, omega)
        inv = [[pow(wi - z, -1, R) for z in pts] for wi in w]
        inv_z = [1] * n
        for i in range(n):
            for j in range(t):
                inv_z[i] = inv_z[i] * inv[i][j] % R
        wj = []
        for j, z in enumerate(pts):
            d = 1
            for k, zk in enumerate(pts):
                if k != j:
                    d = d * (z - zk) % R
            wj.append(pow(d, -1, R))
        y = [(pow(z, n, R) - 1) * pow(n, -1, R) * sum(f[i] * w[i] * -inv[i][j] for i in range(n)) % R
             for j, z in enumerate(pts)]
        q = [(f[i] * inv_z[i] - sum(y[j] * wj[j] * inv[i][j] for j in range(t))) % R for i in range(n)]
        assert (q, y) == (want_q, want_y), (n, t)


def test_model_verifier_accepts_and_rejects():
    tau = 0x1234567
    t = 3
    tau_g1, tau_g2 = ks.string(t, tau)
    g1 = tau_g1[0]
    p, pts = _poly(6), _points(t, ())
    q, values = ks.div_set(p, pts)
    full_g1 = [kr.g1_mul(g1, pow(tau, i, R)) for i in range(6)]
    C, pi = kr.commit(full_g1, p), kr.commit(full_g1, q)
    assert pi == kr.g1_mul(g1, kr.horner(q, tau))
    assert ks.verify(tau_g1, tau_g2, C, pts, values, pi)
    assert not ks.verify(tau_g1, tau_g2, kr.g1_add(C, g1), pts, values, pi)
    assert not ks.verify(tau_g1, tau_g2, C, [(pts[0] + 1) % R] + pts[1:], values, pi)
    assert not ks.verify(tau_g1, tau_g2, C, pts, values[:2] + [(values[2] + 1) % R], pi)
    assert not ks.verify(tau_g1, tau_g2, C, pts, values, kr.g1_add(pi, g1))
    # len <= t: the polynomial is its own interpolant, pi = O; with pi = O a polynomial of higher degree fails
    zero = o.G1.to_affine(o.G1.zero)
    low = _poly(t)
    q_low, v_low = ks.div_set(low, pts)
    assert q_low == [0] * t
    assert ks.verify(tau_g1, tau_g2, kr.commit(full_g1, low), pts, v_low, zero)
    assert not ks.verify(tau_g1, tau_g2, C, pts, values, zero)
    # a set through tau itself: [Z_S(tau)] g2 = O is refused
    assert not ks.verify(tau_g1, tau_g2, C, [tau] + pts[1:], values, pi)


# ---------------------------------------------------------------------------- the kernels' per-lane pieces
@pytest.fixture(scope="module")
def hc():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("kzg_set.cuh", "kzg.cuh", "fp29.cuh", "consts_gen.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


def _words(values):
    b = b"".join(kr.le(v) for v in values)
    return (ctypes.c_uint32 * (len(b) // 4)).from_buffer_copy(b)


def _out(n):
    return (ctypes.c_uint32 * (8 * n))()


def _h(m, zs):
    """the complete homogeneous polynomial of degree m in zs"""
    if m == 0:
        return 1
    if not zs:
        return 0
    return sum(pow(zs[0], k, R) * _h(m - k, zs[1:]) for k in range(m + 1)) % R


@pytest.mark.parametrize("t", [1, 2, 3, 8])
def test_table_and_carries(hc, t):
    """T[s][i] = z_i^s / prod_{k <= s, k != i} (z_i - z_k), and the carries it gives are the stages' values at a
    boundary: sum_k p_k h_k(z_0 .. z_s) for the tail p above it"""
    assert hc.kzgsethc_t_max() == 32 and hc.kzgsethc_ev_t_max() == 8
    pts = _points(t)
    pts[0] += R if t > 1 else 0                              # a point written as z + r
    red = [z % R for z in pts]
    out = _out(t * (t + 1) // 2)
    hc.kzgsethc_table(_words(pts), t, out)
    got = kr.ints(bytes(out))
    for s in range(t):
        for i in range(s + 1):
            d = 1
            for k in range(s + 1):
                if k != i:
                    d = d * (red[i] - red[k]) % R
            assert got[s * (s + 1) // 2 + i] == pow(red[i], s, R) * pow(d, -1, R) % R, (t, s, i)
    tail = _poly(4)
    carries = _out(t)
    hc.kzgsethc_carries(_words(pts), t, _words([kr.horner(tail, z) for z in red]), carries)
    want = [sum(c * _h(k, red[:s + 1]) for k, c in enumerate(tail)) % R for s in range(t)]
    assert kr.ints(bytes(carries)) == want
    assert hc.kzgsethc_distinct(_words(pts), t) == 1
    if t > 1:
        assert hc.kzgsethc_distinct(_words(pts[:-1] + [red[0]]), t) == 0      # equal mod r, written differently


@pytest.mark.parametrize("chunk", [1, 2, 7])
def test_pieces_stages_carries_and_application(hc, chunk):
    """pieces of `chunk` coefficients: their values at every point, the tails, the mixed carries, the t stages from them"""
    for t in (1, 2, 3, 8):
        for n in (1, 2, t, t + 1, chunk + 1, 3 * chunk + 2, 23):
            p = _poly(n)
            p[0] += R if p[0] < (1 << 256) - R else 0            # a coefficient written as p + r
            pts = _points(t)
            quot, values = _out(n), _out(t)
            hc.kzgsethc_open(_words(p), n, chunk, _words(pts), t, quot, values)
            q, y = ks.div_set([c % R for c in p], pts)
            assert (kr.ints(bytes(quot)), kr.ints(bytes(values))) == (q, y), (n, chunk, t)


def test_inverses_from_one_inverse_per_element(hc):
    batch = hc.kzgsethc_batch()
    assert batch >= 3
    for t in (1, 2, 3, 8):
        pts = _points(t)
        for n in (batch, batch - 1, 1):
            for zeros in ((), (0,), (batch // 2,), (n - 1,)):
                # an element equal to a point: its product is zero and it is left out of the chunk's inversion
                w = [pts[k % t] if k in zeros else rng.randrange(R) for k in range(n)]
                inv_z, inv = _out(n), _out(n * t)
                hc.kzgsethc_inverses(_words(w), n, _words(pts), t, inv_z, inv)
                got_z, got = kr.ints(bytes(inv_z)), kr.ints(bytes(inv))
                for k in range(n):
                    live = k not in zeros
                    prod = 1
                    for z in pts:
                        prod = prod * (w[k] - z) % R
                    assert got_z[k] == (pow(prod, -1, R) if live else 0), (t, n, zeros, k)
                    assert got[k * t:(k + 1) * t] == [pow(w[k] - z, -1, R) if live else 0 for z in pts]


# ---------------------------------------------------------------------------- bytes
def _opening_fields(t=3):
    tau_g1, _ = kr.string(2, 5)
    C, pi = kr.g1_mul(tau_g1[0], 11), kr.g1_mul(tau_g1[0], 13)
    return C, list(range(3, 3 + t)), list(range(40, 40 + t)), pi


def test_set_opening_bytes_round_trip_and_failures():
    from octopuszk_amd import kzg
    for t in (1, 3, 32):
        C, zs, ys, pi = _opening_fields(t)
        b = ks.opening_bytes(C, zs, ys, pi)
        op = kzg.SetOpening.from_bytes(b)
        assert (op.c, op.points, op.values, op.pi) == (ref.encode_g1(C), tuple(zs), tuple(ys), ref.encode_g1(pi))
        assert op.to_bytes() == b and len(b) == 68 + 64 * t and op.t == t
    C, zs, ys, pi = _opening_fields(3)
    b = ks.opening_bytes(C, zs, ys, pi)
    inf = o.G1.to_affine(o.G1.zero)
    assert kzg.SetOpening.from_bytes(ks.opening_bytes(inf, zs, ys, inf)).pi == kzg._G1_INF

    def with_t(t):
        return b[:32] + t.to_bytes(4, "little") + b[36:]

    for bad in (b[:-1], b + b"\x00", b[:35], with_t(2), with_t(4)):
        with pytest.raises(ValueError, match="set opening: length"):
            kzg.SetOpening.from_bytes(bad)
    for t in (0, 33, 1 << 31):
        with pytest.raises(ValueError, match="set opening: t = "):
            kzg.SetOpening.from_bytes(with_t(t))
    with pytest.raises(ValueError, match="set opening: z is not below r"):
        kzg.SetOpening.from_bytes(b[:68] + kr.le(R) + b[100:])
    with pytest.raises(ValueError, match="set opening: y is not below r"):
        kzg.SetOpening.from_bytes(b[:132] + kr.le(R + 1) + b[164:])
    with pytest.raises(ValueError, match="set opening: z has repeated points"):
        kzg.SetOpening.from_bytes(b[:68] + b[36:68] + b[100:])
    no_point = next(kr.le(x) for x in range(2, 50) if ref.decode_g1(kr.le(x))[0] == 3)
    with pytest.raises(ValueError, match="set opening: C does not decode"):
        kzg.SetOpening.from_bytes(no_point + b[32:])
    with pytest.raises(ValueError, match="set opening: pi does not decode"):
        kzg.SetOpening.from_bytes(b[:-32] + kr.le(o.Q))
    # the constructor holds the same rules
    enc = ref.encode_g1(C)
    for args, what in ((([R], [0]), "set opening: z"), (([0], [R]), "set opening: y"), (([1, 1], [0, 0]), "repeated"),
                       (([], []), "t = 0"), ((list(range(33)), [0] * 33), "t = 33"), (([1, 2], [0]), "1 values for 2")):
        with pytest.raises(ValueError, match=what):
            kzg.SetOpening(enc, args[0], args[1], enc)


def _subgroup_model(points, encodings):
    code, P = ref.decode_g2(encodings)
    return code == 0 and o.G2.is_zero(o.G2.mul(P, R))


def test_set_verify_key_bytes_round_trip_and_failures(monkeypatch):
    from octopuszk_amd import kzg
    t_max = 2
    tau_g1, tau_g2 = ks.string(t_max, 9)
    b = ks.vk_bytes(tau_g1, tau_g2)
    assert len(b) == 4 + 32 * t_max + 64 * (t_max + 1)
    # the subgroup test runs on the device (vectors.in_subgroup_g2): here the model's stands in for it, fed by what
    # from_bytes hands it
    monkeypatch.setattr(kzg.SetVerifyKey, "points", lambda self: (None, bytes(192 * (self.t_max + 1))))
    monkeypatch.setattr(kzg, "_g2_in_subgroup", _subgroup_model)
    vk = kzg.SetVerifyKey.from_bytes(b)
    assert (vk.t_max, vk.g1s, vk.g2s) == (t_max, b[4:68], b[68:]) and vk.to_bytes() == b
    for bad in (b + b"\x00", b[:-1], b[:3], (1).to_bytes(4, "little") + b[4:]):
        with pytest.raises(ValueError, match="set verification key: length"):
            kzg.SetVerifyKey.from_bytes(bad)
    for t in (0, 33):
        with pytest.raises(ValueError, match="set verification key: t_max = %d" % t):
            kzg.SetVerifyKey.from_bytes(t.to_bytes(4, "little") + b[4:])
    no1 = next(kr.le(x) for x in range(2, 50) if ref.decode_g1(kr.le(x))[0] == 3)
    with pytest.raises(ValueError, match=r"set verification key: tau_g1\[1\] does not decode"):
        kzg.SetVerifyKey.from_bytes(b[:36] + no1 + b[68:])
    with pytest.raises(ValueError, match=r"set verification key: tau_g2\[0\] does not decode"):
        kzg.SetVerifyKey.from_bytes(b[:68] + kr.le(o.Q) + b[100:])
    with pytest.raises(ValueError, match=r"set verification key: tau_g2\[2\] does not decode"):
        kzg.SetVerifyKey.from_bytes(b[:196] + kr.le(o.Q) + b[228:])
    inf1, inf2 = ref.encode_g1(o.G1.to_affine(o.G1.zero)), ref.encode_g2(o.G2.to_affine(o.G2.zero))
    with pytest.raises(ValueError, match=r"set verification key: tau_g1\[0\] is the point at infinity"):
        kzg.SetVerifyKey.from_bytes(b[:4] + inf1 + b[36:])
    with pytest.raises(ValueError, match=r"set verification key: tau_g2\[2\] is the point at infinity"):
        kzg.SetVerifyKey.from_bytes(b[:196] + inf2)
    outside = ref.encode_g2(cref.twist_point_outside_the_subgroup())
    with pytest.raises(ValueError, match=r"set verification key: tau_g2\[1\] is not in the order-r subgroup"):
        kzg.SetVerifyKey.from_bytes(b[:132] + outside + b[196:])
    with pytest.raises(ValueError, match=r"set verification key: tau_g2\[0\] is not in the order-r subgroup"):
        kzg.SetVerifyKey.from_bytes(b[:68] + outside + b[132:])


def test_streams_match_literal_recomputation():
    from octopuszk_amd import kzg, transcript
    seed = bytes(range(32))
    assert kzg._SET_RHO_TAG == b"OZK-kzg-set-rho" and kzg._SET_GAMMA_TAG == b"OZK-kzg-set-gamma"
    got = kr.ints(transcript.weights(seed, 5, kzg._SET_RHO_TAG))
    blocks = [hashlib.sha256(b"OZK-kzg-set-rho" + seed + j.to_bytes(8, "little")).digest() for j in range(3)]
    want = [int.from_bytes(blk[h:h + 16], "little") or 1 for blk in blocks for h in (0, 16)][:5]
    assert got == want == ks.rho(seed, 5) and got != kr.rho(seed, 5)
    cs = [kr.le(i + 1) for i in range(2)]
    pts, values = [7, 8, 9], [[1, 2, 3], [4, 5, 6]]
    body = (b"OZK-kzg-set-gamma" + (2).to_bytes(8, "little") + (3).to_bytes(8, "little")
            + b"".join(kr.le(v) for v in pts) + b"".join(cs) + b"".join(kr.le(v) for v in (1, 2, 3, 4, 5, 6)))
    want = int.from_bytes(hashlib.sha256(body).digest()[:16], "little") or 1
    assert kzg.set_combine_challenge(pts, cs, values) == want == ks.gamma(pts, cs, values)
    assert 1 <= want < 1 << 128


def test_host_polynomials_match_the_model():
    from octopuszk_amd import kzg
    for t in (1, 2, 5):
        pts, ys = _points(t), _poly(t)
        assert kzg._vanishing(tuple(pts)) == ks.vanishing(pts)
        assert kzg._interpolant(tuple(pts), tuple(ys)) == ks.interpolate(pts, ys)


# ---------------------------------------------------------------------------- argument errors, the library absent
class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was reached: %s" % name)


class _FakeSrs:
    m = 4
    tau_g1 = torch.zeros(96 * 9, dtype=torch.uint8)
    tau_g2 = torch.zeros(192 * 4, dtype=torch.uint8)


class _Shaped:
    """what _rows reads of a tensor, with a CUDA tensor's answers: the point checks run where there is no GPU"""

    def __init__(self, shape, stride, ptr=256):
        self.shape, self._stride, self._ptr, self.dtype, self.is_cuda = shape, stride, ptr, torch.uint8, True

    def dim(self):
        return len(self.shape)

    def numel(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def stride(self, i):
        return self._stride[i]

    def data_ptr(self):
        return self._ptr

    def unsqueeze(self, _):
        return _Shaped((1,) + tuple(self.shape), (self.shape[0],) + tuple(self._stride), self._ptr)


def test_argument_errors_come_before_any_library_call(monkeypatch):
    from octopuszk_amd import kzg, lib
    monkeypatch.setattr(lib, "load", lambda: _NoLibrary())
    monkeypatch.setattr(kzg._lib, "load", lambda: _NoLibrary())
    ck = kzg.CommitKey.from_srs(_FakeSrs(), 8)
    cpu = torch.zeros(32 * 8, dtype=torch.uint8)
    for call in (lambda t: ck.open_set(t, [1]), lambda t: ck.open_set_evals(t, [2]),
                 lambda t: ck.open_set_combined(t, [1])):
        with pytest.raises(TypeError, match="CUDA"):           # the device
            call(cpu)
        with pytest.raises(TypeError, match="uint8"):          # the dtype
            call(cpu.to(torch.int32))
    # the points, past the row checks
    monkeypatch.setattr(kzg.torch, "Tensor", _Shaped)
    one, two = _Shaped((256,), (1,)), _Shaped((2, 256), (256, 1))
    with pytest.raises(ValueError, match="the key has n = 8"):
        ck.open_set(_Shaped((64,), (1,)), [1])
    for call in (ck.open_set, ck.open_set_evals, ck.open_set_combined):
        with pytest.raises(TypeError, match="list of points"):
            call(one, 5)
        with pytest.raises(ValueError, match="empty"):
            call(one, [])
        with pytest.raises(ValueError, match="repeated"):
            call(one, [3, 7, 3])
        with pytest.raises(ValueError, match=r"\[0, r\)"):
            call(one, [3, R])
        with pytest.raises(ValueError, match=r"\[0, r\)"):
            call(one, [-1])
        with pytest.raises(ValueError, match="t = 4 points: 1 <= t <= 3"):      # beyond the key: m = 4
            call(one, [2, 3, 5, 7])
    for call in (ck.open_set, ck.open_set_evals):
        with pytest.raises(ValueError, match="ragged"):
            call(two, [[2, 3], [5]])
        with pytest.raises(ValueError, match="3 lists of points for 2 rows"):
            call(two, [[2], [3], [5]])
        with pytest.raises(ValueError, match="not a mix"):
            call(two, [[2], 3])
    with pytest.raises(ValueError, match="one list of points"):
        ck.open_set_combined(two, [[2], [3]])
    for inside in (1, R - 1, kr.root(8)):
        with pytest.raises(ValueError, match="lies in the domain"):
            ck.open_set_evals(one, [5, inside])
    with pytest.raises(ValueError, match="power of two"):
        kzg.CommitKey.from_srs(_FakeSrs(), 6).open_set_evals(_Shaped((192,), (1,)), [5])
    # t beyond what either form takes, on a longer string
    class _Long(_FakeSrs):
        m = 64
    big = kzg.CommitKey.from_srs(_Long(), 8)
    with pytest.raises(ValueError, match="t = 33 points: 1 <= t <= 32"):
        big.open_set(one, list(range(2, 35)))
    with pytest.raises(ValueError, match="t = 9 points: 1 <= t <= 8"):
        big.open_set_evals(one, list(range(2, 11)))
    # keys and verification
    for bad in (0, 4, 33):
        with pytest.raises(ValueError, match="t_max = %d" % bad):
            kzg.SetVerifyKey.from_srs(_FakeSrs(), bad)
    vk = kzg.SetVerifyKey(2, bytes(64), bytes(192))
    enc = bytes(32)
    with pytest.raises(ValueError, match="the key covers t_max = 2"):
        kzg.verify_set(vk, kzg.SetOpening(enc, [1, 2, 3], [0, 0, 0], enc))
    with pytest.raises(ValueError, match="the key covers t_max = 2"):
        kzg.verify_set_all(vk, [kzg.SetOpening(enc, [1], [0], enc), kzg.SetOpening(enc, [1, 2, 3], [0, 0, 0], enc)])
    with pytest.raises(ValueError, match="set opening: length"):
        kzg.verify_set(vk, bytes(35))
    with pytest.raises(ValueError, match="no commitment"):
        kzg.verify_set_combined(vk, [], [1], [], enc)
    with pytest.raises(ValueError, match="t = 3 points"):
        kzg.verify_set_combined(vk, [enc], [1, 2, 3], [[0, 0, 0]], enc)
    with pytest.raises(ValueError, match="repeated"):
        kzg.verify_set_combined(vk, [enc], [1, 1], [[0, 0]], enc)
    with pytest.raises(ValueError, match="values: 1 rows of 2 for 2 commitments"):
        kzg.verify_set_combined(vk, [enc, enc], [1, 2], [[0, 0]], enc)
    with pytest.raises(ValueError, match=r"\[0, r\)"):
        kzg.verify_set_combined(vk, [enc], [1, 2], [[0, R]], enc)
    with pytest.raises(ValueError, match="commitment: 31 bytes"):
        kzg.verify_set_combined(vk, [bytes(31)], [1, 2], [[0, 0]], enc)
