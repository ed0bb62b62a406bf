"""No-GPU checks of the KZG multi-opening: the integer model against itself and against the
model pairing, the opening's bytes and every strict-parse rejection, the two challenges pinned to literal values, and
every argument error raised before the library is touched."""
import hashlib
import random

import pytest
import torch

import codec_ref as ref
import kzg_multi_ref as km
import kzg_ref as kr
import kzg_set_ref as ks
from oracle import bn254 as o

R = o.R
TAU = 0x1234567
rng = random.Random(28)


def _poly(n):
    return [rng.randrange(R) for _ in range(n)]


def _distinct(t):
    out = []
    while len(out) < t:
        z = rng.randrange(R)
        if z not in out:
            out.append(z)
    return out


def _cases():
    """(n, the sets of the rows): the shapes the protocol's algebra was checked at"""
    a, b, c, d = _distinct(4)
    return [
        (1, [[a], [b]]),                                           # two singleton sets
        (2, [[a], [a, b], [a]]),                                   # three rows in two groups
        (65, [[a], [a, b], [c], [b, a], [a]]),                     # five rows, three groups, one written in two orders
        (9, [[a, b, c], [d]]),                                     # sets of 3 and 1 points, |T| = 4
        (4, [[a, b], [a, b], [a, b]]),                             # one group
        (3, [[a, b, c, d], [a]]),                                  # t > n: that row is its own interpolant
    ]


# ---------------------------------------------------------------------------- the model against itself
def test_model_kernels():
    rows = [_poly(5) for _ in range(4)]
    weights = _poly(4)
    got = km.combine_groups(rows, weights, [2, 0, 2, 0], 4)
    assert got[0] == kr.combine([rows[1], rows[3]], [weights[1], weights[3]])
    assert got[2] == kr.combine([rows[0], rows[2]], [weights[0], weights[2]])
    assert got[1] == got[3] == [0] * 5
    assert km.combine_groups(rows, weights, [0] * 4, 1) == [kr.combine(rows, weights)]
    sets = [[3, 3, 7], [0, 1, R - 1], [5, 5, 5], [9, 8, 7]]
    values = km.values_at(rows, sets)
    assert values[0][0] == values[0][1] == ks.div_set(rows[0], [3])[1][0]
    assert values[1] == ks.div_set(rows[1], sets[1])[1] and values[3] == ks.div_set(rows[3], sets[3])[1]


def test_model_identity_at_z():
    """L(z) = sum_i gamma^i c_{g(i)} r_i(z), whatever z is: the prover's remainder is what the verifier subtracts"""
    for n, sets in _cases():
        proof = km.prove([_poly(n) for _ in sets], sets, TAU)
        assert proof["l_at_z"] == proof["sum_at_z"], (n, sets)
        assert 1 <= proof["gamma"] < 1 << 128 and 1 <= proof["z"] < 1 << 128
    # a row whose set holds more points than it has coefficients contributes no quotient
    n, sets = 2, [[1, 2, 3], [4, 5]]
    proof = km.prove([_poly(n) for _ in sets], sets, TAU)
    assert proof["w_log"] == 0 and proof["l_at_z"] == proof["sum_at_z"]


def _string():
    g1 = o.G1.to_affine(o.G1.one)
    _, (g2, tau_g2) = kr.string(1, TAU)
    return g1, g2, tau_g2


def _other(enc):
    """another point than the one encoded"""
    code, P = ref.decode_g1(enc)
    return ref.encode_g1(kr.g1_add(o.G1.to_affine(P), o.G1.to_affine(o.G1.one)))


def test_model_verifier_accepts_and_rejects():
    g1, g2, tau_g2 = _string()
    for n, sets in _cases()[:2] + [(4, [[5, 6], [7], [6, 5]])]:
        rows = [_poly(n) for _ in sets]
        proof = km.prove(rows, sets, TAU)
        cs, ys, w, w2 = proof["commitments"], proof["values"], proof["w"], proof["w2"]
        assert km.verify(g1, g2, tau_g2, km.opening_bytes(cs, sets, ys, w, w2)), (n, sets)
        bumped = [list(row) for row in ys]
        bumped[-1][0] = (bumped[-1][0] + 1) % R
        moved = [list(s) for s in sets]
        moved[0][0] = (moved[0][0] + 1) % R
        bad = [
            km.opening_bytes(cs, sets, bumped, w, w2),                          # a value
            km.opening_bytes([_other(cs[0])] + cs[1:], sets, ys, w, w2),        # a commitment
            km.opening_bytes(cs, sets, ys, _other(w), w2),                      # W
            km.opening_bytes(cs, sets, ys, w, _other(w2)),                      # W'
        ]
        if n > 1:                                           # (a constant opens alike everywhere, with W = W' = O)
            bad.append(km.opening_bytes(cs, moved, ys, w, w2))                  # a point
            bad.append(km.opening_bytes(cs, sets, ys, w2, w))                   # W and W' swapped
        for b in bad:
            assert not km.verify(g1, g2, tau_g2, b), (n, sets)
    # the sets of two rows swapped, values with them
    n, sets = 4, [[5, 6], [7]]
    proof = km.prove([_poly(n) for _ in sets], sets, TAU)
    swapped = km.opening_bytes(proof["commitments"], sets[::-1], proof["values"][::-1], proof["w"], proof["w2"])
    assert not km.verify(g1, g2, tau_g2, swapped)
    # every row its own interpolant: W = W' = O is accepted, and O for one of them alone is not
    inf = ref.encode_g1(o.G1.to_affine(o.G1.zero))
    proof = km.prove([_poly(1), _poly(1)], [[3], [4]], TAU)
    assert (proof["w"], proof["w2"]) == (inf, inf)
    assert km.verify(g1, g2, tau_g2, km.opening_of(proof, [[3], [4]]))
    proof = km.prove([_poly(3), _poly(3)], [[3], [4]], TAU)
    args = (proof["commitments"], [[3], [4]], proof["values"])
    assert not km.verify(g1, g2, tau_g2, km.opening_bytes(*args, proof["w"], inf))
    assert not km.verify(g1, g2, tau_g2, km.opening_bytes(*args, inf, proof["w2"]))


# ---------------------------------------------------------------------------- bytes
def _fields():
    g = o.G1.to_affine(o.G1.one)
    cs = [ref.encode_g1(kr.g1_mul(g, 11 + i)) for i in range(3)]
    sets, values = [[3], [4, 5, 6], [5, 4]], [[40], [41, 42, 43], [44, 45]]
    return cs, sets, values, ref.encode_g1(kr.g1_mul(g, 21)), ref.encode_g1(kr.g1_mul(g, 22))


def test_multi_opening_bytes_round_trip_and_failures():
    from octopuszk_amd import kzg
    cs, sets, values, w, w2 = _fields()
    b = km.opening_bytes(cs, sets, values, w, w2)
    op = kzg.MultiOpening.from_bytes(b)
    assert (list(op.commitments), [list(s) for s in op.point_sets], [list(v) for v in op.values], op.w, op.w2) == (
        cs, sets, values, w, w2)
    assert op.to_bytes() == b and op.k == 3 and len(b) == 4 + 3 * 36 + 64 * 6 + 64
    assert km.parse_opening(kzg.MultiOpening(cs, sets, values, w, w2).to_bytes()) == (cs, sets, values, w, w2)
    inf = ref.encode_g1(o.G1.to_affine(o.G1.zero))
    assert kzg.MultiOpening.from_bytes(km.opening_bytes(cs, sets, values, inf, inf)).w2 == kzg._G1_INF
    big = kzg.MultiOpening([cs[0]] * 256, [list(range(32))] * 256, [[0] * 32] * 256, w, w2)
    assert kzg.MultiOpening.from_bytes(big.to_bytes()).to_bytes() == big.to_bytes()

    def with_k(k):
        return k.to_bytes(4, "little") + b[4:]

    def with_t0(t):
        return b[:36] + t.to_bytes(4, "little") + b[40:]

    for bad in (b[:-1], b + b"\x00", b[:3], b[:39], b[:4 + 36 + 63], with_k(2), b[:-64], b[:-32]):
        with pytest.raises(ValueError, match="multi opening: length"):
            kzg.MultiOpening.from_bytes(bad)
    for bad in (with_k(4), with_t0(2), b[:4 + 100] + b[-64:]):     # a count that disagrees with what follows
        with pytest.raises(ValueError, match="multi opening: "):
            kzg.MultiOpening.from_bytes(bad)
    for k in (0, 257, 1 << 31):
        with pytest.raises(ValueError, match="multi opening: K = "):
            kzg.MultiOpening.from_bytes(with_k(k))
    for t in (0, 33, 1 << 31):
        with pytest.raises(ValueError, match="multi opening: t = "):
            kzg.MultiOpening.from_bytes(with_t0(t))
    z0, y0 = 4 + 36, 4 + 36 + 32                                  # row 0's point and value
    with pytest.raises(ValueError, match="multi opening: z is not below r"):
        kzg.MultiOpening.from_bytes(b[:z0] + kr.le(R) + b[z0 + 32:])
    with pytest.raises(ValueError, match="multi opening: y is not below r"):
        kzg.MultiOpening.from_bytes(b[:y0] + kr.le(R + 1) + b[y0 + 32:])
    z1 = 4 + 100 + 36                                             # row 1's first point
    with pytest.raises(ValueError, match="multi opening: z has repeated points"):
        kzg.MultiOpening.from_bytes(b[:z1 + 32] + b[z1:z1 + 32] + b[z1 + 64:])
    no_point = next(kr.le(x) for x in range(2, 50) if ref.decode_g1(kr.le(x))[0] == 3)
    with pytest.raises(ValueError, match=r"multi opening: C\[0\] does not decode"):
        kzg.MultiOpening.from_bytes(b[:4] + no_point + b[36:])
    with pytest.raises(ValueError, match=r"multi opening: C\[1\] does not decode"):
        kzg.MultiOpening.from_bytes(b[:104] + no_point + b[136:])
    with pytest.raises(ValueError, match="multi opening: W does not decode"):
        kzg.MultiOpening.from_bytes(b[:-64] + kr.le(o.Q) + b[-32:])
    with pytest.raises(ValueError, match="multi opening: W' does not decode"):
        kzg.MultiOpening.from_bytes(b[:-32] + no_point)
    # the same points in two rows are no repetition
    assert kzg.MultiOpening.from_bytes(km.opening_bytes(cs, [[3], [3, 4, 5], [4, 3]], values, w, w2)).k == 3
    # the constructor holds the same rules
    enc = cs[0]
    for args, what in ((([[R]], [[0]]), "multi opening: z"), (([[0]], [[R]]), "multi opening: y"),
                       (([[1, 1]], [[0, 0]]), "repeated"), (([[]], [[]]), "t = 0"),
                       (([list(range(33))], [[0] * 33]), "t = 33"), (([[1, 2]], [[0]]), "one per point"),
                       (([[1], [2]], [[0], [0]]), "2 lists of points for 1 rows"), (([3], [[0]]), "not a mix")):
        with pytest.raises(ValueError, match=what):
            kzg.MultiOpening([enc], args[0], args[1], enc, enc)
    with pytest.raises(ValueError, match="K = 0"):
        kzg.MultiOpening([], [], [], enc, enc)
    with pytest.raises(ValueError, match="K = 257"):
        kzg.MultiOpening([enc] * 257, [[1]] * 257, [[0]] * 257, enc, enc)
    with pytest.raises(ValueError, match="multi opening: W': 31 bytes"):
        kzg.MultiOpening([enc], [[1]], [[0]], enc, enc[:31])


# ---------------------------------------------------------------------------- the challenges
GAMMA_PINNED = 0x23e1ba6cce86944bed1a8fbd2dde25e8
Z_PINNED = 0xa6376ff9fc02a2b8aea7b011c70055e3


def test_challenges_match_literal_values():
    from octopuszk_amd import kzg, transcript
    assert (kzg._MULTI_GAMMA_TAG, kzg._MULTI_Z_TAG, kzg._MULTI_RHO_TAG) == (
        b"OZK-kzg-multi-gamma", b"OZK-kzg-multi-z", b"OZK-kzg-multi-rho")
    cs = [kr.le(i + 1) for i in range(2)]
    sets, values, w = [[7], [8, 9]], [[1], [2, 3]], kr.le(5)
    body = ((2).to_bytes(8, "little")
            + (1).to_bytes(8, "little") + kr.le(7) + cs[0] + kr.le(1)
            + (2).to_bytes(8, "little") + kr.le(8) + kr.le(9) + cs[1] + kr.le(2) + kr.le(3))
    d = hashlib.sha256(b"OZK-kzg-multi-gamma" + body).digest()
    gamma = int.from_bytes(d[:16], "little") or 1
    z = int.from_bytes(hashlib.sha256(b"OZK-kzg-multi-z" + d + w).digest()[:16], "little") or 1
    assert kzg.multi_challenges(cs, sets, values, w) == (gamma, z) == km.challenges(cs, sets, values, w)
    assert (gamma, z) == (GAMMA_PINNED, Z_PINNED)
    # the order of a set's points, and of the rows, is part of the transcript
    assert kzg.multi_challenges(cs, [[7], [9, 8]], [[1], [3, 2]], w)[0] != gamma
    assert kzg.multi_challenges(cs, sets, values, kr.le(6)) == (gamma, kzg.multi_challenges(cs, sets, values, kr.le(6))[1])
    assert kzg.multi_challenges(cs, sets, values, kr.le(6))[1] != z
    seed = bytes(range(32))
    got = kr.ints(transcript.weights(seed, 5, kzg._MULTI_RHO_TAG))
    assert got == km.rho(seed, 5) and got != ks.rho(seed, 5)
    for args, what in (((cs, [[7]], values, w), "1 lists of points for 2 rows"), ((cs, sets, [[1], [2]], w), "one per point"),
                       ((cs, sets, [[1], [2, R]], w), r"\[0, r\)"), ((cs, [[7], [8, 8]], values, w), "repeated"),
                       (([cs[0], b"x"], sets, values, w), "commitment: 1 bytes"), ((cs, sets, values, b""), "W: 0 bytes")):
        with pytest.raises(ValueError, match=what):
            kzg.multi_challenges(*args)


def test_host_scalars_match_the_model():
    from octopuszk_amd import kzg
    for n, sets in _cases():
        values = [_poly(len(s)) for s in sets]
        gamma, z = rng.randrange(1, 1 << 128), rng.randrange(1, 1 << 128)
        groups, group_of = kzg._multi_groups([tuple(s) for s in sets])
        assert [len(g) for g in groups] == sorted(len(g) for g in groups)
        assert all(set(groups[g]) == set(s) for g, s in zip(group_of, sets))
        assert len({frozenset(g) for g in groups}) == len(groups) == len(km.group_rows(sets)[0])
        c, weights, total, z_t = kzg._multi_at([tuple(s) for s in sets], values, groups, group_of, gamma, z)
        assert (weights, total, z_t) == km.at_z(sets, values, gamma, z)
        assert weights == [pow(gamma, i, R) * c[g] % R for i, g in enumerate(group_of)]
    # z inside T: no division anywhere
    sets, values = [[5, 6], [7]], [[1, 2], [3]]
    groups, group_of = kzg._multi_groups([tuple(s) for s in sets])
    assert kzg._multi_at([tuple(s) for s in sets], values, groups, group_of, 9, 7)[1:] == km.at_z(sets, values, 9, 7)


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
        self.device = "cpu"

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
    with pytest.raises(TypeError, match="CUDA"):
        ck.open_multi(cpu, [[1]])
    with pytest.raises(TypeError, match="uint8"):
        ck.open_multi(cpu.to(torch.int32), [[1]])
    monkeypatch.setattr(kzg.torch, "Tensor", _Shaped)
    one, two = _Shaped((256,), (1,)), _Shaped((2, 256), (256, 1))
    with pytest.raises(ValueError, match="the key has n = 8"):
        ck.open_multi(_Shaped((64,), (1,)), [[1]])
    with pytest.raises(ValueError, match="multiple of 32"):                     # the row layout
        ck.open_multi(_Shaped((2, 256), (250, 1)), [[1], [2]])
    with pytest.raises(ValueError, match="16-byte aligned"):
        ck.open_multi(_Shaped((256,), (1,), ptr=8), [[1]])
    with pytest.raises(TypeError, match="one list of points per row"):
        ck.open_multi(one, 5)
    with pytest.raises(ValueError, match="not a mix"):
        ck.open_multi(one, [5])
    with pytest.raises(ValueError, match="not a mix"):
        ck.open_multi(two, [[2], 3])
    with pytest.raises(ValueError, match="3 lists of points for 2 rows"):
        ck.open_multi(two, [[2], [3], [5]])
    with pytest.raises(ValueError, match="0 lists of points for 1 rows"):
        ck.open_multi(one, [])
    with pytest.raises(ValueError, match="t = 0 points"):
        ck.open_multi(two, [[2], []])
    with pytest.raises(ValueError, match="t = 33 points: 1 <= t <= 32"):
        ck.open_multi(one, [list(range(33))])
    with pytest.raises(ValueError, match="repeated"):
        ck.open_multi(two, [[2], [3, 7, 3]])
    with pytest.raises(ValueError, match=r"\[0, r\)"):
        ck.open_multi(two, [[2], [3, R]])
    with pytest.raises(ValueError, match=r"\[0, r\)"):
        ck.open_multi(one, [[-1]])
    many = _Shaped((257, 256), (256, 1))
    with pytest.raises(ValueError, match="K = 257 rows: 1 <= K <= 256"):
        ck.open_multi(many, [[1]] * 257)
    rows33 = _Shaped((33, 256), (256, 1))
    with pytest.raises(ValueError, match="33 distinct sets of points: at most 32"):
        ck.open_multi(rows33, [[i + 1] for i in range(33)])
    enc = bytes(32)
    with pytest.raises(ValueError, match="1 commitments for 2 rows"):
        ck.open_multi(two, [[2], [3]], commitments=[enc])
    with pytest.raises(ValueError, match="commitment: 31 bytes"):
        ck.open_multi(two, [[2], [3]], commitments=[enc, enc[:31]])
    # t is not bounded by the string: m = 4 here, and 32 points pass the checks (the values are asked for)
    with pytest.raises(AssertionError, match="the library was reached: ozk_fr_poly_eval_set_workspace_bytes"):
        ck.open_multi(one, [list(range(32))], commitments=[enc])
    # verification
    vk = kzg.VerifyKey(enc, bytes(64), bytes(64))
    for call in (kzg.verify_multi, lambda k, b: kzg.verify_multi_all(k, [b]), lambda k, b: kzg.verify_multi_each(k, [b])):
        with pytest.raises(ValueError, match="multi opening: length"):
            call(vk, bytes(3))
    assert kzg.verify_multi_all(vk, []) and kzg.verify_multi_each(vk, []) == []
