"""GPU tests of KZG openings at every coset at once (octopuszk_amd/kzg.py OpenAllKey) over a string
of known tau: every proof is [q_k(tau)] g1 for the quotient of the integer model (tests/kzg_all_ref.py, which
tests/test_kzg_all_cpu.py holds against the direct definition), byte for byte, and equals the pi of the single
openings CommitKey.open / open_set give; the values are Horner's; the openings pass the existing verifiers unchanged.
The largest transform is 128 points."""
import functools
import random

import pytest

import kzg_all_ref as ka
import kzg_ref as kr
import srs_gpu_util as u
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

R = o.R
TAU = 0x5eed0123456789abcdef0123456789abcdef0123456789abcdef % R
M = 512                        # as tests/test_kzg_set_gpu.py: 1025 powers in G1, 512 in G2
COSETS = (1, 2, 4, 8, 16, 32)
SHAPES = [(n, l) for n in (2, 4, 16, 64) for l in sorted({1, 2, 4, 8, 32, n}) if l <= n and l in COSETS]
PAD = 3                        # elements between two rows of a padded tensor


@pytest.fixture(scope="module")
def string():
    from octopuszk_amd import kzg, srs
    s = srs.Srs.from_secrets(M, TAU, 1, 1, generator=1)
    return s, kzg.VerifyKey.from_srs(s), kzg.SetVerifyKey.from_srs(s, 32)


@functools.lru_cache(maxsize=None)
def _rows(n, l):
    """(label, the row as written, the row reduced): random, zero, constant, degree exactly l - 1 and exactly l, and a
    random row with one coefficient written as p + r"""
    rng = random.Random(1000 * n + l)
    rnd = [rng.randrange(R) for _ in range(n)]
    out = [("random", rnd), ("zero", [0] * n), ("constant", [rng.randrange(1, R)] + [0] * (n - 1))]
    out.append(("degree l - 1", [rng.randrange(1, R) for _ in range(l)] + [0] * (n - l)))
    if l < n:
        out.append(("degree l", [rng.randrange(1, R) for _ in range(l + 1)] + [0] * (n - l - 1)))
    written = [rng.randrange(R) for _ in range(n)]
    written[n // 2] += R                                                  # p + r < 2^255 fits the 32 bytes
    out.append(("a coefficient written as p + r", written))
    return tuple((label, tuple(row), tuple(c % R for c in row)) for label, row in out)


def _dev_rows(rows, pad=0):
    """K rows as a [K, 32 n] view of a tensor whose rows lie n + pad elements apart"""
    n = len(rows[0])
    flat = [v for row in rows for v in list(row) + [R - 1] * pad]
    return u.dev(b"".join(kr.le(v) for v in flat)).view(len(rows), -1)[:, :32 * n]


def _single_proofs(ck, d_row, n, l, ks):
    """the pi of CommitKey.open / open_set of the one row at omega^k / S_k, k in ks"""
    if l == 1:
        return [op.pi for op in ck.open_many_points(d_row, [pow(kr.root(n), k, R) for k in ks])]
    return [op.pi for op in ck.open_set(d_row.unsqueeze(0).repeat(len(ks), 1), [ka.coset(n, l, k) for k in ks])]


@pytest.mark.parametrize("n,l", SHAPES)
def test_open_all(string, n, l):
    from octopuszk_amd import kzg
    s, vk, svk = string
    r = n // l
    ck = kzg.CommitKey.from_srs(s, n)
    key = kzg.OpenAllKey.from_srs(s, n, coset=l, commit_key=ck)
    assert (key.n, key.coset, key.cosets) == (n, l, r)
    rows = _rows(n, l)
    got = key.open_all(_dev_rows([written for _, written, _ in rows], PAD))
    assert len(got) == len(rows)
    # every proof and every commitment against the model, in one batch of expected encodings
    logs = []
    for _, _, p in rows:
        logs += [kr.horner(p, TAU)] + ka.model(list(p), l, TAU)[0]
    want = u.expected(1, logs)
    ks = list(range(r)) if n <= 16 else sorted({0, 1, r - 1})
    for y, ((label, written, p), a) in enumerate(zip(rows, got)):
        enc = want[32 * (r + 1) * y:32 * (r + 1) * (y + 1)]
        assert a.c == enc[:32], label
        assert u.host(a.proofs) == enc[32:], label
        assert kr.ints(u.host(a.values)) == ka.values(list(p)), label
        assert (a.n, a.coset, a.cosets) == (n, l, r)
        # the proofs of the single openings there were
        single = _single_proofs(ck, _dev_rows([written])[0], n, l, ks)
        assert [u.host(a.proofs)[32 * k:32 * k + 32] for k in ks] == single, label
        # the existing verifiers, unchanged
        ops = [a.opening(k) for k in range(r)]
        if l == 1:
            assert all(isinstance(op, kzg.Opening) for op in ops) and kzg.verify_all(vk, ops, bytes(range(32))), label
        else:
            assert all(isinstance(op, kzg.SetOpening) for op in ops), label
            assert [op.points for op in ops] == [tuple(ka.coset(n, l, k)) for k in range(r)]
            assert kzg.verify_set_all(svk, ops, bytes(range(32))), label
    assert got[1].c == kzg._G1_INF and u.host(got[1].proofs) == kzg._G1_INF * r             # the zero row
    assert u.host(got[2].proofs) == kzg._G1_INF * r                                         # a constant
    assert u.host(got[3].proofs) == kzg._G1_INF * r                                         # degree l - 1
    if l < n:
        assert kzg._G1_INF not in [u.host(got[4].proofs)[32 * k:32 * k + 32] for k in range(r)]   # degree l: q = p_l
    # single verification of the random row's openings, and a changed value
    a = got[0]
    for k in ks:
        op = a.opening(k)
        if l == 1:
            assert kzg.verify(vk, op)
            assert not kzg.verify(vk, kzg.Opening(op.c, op.z, (op.y + 1) % R, op.pi))
        else:
            assert kzg.verify_set(svk, op)
            j = k % l
            bumped = op.values[:j] + ((op.values[j] + 1) % R,) + op.values[j + 1:]
            assert not kzg.verify_set(svk, kzg.SetOpening(op.c, op.points, bumped, op.pi))


def test_three_rows_at_a_padded_stride_equal_the_rows_alone(string):
    from octopuszk_amd import kzg
    s, _, _ = string
    n, l = 16, 4
    rng = random.Random(33)
    key = kzg.OpenAllKey.from_srs(s, n, coset=l)
    rows = [[rng.randrange(R) for _ in range(n)] for _ in range(3)]
    together = key.open_all(_dev_rows(rows, PAD))
    packed = key.open_all(_dev_rows(rows))
    for y in range(3):
        alone = key.open_all(_dev_rows([rows[y]])[0])[0]
        for other in (together[y], packed[y]):
            assert (other.c, u.host(other.values), u.host(other.proofs)) == (alone.c, u.host(alone.values),
                                                                             u.host(alone.proofs))
        assert alone.c == u.expected(1, [kr.horner(rows[y], TAU)])
        assert u.host(alone.proofs) == u.expected(1, ka.model(rows[y], l, TAU)[0])


def test_a_commit_key_of_another_size_is_refused(string):
    from octopuszk_amd import kzg
    s, _, _ = string
    with pytest.raises(ValueError, match="commit key"):
        kzg.OpenAllKey.from_srs(s, 16, coset=2, commit_key=kzg.CommitKey.from_srs(s, 32))
    with pytest.raises(ValueError, match="n = 16"):
        kzg.OpenAllKey.from_srs(s, 16).open_all(u.dev(bytes(32 * 8)))
