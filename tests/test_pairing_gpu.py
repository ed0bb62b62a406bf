"""ozk_reduced_pairing_dev / ozk_pairing_g2_prepare_dev on hardware against tests/pairing_ref.py: bytes of 32 pairs
(random, infinity on either side, Z != 1), prepared against inline G2 steps, and batches of 1 .. 4097 pairs."""
import random

import pytest
import torch

import pairing_ref as pr
from oracle import bn254 as o
from test_pairing_cpu import g2_flat, pairing_cases

pytestmark = pytest.mark.gpu


def _dev(points, flat=lambda P: P):
    b = b"".join(int(v).to_bytes(32, "little") for P in points for v in flat(P))
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _gt(t, n):
    raw = bytes(t.cpu().numpy())
    return [raw[384 * i:384 * (i + 1)] for i in range(n)]


def test_32_pairs_bytes_equal_the_oracle_prepared_and_inline():
    from octopuszk_amd import pairing as pa
    cases = pairing_cases(29, 29)
    assert len(cases) == 32
    P = _dev([c[0] for c in cases])
    Qd = _dev([c[1] for c in cases], g2_flat)
    inline = pa.reduced_pairing(P, Qd)
    prepared = pa.reduced_pairing(P, pa.prepare_g2(Qd))
    torch.cuda.synchronize()
    want = [pr.reduced_pairing_bytes(p, q) for p, q in cases]
    assert _gt(inline, 32) == want
    assert _gt(prepared, 32) == want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_batches(n):
    """position j pairs (P_i, Q_i), (a P_i, Q_i) or (P_i, a Q_i) for i = (j / 3) % 8: every position is checked
    against the oracle's value of its pair, the same pair gives the same bytes wherever it sits, and
    e(aP, Q) = e(P, aQ) with both sides from the device"""
    from octopuszk_amd import pairing as pa
    rng = random.Random(n)
    a = rng.randrange(2, o.R)
    base = [(o.G1.mul(o.G1.one, rng.randrange(1, o.R)), o.G2.mul(o.G2.one, rng.randrange(1, o.R))) for _ in range(8)]
    kinds = [(P, Qp) for P, Qp in base] + [(o.G1.mul(P, a), Qp) for P, Qp in base] + [(P, o.G2.mul(Qp, a)) for P, Qp in base]
    idx = [(j % 3) * 8 + (j // 3) % 8 for j in range(n)]
    got = _gt(pa.reduced_pairing(_dev([kinds[k][0] for k in idx]), _dev([kinds[k][1] for k in idx], g2_flat)), n)
    torch.cuda.synchronize()
    want = {}
    for k in sorted(set(idx)):
        want[k] = pr.reduced_pairing_bytes(*kinds[k]) if k < 16 or k - 8 not in want else want[k - 8]
    for j in range(n):
        assert got[j] == want[idx[j]], j
    firsts = {}
    for j, k in enumerate(idx):
        firsts.setdefault(k, got[j])
        assert got[j] == firsts[k]
    for i in range(8):
        if 8 + i in firsts and 16 + i in firsts:
            assert firsts[8 + i] == firsts[16 + i]   # e(aP, Q) == e(P, aQ), both from the device
