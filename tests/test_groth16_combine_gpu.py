"""ozk_groth16_combine_dev (k_groth16_combine): `world` gathered 768-byte partials A_r (G1) | B_r (G2) | C_r (G1) ->
the sharded proof A | B | C in one launch.  Against the oracle's sums and against three ozk_points_sum_dev calls
over the same parts: random records, records that are infinity, P / -P pairs that cancel, equal records (the
doubling branch of the mixed addition)."""
import random

import pytest
import torch

from oracle import bn254 as o

pytestmark = pytest.mark.gpu

WORLDS = [1, 2, 3, 8, 64]


def _points(rng, C, world, case):
    if case == "infinity":
        return [C.zero] * world
    if case == "equal":
        P = C.mul(C.one, rng.randrange(1, 1 << 64))
        return [P] * world
    pts = [C.mul(C.one, rng.randrange(1, 1 << 64)) for _ in range(world)]
    if case == "cancel":   # P_0, -P_0, P_2, -P_2, ...; an odd world ends with infinity
        for i in range(0, world - 1, 2):
            pts[i + 1] = C.negate(pts[i])
        if world % 2:
            pts[-1] = C.zero
    elif case == "some_infinity":
        for i in range(0, world, 3):
            pts[i] = C.zero
    return pts


def _records(world, case, seed):
    rng = random.Random(seed)
    a = _points(rng, o.G1, world, case)
    b = _points(rng, o.G2, world, case)
    c = _points(rng, o.G1, world, case)
    raw = b"".join(o.g1_out_le(o.G1.to_affine(a[k])) + o.g2_out_le(o.G2.to_affine(b[k])) +
                   o.g1_out_le(o.G1.to_affine(c[k])) for k in range(world))
    want = [o.G1.zero, o.G2.zero, o.G1.zero]
    for k in range(world):
        want = [o.G1.add(want[0], a[k]), o.G2.add(want[1], b[k]), o.G1.add(want[2], c[k])]
    want = (o.g1_out_le(o.G1.to_affine(want[0])), o.g2_out_le(o.G2.to_affine(want[1])),
            o.g1_out_le(o.G1.to_affine(want[2])))
    return raw, want


@pytest.mark.parametrize("case", ["random", "infinity", "cancel", "some_infinity", "equal"])
@pytest.mark.parametrize("world", WORLDS)
def test_combine_equals_oracle_and_points_sum(world, case):
    from octopuszk_amd import device as dev
    raw, want = _records(world, case, seed=world * 31 + len(case))
    d_rec = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()
    proof = dev.groth16_combine(d_rec, world)
    got = (proof.g_a, proof.g_b, proof.g_c)
    assert got == want
    if case in ("infinity", "cancel"):
        assert proof.g_a == o.g1_out_le((0, 1, 0)) and proof.g_c == o.g1_out_le((0, 1, 0))
        assert proof.g_b == o.g2_out_le(((0, 0), (1, 0), (0, 0)))
    # the same bytes as three ozk_points_sum_dev calls over the parts
    rec = d_rec.view(world, 768)
    sums = (dev.points_sum(rec[:, :192].contiguous().view(-1), world, 1),
            dev.points_sum(rec[:, 192:576].contiguous().view(-1), world, 2),
            dev.points_sum(rec[:, 576:].contiguous().view(-1), world, 1))
    torch.cuda.synchronize()
    assert tuple(bytes(t.cpu().numpy()) for t in sums) == got


def test_combine_refuses_an_empty_world():
    from octopuszk_amd import lib
    L = lib.load()
    d_rec = torch.zeros(768, dtype=torch.uint8, device="cuda")
    out = torch.zeros(768, dtype=torch.uint8, device="cuda")
    st = int(torch.cuda.current_stream().cuda_stream)
    for world in (0, -1):
        rc = L.ozk_groth16_combine_dev(int(d_rec.data_ptr()), world, int(out.data_ptr()), st)
        assert rc == -1   # OZK_E_INVALID
        assert L.ozk_last_error()
    torch.cuda.synchronize()
    assert not out.any()
