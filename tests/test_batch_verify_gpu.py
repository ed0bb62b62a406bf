"""Randomized batch verification on hardware: pairing products, GT powers and well-formedness flags against the
oracle, Verifier.verify_all over valid batches up to 4097 proofs and over every tampering, the cancelling pair,
verify_batch_rlc against verify_batch, and the 2^20 proof."""
import os
import random

import pytest
import torch

import batch_verify_ref as bv
import pairing_ref as pr
from oracle import bn254 as o
from test_batch_verify_cpu import _g1_out, _g2_out, _jac_g1, _jac_g2, _twist_point
from test_pairing_cpu import tamperings

pytestmark = pytest.mark.gpu

NC, NI = 1 << 10, 15


def _dev(b: bytes):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    torch.cuda.synchronize()
    return bytes(t.cpu().numpy())


def _to_proof(z, A, B, C):
    return z.Proof(o.g1_out_le(o.G1.to_affine(A)), o.g2_out_le(o.G2.to_affine(B)), o.g1_out_le(o.G1.to_affine(C)))


def _points(P):
    return (o.g1_from_out_le(bytes(P.g_a)), o.g2_from_out_le(bytes(P.g_b)), o.g1_from_out_le(bytes(P.g_c)))


@pytest.fixture(scope="module")
def setup():
    from octopuszk_amd import distributed as D
    from octopuszk_amd import zksnark as z
    r1cs, primary, auxiliary = z.serial_construct(NC, NI)
    crs = z.serial_setup_generate(r1cs)
    vk = z.verification_key(crs)
    prover = z.SerialProver(crs.proving_key)
    try:
        proofs = [prover.prove(primary, auxiliary, seed=1000 + i) for i in range(64)]
    finally:
        prover.close()
    sharded = z.ShardedProver(crs.proving_key, 0, 1)
    try:
        proofs.append(D.distributed_prove(sharded, primary, auxiliary, 77, gather=D.all_gather_partials_host))
    finally:
        sharded.close()
    assert len({bytes(p.g_a) for p in proofs}) == 65
    return vk, primary, proofs


def _verdict(z, vk, primaries, proofs, seed):
    """the device check's own verdict and coverage (not the fallback's booleans)"""
    return z.Verifier._rlc(vk, list(primaries), list(proofs), seed)


# ---------------------------------------------------------------------------- pairing products, powers, flags
def _pairs(seed, n):
    rng = random.Random(seed)
    P, Qs = [], []
    for _ in range(n):
        P.append(_jac_g1(rng, o.G1.mul(o.G1.one, rng.randrange(1, o.R))))
        Qs.append(o.G2.mul(o.G2.one, rng.randrange(1, o.R)))
    return P, Qs


def test_pairing_product_small_n_equals_the_oracle():
    from octopuszk_amd import pairing as pa
    P, Qs = _pairs(3, 3)
    for n in (1, 2, 3):
        want = pr.F12_ONE
        for p, q in zip(P[:n], Qs[:n]):
            want = pr.f12_mul(want, pr.reduced_pairing(p, q))
        dp = _dev(b"".join(o.g1_to_wire(p) for p in P[:n]))
        dq = _dev(b"".join(o.g2_to_wire(q) for q in Qs[:n]))
        assert _host(pa.pairing_product(dp, dq)) == pr.gt_bytes(want), n
        assert _host(pa.pairing_product(dp, pa.prepare_g2(dq))) == pr.gt_bytes(want), n


@pytest.mark.parametrize("n", [64, 4097])
def test_pairing_product_equals_the_product_of_device_pairings(n):
    from octopuszk_amd import device as dev
    from octopuszk_amd import pairing as pa
    P = dev.gen_g1_bases(n, seed=n)
    rng = random.Random(n)
    qs = [o.G2.to_affine(o.G2.mul(o.G2.one, rng.randrange(1, o.R))) for _ in range(8)]
    dq = _dev(b"".join(o.g2_to_wire(qs[i % 8]) for i in range(n)))
    gts = _host(pa.reduced_pairing(P, dq))
    want = pr.F12_ONE
    for i in range(n):
        want = pr.f12_mul(want, pr.gt_from_bytes(gts[384 * i:384 * i + 384]))
    assert _host(pa.pairing_product(P, dq)) == pr.gt_bytes(want)


def test_gt_pow_equals_the_cyclotomic_exponentiation():
    from octopuszk_amd import pairing as pa
    P, Qs = _pairs(5, 4)
    gts = [pr.reduced_pairing(p, q) for p, q in zip(P, Qs)]
    rng = random.Random(9)
    exps = [0, 1, o.R, (1 << 256) - 1, rng.randrange(1 << 145), rng.randrange(1 << 256), 2, o.R - 1]
    src = [gts[i % 4] for i in range(len(exps))]
    got = _host(pa.gt_pow(_dev(b"".join(pr.gt_bytes(a) for a in src)), exps))
    for i, (a, e) in enumerate(zip(src, exps)):
        want = pr.f12_cyclotomic_exp(a, e) if e else pr.F12_ONE
        assert got[384 * i:384 * i + 384] == pr.gt_bytes(want), e


def _mixed_records(seed):
    """records that are well-formed and records that break each rule once"""
    rng = random.Random(seed)
    A = _jac_g1(rng, o.G1.mul(o.G1.one, 5))
    C = _jac_g1(rng, o.G1.mul(o.G1.one, 6))
    B = _jac_g2(rng, o.G2.mul(o.G2.one, 7))
    good = (_g1_out(A), _g2_out(B), _g1_out(C))
    bad_b = _g2_out(_jac_g2(rng, _twist_point(rng)))
    off_a = _g1_out((A[0], (A[1] + 1) % o.Q, A[2]))
    big = bytearray(good[0])
    big[40] ^= 0xFF   # upper half of X
    recs = [b"".join(good),
            off_a + good[1] + good[2],
            good[0] + bad_b + good[2],
            good[0] + _g2_out(((0, 0), (1, 0), (0, 0))) + good[2],
            good[0] + good[1] + _g1_out((0, 1, 0)),
            bytes(big) + good[1] + good[2],
            good[0] + _g2_out((B[0], B[1], (0, 0))) + good[2],
            good[2] + good[1] + good[0]]
    return recs


def test_flags_equal_the_oracle(setup):
    from octopuszk_amd import pairing as pa
    from octopuszk_amd import zksnark as z
    _, _, proofs = setup
    recs = _mixed_records(13) + [z.proof_record(p) for p in proofs[:5]]
    got = pa.wellformed(_dev(b"".join(recs))).cpu().tolist()
    want = [int(bv.record_wellformed(r)) for r in recs]
    assert got == want
    assert want[:8] == [1, 0, 0, 0, 0, 0, 0, 1] and want[8:] == [1] * 5


# ---------------------------------------------------------------------------- verify_all
def test_verify_all_accepts_valid_batches(setup):
    from octopuszk_amd import zksnark as z
    vk, primary, proofs = setup
    for k in (1, 2, 63, 64, 65):
        assert z.Verifier.verify_all(vk, [primary] * k, proofs[:k], seed=k) is True, k
        assert _verdict(z, vk, [primary] * k, proofs[:k], k) == (1, [True] * k), k
    assert z.Verifier.verify_all(vk, [primary], [proofs[64]]) is True     # the sharded proof, secrets weights
    assert _verdict(z, vk, [primary], [proofs[64]], None) == (1, [True])
    k = 4097
    batch = [proofs[i % 65] for i in range(k)]
    assert z.Verifier.verify_all(vk, [primary] * k, batch, seed=1) is True
    assert _verdict(z, vk, [primary] * k, batch, 1) == (1, [True] * k)


def test_each_tampering_anywhere_rejects(setup):
    from octopuszk_amd import zksnark as z
    vk, primary, proofs = setup
    bad = [(name, pri, _to_proof(z, *prf)) for name, pri, prf in tamperings(primary, _points(proofs[0]))]
    for name, pri, prf in bad:
        for pos in (0, 128, 255):
            prims = [primary] * 256
            batch = [proofs[i % 65] for i in range(256)]
            prims[pos], batch[pos] = pri, prf
            assert z.Verifier.verify_all(vk, prims, batch, seed=pos) is False, (name, pos)
            assert _verdict(z, vk, prims, batch, pos) == (0, [True] * 256), (name, pos)


def test_cancelling_pair_rejects(setup):
    from octopuszk_amd import zksnark as z
    vk, primary, proofs = setup
    pair = [_to_proof(z, *p) for p in bv.cancelling_pair(_points(proofs[0]))]
    assert z.Verifier.verify_batch(vk, [primary] * 2, pair) == [False, False]
    assert z.Verifier.verify_all(vk, [primary] * 2, pair, seed=3) is False
    assert z.Verifier.verify_all(vk, [primary] * 4, proofs[1:3] + pair, seed=4) is False
    assert _verdict(z, vk, [primary] * 2, pair, 3) == (0, [True, True])
    assert _verdict(z, vk, [primary] * 4, proofs[1:3] + pair, 4) == (0, [True] * 4)


def test_same_seed_same_verdict(setup):
    from octopuszk_amd import zksnark as z
    vk, primary, proofs = setup
    for _ in range(2):
        assert z.Verifier.verify_all(vk, [primary] * 8, proofs[:8], seed=99) is True
    assert z.Verifier._rlc(vk, [primary] * 8, proofs[:8], 99) == z.Verifier._rlc(vk, [primary] * 8, proofs[:8], 99)


def test_bad_arguments_raise(setup):
    from octopuszk_amd import zksnark as z
    vk, primary, proofs = setup
    bad0 = list(primary)
    bad0[0] = 2
    with pytest.raises(ValueError):
        z.Verifier.verify_all(vk, [bad0], proofs[:1])
    with pytest.raises(ValueError):
        z.Verifier.verify_all(vk, [primary] * 2, proofs[:3])
    with pytest.raises(ValueError):
        z.Verifier.verify_all(vk, [], [])
    with pytest.raises(ValueError):
        z.Verifier.verify_batch_rlc(vk, [primary[:-1]], proofs[:1])


# ---------------------------------------------------------------------------- verify_batch_rlc
def test_verify_batch_rlc_equals_verify_batch_on_the_256_mix(setup):
    from octopuszk_amd import zksnark as z
    vk, primary, proofs = setup
    bad = [(pri, _to_proof(z, *prf)) for _, pri, prf in tamperings(primary, _points(proofs[0]))]
    prims, batch = [], []
    for j in range(256):
        if j % 7 == 3:
            pri, prf = bad[(j // 7) % len(bad)]
        else:
            pri, prf = primary, proofs[j % 65]
        prims.append(pri)
        batch.append(prf)
    want = z.Verifier.verify_batch(vk, prims, batch)
    assert want.count(False) == len(range(3, 256, 7))
    assert z.Verifier.verify_batch_rlc(vk, prims, batch, seed=5) == want


def test_verify_batch_rlc_with_malformed_proofs(setup):
    from octopuszk_amd import zksnark as z
    vk, primary, proofs = setup
    A, B, C = _points(proofs[0])
    rng = random.Random(17)
    Ax, Ay, Az = o.G1.to_affine(A)
    malformed = [
        z.Proof(o.g1_out_le((Ax, (Ay + 1) % o.Q, 1)), proofs[0].g_b, proofs[0].g_c),         # A off the curve
        z.Proof(proofs[0].g_a, _g2_out(_twist_point(rng)), proofs[0].g_c),                     # B outside G2
        z.Proof(proofs[0].g_a, _g2_out(((0, 0), (1, 0), (0, 0))), proofs[0].g_c),              # B at infinity
    ]
    batch = proofs[:10] + malformed + proofs[10:20]
    prims = [primary] * len(batch)
    want = z.Verifier.verify_batch(vk, prims, batch)
    assert want == [True] * 10 + [False] * 3 + [True] * 10
    assert z.Verifier.verify_batch_rlc(vk, prims, batch, seed=6) == want
    assert z.Verifier.verify_all(vk, prims, batch, seed=6) is False
    assert _verdict(z, vk, prims, batch, 6) == (1, [True] * 10 + [False] * 3 + [True] * 10)
    assert z.Verifier.verify_all(vk, prims[:10] + prims[13:], proofs[:20], seed=6) is True


def test_2p20_proof_batch_verifies():
    """2^20 constraints, 1023 inputs: accepted, and rejected with C + G"""
    from octopuszk_amd import zksnark as z
    logn = int(os.environ.get("OZK_TEST_GROTH16_LOGN", "20"))
    r1cs, primary, auxiliary = z.serial_construct(1 << logn, 1023)
    crs = z.serial_setup_generate(r1cs)
    vk = z.verification_key(crs)
    prover = z.SerialProver(crs.proving_key)
    try:
        proof = prover.prove(primary, auxiliary)
    finally:
        prover.close()
    assert z.Verifier.verify_all(vk, [primary], [proof], seed=1) is True
    assert _verdict(z, vk, [primary], [proof], 1) == (1, [True])
    assert z.Verifier.verify_all(vk, [primary] * 3, [proof] * 3) is True
    C = o.G1.add(o.g1_from_out_le(bytes(proof.g_c)), o.G1.one)
    bad = z.Proof(proof.g_a, proof.g_b, o.g1_out_le(o.G1.to_affine(C)))
    assert z.Verifier.verify_all(vk, [primary, primary], [proof, bad], seed=2) is False
    assert _verdict(z, vk, [primary, primary], [proof, bad], 2) == (0, [True, True])
    assert z.Verifier.verify_batch_rlc(vk, [primary, primary], [proof, bad], seed=2) == [True, False]


def test_numpy_object_rows_are_checked_against_their_own_inputs(setup):
    """rows of a numpy object array are temporaries: a proof submitted against other inputs must still fail"""
    import numpy as np
    from octopuszk_amd import zksnark as z
    vk, primary, proofs = setup
    other = list(primary)
    other[1] = (other[1] + 1) % o.R
    arr = np.array([primary, primary, other, primary, other], dtype=object)
    batch = proofs[:5]
    want = z.Verifier.verify_batch(vk, [list(r) for r in arr], batch)
    assert want == [True, True, False, True, False]
    assert z.Verifier.verify_batch_rlc(vk, arr, batch, seed=8) == want
    assert z.Verifier.verify_all(vk, arr, batch, seed=8) is False
    assert z.Verifier.verify_all(vk, (list(r) for r in arr[[0, 1, 3]]), (p for p in proofs[:3]), seed=9) is True
    assert _verdict(z, vk, arr, batch, 8)[0] == 0

