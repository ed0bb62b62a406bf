"""zksnark.Verifier on hardware (ozk_groth16_verify_dev): the verification key's alphaG1betaG2 against the oracle,
SerialProver's and ShardedProver's 2^10 proofs accepted, the five tamperings rejected with the verdict of
pairing_ref.verify, the 2^20 profiler circuit checked with real pairings, and verify_batch over 256 proofs."""
import os

import pytest
import torch

import pairing_ref as pr
from oracle import bn254 as o
from oracle import groth16 as g
from test_pairing_cpu import tamperings

pytestmark = pytest.mark.gpu

NC, NI = 1 << 10, 15


def _aff_g1(b):
    return o.g1_from_out_le(b)


def _aff_g2(b):
    return o.g2_from_out_le(b)


def _to_proof(z, A, B, C):
    return z.Proof(o.g1_out_le(o.G1.to_affine(A)), o.g2_out_le(o.G2.to_affine(B)), o.g1_out_le(o.G1.to_affine(C)))


@pytest.fixture(scope="module")
def setup_2p10():
    from octopuszk_amd import zksnark as z
    r1cs, primary, auxiliary = z.serial_construct(NC, NI)
    crs = z.serial_setup_generate(r1cs)
    vk = z.verification_key(crs)
    prover = z.SerialProver(crs.proving_key)
    try:
        proof = prover.prove(primary, auxiliary)
    finally:
        prover.close()
    r1cs_o, _, _ = g.serial_construct(NC, NI)
    crs_o = g.serial_setup(r1cs_o)
    return crs, vk, primary, auxiliary, proof, crs_o


def test_alpha_beta_equals_the_oracle(setup_2p10):
    crs, vk, _, _, _, crs_o = setup_2p10
    torch.cuda.synchronize()
    assert bytes(vk.alpha_g1_beta_g2.cpu().numpy()) == pr.gt_bytes(pr.reduced_pairing(crs_o.alpha_g1, crs_o.beta_g2))


def test_serial_proof_verifies_and_tamperings_fail(setup_2p10):
    from octopuszk_amd import zksnark as z
    crs, vk, primary, _, proof, crs_o = setup_2p10
    assert z.Verifier.verify(vk, primary, proof) is True
    ab = pr.reduced_pairing(crs_o.alpha_g1, crs_o.beta_g2)
    P = (_aff_g1(proof.g_a), _aff_g2(proof.g_b), _aff_g1(proof.g_c))
    for name, pri, prf in tamperings(primary, P):
        got = z.Verifier.verify(vk, pri, _to_proof(z, *prf))
        assert got is False, name
        assert got == pr.verify(ab, crs_o.gamma_g2, crs_o.delta_g2, crs_o.gamma_abc_g1, pri, prf), name


def test_sharded_proofs_verify(setup_2p10):
    from octopuszk_amd import distributed as D
    from octopuszk_amd import zksnark as z
    from test_sharded_prover_gpu import _run_world
    crs, vk, primary, auxiliary, proof, _ = setup_2p10
    prover = z.ShardedProver(crs.proving_key, 0, 1)
    try:
        p1 = D.distributed_prove(prover, primary, auxiliary, z.SEED, gather=D.all_gather_partials_host)
    finally:
        prover.close()
    assert z.Verifier.verify(vk, primary, p1)
    got = _run_world(2, NC, NI)
    p2 = z.Proof(*got[0]["proof"])
    assert z.Verifier.verify(vk, primary, p2)


def test_verify_batch_256(setup_2p10):
    from octopuszk_amd import zksnark as z
    _, vk, primary, _, proof, _ = setup_2p10
    P = (_aff_g1(proof.g_a), _aff_g2(proof.g_b), _aff_g1(proof.g_c))
    bad = [(pri, _to_proof(z, *prf)) for _, pri, prf in tamperings(primary, P)]
    prims, proofs, mask = [], [], []
    for j in range(256):
        if j % 7 == 3:
            pri, prf = bad[(j // 7) % len(bad)]
            prims.append(pri)
            proofs.append(prf)
            mask.append(False)
        else:
            prims.append(primary)
            proofs.append(proof)
            mask.append(True)
    got = z.Verifier.verify_batch(vk, prims, proofs)
    assert got == mask
    assert [z.Verifier.verify(vk, prims[j], proofs[j]) for j in range(0, 256, 37)] == mask[0:256:37]


def test_2p20_profiler_circuit_verifies():
    """2^20 constraints, 1023 inputs: the full-size proof checked with real pairings, without the setup secrets"""
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
    assert z.Verifier.verify(vk, primary, proof)
    C = o.G1.add(_aff_g1(proof.g_c), o.G1.one)
    bad = z.Proof(proof.g_a, proof.g_b, o.g1_out_le(o.G1.to_affine(C)))
    assert not z.Verifier.verify(vk, primary, bad)
