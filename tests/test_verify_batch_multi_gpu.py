"""Verifier.verify_batch with the batched evaluationABC (VerificationKey.evaluation_abc_batch, the shared-base MSM)
on hardware: the points byte for byte against evaluation_abc, and the verdict lists of the three `abc` modes against
each other and against the mask, for the 15-input key and for a 1023-input key (the large-table plan)."""
import pytest
import torch

from oracle import bn254 as o
from test_pairing_cpu import tamperings

pytestmark = pytest.mark.gpu

MODES = ("batched", "per_proof", "auto")


def _to_proof(z, A, B, C):
    return z.Proof(o.g1_out_le(o.G1.to_affine(A)), o.g2_out_le(o.G2.to_affine(B)), o.g1_out_le(o.G1.to_affine(C)))


def _setup(nc, ni):
    from octopuszk_amd import zksnark as z
    r1cs, primary, auxiliary = z.serial_construct(nc, ni)
    crs = z.serial_setup_generate(r1cs)
    vk = z.verification_key(crs)
    prover = z.SerialProver(crs.proving_key)
    try:
        proof = prover.prove(primary, auxiliary)
    finally:
        prover.close()
    P = (o.g1_from_out_le(proof.g_a), o.g2_from_out_le(proof.g_b), o.g1_from_out_le(proof.g_c))
    bad = [(pri, _to_proof(z, *prf)) for _, pri, prf in tamperings(primary, P)]
    return vk, primary, proof, bad


@pytest.fixture(scope="module")
def setup_15():
    return _setup(1 << 10, 15)


@pytest.fixture(scope="module")
def setup_1023():
    # 2^11 constraints, not 2^12: from 7150 key elements the reference's table gives the setup an 11-bit fixed-base
    # window, and 23 windows of 11 bits cover 253 of the 254 scalar bits when the generator's longest coordinate has 253
    # bits (as it has with the fixed seed), which batch_msm_dev refuses (253 = 11 x 23; every other window size
    # rounds up past 254).  2^11 constraints take a 9-bit window.  What is tested here is the key's 1023 inputs.
    return _setup(1 << 11, 1023)


def _mix(setup, k, is_bad):
    vk, primary, proof, bad = setup
    prims, proofs, mask, t = [], [], [], 0
    for j in range(k):
        if is_bad(j):
            pri, prf = bad[t % len(bad)]
            t += 1
            prims.append(pri), proofs.append(prf), mask.append(False)
        else:
            prims.append(primary), proofs.append(proof), mask.append(True)
    return prims, proofs, mask


def test_evaluation_abc_batch_equals_per_proof(setup_15):
    vk, primary, _, bad = setup_15
    rows = [primary] + [pri for pri, _ in bad]
    want = torch.cat([vk.evaluation_abc(row) for row in rows])
    got = vk.evaluation_abc_batch(rows)
    torch.cuda.synchronize()
    assert bytes(got.cpu().numpy()) == bytes(want.cpu().numpy())
    assert bytes(got[:192].cpu().numpy()) != bytes(got[4 * 192:5 * 192].cpu().numpy())   # the tampered input row


def test_verify_batch_256_all_modes(setup_15):
    from octopuszk_amd import zksnark as z
    prims, proofs, mask = _mix(setup_15, 256, lambda j: j % 7 == 3)
    for mode in MODES:
        assert z.Verifier.verify_batch(setup_15[0], prims, proofs, abc=mode) == mask, mode
    with pytest.raises(ValueError):
        z.Verifier.verify_batch(setup_15[0], prims, proofs, abc="other")


def test_verify_batch_4096_all_modes_and_rlc(setup_15):
    from octopuszk_amd import zksnark as z
    prims, proofs, mask = _mix(setup_15, 4096, lambda j: j % 97 == 96)
    assert mask.count(False) == 42
    for mode in MODES:
        assert z.Verifier.verify_batch(setup_15[0], prims, proofs, abc=mode) == mask, mode
    assert z.Verifier.verify_batch_rlc(setup_15[0], prims, proofs, seed=5) == mask


def test_auto_below_the_crossover_is_per_proof():
    from octopuszk_amd import zksnark as z
    vk, primary, proof, bad = _setup(1 << 10, 15)                       # a fresh key: no table yet
    assert z.Verifier.verify_batch(vk, [primary, bad[3][0]], [proof, bad[3][1]]) == [True, False]
    assert vk._multi is None
    k = z.Verifier.ABC_BATCH_CROSSOVER
    assert z.Verifier.verify_batch(vk, [primary] * k, [proof] * k) == [True] * k
    assert vk._multi is not None


def test_1023_inputs_256_proofs(setup_1023):
    from octopuszk_amd import zksnark as z
    vk, primary, _, bad = setup_1023
    assert vk.num_inputs == 1023
    rows = [primary, bad[3][0]]
    want = torch.cat([vk.evaluation_abc(row) for row in rows])
    got = vk.evaluation_abc_batch(rows)
    torch.cuda.synchronize()
    assert bytes(got.cpu().numpy()) == bytes(want.cpu().numpy())
    prims, proofs, mask = _mix(setup_1023, 256, lambda j: j % 7 == 3)
    for mode in MODES:
        assert z.Verifier.verify_batch(vk, prims, proofs, abc=mode) == mask, mode
    assert z.Verifier.verify_batch_rlc(vk, prims, proofs, seed=6) == mask
