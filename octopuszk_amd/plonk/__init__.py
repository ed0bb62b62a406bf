"""A PLONK prover and verifier over the KZG multi-opening: a universal setup.  Whoever holds a
checked powers-of-tau string and a circuit proves and verifies with no per-circuit secrets.

    b = plonk.Builder()                              # variables, gates, copy constraints by variable identity
    x = b.public(); y = b.var(); out = b.var()
    b.mul(x, y, out)                                 # also add, gate(ql, qr, qo, qm, qc, a, b, c), assert_equal
    circuit = b.build()                              # pads to n = 2^k; also plonk.Circuit(n, selectors, wires, n_public)
    pk, vk = plonk.setup(circuit, commit_key)        # 8 commitments; pk keeps the 10 x 4n coset table on the device
    proof = plonk.prove(pk, assignment)              # one Fr value per variable -> Proof, 800 bytes
    assert plonk.verify(vk, kzg_vk, public_inputs, proof)

Vanilla PLONK over BN254 Fr: three wire columns, the gate qL a + qR b + qO c + qM a b + qC + PI = 0, copy constraints
through one permutation of the 3 n cells (identity labels x, k1 x, k2 x with k1 = 5, k2 = 25).  Two deliberate
simplifications: there is NO linearisation polynomial (the proof opens all fourteen polynomials at z and the grand
product at z and z omega with one CommitKey.open_multi call, eight field elements more than the paper's proof), and
there is NO blinding (the KZG layer is non-hiding: proofs are sound, not zero-knowledge).

Out of scope: blinding, the linearisation polynomial, custom gates, lookups, import of R1CS.  There is no CPU path.
"""
from .circuit import Builder, Circuit
from .protocol import PROOF_BYTES, Proof, ProvingKey, VerifyingKey, challenges, prove, setup, verify

__all__ = ["Builder", "Circuit", "PROOF_BYTES", "Proof", "ProvingKey", "VerifyingKey", "challenges", "prove", "setup",
           "verify"]
