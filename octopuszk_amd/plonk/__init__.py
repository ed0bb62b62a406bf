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
a proof is zero-knowledge only under a key of setup(zk=True) (below; the KZG layer itself is non-hiding).

Lookups: one table of three-column tuples, logUp as a running sum beside the grand product.

    b.table([(x, y, x ^ y) for x in range(16) for y in range(16)])      # once per builder
    b.lookup(u, v, w)                                # (u, v, w) is a row of the table: one row, every selector 0
    circuit = b.build()                              # a plonk.LookupCircuit; n is also at least the table's length
    pk, vk = plonk.setup(circuit, commit_key)        # 12 commitments, 392 bytes; pk keeps a 14 x 4n coset table
    proof = plonk.prove(pk, assignment)              # a LookupProof, 1088 bytes; ValueError names a row not in the table
    assert plonk.verify(vk, kzg_vk, public_inputs, proof)

setup, prove and verify dispatch on the type of the circuit or key; the transcript of a proof with lookups has tags of
its own, so neither kind of proof can be read as the other.

Import of R1CS: an R1CS in CSR form (A, B, C with ptr, index, value; num_inputs, num_auxiliary:
the shape of zksnark.R1CSRelation) compiles to a vanilla circuit, one gate a constraint and one addition gate for
every term of a linear combination past its first.

    circuit = plonk.from_r1cs(r1cs)                  # a plonk.R1CSCircuit; n_public = num_inputs, the leading one included
    pk, vk = plonk.setup(circuit, commit_key)        # a plonk.R1CSProvingKey and an ordinary VerifyingKey
    proof = plonk.prove(pk, full)                    # the R1CS assignment: ints, bytes, or a uint8 CUDA tensor
    assert plonk.verify(vk, kzg_vk, primary, proof)

An assignment that is already on the device (a uint8 CUDA tensor of 32-byte records, for any circuit) never visits the
host: the wire columns are gathered there, and for an imported R1CS the chains' running sums are computed there.

Zero knowledge: a key over ZK_PAD = 8 more bases blinds every polynomial the prover commits to by
a multiple of Z_H, and the quotient's parts by terms that cancel; verifying key, proof bytes and verifier are the same.

    pk, vk = plonk.setup(circuit, kzg.CommitKey.from_srs(srs, circuit.n + plonk.ZK_PAD), zk=True)     # n >= 8
    proof = plonk.prove(pk, assignment)              # 13 blinders (18 with lookups) from secrets.randbelow
    assert plonk.verify(vk, kzg_vk, public_inputs, proof)               # vk: byte for byte the one of zk=False

Many proofs of one circuit: K proofs under one key, one pairing product whatever K is.

    assert plonk.verify_all(vk, kzg_vk, public_rows, proofs)            # objects, bytes, or K x 800 bytes on the device
    verdicts = plonk.verify_each(vk, kzg_vk, public_rows, proofs)       # singles only when the batch check fails

Out of scope: the linearisation polynomial, mixed keys in one batch, custom gates, several tables, tables wider than three columns,
lookups in an imported R1CS.  There is no CPU path.
"""
from .circuit import Builder, Circuit, LookupCircuit, R1CSCircuit, from_r1cs
from .protocol import (BATCH_STAGES, LOOKUP_PROOF_BYTES, LOOKUP_STAGES, LOOKUP_VK_BYTES, PROOF_BYTES, LookupProof, LookupProvingKey,
                       LookupVerifyingKey, Proof, ProvingKey, R1CSProvingKey, VerifyingKey, ZK_BLINDERS, ZK_LOOKUP_BLINDERS,
                       ZK_PAD, challenges, lookup_challenges, prove, setup, verify, verify_all, verify_each)

__all__ = ["BATCH_STAGES", "Builder", "Circuit", "LookupCircuit", "LOOKUP_PROOF_BYTES", "LOOKUP_STAGES", "LOOKUP_VK_BYTES", "LookupProof",
           "LookupProvingKey", "LookupVerifyingKey", "PROOF_BYTES", "Proof", "ProvingKey", "R1CSCircuit", "R1CSProvingKey",
           "VerifyingKey", "ZK_BLINDERS", "ZK_LOOKUP_BLINDERS", "ZK_PAD", "challenges", "from_r1cs", "lookup_challenges", "prove", "setup", "verify", "verify_all", "verify_each"]
