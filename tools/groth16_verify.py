#!/usr/bin/env python3
"""Timing of the device pairing and the Groth16 verifier; prints one JSON line.

    python tools/groth16_verify.py [--quick]

  * reduced pairings / s at n = 1, 1024, 65536 (random pairs, G2 steps inline; median of a few runs);
  * one 2^10-constraint proof (15 inputs): Verifier.verify latency, with the evaluationABC MSM shown separately;
  * Verifier.verify_batch proofs / s at K = 64, 4096 (the ABC MSMs, one per proof, included and shown apart);
  * Verifier.verify_all and verify_batch_rlc (the randomized batch check) at K = 1, 64, 4096, 65536, with the stage
    split of verify_all (upload, combination, MSMs, Miller loops, product tree, final exponentiation), repeated
    copies of the one proof.  `rlc_floor_ok`: verify_all at K = 4096 within 150 ms and >= 20x verify_batch's rate.
The floor the issue sets is 1 M reduced pairings / s at n = 65536; `floor_ok` reports it.  The counted figures are
the Fq multiplications per reduced pairing taken from the code."""
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _points(n, seed):
    from octopuszk_amd import device as dev
    p = dev.gen_g1_bases(n, seed=seed)                 # n x 96 B wire-in G1 (affine, Z = 1)
    return p


def _timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts)


def main():
    quick = "--quick" in sys.argv
    from octopuszk_amd import pairing as pa
    from octopuszk_amd import zksnark as z
    torch.cuda.set_device(0)
    out = {"metric": "groth16_verify"}
    # one G2 point repeated (the G2 generator, wire-in), n G1 points
    g2 = b"".join(int(v).to_bytes(32, "little") for x in z.G2_ONE for v in x)
    res = {}
    for n in ([1, 1024] if quick else [1, 1024, 65536]):
        P = _points(n, 3)
        Qd = torch.frombuffer(bytearray(g2 * n), dtype=torch.uint8).cuda()
        pa.reduced_pairing(P, Qd)
        t = _timed(lambda: pa.reduced_pairing(P, Qd), 3)
        res[str(n)] = {"ms": round(t * 1e3, 3), "pairings_per_s": round(n / t, 1)}
    out["reduced_pairing"] = res
    if not quick:
        out["floor_ok"] = res["65536"]["pairings_per_s"] >= 1e6
    # one proof at 2^10
    r1cs, primary, auxiliary = z.serial_construct(1 << 10, 15)
    crs = z.serial_setup_generate(r1cs)
    vk = z.verification_key(crs)
    prover = z.SerialProver(crs.proving_key)
    proof = prover.prove(primary, auxiliary)
    prover.close()
    assert z.Verifier.verify(vk, primary, proof)
    out["verify_one_ms"] = round(_timed(lambda: z.Verifier.verify(vk, primary, proof), 5) * 1e3, 3)
    out["abc_msm_one_ms"] = round(_timed(lambda: vk.evaluation_abc(primary), 5) * 1e3, 3)
    batch = {}
    for k in ([64] if quick else [64, 4096]):
        prims, proofs = [primary] * k, [proof] * k
        t = _timed(lambda: z.Verifier.verify_batch(vk, prims, proofs), 2)
        t_abc = _timed(lambda: [vk.evaluation_abc(p) for p in prims], 1)
        batch[str(k)] = {"ms": round(t * 1e3, 2), "proofs_per_s": round(k / t, 1), "abc_msm_ms": round(t_abc * 1e3, 2)}
    out["verify_batch"] = batch
    rlc = {}
    for k in ([1, 64] if quick else [1, 64, 4096, 65536]):
        prims, proofs = [primary] * k, [proof] * k
        assert z.Verifier.verify_all(vk, prims, proofs)
        t_all = _timed(lambda: z.Verifier.verify_all(vk, prims, proofs), 3)
        t_rlc = _timed(lambda: z.Verifier.verify_batch_rlc(vk, prims, proofs), 3)
        stages = {}
        z.Verifier.verify_all(vk, prims, proofs, stage_ms=stages)
        rlc[str(k)] = {"verify_all_ms": round(t_all * 1e3, 2), "verify_all_proofs_per_s": round(k / t_all, 1),
                       "verify_batch_rlc_ms": round(t_rlc * 1e3, 2),
                       "stages_ms": {n: round(v, 3) for n, v in stages.items()}}
    out["verify_all"] = rlc
    if not quick:
        t = rlc["4096"]["verify_all_ms"]
        out["rlc_speedup_4096"] = round(rlc["4096"]["verify_all_proofs_per_s"] / batch["4096"]["proofs_per_s"], 1)
        out["rlc_floor_ok"] = t <= 150 and out["rlc_speedup_4096"] >= 20
    print(json.dumps(out))


if __name__ == "__main__":
    main()
