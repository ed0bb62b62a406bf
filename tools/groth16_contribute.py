#!/usr/bin/env python3
"""Contribute to a saved Groth16 key, or measure a contribution.

    python tools/groth16_contribute.py IN.ozkpk IN.vk OUT.ozkpk OUT.vk OUT.receipt [--previous FILE]
    python tools/groth16_contribute.py --measure LOGN

The first form loads the proving key and the verification key, draws a secret d, writes the key after the
contribution, its verification key and the 296-byte receipt, verifies its own contribution, and forgets d.
--previous names the receipt of the contribution before this one (none: this is the first).

--measure runs on a fresh key of 2^LOGN constraints (15 inputs): setup, contribute, verify the contribution, prove
with the new key, verify that proof.  It prints one JSON line: the time of every scale_points call of the
contribution, the stage times of verify_contribution, the number of points scaled and the SHA-256 of the new key
file, and exits non-zero unless the proof verifies under the new verification key and is rejected under the old."""
import hashlib
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _timed_scale(ceremony, log):
    """scale_points with every call timed (device time, a synchronise on both sides)"""
    inner = ceremony.scale_points

    def scale_points(points, k, type_):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = inner(points, k, type_)
        torch.cuda.synchronize()
        log.append({"type": "G1" if type_ == 1 else "G2", "points": points.numel() // (96 * type_),
                    "ms": round((time.perf_counter() - t0) * 1e3, 3)})
        return out

    return scale_points


def measure(logn):
    from octopuszk_amd import ceremony
    from octopuszk_amd import zksnark as z
    nc, ni = 1 << logn, 15
    res = {"constraints": nc, "inputs": ni}
    t0 = time.perf_counter()
    r1cs, primary, auxiliary = z.serial_construct(nc, ni)
    crs = z.serial_setup_generate(r1cs)
    pk, vk = crs.proving_key, z.verification_key(crs)
    torch.cuda.synchronize()
    res["setup_s"] = round(time.perf_counter() - t0, 2)
    ceremony.scale_points(pk.delta_g1, 3, 1)                        # loads the code object outside the timed calls
    calls, inner = [], ceremony.scale_points
    ceremony.scale_points = _timed_scale(ceremony, calls)
    try:
        t0 = time.perf_counter()
        pk2, vk2, receipt = ceremony.contribute(pk, vk)
        torch.cuda.synchronize()
        res["contribute_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    finally:
        ceremony.scale_points = inner
    res["scale_points_calls"] = calls
    res["points_scaled"] = sum(c["points"] for c in calls)
    stage_ms, why = {}, []
    t0 = time.perf_counter()
    res["contribution_verified"] = ceremony.verify_contribution(pk, pk2, receipt, vk_before=vk, vk_after=vk2, why=why,
                                                                stage_ms=stage_ms)
    res["verify_contribution_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    res["verify_contribution_stage_ms"] = {k: round(v, 3) for k, v in stage_ms.items()}
    res["why"] = why
    prover = z.SerialProver(pk2)
    proof = prover.prove(primary, auxiliary)
    prover.close()
    res["proof_verifies_under_new_vk"] = bool(z.Verifier.verify(vk2, primary, proof))
    res["proof_rejected_under_old_vk"] = not z.Verifier.verify(vk, primary, proof)
    res["new_key_sha256"] = hashlib.sha256(pk2.to_bytes()).hexdigest()
    print(json.dumps(res))
    ok = res["contribution_verified"] and res["proof_verifies_under_new_vk"] and res["proof_rejected_under_old_vk"]
    return 0 if ok else 1


def contribute(args):
    from octopuszk_amd import ceremony
    from octopuszk_amd import zksnark as z
    previous = b""
    if "--previous" in args:
        i = args.index("--previous")
        with open(args[i + 1], "rb") as f:
            previous = f.read()
        ceremony.Receipt.from_bytes(previous)                       # strict: a broken link is refused here
        args = args[:i] + args[i + 2:]
    if len(args) != 5:
        sys.stderr.write(__doc__)
        return 2
    in_pk, in_vk, out_pk, out_vk, out_receipt = args
    pk = z.ProvingKey.load(in_pk)
    with open(in_vk, "rb") as f:
        vk = z.VerificationKey.from_bytes(f.read())
    pk2, vk2, receipt = ceremony.contribute(pk, vk, previous=previous)
    why = []
    if not ceremony.verify_contribution(pk, pk2, receipt, vk_before=vk, vk_after=vk2, why=why):
        sys.stderr.write("the contribution does not verify: %s\n" % why)
        return 1
    pk2.save(out_pk)
    with open(out_vk, "wb") as f:
        f.write(vk2.to_bytes())
    with open(out_receipt, "wb") as f:
        f.write(receipt.to_bytes())
    print(json.dumps({"receipt_sha256": hashlib.sha256(receipt.to_bytes()).hexdigest(),
                      "points_scaled": (pk.delta_abc_g1.numel() + pk.query_h.numel()) // 96 + 2}))
    return 0


def main():
    args = sys.argv[1:]
    if args[:1] == ["--measure"] and len(args) == 2:
        return measure(int(args[1]))
    return contribute(args)


if __name__ == "__main__":
    sys.exit(main())
