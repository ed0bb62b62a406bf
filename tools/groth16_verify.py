#!/usr/bin/env python3
"""Timing of the device pairing and the Groth16 verifier; prints one JSON line.

    python tools/groth16_verify.py [--quick | --multi-only | --compressed-only] [--compressed]

  * reduced pairings / s at n = 1, 1024, 65536 (random pairs, G2 steps inline; median of a few runs);
  * one 2^10-constraint proof (15 inputs): Verifier.verify latency, with the evaluationABC MSM shown separately;
  * Verifier.verify_batch proofs / s at K = 64, 4096 with abc="per_proof" (the ABC MSMs, one per proof, included and
    shown apart: the path of every release before the batched MSM), and at K = 64, 4096, 65536 with abc="batched"
    (`verify_batch_batched`: the ABC stage and the pairing stage apart, device work only, and the table build);
    `batched_speedup_4096` and `batched_floor_ok` (>= 20x at K = 4096); the same two stages for a 1023-input key (2^11 constraints);
  * verify_batch_rlc at K = 4096 with ONE tampered proof, with the batched and with the per-proof fallback;
  * `multi_msm`: device.SharedBaseMsm alone at (n, K) in {15, 1023} x {64, 4096, 65536}: Mscalar-mul/s and GB/s of
    gathered table records (--multi-only prints just this; OZK_MM_WS=7 in the environment forces the 7-bit table);
  * Verifier.verify_all and verify_batch_rlc (the randomized batch check) at K = 1, 64, 4096, 65536, with the stage
    split of verify_all (upload, combination, MSMs, Miller loops, product tree, final exponentiation), repeated
    copies of the one proof.  `rlc_floor_ok`: verify_all at K = 4096 within 150 ms and >= 20x verify_batch's per-proof rate.
  * --compressed: next to every K of the previous item, `compressed`: the device time of
    ozk_groth16_proofs_decompress_dev on K x 128 bytes already in HBM, Verifier.verify_all_bytes (upload of the
    compressed buffer included, like verify_all's upload of the records) against verify_all on Proof objects from the
    same loop, its stage split, and the host time of the Python-integer model (tests/codec_ref.py) decoding a sample of
    256 proofs, scaled to K: a Python-integer baseline, not a tuned host decoder.  --compressed-only prints just the
    verify_all item with this addition.
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


def _random_scalars(k, n, seed):
    """k x n canonical scalars in HBM (top byte below 0x30: < r)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    s = torch.randint(0, 256, (k * n, 32), dtype=torch.uint8, device="cuda", generator=g)
    s[:, 31] %= 0x30
    return s.reshape(-1)


def _multi_msm(quick):
    """device.SharedBaseMsm alone: table build and run times"""
    from octopuszk_amd import device as dev
    res = {}
    for n in (15, 1023):
        bases = _points(n, 7)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        msm = dev.SharedBaseMsm(bases, n)
        torch.cuda.synchronize()
        entry = {"window_bits": msm.window_bits, "windows": msm.windows, "table_mib": round(msm.table_bytes / 2**20, 2),
                 "table_build_ms": round((time.perf_counter() - t0) * 1e3, 3)}
        for k in ([64] if quick else [64, 4096, 65536]):
            sc = _random_scalars(k, n, k)
            msm.run(sc, k)
            t = _timed(lambda: msm.run(sc, k), 5)
            entry[str(k)] = {"ms": round(t * 1e3, 3), "mscalar_mul_per_s": round(n * k / t / 1e6, 2),
                             "gather_gb_per_s": round(n * k * 2 * msm.windows * 64 / t / 1e9, 1)}
            del sc
        res[str(n)] = entry
        del msm
    return res


def _batched_stages(z, pa, vk, prims, proofs):
    """device time of the two stages of verify_batch(abc="batched") on inputs already in HBM"""
    from octopuszk_amd import wire
    k = len(proofs)
    d_rows = wire.dev_bytes(b"".join(wire.le32(p) for p in prims))
    recs = wire.dev_bytes(b"".join(z.proof_record(p) for p in proofs))
    abc = vk.evaluation_abc_batch(prims[:1])   # (the table exists from here on)
    t_abc = _timed(lambda: vk._multi.run(d_rows, k), 5)
    abc = vk._multi.run(d_rows, k)
    t_pair = _timed(lambda: pa.groth16_verify(vk.alpha_g1_beta_g2, vk.gamma_prep, vk.delta_prep, recs, abc), 3)
    return round(t_abc * 1e3, 3), round(t_pair * 1e3, 3)


def _compressed(z, vk, prims, proof, k, t_all):
    """the compressed-proof path at K = k: decoding alone, verify_all_bytes, and the Python-integer baseline"""
    from octopuszk_amd import codec, wire
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import codec_ref
    one = proof.to_bytes()
    assert z.proof_record(z.Proof.from_bytes(one)) == z.proof_record(proof)
    buf = one * k
    d_buf = wire.dev_bytes(buf)
    recs, codes = codec.decompress_proofs(d_buf)
    assert not codes.any().item()
    t_dec = _timed(lambda: codec.decompress_proofs(d_buf), 5)
    assert z.Verifier.verify_all_bytes(vk, prims, buf)
    t_bytes = _timed(lambda: z.Verifier.verify_all_bytes(vk, prims, buf), 3)
    stages = {}
    z.Verifier.verify_all_bytes(vk, prims, buf, stage_ms=stages)
    sample = 256
    t0 = time.perf_counter()
    for _ in range(sample):
        code, rec = codec_ref.proof_record(one)
    t_model = (time.perf_counter() - t0) / sample
    assert code == 0 and rec == z.proof_record(proof)
    return {"decompress_ms": round(t_dec * 1e3, 3), "decompress_proofs_per_s": round(k / t_dec, 1),
            "verify_all_bytes_ms": round(t_bytes * 1e3, 2), "verify_all_objects_ms": round(t_all * 1e3, 2),
            "bytes_minus_objects_ms": round((t_bytes - t_all) * 1e3, 2),
            "stages_ms": {n: round(v, 3) for n, v in stages.items()},
            "python_int_model_ms_per_proof": round(t_model * 1e3, 3),
            "python_int_model_scaled_ms": round(t_model * k * 1e3, 1)}


def _verify_all(z, vk, primary, proof, quick, compressed):
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
        if compressed:
            rlc[str(k)]["compressed"] = _compressed(z, vk, prims, proof, k, t_all)
    return rlc


def main():
    quick = "--quick" in sys.argv
    compressed_only = "--compressed-only" in sys.argv
    compressed = compressed_only or "--compressed" in sys.argv
    from octopuszk_amd import pairing as pa
    from octopuszk_amd import zksnark as z
    torch.cuda.set_device(0)
    if "--multi-only" in sys.argv:
        print(json.dumps({"metric": "multi_msm", "multi_msm": _multi_msm(False)}))
        return
    out = {"metric": "groth16_verify"}
    # one G2 point repeated (the G2 generator, wire-in), n G1 points
    g2 = b"".join(int(v).to_bytes(32, "little") for x in z.G2_ONE for v in x)
    res = {}
    for n in ([] if compressed_only else [1, 1024] if quick else [1, 1024, 65536]):
        P = _points(n, 3)
        Qd = torch.frombuffer(bytearray(g2 * n), dtype=torch.uint8).cuda()
        pa.reduced_pairing(P, Qd)
        t = _timed(lambda: pa.reduced_pairing(P, Qd), 3)
        res[str(n)] = {"ms": round(t * 1e3, 3), "pairings_per_s": round(n / t, 1)}
    out["reduced_pairing"] = res
    if not quick and not compressed_only:
        out["floor_ok"] = res["65536"]["pairings_per_s"] >= 1e6
    # one proof at 2^10
    r1cs, primary, auxiliary = z.serial_construct(1 << 10, 15)
    crs = z.serial_setup_generate(r1cs)
    vk = z.verification_key(crs)
    prover = z.SerialProver(crs.proving_key)
    proof = prover.prove(primary, auxiliary)
    prover.close()
    assert z.Verifier.verify(vk, primary, proof)
    if compressed_only:
        out = {"metric": "groth16_verify_compressed", "verify_all": _verify_all(z, vk, primary, proof, quick, True)}
        print(json.dumps(out))
        return
    out["verify_one_ms"] = round(_timed(lambda: z.Verifier.verify(vk, primary, proof), 5) * 1e3, 3)
    out["abc_msm_one_ms"] = round(_timed(lambda: vk.evaluation_abc(primary), 5) * 1e3, 3)
    batch = {}
    for k in ([64] if quick else [64, 4096]):
        prims, proofs = [primary] * k, [proof] * k
        t = _timed(lambda: z.Verifier.verify_batch(vk, prims, proofs, abc="per_proof"), 2)
        t_abc = _timed(lambda: [vk.evaluation_abc(p) for p in prims], 1)
        batch[str(k)] = {"ms": round(t * 1e3, 2), "proofs_per_s": round(k / t, 1), "abc_msm_ms": round(t_abc * 1e3, 2)}
    out["verify_batch"] = batch
    # the batched evaluationABC: table build, then the same batches (and K = 65536)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    vk.evaluation_abc_batch([primary])
    torch.cuda.synchronize()
    out["abc_table_build_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    bb = {}
    for k in ([64] if quick else [64, 4096, 65536]):
        prims, proofs = [primary] * k, [proof] * k
        assert all(z.Verifier.verify_batch(vk, prims, proofs, abc="batched"))
        t = _timed(lambda: z.Verifier.verify_batch(vk, prims, proofs, abc="batched"), 2)
        t_abc, t_pair = _batched_stages(z, pa, vk, prims, proofs)
        bb[str(k)] = {"ms": round(t * 1e3, 2), "proofs_per_s": round(k / t, 1), "abc_stage_ms": t_abc,
                      "pairing_stage_ms": t_pair}
    out["verify_batch_batched"] = bb
    if not quick:
        out["batched_speedup_4096"] = round(batch["4096"]["ms"] / bb["4096"]["ms"], 1)
        out["batched_floor_ok"] = out["batched_speedup_4096"] >= 20
        # the 1023-input key (2^11 constraints: the setup's 11-bit window at 2^12 does not cover a 254-bit scalar):
        # the two stages at K = 4096
        r2, primary2, auxiliary2 = z.serial_construct(1 << 11, 1023)
        crs2 = z.serial_setup_generate(r2)
        vk2 = z.verification_key(crs2)
        prover2 = z.SerialProver(crs2.proving_key)
        proof2 = prover2.prove(primary2, auxiliary2)
        prover2.close()
        assert z.Verifier.verify_batch(vk2, [primary2] * 4, [proof2] * 4, abc="batched") == [True] * 4
        t_abc, t_pair = _batched_stages(z, pa, vk2, [primary2] * 4096, [proof2] * 4096)
        out["stages_1023_inputs_4096"] = {"abc_stage_ms": t_abc, "pairing_stage_ms": t_pair,
                                          "window_bits": vk2._multi.window_bits}
        del vk2, crs2
        # the worst case of the randomized check: ONE tampered proof in 4096 sends the whole batch to verify_batch
        from oracle import bn254 as o
        bad_c = o.g1_out_le(o.G1.to_affine(o.G1.add(o.g1_from_out_le(proof.g_c), o.G1.one)))
        prims = [primary] * 4096
        proofs = [proof] * 4096
        proofs[1234] = z.Proof(proof.g_a, proof.g_b, bad_c)
        want = [True] * 4096
        want[1234] = False
        assert z.Verifier.verify_batch_rlc(vk, prims, proofs) == want
        t_b = _timed(lambda: z.Verifier.verify_batch_rlc(vk, prims, proofs), 2)
        vk_pp = z.VerificationKey(vk.alpha_g1_beta_g2, vk.gamma_g2, vk.delta_g2, vk.gamma_abc_g1)   # no table
        keep, z.Verifier.ABC_BATCH_CROSSOVER = z.Verifier.ABC_BATCH_CROSSOVER, 1 << 62              # auto -> per proof
        try:
            assert z.Verifier.verify_batch_rlc(vk_pp, prims, proofs) == want
            t_p = _timed(lambda: z.Verifier.verify_batch_rlc(vk_pp, prims, proofs), 1)
        finally:
            z.Verifier.ABC_BATCH_CROSSOVER = keep
        out["rlc_one_tampered_4096"] = {"batched_fallback_ms": round(t_b * 1e3, 2), "per_proof_fallback_ms": round(t_p * 1e3, 2)}
    out["multi_msm"] = _multi_msm(quick)
    rlc = _verify_all(z, vk, primary, proof, quick, compressed)
    out["verify_all"] = rlc
    if not quick:
        t = rlc["4096"]["verify_all_ms"]
        out["rlc_speedup_4096"] = round(rlc["4096"]["verify_all_proofs_per_s"] / batch["4096"]["proofs_per_s"], 1)
        out["rlc_floor_ok"] = t <= 150 and out["rlc_speedup_4096"] >= 20
    print(json.dumps(out))


if __name__ == "__main__":
    main()
