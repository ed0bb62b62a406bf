#!/usr/bin/env python3
"""A Groth16 proving key through the key file on one MI355X: set up a 2^LOGN-constraint
synthetic circuit, save the key, load it both ways and prove, and print one JSON line.

    python tools/groth16_keyfile.py [LOGN=20] [key file path]

fused:    SerialProver.from_key_file — rows read by offset, uploaded compressed, decoded straight into the prepared
          bases (ozk_points_decompress_prepared_dev); once without and once with the G2 subgroup check, whose time is
          the difference of the two decode times.
unfused:  ProvingKey.load + SerialProver(pk) — decoded into wire-in tensors (ozk_points_decompress_dev), then
          prepared (ozk_var_msm_prepare_dev).
Each time is a wall time with a synchronise before and after; the peaks are torch.cuda.max_memory_allocated over the
route, from a reset taken after the route before it was freed.  The proofs of both loaded provers must equal the
in-memory prover's, byte for byte."""
import gc
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from octopuszk_amd import zksnark as z  # noqa: E402


def _proof_bytes(p):
    return bytes(p.g_a) + bytes(p.g_b) + bytes(p.g_c)


def _route(make):
    """(what make() returns, wall seconds, peak bytes allocated above the level at the start)"""
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    out = make()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0, torch.cuda.max_memory_allocated() - base


def main():
    logn = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    nc, ni = 1 << logn, min(1023, 1 << logn)
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(tempfile.mkdtemp(prefix="ozkpk"), "proving.ozkpk")
    r1cs, primary, auxiliary = z.serial_construct(nc, ni)
    crs = z.serial_setup_generate(r1cs)
    pk = crs.proving_key
    full_bytes = z.assignment_bytes(primary + auxiliary)
    prover = z.SerialProver(pk)
    want = _proof_bytes(prover.prove(primary, auxiliary, full_bytes=full_bytes))
    prover.close()
    t0 = time.perf_counter()
    pk.save(path)
    t_save = time.perf_counter() - t0
    size = os.path.getsize(path)
    del prover, pk, crs, r1cs
    out = {"workload": "Groth16 proving key file, synthetic R1CS 2^%d constraints, %d inputs" % (logn, ni),
           "file_bytes": size, "save_s": round(t_save, 3)}

    def proves(p):
        ok = _proof_bytes(p.prove(primary, auxiliary, full_bytes=full_bytes)) == want
        p.close()
        return ok

    fused = {}
    for label, check in (("no_subgroup_check", False), ("subgroup_check", True)):
        T = {}
        p, wall, peak = _route(lambda: z.SerialProver.from_key_file(path, check_subgroup=check, timing=T))
        fused[label] = {"total_s": round(wall, 3), "read_s": round(T["read_s"], 3), "upload_s": round(T["upload_s"], 3),
                        "decode_ms": round(T["decode_s"] * 1e3, 2), "peak_bytes": int(peak),
                        "prepared_key_bytes": p.key_bytes["rank"], "proof_matches": proves(p)}
        del p
    fused["subgroup_check_ms"] = round(fused["subgroup_check"]["decode_ms"] - fused["no_subgroup_check"]["decode_ms"], 2)
    out["fused"] = fused

    def unfused():
        t0 = time.perf_counter()
        pk2 = z.ProvingKey.load(path)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        p = z.SerialProver(pk2)
        torch.cuda.synchronize()
        return p, t1 - t0, time.perf_counter() - t1

    (p, t_load, t_prep), wall, peak = _route(unfused)
    out["unfused"] = {"total_s": round(wall, 3), "load_s": round(t_load, 3), "prepare_s": round(t_prep, 3),
                      "peak_bytes": int(peak), "proof_matches": proves(p)}
    del p
    print(json.dumps(out))
    return 0 if fused["subgroup_check"]["proof_matches"] and fused["no_subgroup_check"]["proof_matches"] \
        and out["unfused"]["proof_matches"] else 1


if __name__ == "__main__":
    sys.exit(main())
