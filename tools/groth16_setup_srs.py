#!/usr/bin/env python3
"""Build a Groth16 key file from a powers-of-tau string, or measure that setup.

    python tools/groth16_setup_srs.py LOGN OUT.ozkpk OUT.vk [--inputs NI] [--contributions K]
    python tools/groth16_setup_srs.py --measure LOGN

The first form builds the R1CS of serial_construct with 2^LOGN constraints (NI inputs, default 15), a string from
Srs.from_secrets, checks the string, runs setup_from_srs, optionally applies K phase-2 contributions (their receipts
go to OUT.ozkpk.receipt1 ..), and writes the key file and the verification key.  THE STRING'S SECRETS ARE KNOWN TO
THIS PROCESS: the key is for tests and measurements, not for anybody to trust.

--measure times Srs.check and every stage of the setup (setup_from_srs synchronises on both sides of each), proves
with the key, verifies, and writes profiles/setup_srs_2pLOGN.json with the counted time of DESIGN.md section 16 next
to each measured one.  It exits non-zero unless the string checks and the proof verifies."""
import json
import math
import os
import secrets
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MULMOD_PER_S = 170e9
WARNING = "THE SECRETS OF THIS STRING (TAU, ALPHA, BETA) ARE KNOWN TO THE PROCESS THAT MADE IT: DO NOT TRUST THIS KEY"


def _make(logn, ni):
    from octopuszk_amd import srs
    from octopuszk_amd import zksnark as z
    from octopuszk_amd.fft import FR
    r1cs, primary, auxiliary = z.serial_construct(1 << logn, ni)
    m = z.lowest_power_of_two((1 << logn) + ni)
    print(WARNING, file=sys.stderr)
    string = srs.Srs.from_secrets(m, *(secrets.randbelow(FR - 1) + 1 for _ in range(3)))
    return r1cs, primary, auxiliary, string, m


def counted_s(m):
    """the counts of DESIGN.md section 16, in seconds at MULMOD_PER_S"""
    ladders = m // 2 * int(math.log2(m)) - (m - 1) + m // 2
    g1 = (ladders * 1610 + m // 2 * int(math.log2(m)) * 22) / MULMOD_PER_S
    g2 = (ladders * (253 * 7 + 85 * 11) * 3 + m // 2 * int(math.log2(m)) * 66) / MULMOD_PER_S
    return {"fft_tau_s": g1, "fft_alpha_s": g1, "fft_beta_s": g1, "fft_g2_s": g2}


def measure(logn):
    from octopuszk_amd import zksnark as z
    r1cs, primary, auxiliary, string, m = _make(logn, 15)
    res = {"constraints": 1 << logn, "inputs": 15, "m": m}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    why = []
    res["string_checks"] = bool(string.check(why=why))
    torch.cuda.synchronize()
    res["check_s"], res["why"] = round(time.perf_counter() - t0, 4), why
    t0 = time.perf_counter()
    crs = z.setup_from_srs(r1cs, string)
    torch.cuda.synchronize()
    res["setup_s"] = round(time.perf_counter() - t0, 4)
    counted = counted_s(m)
    res["stages"] = {k: {"measured_s": round(v, 5), "counted_s": round(counted[k], 5) if k in counted else None}
                     for k, v in crs.timing.items()}
    vk = z.verification_key(crs)
    prover = z.SerialProver(crs.proving_key)
    proof = prover.prove(primary, auxiliary)
    prover.close()
    res["proof_verifies"] = bool(z.Verifier.verify(vk, primary, proof))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "setup_srs_2p%d.json" % logn), "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))
    return 0 if res["string_checks"] and res["proof_verifies"] else 1


def build(args):
    from octopuszk_amd import zksnark as z
    opts = {"--inputs": 15, "--contributions": 0}
    for name in opts:
        if name in args:
            i = args.index(name)
            opts[name] = int(args[i + 1])
            args = args[:i] + args[i + 2:]
    if len(args) != 3:
        sys.stderr.write(__doc__)
        return 2
    logn, out_pk, out_vk = int(args[0]), args[1], args[2]
    r1cs, _, _, string, _ = _make(logn, opts["--inputs"])
    why = []
    if not string.check(why=why):
        sys.stderr.write("the string does not check: %s\n" % why)
        return 1
    crs = z.setup_from_srs(r1cs, string, log=lambda s: print(s, file=sys.stderr))
    pk, vk = crs.proving_key, z.verification_key(crs)
    previous = b""
    for k in range(opts["--contributions"]):
        pk, vk, receipt = pk.contribute(vk, previous=previous)
        previous = receipt.to_bytes()
        with open("%s.receipt%d" % (out_pk, k + 1), "wb") as f:
            f.write(previous)
    pk.save(out_pk)
    with open(out_vk, "wb") as f:
        f.write(vk.to_bytes())
    print(json.dumps({"constraints": 1 << logn, "inputs": opts["--inputs"], "contributions": opts["--contributions"],
                      "secrets_known_to_the_maker": True}))
    print(WARNING, file=sys.stderr)
    return 0


def main():
    args = sys.argv[1:]
    if args[:1] == ["--measure"] and len(args) == 2:
        return measure(int(args[1]))
    return build(args)


if __name__ == "__main__":
    sys.exit(main())
