"""Times the batched PLONK verifier on one GPU.  One JSON line.

A circuit of 2^k rows is generated as tools/plonk_prove.py generates it (a chain of additions and multiplications; with
--lookups a share of lookup rows; with --r1cs the import of serial_construct), set up over a string of known tau, and
--distinct proofs of different assignments are made and checked one by one.  They are cycled to fill batches of K
proofs, and for every K of --batch the run reports

(a) plonk.verify_all over host bytes, by a host clock around work that ends in a synchronise: the median of --reps
    runs after one warm-up, and the proofs per second it makes;
(b) every stage of BATCH_STAGES (upload, challenges, scalars, decode, the two MSMs, the pairing product), the medians
    of --reps runs with a synchronisation after each stage, and the same with proofs and public inputs already on the
    device;
(c) in the same process, plonk.verify called once per proof, which is the only path without this section: over all K
    proofs up to --loop-max, over that many and scaled to K beyond ("verify_loop_projected").

    python tools/plonk_verify.py --log-n 10 --batch 1,64,4096 [--lookups 0.5] [--reps 5]
    python tools/plonk_verify.py --r1cs 8 --inputs 255 --batch 1,64,4096
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import kzg_bench as kb  # noqa: E402
import plonk_prove as pp  # noqa: E402
from octopuszk_amd import kzg, plonk, wire  # noqa: E402
from octopuszk_amd.fft import FR  # noqa: E402


def chain_values(n_public, end, salt):
    """the assignment of plonk_prove.chain_columns's gates from other public inputs"""
    values = [(0x9e3779b97f4a7c15f39cc0605cedc835 * (i + 1) + salt) % FR for i in range(n_public)]
    prev = 0
    for row in range(n_public, end):
        other = 0 if row % 3 == 0 else prev
        values.append(values[prev] * values[other] % FR if row % 2 else (values[prev] + values[other]) % FR)
        prev = len(values) - 1
    return values


def cases(a):
    """(circuit, [(public inputs, assignment)] of --distinct different assignments)"""
    n = 1 << a.log_n
    if a.r1cs is not None:
        from octopuszk_amd import zksnark
        made = [zksnark.serial_construct(1 << a.r1cs, a.public, seed=zksnark.SEED + i) for i in range(a.distinct)]
        return plonk.from_r1cs(made[0][0]), [(list(primary), list(primary + auxiliary)) for _, primary, auxiliary in made]
    if a.lookups:
        circuit, first = pp.chain_with_lookups(n, a.public, a.lookups, pp.xor_table(a.table_rows))
        end = n - sum(circuit.q_lookup)
    else:
        circuit, first = pp.chain(n, a.public)
        end = n - 1
    chain_len = len(chain_values(a.public, end, 0))
    out = []
    for i in range(a.distinct):
        values = chain_values(a.public, end, i) + first[chain_len:]
        out.append((values[:a.public], values))
    return circuit, out


def _median_ms(samples):
    return statistics.median(samples) * 1e3


def batch_rounds(vk, kvk, publics, proofs, k, reps, loop_max):
    xs = [publics[m % len(publics)] for m in range(k)]
    ps = [proofs[m % len(proofs)] for m in range(k)]
    host_proofs, host_public = b"".join(ps), wire.le32(x for row in xs for x in row)
    assert plonk.verify_all(vk, kvk, host_public, host_proofs)            # the warm-up
    whole, staged, resident = [], {name: [] for name in plonk.BATCH_STAGES}, {name: [] for name in plonk.BATCH_STAGES}
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ok = plonk.verify_all(vk, kvk, host_public, host_proofs)
        torch.cuda.synchronize()
        whole.append(time.perf_counter() - t0)
        assert ok
    d_proofs, d_public = wire.dev_bytes(host_proofs), wire.dev_bytes(host_public)
    for into, given in ((staged, (host_public, host_proofs)), (resident, (d_public, d_proofs))):
        for _ in range(reps):
            timings = {}
            assert plonk.verify_all(vk, kvk, given[0], given[1], timings=timings)
            for name in into:
                into[name].append(timings.get(name, 0.0))
    loop = min(k, loop_max)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for m in range(loop):
        assert plonk.verify(vk, kvk, xs[m], ps[m])
    torch.cuda.synchronize()
    per_proof = (time.perf_counter() - t0) / loop
    all_ms = _median_ms(whole)
    stages = {name: _median_ms(v) for name, v in staged.items()}
    return {"K": k, "verify_all_ms": all_ms, "verify_all_rounds_ms": [x * 1e3 for x in whole],
            "proofs_per_s": k / (all_ms * 1e-3), "stages_ms": stages, "bounding_stage": max(stages, key=stages.get),
            "stages_device_resident_ms": {name: _median_ms(v) for name, v in resident.items()},
            "verify_per_proof_ms": per_proof * 1e3, "verify_loop_ms": per_proof * 1e3 * k, "verify_loop_proofs": loop,
            "verify_loop_projected": loop < k, "speedup_over_loop": per_proof * 1e3 * k / all_ms}


def run(a):
    circuit, made = cases(a)
    n = circuit.n
    s = kb._String(n // 2)
    ck, kvk = kzg.CommitKey.from_srs(s, n), kzg.VerifyKey.from_srs(s)
    pk, vk = plonk.setup(circuit, ck)
    publics, proofs = [], []
    for public, assignment in made:
        proof = plonk.prove(pk, assignment)
        assert plonk.verify(vk, kvk, public, proof)
        publics.append(public)
        proofs.append(proof.to_bytes())
    assert len(set(proofs)) == len(proofs)
    kind = "r1cs" if a.r1cs is not None else "lookup" if a.lookups else "vanilla"
    res = {"kind": kind, "n": n, "n_public": vk.n_public, "proof_bytes": len(proofs[0]), "distinct_proofs": len(proofs)}
    res["batches"] = [batch_rounds(vk, kvk, publics, proofs, k, a.reps, a.loop_max) for k in a.batch]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--public", type=int, default=3)
    ap.add_argument("--lookups", type=float, default=0.0, help="the share of rows that are lookups (0: none)")
    ap.add_argument("--table-rows", type=int, default=256)
    ap.add_argument("--r1cs", type=int, default=None, metavar="LOG_NC",
                    help="verify proofs of the import of serial_construct(2^LOG_NC, --inputs)")
    ap.add_argument("--inputs", type=int, default=None, help="the R1CS's num_inputs (default: min(1023, 2^LOG_NC))")
    ap.add_argument("--batch", type=lambda t: [int(x) for x in t.split(",")], default=[1, 64, 4096])
    ap.add_argument("--distinct", type=int, default=4, help="different proofs that are cycled to fill a batch")
    ap.add_argument("--loop-max", type=int, default=256, help="at most so many single verify calls are timed per K")
    a = ap.parse_args()
    if a.r1cs is not None:
        if not 1 <= a.r1cs <= 20 or a.lookups:
            ap.error("1 <= --r1cs <= 20, without --lookups")
        a.public = min(1023, 1 << a.r1cs) if a.inputs is None else a.inputs
        if not 1 <= a.public <= (1 << a.r1cs) + 1:
            ap.error("1 <= --inputs <= 2^LOG_NC + 1")
    elif not 2 <= a.log_n <= 22 or not 1 <= a.public < (1 << a.log_n) - 1:
        ap.error("2 <= --log-n <= 22 and 1 <= --public < 2^log-n - 1")
    if not 0 <= a.lookups <= 1 or (a.lookups and not 1 <= a.table_rows <= 1 << a.log_n):
        ap.error("0 <= --lookups <= 1 and 1 <= --table-rows <= 2^log-n")
    if not a.batch or any(not 1 <= k <= 1 << 16 for k in a.batch) or a.distinct < 1 or a.reps < 1 or a.loop_max < 1:
        ap.error("1 <= K <= 2^16 for every K of --batch; --distinct, --reps, --loop-max >= 1")
    torch.cuda.set_device(0)
    out = {"bench": "plonk_verify", "device": torch.cuda.get_device_name(0), "reps": a.reps, "result": run(a)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
