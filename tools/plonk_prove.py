"""Times the PLONK prover and verifier on one GPU at n = 2^k gates.  One JSON line.

The circuit is generated: a few public inputs, then a chain of multiplications and additions in which the first input
feeds every third gate, padded to 2^k rows.  The string is built from a known tau, so the proof verifies.

(a) every stage of plonk.prove (witness upload, witness transforms, grand product, coset transforms, quotient kernel,
    commitments, multi-opening) and plonk.verify, by a host clock around work that ends in a synchronise: the median of
    --reps proofs after one warm-up;
(b) the whole prove by the same clock, beside the sum of the MSM and transform calls it makes (9 MSMs of n, 5
    transforms of n, 6 of 4 n), each timed alone in the same run;
(c) the grand-product and quotient entry points alone under device events, with the bytes per second of their counted
    traffic: 32 len (12 reads + 1 write) and 32 (4 n) (16 reads + 1 write).

    python tools/plonk_prove.py [--log-n 16] [--reps 5] [--public 3]
"""
import argparse
import ctypes
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
from octopuszk_amd import kzg, lib as _lib, plonk, vectors, wire  # noqa: E402
from octopuszk_amd.device import VarMsmWorkspace, _ptr, _stream  # noqa: E402
from octopuszk_amd.fft import FR, root_of_unity  # noqa: E402
from octopuszk_amd.plonk import protocol  # noqa: E402
from octopuszk_amd.plonk.circuit import K  # noqa: E402


def chain(n, n_public):
    """(circuit, assignment): n_public inputs, n - n_public - 1 gates alternating addition and multiplication, one
    padding row"""
    values = [(0x9e3779b97f4a7c15f39cc0605cedc835 * (i + 1)) % FR for i in range(n_public)]
    sel, wires = [[0] * n for _ in range(5)], [[0] * n for _ in range(3)]
    for v in range(n_public):
        sel[0][v] = 1
        wires[0][v] = wires[1][v] = wires[2][v] = v
    prev = 0
    for row in range(n_public, n - 1):
        other = 0 if row % 3 == 0 else prev
        new = len(values)
        if row % 2:
            values.append(values[prev] * values[other] % FR)
            sel[3][row], sel[2][row] = 1, FR - 1
        else:
            values.append((values[prev] + values[other]) % FR)
            sel[0][row], sel[1][row], sel[2][row] = 1, 1, FR - 1
        wires[0][row], wires[1][row], wires[2][row] = prev, other, new
        prev = new
    return plonk.Circuit(n, sel, wires, n_public), values


def _median_ms(samples):
    return statistics.median(samples) * 1e3


def run(log_n, reps, n_public):
    n = 1 << log_n
    L = _lib.load()
    t0 = time.perf_counter()
    circuit, assignment = chain(n, n_public)
    public = assignment[:n_public]
    s = kb._String(n // 2)
    ck = kzg.CommitKey.from_srs(s, n)
    kvk = kzg.VerifyKey.from_srs(s)
    ck.bases()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    pk, vk = plonk.setup(circuit, ck)
    torch.cuda.synchronize()
    res = {"n": n, "n_public": n_public, "circuit_and_string_s": t1 - t0, "setup_s": time.perf_counter() - t1,
           "proving_key_table_bytes": pk.table.numel()}

    # (a), (b): whole proofs
    as_ints = assignment
    assignment = wire.le32(as_ints)                                      # the 32-byte records: no per-value host work
    proof = plonk.prove(pk, assignment)                                  # the warm-up
    assert proof.to_bytes() == plonk.prove(pk, as_ints).to_bytes()
    assert plonk.verify(vk, kvk, public, proof)
    stages, whole, verify = {name: [] for name in plonk.protocol.STAGES}, [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plonk.prove(pk, assignment)
        torch.cuda.synchronize()
        whole.append(time.perf_counter() - t0)
    for _ in range(reps):
        timings = {}
        proof = plonk.prove(pk, assignment, timings)
        for name in stages:
            stages[name].append(timings.get(name, 0.0))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert plonk.verify(vk, kvk, public, proof)
        torch.cuda.synchronize()
        verify.append(time.perf_counter() - t0)
    res["stages_ms"] = {name: _median_ms(v) for name, v in stages.items()}
    res["stages_ms"]["verification"] = _median_ms(verify)
    res["prove_ms"] = _median_ms(whole)
    res["prove_rounds_ms"] = [x * 1e3 for x in whole]
    res["proof_bytes"] = len(proof.to_bytes())

    # (b) the MSM and the transforms alone
    rows = kb._random_rows(1, 4 * n, log_n)
    msm = VarMsmWorkspace(n, 1)
    res["msm_n_ms"] = kb._event_ms(lambda: msm.run(ck.bases(), rows[0][:32 * n], prepared=True), reps)
    out = torch.empty(32 * 4 * n, dtype=torch.uint8, device="cuda")
    res["fft_n_ms"] = kb._median_ms(lambda: vectors.fr_fft(rows[0][:32 * n], n, root_of_unity(n), out[:32 * n]), reps)
    res["fft_4n_ms"] = kb._median_ms(lambda: vectors.fr_fft(rows[0], 4 * n, root_of_unity(4 * n), out), reps)
    res["msm_and_fft_calls_ms"] = 9 * res["msm_n_ms"] + 5 * res["fft_n_ms"] + 6 * res["fft_4n_ms"]

    # (c) the two kernels alone
    wires = protocol._rows(circuit.wire_values(as_ints))
    z = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
    tail = torch.empty(48, dtype=torch.uint8, device="cuda")
    ws = torch.empty(max(int(L.ozk_fr_perm_product_workspace_bytes(n)), 256), dtype=torch.uint8, device="cuda")
    le = lambda vs: wire.le32([int(v) % FR for v in vs])
    beta, gamma, alpha = 0x1234567 + n, 0x7654321 + n, 0x1357 + n
    args = [le([root_of_unity(n)]), le(K), le([beta]), le([gamma]), le([alpha]), le(protocol.zh_inverses(n))]
    vps = [ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in args]

    def product():
        _lib.check(L.ozk_fr_perm_product_dev(_ptr(wires), _ptr(pk.sigma), n, n, vps[0], vps[1], vps[2], vps[3], _ptr(z),
                                             _ptr(tail), _ptr(tail[32:]), _ptr(ws), ws.numel(), _stream()))

    ms = kb._event_ms(product, reps)
    res["perm_product"] = {"ms": ms, "counted_bytes": 32 * n * 13, "bytes_per_s": 32 * n * 13 / (ms * 1e-3)}
    wit = torch.cat([rows[0].view(1, -1)] * 5)

    def quotient():
        _lib.check(L.ozk_plonk_quotient_dev(_ptr(wit), 4 * n, _ptr(pk.table), 4 * n, n, vps[4], vps[2], vps[3], vps[1],
                                            vps[5], _ptr(out), _stream()))

    ms = kb._event_ms(quotient, reps)
    res["quotient"] = {"ms": ms, "counted_bytes": 32 * 4 * n * 17, "bytes_per_s": 32 * 4 * n * 17 / (ms * 1e-3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--public", type=int, default=3)
    a = ap.parse_args()
    if not 2 <= a.log_n <= 22 or not 1 <= a.public < (1 << a.log_n) - 1:
        ap.error("2 <= --log-n <= 22 and 1 <= --public < 2^log-n - 1")
    torch.cuda.set_device(0)
    out = {"bench": "plonk_prove", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "result": run(a.log_n, a.reps, a.public)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
