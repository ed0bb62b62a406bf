"""BACE prover / verifier / naive evaluator timing on one GPU: prints one JSON line.

    timeout -k 10 300 python tools/bace_prove.py            # n = 64, N = 2^14, ~1000 gates of degree 4: D = 2^16
    timeout -k 10 600 python tools/bace_prove.py --large    # n = 16, N = 2^18, degree 4: D = 2^20

Times are medians of --reps runs between HIP events.  The prover split: circuit_ms is the interpreter alone at the D
points (the naive evaluator over D rows), final_ifft_ms one inverse transform of size D, and lde_ms_derived the rest
of the prove (columns, batched inverse transforms of size N, forward transforms of size D).  lde_per_column_loop_ms is
the same LDE as a loop of ozk_fft_compact_dev calls, one inverse and one forward transform per column.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import bace_util as bu  # noqa: E402
from octopuszk_amd import bace  # noqa: E402
from octopuszk_amd import lib as _lib  # noqa: E402
from octopuszk_amd.fft import root_of_unity  # noqa: E402


def _ms(fn, reps):
    torch.cuda.synchronize()
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        t.append(a.elapsed_time(b))
    t.sort()
    return t[len(t) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--large", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    n, logN = (16, 18) if args.large else (64, 14)
    N = 1 << logN
    circ = bu.random_dag(n, 1000, 4, seed=1, const_rate=0.02, recent=24)
    assert circ.total_degree() == 4
    prog, n_slots, consts = circ.compile()
    D = bace.proof_size(circ, N)
    g = torch.Generator(device="cuda").manual_seed(5)
    raw = torch.randint(0, 256, (n * N, 32), dtype=torch.uint8, device="cuda", generator=g)
    raw[:, 31] &= 0x1F                                   # < 2^253 < r
    inputs = raw.reshape(-1).contiguous()
    t0 = time.time()
    prover = bace.Prover(circ, inputs, N)
    _, proof = prover.compute_proof()
    torch.cuda.synchronize()
    first_s = time.time() - t0
    prove_ms = _ms(lambda: prover.compute_proof(), args.reps)

    L = _lib.load()
    st = int(torch.cuda.current_stream().cuda_stream)
    naive = bace.NaiveEvaluator(circ, inputs, N)
    naive_ms = _ms(lambda: naive.get_result(), args.reps)
    big = torch.randint(0, 256, (n * D, 32), dtype=torch.uint8, device="cuda", generator=g)
    big[:, 31] &= 0x1F
    circuit_ms = _ms(lambda: bace.NaiveEvaluator._evaluate(circ, big.reshape(-1), D), args.reps)
    del big
    fws = torch.empty(int(L.ozk_fft_workspace_bytes(D)), dtype=torch.uint8, device="cuda")
    fout = torch.empty(D * 32, dtype=torch.uint8, device="cuda")
    om_i = pow(root_of_unity(D), -1, bace.FR).to_bytes(32, "little")
    om_f = root_of_unity(D).to_bytes(32, "little")
    om_n = pow(root_of_unity(N), -1, bace.FR).to_bytes(32, "little")
    final_ms = _ms(lambda: _lib.check(L.ozk_fft_compact_dev(proof.data_ptr(), D, ctypes.c_char_p(om_i), fout.data_ptr(),
                                                            fws.data_ptr(), fws.numel(), st)), args.reps)

    colbuf = torch.zeros(n, D * 32, dtype=torch.uint8, device="cuda")
    cols = inputs.view(N, n, 32).transpose(0, 1).contiguous()
    evals = torch.empty(n, D * 32, dtype=torch.uint8, device="cuda")

    def per_column():
        for j in range(n):
            _lib.check(L.ozk_fft_compact_dev(cols[j].data_ptr(), N, ctypes.c_char_p(om_n), colbuf[j].data_ptr(),
                                             fws.data_ptr(), fws.numel(), st))
            _lib.check(L.ozk_fft_compact_dev(colbuf[j].data_ptr(), D, ctypes.c_char_p(om_f), evals[j].data_ptr(),
                                             fws.data_ptr(), fws.numel(), st))
    loop_ms = _ms(per_column, args.reps)
    del colbuf, evals, cols

    ver = bace.Verifier(circ, (D, proof), inputs, N)
    ok = ver.verify_proof(seed=57)
    verify_ms = _ms(lambda: ver.verify_proof(seed=57), args.reps)
    res_ms = _ms(lambda: ver.get_result(), args.reps)
    same = torch.equal(ver.get_result(), naive.get_result())
    torch.cuda.synchronize()
    print(json.dumps({
        "shape": "large" if args.large else "default", "n": n, "N": N, "D": D, "ops": int(prog.shape[0]),
        "slots": n_slots, "consts": len(consts), "prove_ms": round(prove_ms, 3),
        "lde_ms_derived": round(max(prove_ms - circuit_ms - final_ms, 0.0), 3), "circuit_ms": round(circuit_ms, 3),
        "final_ifft_ms": round(final_ms, 3), "lde_per_column_loop_ms": round(loop_ms, 3),
        "verify_ms": round(verify_ms, 3), "get_result_ms": round(res_ms, 3), "naive_ms": round(naive_ms, 3),
        "verified": bool(ok), "result_equals_naive": bool(same), "first_call_s": round(first_s, 3),
        "proof_sha256": hashlib.sha256(bytes(proof.cpu().numpy().tobytes())).hexdigest(),
    }), flush=True)


if __name__ == "__main__":
    main()
