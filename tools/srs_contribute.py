#!/usr/bin/env python3
"""Phase-1 contributions to a powers-of-tau string kept in OZKSRS files.

    python tools/srs_contribute.py --init M OUT.ozksrs              the public start: tau = alpha = beta = 1
    python tools/srs_contribute.py IN.ozksrs OUT.ozksrs RECEIPT [--previous RECEIPT_BEFORE]
    python tools/srs_contribute.py --verify S0 S1 .. Sk -- R1 .. Rk   a chain of string files and its receipts
    python tools/srs_contribute.py --measure LOGN

The second form checks IN, draws tau, alpha, beta from the system, multiplies them into the string, writes OUT and
the 432-byte receipt, and forgets the secrets when the process ends.  --verify loads every file, checks the first
string, and runs verify_chain; it exits non-zero with the name of the failed check.

--measure times, at m = 2^LOGN and with a synchronise on both sides, each of the five scalings of a contribution,
contribute, save, load and verify_contribution; compares ozk_points_mul_dev with the diagonal-matrix route through
ozk_sparse_mat_points_dev over the same points and scalars; builds a key from the contributed string, proves and
verifies; and writes profiles/srs_contribute_2pLOGN.json with the counted figure next to each measured one.  It exits
non-zero unless the contribution verifies, the two routes agree, the new kernel is the faster and the proof verifies."""
import json
import os
import secrets
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MULMOD_PER_S = 170e9
G1_MULS, G2_MULS = 128 * 18, 253 * (7 + 11) * 3   # per point: a doubling and an addition at almost every step


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def init(m, out):
    from octopuszk_amd import srs
    srs.Srs.initial(m).save(out)
    print(json.dumps({"m": m, "file_bytes": srs.string_file_size(m)}))
    return 0


def contribute(args):
    from octopuszk_amd import srs
    previous = b""
    if "--previous" in args:
        i = args.index("--previous")
        previous = _read(args[i + 1])
        args = args[:i] + args[i + 2:]
    if len(args) != 3:
        sys.stderr.write(__doc__)
        return 2
    before = srs.Srs.load(args[0])
    why = []
    if not before.check(why=why):
        sys.stderr.write("the string does not check: %s\n" % why)
        return 1
    after, receipt = before.contribute(previous=previous)
    after.save(args[1])
    with open(args[2], "wb") as f:
        f.write(receipt)
    print(json.dumps({"m": before.m, "receipt_sha256": __import__("hashlib").sha256(receipt).hexdigest()}))
    return 0


def verify(args):
    from octopuszk_amd import srs
    if "--" not in args:
        sys.stderr.write(__doc__)
        return 2
    i = args.index("--")
    strings, receipts = [srs.Srs.load(p) for p in args[:i]], [_read(p) for p in args[i + 1:]]
    why = []
    ok = strings[0].check(why=why) and srs.verify_chain(strings, receipts, why=why)
    print(json.dumps({"steps": len(receipts), "verifies": bool(ok), "why": why}))
    return 0 if ok else 1


def _timed(fn, repeat=1):
    """(the result, the best wall time of `repeat` runs in seconds), a synchronise on both sides"""
    best, out = None, None
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return out, best


def measure(logn):
    from octopuszk_amd import srs, vectors, wire
    from octopuszk_amd import lib as _lib
    from octopuszk_amd import zksnark as z
    from octopuszk_amd.device import _ptr, _stream
    from octopuszk_amd.fft import FR
    m = 1 << logn
    L = _lib.load()
    rnd = lambda: secrets.randbelow(FR - 1) + 1
    before = srs.Srs.from_secrets(m, rnd(), rnd(), rnd())
    s, a, b = rnd(), rnd(), rnd()
    res = {"m": m, "mulmod_per_s": MULMOD_PER_S, "stages": {}}

    def stage(name, seconds, points=None, muls=None):
        res["stages"][name] = {"measured_s": round(seconds, 5), "points": points,
                               "counted_s": None if muls is None else round(points * muls / MULMOD_PER_S, 5)}

    def powers(k, n):
        d_sc = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        wsb = int(L.ozk_fr_powers_workspace_bytes(n))
        ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device="cuda")
        _lib.check(L.ozk_fr_powers_dev(wire.vp(wire.le32([s])), wire.vp(wire.le32([k])), n, _ptr(d_sc), _ptr(ws), wsb,
                                       _stream()))
        torch.cuda.synchronize()
        return d_sc

    # the five scalings, one by one (warm the kernels on a few points first)
    pw, pa, pb = powers(1, 2 * m + 1), powers(a, m), powers(b, m)
    vectors.mul_points(before.tau_g1.reshape(-1)[:96 * 64], pw[:32 * 64], 1)
    vectors.mul_points(before.tau_g2.reshape(-1)[:192 * 64], pw[:32 * 64], 2)
    for name, points, sc, type_, n in (("tau_g1", before.tau_g1, pw, 1, 2 * m + 1), ("tau_g2", before.tau_g2, pw[:32 * m], 2, m),
                                       ("alpha_tau_g1", before.alpha_tau_g1, pa, 1, m), ("beta_tau_g1", before.beta_tau_g1, pb, 1, m)):
        _, dt = _timed(lambda: vectors.mul_points(points, sc, type_), repeat=2)
        stage("mul_" + name, dt, n, G1_MULS if type_ == 1 else G2_MULS)
    _, dt = _timed(lambda: vectors.scale_points(before.beta_g2, b, 2), repeat=2)
    stage("scale_beta_g2", dt, 1)
    # the comparison: the diagonal matrix of the same scalars over the same points
    n = min(m, 1 << 20)
    ks = wire.ints32(wire.host_bytes(pa[:32 * n]))
    mat = z._CsrDevice(np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int64), np.array(ks, dtype=object))
    pts = before.alpha_tau_g1.reshape(-1)[:96 * n]
    new, t_new = _timed(lambda: vectors.mul_points(pts, pa[:32 * n], 1), repeat=3)
    old, t_old = _timed(lambda: vectors.sparse_mat_points(mat, pts, 1), repeat=3)
    res["comparison"] = {"points": n, "points_mul_s": round(t_new, 5), "diagonal_sparse_mat_points_s": round(t_old, 5),
                         "ratio": round(t_old / t_new, 3), "counted_ratio": round(254 * 18 / G1_MULS, 2),
                         "bit_equal": bool(torch.equal(new, old))}
    del new, old, mat, pts, pw, pa, pb
    # the whole protocol
    (after, receipt), dt = _timed(lambda: before.contribute(s, a, b))
    stage("contribute", dt, 4 * m + 1 + m + 1)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "string.ozksrs")
        _, dt = _timed(lambda: after.save(path))
        stage("save", dt)
        res["file_bytes"] = os.path.getsize(path)
        loaded, dt = _timed(lambda: srs.Srs.load(path))
        stage("load", dt)
    why = []
    ok, dt = _timed(lambda: srs.verify_contribution(before, loaded, receipt, why=why))
    stage("verify_contribution", dt)
    res["contribution_verifies"], res["why"] = bool(ok), why
    del before, after
    # a key from the contributed string
    r1cs, primary, auxiliary = z.serial_construct(m - 15, 15)
    crs, dt = _timed(lambda: z.setup_from_srs(r1cs, loaded))
    stage("setup_from_srs", dt)
    vk = z.verification_key(crs)
    prover = z.SerialProver(crs.proving_key)
    proof = prover.prove(primary, auxiliary)
    prover.close()
    res["proof_verifies"] = bool(z.Verifier.verify(vk, primary, proof))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "srs_contribute_2p%d.json" % logn), "w") as f:
        f.write(json.dumps(res) + "\n")
    print(json.dumps(res))
    c = res["comparison"]
    return 0 if ok and res["proof_verifies"] and c["bit_equal"] and c["ratio"] > 1 else 1


def main():
    args = sys.argv[1:]
    if args[:1] == ["--measure"] and len(args) == 2:
        return measure(int(args[1]))
    if args[:1] == ["--init"] and len(args) == 3:
        return init(int(args[1]), args[2])
    if args[:1] == ["--verify"]:
        return verify(args[1:])
    return contribute(args)


if __name__ == "__main__":
    sys.exit(main())
