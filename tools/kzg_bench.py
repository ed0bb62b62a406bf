"""Timings of the KZG layer on one GPU: commit, open, open_evals and verify at K = 1 for
n = 2^16 and 2^20, verify_all at K = 64, the two opening kernels alone under HIP events, and beside them the lone
G1 MSM of the same n through the existing entry point.  One JSON line.

    python tools/kzg_bench.py [--logs 16,20] [--reps 5] [--k 64]

The string is built from a known tau (G1 powers and two G2 points only), so every opening verifies.
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from octopuszk_amd import kzg, lib as _lib, wire  # noqa: E402
from octopuszk_amd import zksnark as z  # noqa: E402
from octopuszk_amd.device import VarMsmWorkspace, _ptr, _stream  # noqa: E402
from octopuszk_amd.fft import FR, root_of_unity  # noqa: E402

TAU = 0x1d2c3b4a5968778695a4b3c2d1e0f0123456789abcdef % FR


class _String:
    """what CommitKey.from_srs and VerifyKey.from_srs read of an Srs: m, tau_g1 (2 m + 1 powers), tau_g2 (two here)"""

    def __init__(self, m):
        from octopuszk_amd.fixed_base_msm import G1_WINDOW_TABLE, get_window_size
        L = _lib.load()
        n = 2 * m + 1
        d_sc = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        wsb = int(L.ozk_fr_powers_workspace_bytes(n))
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        tb, kb = wire.le32([TAU]), wire.le32([1])
        _lib.check(L.ozk_fr_powers_dev(wire.vp(tb), wire.vp(kb), n, _ptr(d_sc), _ptr(ws), wsb, _stream()))
        torch.cuda.synchronize()
        self.m = m
        self.tau_g1 = z.batch_msm_dev(254, get_window_size(n, G1_WINDOW_TABLE), wire.g1_wire(z.G1_ONE), d_sc, 1)
        self.tau_g2 = z.batch_msm_dev(254, 16, wire.g2_wire(z.G2_ONE), [1, TAU], 2)


def _median_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(out), 4)


def _event_ms(enqueue, reps):
    enqueue()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        enqueue()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return round(statistics.median(out), 4)


def _random_rows(k, n, seed):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, size=(k, n, 32), dtype=np.uint8)
    raw[:, :, 31] &= 0x1F                      # below 2^253 < r: canonical
    return torch.from_numpy(raw.reshape(k, n * 32)).cuda()


def run(log, reps, kbatch):
    n = 1 << log
    L = _lib.load()
    s = _String(n // 2)
    ck = kzg.CommitKey.from_srs(s, n)
    vk = kzg.VerifyKey.from_srs(s)
    rows = _random_rows(1, n, log)
    zpt = [0x123456789abcdef0123456789 % FR]
    ck.bases(), ck.lagrange(n)
    torch.cuda.synchronize()
    res = {"n": n}
    res["commit_ms"] = _median_ms(lambda: ck.commit(rows), reps)
    res["open_ms"] = _median_ms(lambda: ck.open(rows, zpt), reps)
    res["open_evals_ms"] = _median_ms(lambda: ck.open_evals(rows, zpt), reps)
    op = ck.open(rows, zpt)[0]
    assert kzg.verify(vk, op) and kzg.verify(vk, ck.open_evals(rows, zpt)[0])
    res["verify_ms"] = _median_ms(lambda: kzg.verify(vk, op), reps)
    # the kernels alone
    quot = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    val = torch.empty(32, dtype=torch.uint8, device="cuda")
    pts = wire.dev_bytes(wire.le32(zpt))
    wsb = int(L.ozk_fr_poly_open_workspace_bytes(1, n))
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device="cuda")
    res["poly_open_kernel_ms"] = _event_ms(lambda: _lib.check(L.ozk_fr_poly_open_dev(
        _ptr(rows), 1, n, n, _ptr(pts), _ptr(quot), n, _ptr(val), _ptr(ws), ws.numel(), _stream())), reps)
    wsb = int(L.ozk_fr_evals_open_workspace_bytes(1, n))
    ws2 = torch.empty(max(wsb, 256), dtype=torch.uint8, device="cuda")
    om = wire.le32([root_of_unity(n)])
    res["evals_open_kernel_ms"] = _event_ms(lambda: _lib.check(L.ozk_fr_evals_open_dev(
        _ptr(rows), 1, n, n, wire.vp(om), _ptr(pts), _ptr(quot), n, _ptr(val), _ptr(ws2), ws2.numel(), _stream())), reps)
    # the lone MSM of the same n over the same prepared bases
    msm = VarMsmWorkspace(n, 1)
    res["msm_ms"] = _event_ms(lambda: msm.run(ck.bases(), rows.reshape(-1), prepared=True), reps)
    # a batch of openings of short polynomials against the same key
    if kbatch:
        small = kzg.CommitKey.from_srs(s, 64)
        many = small.open(_random_rows(kbatch, 64, 99), [(i * i + 3) % FR for i in range(kbatch)])
        assert kzg.verify_all(vk, many)
        res["verify_all_k%d_ms" % kbatch] = _median_ms(lambda: kzg.verify_all(vk, many), reps)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logs", default="16,20")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=64)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"bench": "kzg", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "sizes": [run(int(x), a.reps, a.k) for x in a.logs.split(",")]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
