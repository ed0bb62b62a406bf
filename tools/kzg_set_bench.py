"""Timings of KZG set openings on one GPU, n = 2^20 by default: for t in 1, 2, 4, 8, 32 the
coefficient-form kernel alone under HIP events, beside it t chained calls of the single-point kernel over the same row
(the baseline a caller had before), the evaluation-form kernel for t <= 8, the lone G1 MSM of the same n, and
open_set / verify_set at K = 1 and verify_set_all at K = 64.  One JSON line.

    python tools/kzg_set_bench.py [--log 20] [--reps 5] [--k 64] [--ts 1,2,4,8,32]

The string is built from a known tau (G1 powers and 33 G2 powers), so every opening verifies.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import kzg_bench as kb  # noqa: E402
from octopuszk_amd import kzg, lib as _lib, wire  # noqa: E402
from octopuszk_amd import zksnark as z  # noqa: E402
from octopuszk_amd.device import VarMsmWorkspace, _ptr, _stream  # noqa: E402
from octopuszk_amd.fft import FR, root_of_unity  # noqa: E402


class _String(kb._String):
    """kzg_bench's string with the G2 powers a SetVerifyKey of t_max = 32 reads"""

    def __init__(self, m):
        super().__init__(m)
        self.tau_g2 = z.batch_msm_dev(254, 16, wire.g2_wire(z.G2_ONE), [pow(kb.TAU, i, FR) for i in range(33)], 2)


def _points(t, salt=0):
    return [(0x123456789abcdef0123456789 * (i + 1) + salt) % FR for i in range(t)]


def run(log, reps, kbatch, ts):
    n = 1 << log
    L = _lib.load()
    s = _String(n // 2)
    ck = kzg.CommitKey.from_srs(s, n)
    vk = kzg.SetVerifyKey.from_srs(s, 32)
    rows = kb._random_rows(1, n, log)
    ck.bases(), ck.lagrange(n)
    torch.cuda.synchronize()
    res = {"n": n, "t": {}}
    quot = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    other = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
    val = torch.empty(32 * 32, dtype=torch.uint8, device="cuda")
    wsb = int(L.ozk_fr_poly_open_workspace_bytes(1, n))
    ws1 = torch.empty(max(wsb, 256), dtype=torch.uint8, device="cuda")
    om = wire.le32([root_of_unity(n)])
    msm = VarMsmWorkspace(n, 1)
    res["msm_ms"] = kb._event_ms(lambda: msm.run(ck.bases(), rows.reshape(-1), prepared=True), reps)
    for t in ts:
        pts = _points(t)
        host = wire.le32(pts)
        d_pts = wire.dev_bytes(host)
        r = {}
        wsb = int(L.ozk_fr_poly_open_set_workspace_bytes(1, n, t))
        ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device="cuda")
        r["poly_open_set_kernel_ms"] = kb._event_ms(lambda: _lib.check(L.ozk_fr_poly_open_set_dev(
            _ptr(rows), 1, n, n, t, wire.vp(host), _ptr(quot), n, _ptr(val), _ptr(ws), ws.numel(), _stream())), reps)

        def chain():
            # t divisions by one linear factor each, the quotient of one the dividend of the next
            src, dst = rows, quot
            for i in range(t):
                _lib.check(L.ozk_fr_poly_open_dev(_ptr(src), 1, n, n, _ptr(d_pts[32 * i:]), _ptr(dst), n, _ptr(val),
                                                  _ptr(ws1), ws1.numel(), _stream()))
                src, dst = dst, (other if dst is quot else quot)

        r["chained_poly_open_ms"] = kb._event_ms(chain, reps)
        if t <= kzg.SET_EVALS_T_MAX:
            wsb = int(L.ozk_fr_evals_open_set_workspace_bytes(1, n, t))
            ws2 = torch.empty(max(wsb, 256), dtype=torch.uint8, device="cuda")
            r["evals_open_set_kernel_ms"] = kb._event_ms(lambda: _lib.check(L.ozk_fr_evals_open_set_dev(
                _ptr(rows), 1, n, n, wire.vp(om), t, wire.vp(host), _ptr(quot), n, _ptr(val), _ptr(ws2), ws2.numel(),
                _stream())), reps)
            assert kzg.verify_set(vk, ck.open_set_evals(rows, pts)[0])
        r["open_set_ms"] = kb._median_ms(lambda: ck.open_set(rows, pts), reps)
        op = ck.open_set(rows, pts)[0]
        assert kzg.verify_set(vk, op)
        r["verify_set_ms"] = kb._median_ms(lambda: kzg.verify_set(vk, op), reps)
        if kbatch:
            # a batch of openings of short polynomials, half at one set and half at another
            small = kzg.CommitKey.from_srs(s, 64)
            short = kb._random_rows(kbatch, 64, 99)
            many = small.open_set(short[:kbatch // 2], pts) + small.open_set(short[kbatch // 2:], _points(t, 7))
            assert kzg.verify_set_all(vk, many)
            r["verify_set_all_k%d_ms" % kbatch] = kb._median_ms(lambda: kzg.verify_set_all(vk, many), reps)
        res["t"][str(t)] = r
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--ts", default="1,2,4,8,32")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"bench": "kzg_set", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "result": run(a.log, a.reps, a.k, [int(x) for x in a.ts.split(",")])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
