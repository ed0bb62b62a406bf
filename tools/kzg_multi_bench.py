"""Timings of the KZG multi-opening on one GPU, n = 2^20 by default, 16 rows.  One JSON line.

(a) ozk_fr_rows_combine_groups_dev at (k, groups) = (16, 2), the rows interleaved, beside two ozk_fr_rows_combine_dev
    calls over all 16 rows with zero weights on the rows of the other group (the only arbitrary grouping that entry
    allows without a copy), under HIP events;
(b) ozk_fr_poly_eval_set_dev at t in 1, 2, 4, 8 over the 16 rows beside t calls of ozk_fr_poly_eval_dev over the same
    rows, under HIP events;
(c) open_multi and verify_multi for 13 rows at {z} and 3 rows at {z, z w} beside the two open_set_combined /
    verify_set_combined calls that cover the same statement, by wall clock with a synchronise, and the lone G1 MSM of
    the same n for scale.

    python tools/kzg_multi_bench.py [--log 20] [--reps 5] [--k 16] [--parts combine,eval,protocol]

--parts names the measurements to make (all three by default); (b) reports the three alternated rounds beside the
middle one.

The string is built from a known tau, so every opening verifies.
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
    """kzg_bench's string with the three G2 powers a SetVerifyKey of t_max = 2 reads"""

    def __init__(self, m):
        super().__init__(m)
        self.tau_g2 = z.batch_msm_dev(254, 16, wire.g2_wire(z.G2_ONE), [pow(kb.TAU, i, FR) for i in range(3)], 2)


def _points(t, salt=0):
    return [(0x123456789abcdef0123456789 * (i + 1) + salt) % FR for i in range(t)]


PARTS = ("combine", "eval", "protocol")


def run(log, reps, k, parts=PARTS):
    n = 1 << log
    L = _lib.load()
    rows = kb._random_rows(k, n, log)
    res = {"n": n, "k": k}

    if "combine" in parts:
        _combine(L, rows, k, n, reps, res)
    if "eval" in parts:
        _eval(L, rows, k, n, reps, res)
    if "protocol" in parts:
        _protocol(rows, k, n, reps, res)
    return res


def _combine(L, rows, k, n, reps, res):
    # (a) the grouped combine
    group_of = [i % 2 for i in range(k)]
    weights = [(0xabcdef0123456789 * (i + 3)) % FR for i in range(k)]
    d_w = wire.dev_bytes(wire.le32(weights))
    d_w0 = [wire.dev_bytes(wire.le32([w if group_of[i] == g else 0 for i, w in enumerate(weights)])) for g in (0, 1)]
    ids = b"".join(g.to_bytes(4, "little") for g in group_of)
    out = torch.empty((2, n * 32), dtype=torch.uint8, device="cuda")
    ref = torch.empty((2, n * 32), dtype=torch.uint8, device="cuda")

    def grouped():
        _lib.check(L.ozk_fr_rows_combine_groups_dev(_ptr(rows), k, n, n, _ptr(d_w), wire.vp(ids), 2, _ptr(out), n, _stream()))

    def zero_weights():
        for g in (0, 1):
            _lib.check(L.ozk_fr_rows_combine_dev(_ptr(rows), k, n, n, _ptr(d_w0[g]), _ptr(ref[g]), _stream()))

    # alternating, so that both see the same machine
    a_ms, b_ms = [], []
    for _ in range(3):
        a_ms.append(kb._event_ms(grouped, reps))
        b_ms.append(kb._event_ms(zero_weights, reps))
    assert torch.equal(out, ref)
    res["combine"] = {"rows_combine_groups_ms": sorted(a_ms)[1], "two_rows_combine_zero_weights_ms": sorted(b_ms)[1],
                      "rows_combine_groups_rounds_ms": a_ms, "two_rows_combine_zero_weights_rounds_ms": b_ms,
                      "bytes_read_grouped": k * n * 32, "bytes_read_zero_weights": 2 * k * n * 32}


def _eval(L, rows, k, n, reps, res):
    # (b) the values
    res["eval"] = {}
    d_val = torch.empty(k * 8 * 32, dtype=torch.uint8, device="cuda")
    ws_e = torch.empty(int(L.ozk_fr_poly_eval_workspace_bytes(k)), dtype=torch.uint8, device="cuda")
    for t in (1, 2, 4, 8):
        pts = _points(t)
        host = wire.le32(pts * k)
        wsb = int(L.ozk_fr_poly_eval_set_workspace_bytes(k, n, t))
        ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device="cuda")
        each = [wire.le32([p]) for p in pts]

        def eval_set():
            _lib.check(L.ozk_fr_poly_eval_set_dev(_ptr(rows), k, n, n, t, wire.vp(host), _ptr(d_val), _ptr(ws), ws.numel(),
                                                  _stream()))

        def eval_calls():
            for i in range(t):
                _lib.check(L.ozk_fr_poly_eval_dev(_ptr(rows), k, n, n, wire.vp(each[i]), _ptr(d_val[32 * k * i:]), _ptr(ws_e),
                                                  ws_e.numel(), _stream()))

        a_ms, b_ms = [], []
        for _ in range(3):
            a_ms.append(kb._event_ms(eval_set, reps))
            b_ms.append(kb._event_ms(eval_calls, reps))
        res["eval"][str(t)] = {"poly_eval_set_ms": sorted(a_ms)[1], "t_poly_eval_calls_ms": sorted(b_ms)[1],
                               "t_poly_eval_calls_rounds_ms": b_ms}


def _protocol(rows, k, n, reps, res):
    # (c) the protocol
    s = _String(n // 2)
    ck = kzg.CommitKey.from_srs(s, n)
    vk, svk = kzg.VerifyKey.from_srs(s), kzg.SetVerifyKey.from_srs(s, 2)
    ck.bases()
    torch.cuda.synchronize()
    msm = VarMsmWorkspace(n, 1)
    res["msm_ms"] = kb._event_ms(lambda: msm.run(ck.bases(), rows[0], prepared=True), reps)
    zpt = 0x123456789abcdef0123456789 % FR
    both = [zpt, zpt * root_of_unity(n) % FR]
    pair = max(k - 3, 1)                                  # the rows opened at z alone; the rest also at z w
    sets = [[zpt]] * pair + [both] * (k - pair)
    commitments = ck.commit(rows)
    res["commit_ms"] = kb._median_ms(lambda: ck.commit(rows), reps)
    res["open_multi_ms"] = kb._median_ms(lambda: ck.open_multi(rows, sets), reps)
    res["open_multi_given_commitments_ms"] = kb._median_ms(lambda: ck.open_multi(rows, sets, commitments=commitments), reps)
    op = ck.open_multi(rows, sets, commitments=commitments)
    assert kzg.verify_multi(vk, op)
    res["verify_multi_ms"] = kb._median_ms(lambda: kzg.verify_multi(vk, op), reps)

    def two_set_openings():
        return ck.open_set_combined(rows[:pair], [zpt]), ck.open_set_combined(rows[pair:], both)

    res["two_open_set_combined_ms"] = kb._median_ms(two_set_openings, reps)
    (c1, y1, pi1), (c2, y2, pi2) = two_set_openings()

    def two_set_checks():
        return kzg.verify_set_combined(svk, c1, [zpt], y1, pi1) and kzg.verify_set_combined(svk, c2, both, y2, pi2)

    assert two_set_checks()
    res["two_verify_set_combined_ms"] = kb._median_ms(two_set_checks, reps)
    values = sum(len(row) for row in sets)
    res["bytes"] = {"multi_opening": len(op.to_bytes()), "multi_proof_points": 64, "two_set_proofs": 64,
                    "verify_key": len(vk.to_bytes()), "set_verify_key_t2": len(svk.to_bytes()),
                    "statement_values": values}
    res["pairings"] = {"verify_multi": 2, "two_verify_set_combined": 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--parts", default=",".join(PARTS))
    a = ap.parse_args()
    parts = tuple(a.parts.split(","))
    if not parts or any(p not in PARTS for p in parts):
        ap.error("--parts takes a comma-separated subset of %s" % ", ".join(PARTS))
    torch.cuda.set_device(0)
    out = {"bench": "kzg_multi", "device": torch.cuda.get_device_name(0), "reps": a.reps, "result": run(a.log, a.reps, a.k, parts)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
