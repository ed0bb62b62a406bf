"""Timings of KZG openings at every coset at once on one GPU; writes profiles/kzg_all_2pL.json and
prints the same JSON as one line.

    python tools/kzg_all_bench.py --logn 16 --coset 1 [--reps 5] [--mac-terms 16] [--mac-logn 17] [--out PATH]

open_all at n = 2^L and the given coset size, each stage by wall clock with a synchronise on both sides (median of
--reps): the key build (once), the Fr transforms, the multiply-accumulate, the inverse group FFT, the group FFT, the
compression; the whole open_all and its time per proof; CommitKey.open at one point of the same n (median of five)
as the baseline for the whole.  Three proofs are compared with the single openings' bytes.

The multiply-accumulate alone at --mac-terms terms over 2^--mac-logn outputs, under HIP events (the ozk_points_mac_dev
call: its recoding kernel and its accumulating kernel), and in the same run on the same points and scalars its
baseline: `terms` calls of ozk_points_mul_dev joined by `terms - 1` of ozk_points_add_dev.  The two outputs must be
equal byte for byte.

Beside each measured figure stands the counted one (DESIGN.md sections 15, 16, 21): multiplications at about 170 G
mulmod/s; a ladder whose wave adds at every step (64 lanes, 64 scalars) is 128 x (7 + 11) = 2300 and two inversions
of 35, the group FFT's butterfly ladder 1610 + 22, the multiply-accumulate 128 x 7 + terms x 128 x 11 and one inversion
per output.  chain_over_mac_counted_uniform_waves is the ratio were no lane to wait for another (1610 per ladder
against 127 x 7 + terms x 64 x 11).
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
from octopuszk_amd import codec, kzg, lib as _lib, vectors  # noqa: E402
from octopuszk_amd import device as dev  # noqa: E402
from octopuszk_amd.device import _ptr, _stream  # noqa: E402
from octopuszk_amd.fft import FR, root_of_unity  # noqa: E402

RATE = 170e9                   # mulmod/s, DESIGN.md section 3
LADDER, LADDER_DIVERGED, BUTTERFLY, INVERSION = 1610, 128 * (7 + 11), 22, 35


def _ms(mults):
    return round(mults / RATE * 1e3, 4)


def _fft_ladders(m, inverse):
    """the ladders of one group FFT of m points"""
    log = m.bit_length() - 1
    return (m // 2) * log - (m - 1) + (m // 2 if inverse else 0)


def open_all_stages(log, l, reps):
    n = 1 << log
    r = n // l
    s = kb._String(n // 2)
    ck = kzg.CommitKey.from_srs(s, n)
    ck.bases()
    rows = kb._random_rows(1, n, log)
    row = rows[0]
    torch.cuda.synchronize()
    key = kzg.OpenAllKey.from_srs(s, n, coset=l, commit_key=ck)
    res = {"n": n, "coset": l, "cosets": r}
    res["key_build_ms"] = kb._median_ms(lambda: (setattr(key, "_tables", None), key.tables()), 1)
    res["key_build_counted_ms"] = _ms(l * _fft_ladders(2 * r, False) * (LADDER + BUTTERFLY))
    c = key.coefficient_ffts(row)
    u = key.mac(c)
    h = key.upper_half(u)
    pts = key.proofs_of(h)
    res["values_fft_ms"] = kb._median_ms(lambda: key.values(row), reps)
    res["coefficient_ffts_ms"] = kb._median_ms(lambda: key.coefficient_ffts(row), reps)
    res["mac_ms"] = kb._median_ms(lambda: key.mac(c), reps)
    res["mac_counted_ms"] = _ms(2 * r * 128 * (7 + 11 * l))
    res["inverse_group_fft_ms"] = kb._median_ms(lambda: key.upper_half(u), reps)
    res["inverse_group_fft_counted_ms"] = _ms(_fft_ladders(2 * r, True) * (LADDER + BUTTERFLY))
    res["group_fft_ms"] = kb._median_ms(lambda: key.proofs_of(h), reps)
    res["group_fft_counted_ms"] = _ms(_fft_ladders(r, False) * (LADDER + BUTTERFLY))
    res["compress_ms"] = kb._median_ms(lambda: codec.compress_g1(pts), reps)
    res["commit_ms"] = kb._median_ms(lambda: ck.commit(rows), reps)
    res["open_all_ms"] = kb._median_ms(lambda: key.open_all(rows), reps)
    res["open_all_per_proof_us"] = round(res["open_all_ms"] * 1e3 / r, 4)
    counted = res["mac_counted_ms"] + res["inverse_group_fft_counted_ms"] + res["group_fft_counted_ms"]
    res["open_all_counted_per_proof_us"] = round(counted * 1e3 / r, 4)
    z = [pow(root_of_unity(n), 1, FR)]
    res["single_open_ms"] = kb._median_ms(lambda: ck.open(rows, z), 5)
    res["per_proof_over_single_open"] = round(res["open_all_per_proof_us"] / (res["single_open_ms"] * 1e3), 6)
    res["per_proof_below_1_percent_of_single_open"] = res["per_proof_over_single_open"] < 0.01
    # three proofs against the single openings' bytes
    a = key.open_all(rows)[0]
    proofs = bytes(a.proofs.cpu().numpy())
    omega = root_of_unity(n)
    for k in sorted({0, 1, r - 1}):
        if l == 1:
            want = ck.open(rows, [pow(omega, k, FR)])[0].pi
        else:
            want = ck.open_set(rows, [pow(omega, k + r * j, FR) for j in range(l)])[0].pi
        assert proofs[32 * k:32 * k + 32] == want, "proof %d differs from the single opening" % k
    res["proofs_checked_against_single_openings"] = 3
    return res


def mac_against_chain(terms, log, reps):
    n = 1 << log
    L = _lib.load()
    points = dev.gen_g1_bases(terms * n, seed=23)
    scalars = kb._random_rows(1, terms * n, 7).reshape(-1)
    table = vectors.points_mac_prepare(points, terms, n)
    ws = torch.empty(int(L.ozk_points_mac_workspace_bytes(terms, n, 1)), dtype=torch.uint8, device="cuda")
    out = torch.empty(96 * n, dtype=torch.uint8, device="cuda")
    acc, prod = torch.empty_like(out), torch.empty_like(out)
    torch.cuda.synchronize()

    def mac():
        _lib.check(L.ozk_points_mac_dev(_ptr(table), _ptr(scalars), terms, n, 1, _ptr(out), None, _ptr(ws), ws.numel(),
                                        _stream()))

    def chain():
        for v in range(terms):
            dst = acc if v == 0 else prod
            _lib.check(L.ozk_points_mul_dev(_ptr(points[96 * n * v:]), _ptr(scalars[32 * n * v:]), n, 1, _ptr(dst), None,
                                            _stream()))
            if v:
                _lib.check(L.ozk_points_add_dev(_ptr(acc), _ptr(prod), n, 1, 0, _ptr(acc), _stream()))

    res = {"terms": terms, "n": n}
    res["mac_ms"] = kb._event_ms(mac, reps)
    res["chain_ms"] = kb._event_ms(chain, reps)
    res["mac_counted_ms"] = _ms(n * (128 * (7 + 11 * terms) + INVERSION))
    res["chain_counted_ms"] = _ms(n * terms * (LADDER_DIVERGED + 2 * INVERSION))
    res["chain_over_mac_counted_uniform_waves"] = round(terms * LADDER / (127 * 7 + terms * 64 * 11), 4)
    res["chain_over_mac"] = round(res["chain_ms"] / res["mac_ms"], 4)
    res["chain_over_mac_counted"] = round(res["chain_counted_ms"] / res["mac_counted_ms"], 4)
    res["mac_faster_than_chain"] = res["mac_ms"] < res["chain_ms"]
    torch.cuda.synchronize()
    res["outputs_equal"] = bool(torch.equal(out, acc))
    assert res["outputs_equal"], "the multiply-accumulate and its chain differ"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--logn", type=int, default=16)
    ap.add_argument("--coset", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--mac-terms", type=int, default=16)
    ap.add_argument("--mac-logn", type=int, default=17)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"bench": "kzg_all", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "open_all": open_all_stages(a.logn, a.coset, a.reps)}
    if a.mac_terms:
        out["mac"] = mac_against_chain(a.mac_terms, a.mac_logn, a.reps)
    path = a.out or os.path.join(ROOT, "profiles", "kzg_all_2p%d.json" % a.logn)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
