"""The peeled start of a bucket part in the whole-bucket level 1 (msm_var.cuh k_l1_whole: entry 0 is a copy, entry 1 the
affine + affine addition ec.cuh xyzz_add_affine2_lazy, entries 2 and on the mixed addition), against the C oracle's
bytes, with the whole-bucket path on (asserted) and again on the chunked path (OZK_MSM_L1_WHOLE=0).

As in test_l1_whole_buckets_gpu.py the shaped cases use scalars below 2^15 at c = 16: the GLV split of such a scalar
is (k, 0), so every entry lands in window 0 in the bucket of its own value, on a lane pair whose parts are the first
ceil(count / 2) entries and the rest (l1_whole.h whole_part).  The sort ranks the entries of a bucket with atomics, so
their order inside a bucket is not fixed: the doubling case is built from equal entries (any order doubles), the
cancelling and the infinity-marker cases from many buckets in every arrangement, and all of them are correct in any
order.  Sizes: the shaped cases take just over 2^13 pairs (the items of the 2^15-bucket windows of c = 16 must fit the
accumulate scratch, which grows with n: at 4101 pairs the plan keeps the chunked path), the random case 2^13.
"""
import numpy as np
import pytest

from oracle import bn254 as o

pytestmark = pytest.mark.gpu

WHOLE, CHUNKED = 1, 0
N_MAX = 1 << 14
SEED = 53


@pytest.fixture(scope="module")
def g1():
    """bases k_i G in wire form as host records of 96 bytes"""
    import torch
    from octopuszk_amd import device as dev
    d = dev.gen_g1_bases(N_MAX, SEED)
    torch.cuda.synchronize()
    return d.cpu().numpy().copy().reshape(N_MAX, 96)


def _scalars(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(-1, 32).copy()


def _negated(rec):
    y = int.from_bytes(rec[32:64].tobytes(), "little")
    out = rec.copy()
    out[32:64] = np.frombuffer(((o.Q - y) % o.Q).to_bytes(32, "little"), dtype=np.uint8)
    return out


def _infinity(rec):
    out = rec.copy()
    out[64:96] = 0
    return out


def _run(recs, sc, n):
    import torch
    from octopuszk_amd import device as dev, lib
    ws = dev.VarMsmWorkspace(n, 1)
    out = ws.run(torch.from_numpy(recs.reshape(-1).copy()).cuda(), torch.from_numpy(np.ascontiguousarray(sc).reshape(-1)).cuda())
    torch.cuda.synchronize()
    return bytes(out.cpu().numpy()), lib.load().ozk_var_msm_last_l1_path()


def _both_paths(monkeypatch, c, recs, sc):
    from oracle import coracle
    from octopuszk_amd import lib
    L = lib.load()
    n = len(sc)
    assert 4096 < n <= N_MAX and recs.shape == (n, 96)
    want = coracle.pippenger_g1(recs.tobytes(), np.ascontiguousarray(sc).tobytes(), n)
    try:
        monkeypatch.setenv("OZK_MSM_C", str(c))
        for knob, expect in (("1", WHOLE), ("0", CHUNKED)):
            monkeypatch.setenv("OZK_MSM_L1_WHOLE", knob)
            L.ozk_tuning_reload()
            got, took = _run(recs, sc, n)
            print("OZK_MSM_L1_WHOLE=%s c=%d n=%d: path %d (expected %d), bytes %s" % (knob, c, n, took, expect, got == want))
            assert took == expect, (knob, took)
            assert got == want, knob
    finally:
        monkeypatch.delenv("OZK_MSM_C", raising=False)
        monkeypatch.delenv("OZK_MSM_L1_WHOLE", raising=False)
        L.ozk_tuning_reload()
    return want


@pytest.mark.parametrize("count", [1, 2, 3, 4, 5])
def test_buckets_of_exactly(count, g1, monkeypatch):
    """parts of (1, 0), (1, 1), (2, 1), (2, 2) and (3, 2) entries: a copy alone, the peeled addition alone, and the
    first turn of the loop after it"""
    m = 8200 // count + 1
    n = m * count
    vals = [1 + i // count for i in range(n)]
    _both_paths(monkeypatch, 16, g1[:n], _scalars(vals))


def test_equal_entries_double_in_the_peeled_addition(g1, monkeypatch):
    """four copies of one (base, scalar) pair per bucket: each lane's two entries are the same point"""
    m = 2050
    recs = np.repeat(g1[:m], 4, axis=0)
    vals = np.repeat(np.arange(1, m + 1), 4)
    _both_paths(monkeypatch, 16, recs, _scalars(vals))


@pytest.mark.parametrize("count", [4, 6])
def test_cancelling_entries(count, g1, monkeypatch):
    """every bucket holds P, -P and count - 2 other points, in every rotation: where a part starts with P, -P the
    peeled addition gives infinity and the later entries (count 6) and the merge land on it"""
    m = 8400 // count
    recs, vals = [], []
    for b in range(m):
        own = [g1[count * b + k] for k in range(count - 1)]
        bucket = [own[0], _negated(own[0])] + own[1:]
        r = b % count
        recs += bucket[r:] + bucket[:r]
        vals += [b + 1] * count
    _both_paths(monkeypatch, 16, np.stack(recs), _scalars(vals))


def test_cancelling_pairs_alone_sum_to_infinity(g1, monkeypatch):
    """P, -P, P', -P' in every bucket: each lane's part cancels, or the merge does"""
    m = 2050
    recs, vals = [], []
    for b in range(m):
        p, q = g1[2 * b], g1[2 * b + 1]
        recs += [[p, _negated(p), q, _negated(q)], [p, q, _negated(q), _negated(p)]][b % 2]
        vals += [b + 1] * 4
    want = _both_paths(monkeypatch, 16, np.stack(recs), _scalars(vals))
    assert want == o.g1_out_le(o.G1.zero_affine)


@pytest.mark.parametrize("where", ["entry0", "entry1", "both", "mixed"])
def test_infinity_marker_at_the_start_of_a_part(where, g1, monkeypatch):
    """bases with wire Z = 0 as a part's entry 0, as its entry 1 and as both, in buckets of 4 (parts of 2) and of 6
    (parts of 3: a loop turn follows); `mixed` rotates through the three and an all-infinity bucket"""
    patterns = {"entry0": [1, 0, 0], "entry1": [0, 1, 0], "both": [1, 1, 0]}
    recs, vals = [], []
    b = 0
    while len(vals) < 8200:
        b += 1
        per_part = 2 + b % 2
        if where == "mixed":
            pat = [[1, 0, 0], [0, 1, 0], [1, 1, 0], [1, 1, 1]][b % 4]
        else:
            pat = patterns[where]
        for k in range(2 * per_part):
            rec = g1[len(vals)]
            recs.append(_infinity(rec) if pat[k % per_part] else rec)
            vals.append(b)
    _both_paths(monkeypatch, 16, np.stack(recs), _scalars(vals))


def test_random_scalars(g1, monkeypatch):
    """uniform scalars at n = 2^13, c = 11: mean 16 entries per bucket, both signs, four-lane groups in the top window"""
    n = 1 << 13
    rng = np.random.default_rng(211)
    sc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sc[:, 31] &= 0x1F
    _both_paths(monkeypatch, 11, g1[:n], sc)
