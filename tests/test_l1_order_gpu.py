"""The whole-bucket level 1 of the G1 MSM under both item orders (OZK_MSM_L1_ORDER: 0 by rank inside the sort bin, 1 by
part length over the whole MSM) and with the dense merges: the ACCUMULATE stage by itself over a poisoned scratch
(tests/msm_stage_util.py), its bucket records against exact integers (tests/msm_stage_ref.py check_buckets: bases
k_i G with known k_i), then the tail on the same buffer against the C oracle's bytes.  Every case forces
OZK_MSM_L1_WHOLE=1 and asserts which level-1 path ran (ozk_var_msm_last_l1_path).

Size: 2^13 + 5 pairs.  Shapes by the window size and the digit distribution (a scalar below 2^63 splits into (s, 0):
its digits are those of s, every other window gets nothing from it; a zero scalar gives no entry at all):
  c = 8   16 windows of 128 buckets in one sort bin each, four lanes per bucket in the top window: 15 workgroups of
          lane pairs (all merged densely) and 2 of four-lane groups.  Uniform scalars give buckets of ~128 entries
          (keys around 64).
  c = 5   26 windows of 16 buckets: 800 pair lanes padded to 832, then 64 four-lane lanes: workgroup 3 holds 64 lanes
          of pairs (32 of them padding), 64 of four-lane groups and 128 past the grid's end: MIXED and PARTIAL.
  c = 4   32 windows of 8 buckets: 496 pair lanes padded to 512 (two dense workgroups), then 32 four-lane lanes
          padded to 64: the last workgroup is PARTIAL and holds four-lane groups only.
  For c = 5 and c = 4 only the first few hundred scalars are non-zero, so that no bucket exceeds its lane limit.

Bite check (by reading, and on altered host builds of l1_whole.h; no broken kernel was run on a GPU), DESIGN.md
section 35:
  class bases off by one class      (base[k] = items with a key of k or above) the shortest non-empty class of a region
                                    gets slots past the region's end: k_bucket_items raises the fallback flag and
                                    every case here that expects the whole-bucket path fails on the path it asserts;
                                    test_l1_order_cpu.py pins whole_class_bases itself (every table but "zero" fails)
  key without the division by G     both item kernels use the one function, so the items stay a permutation and the
                                    records stay right: the order merely stops matching the trip counts.  No GPU case
                                    can see that; test_l1_order_cpu.py::test_key does
  dense merge pairing L with L + 1  every dense case: bucket j would get the sum of lanes j and j + 1: "point"
  waves 2 and 3 leave early         by reading: they would skip block_sync() while waves 0 and 1 wait: the kernel's
                                    only barrier is placed before the wave test for that reason."""
import numpy as np
import pytest

import msm_stage_ref as ref
import msm_stage_util as util
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

WHOLE, CHUNKED = 1, 0
N = (1 << 13) + 5
SEED = 61
LIMIT = 2 * 255          # l1_whole.h: WHOLE_G * WHOLE_LANE_MAX


@pytest.fixture(scope="module")
def g1():
    """bases k_i G (wire rows on the host) and the k_i"""
    import torch
    from octopuszk_amd import device as dev
    d = dev.gen_g1_bases(N, SEED)
    torch.cuda.synchronize()
    return d.cpu().numpy().reshape(N, 96).copy(), dev.gen_base_logs(N, SEED)


def _oracle(wire, scalars):
    from oracle import coracle
    return coracle.pippenger_g1(np.ascontiguousarray(wire).tobytes(), ref.scalar_bytes(scalars).tobytes(), len(scalars))


def _live_records(lay, tail, hist):
    recs = tail[lay["buckets"]:lay["buckets"] + 4 * lay["NB"] * lay["REC_WORDS"]].view("<u4").reshape(lay["NB"], -1)
    return recs[hist > 0].copy()


def _check_items(lay, items, hist, order):
    """The items k_bucket_items left at the head of the accumulate scratch, (entry offset, count, bucket id, G) per
    bucket: a permutation of the buckets with their counts and entry offsets under either order;
      order 1: the ordinary windows' items first, then the top window's, each region descending by key
               (min(ceil(count / G), 127));
      order 0: item rank * nbins + bin belongs to sort bin `bin`, the counts of a bin descending by rank.
    So a knob that was ignored fails here, though the bucket records are the same under both orders."""
    W, cb, lo, NH, NB = lay["W"], lay["cb"], lay["lo_bits"], lay["NH"], lay["NB"]
    nb, nbins = 1 << lo, W * NH
    off, cnt, bid, G = (items[:, k].astype(np.int64) for k in range(4))
    assert np.array_equal(np.sort(bid), np.arange(NB)), "the items are not a permutation of the buckets"
    assert np.array_equal(cnt, hist[bid])
    assert np.array_equal(off, (np.cumsum(hist) - hist)[bid]), "an item's entries do not start at the prefix sum of the counts"
    top = (bid >> cb) == W - 1
    assert (G[~top] == 2).all() and (G[top] == 4).all()
    key = np.minimum((cnt + G - 1) // G, 127)
    bins = (bid >> cb) * NH + ((bid & ((1 << cb) - 1)) >> lo)
    if order == 1:
        n0 = (W - 1) * NH * nb
        assert not top[:n0].any() and top[n0:].all()
        assert (np.diff(key[:n0]) <= 0).all() and (np.diff(key[n0:]) <= 0).all(), "a region's keys rise somewhere"
    else:
        assert np.array_equal(bins, np.arange(NB) % nbins)
        by_rank = cnt.reshape(nb, nbins)
        assert (np.diff(by_rank, axis=0) <= 0).all(), "a bin's counts rise with the rank"
    return key, top


def _case(monkeypatch, name, c, wire, logs, scalars, path=WHOLE, orders=(0, 1), dense=(1,), repeat=1, inspect=None, mixed_keys=False):
    """SORT once; then ACCUMULATE over a poisoned scratch + tail under every (order, dense) asked for, `repeat` times
    each: the path, the bucket records against the integers, the final bytes against the oracle, and the live records
    equal word for word over all runs of one build of the merges (the two merges add the same two operands)."""
    assert len(scalars) == N
    want_bytes = _oracle(wire, scalars)

    def body():
        st = util.Stages(N, 1)
        lay = st.lay
        assert lay["l1_whole"] == 1
        sorted0 = st.sort(st.upload(wire), st.upload(ref.scalar_bytes(scalars)))
        hist = ref.read_sorted(lay, sorted0)[1]
        if inspect:
            inspect(lay, sorted0)
        expected, first = None, None
        for order in orders:
            for dn in dense:
                def run():
                    nonlocal expected, first
                    for rep in range(repeat):
                        tail, sorted1, took = st.accum(0)
                        print("[l1-order] %s: order %d dense %d run %d: path %d (expected %d)" % (name, order, dn, rep, took, path))
                        assert took == path, (order, dn, took)
                        for off, size in ((lay["hist"], 4 * lay["NB"]), (lay["sent"], 8 * (lay["n"] * lay["W"] + 1))):
                            assert np.array_equal(sorted0[off:off + size], sorted1[off:off + size]), "ACCUMULATE changed the sorted set"
                        if path == WHOLE:      # (the chunked kernels overwrite the items with their slots)
                            items = st.accum_ws[:16 * lay["NB"]].cpu().numpy().view("<u4").reshape(-1, 4)
                            key, top = _check_items(lay, items, hist, order)
                            if mixed_keys and order == 0:   # this input's rank order is NOT the length order
                                assert (np.diff(key[~top]) > 0).any(), "the rank order came out sorted by key"
                        expected = ref.check_buckets(lay, tail, sorted0, logs, expected=expected)
                        recs = _live_records(lay, tail, hist)
                        if path == WHOLE:      # (the chunked path's records depend on no knob of this file)
                            if first is None:
                                first = recs
                            assert np.array_equal(recs, first), "bucket records differ between runs / orders / merges"
                        assert st.tail(1) == want_bytes, (order, dn)
                util.with_knobs(monkeypatch, {"OZK_MSM_L1_ORDER": order, "OZK_MSM_L1_DENSE": dn}, run)
    util.with_knobs(monkeypatch, {"OZK_MSM_C": c, "OZK_MSM_L1_WHOLE": 1, "OZK_MSM_SMALL_SORT": 0}, body)


def _digits(c, *windows):
    """scalars below 2^63 from their window digits: windows[w][i] is digit w of scalar i (0 < digit <= 2^(c-1) - 1
    keeps the signed recoding from carrying); shorter lists are padded with zero scalars"""
    n = max(len(w) for w in windows)
    out = []
    for i in range(n):
        s = 0
        for w, ds in enumerate(windows):
            d = int(ds[i]) if i < len(ds) else 0
            assert 0 <= d < (1 << (c - 1))
            s |= d << (c * w)
        assert s < (1 << 63)
        out.append(s)
    return out + [0] * (N - n)


def _counts_to_digits(counts):
    """digit list in which digit d + 1 occurs counts[d] times"""
    return [d + 1 for d, k in enumerate(counts) for _ in range(k)]


def test_uniform_scalars(g1, monkeypatch):
    """case 1: also the quad-permute merges alone (OZK_MSM_L1_DENSE=0) under both orders"""
    wire, logs = g1
    _case(monkeypatch, "uniform", 8, wire, logs, ref.uniform_scalars(N, 1), dense=(1, 0), mixed_keys=True)


def test_one_bucket_one_class_and_ties_only(g1, monkeypatch):
    """cases 2, 3, 7: window 0: 100 buckets of 4 entries each (one class, ties only); window 1: every digit 77 (one
    bucket of 400 entries: the clamp class alone); windows 2 .. 15: no entry at all"""
    wire, logs = g1
    _case(monkeypatch, "ties", 8, wire, logs, _digits(8, _counts_to_digits([4] * 100), [77] * 400))


def test_counts_1_2_3(g1, monkeypatch):
    """case 4: buckets of 1, 2 and 3 entries: lane 1's part is empty or one entry (keys 1, 1, 2), beside buckets of 40"""
    wire, logs = g1
    _case(monkeypatch, "counts_1_2_3", 8, wire, logs, _digits(8, _counts_to_digits([1, 2, 3] * 30 + [40] * 20)))


@pytest.mark.parametrize("extra,path", [(0, WHOLE), (1, CHUNKED)], ids=["limit", "limit_plus_1"])
def test_lane_limit(extra, path, g1, monkeypatch):
    """case 5: one bucket of exactly 2 x 255 entries takes the whole-bucket path, one more sends the MSM down the
    chunked one; the result is right either way"""
    wire, logs = g1
    _case(monkeypatch, "limit+%d" % extra, 8, wire, logs, _digits(8, _counts_to_digits([LIMIT + extra] + [20] * 100)), path=path)


def test_clamp_class_shared(g1, monkeypatch):
    """case 6: counts 254 (key 127 on its own right), 255, 300, 509 (clamped to 127) beside shorter ones"""
    wire, logs = g1
    _case(monkeypatch, "clamp", 8, wire, logs, _digits(8, _counts_to_digits([254, 255, 300, 509, 253, 252, 100, 7] + [30] * 50)))


def test_halves_that_cancel_double_and_oppose(g1, monkeypatch):
    """cases 8, 9: bases P, -P alternating (even index P).
    window 0, digits 1 .. 100: {P, P, P, -P}: whatever the order inside the bucket, the half that holds -P sums to O
      and the other to 2 P; the sorted set is read back and BOTH arrangements must occur (first half O, second half O);
    window 1, digits 1 .. 50: {P, P}: the lanes hold P and P, the merge doubles;
    window 1, digits 51 .. 100: {P, -P}: the merge adds P and -P."""
    wire, logs = g1
    rec = wire[0].copy()
    y = int.from_bytes(rec[32:64].tobytes(), "little")
    neg = rec.copy()
    neg[32:64] = np.frombuffer((o.Q - y).to_bytes(32, "little"), dtype=np.uint8)
    recs = np.tile(rec, (N, 1))
    recs[1::2] = neg
    lg = [logs[0], -logs[0]] * (N // 2) + [logs[0]]
    sc = [0] * N
    for j in range(100):        # three even pairs (P) and one odd (-P): second of the four by index, or last
        for i in ((0, 1, 2, 4) if j % 2 else (0, 2, 4, 5)):
            sc[8 * j + i] = j + 1
    for j in range(100):        # pairs 1000 + 4 j + {0, 2} are P, + 1 is -P
        for i in ((0, 2) if j < 50 else (0, 1)):
            sc[1000 + 4 * j + i] = (j + 1) << 8

    def inspect(lay, sorted0):
        _, hist, idx, sign, bid = ref.read_sorted(lay, sorted0)
        assert not sign.any()
        first_o = second_o = 0
        for b in range(100):            # (digit d lives in bucket d - 1 of its window)
            e = np.nonzero(bid == b)[0]
            assert len(e) == 4 and hist[b] == 4
            s = [1 - 2 * int(idx[k] % 2) for k in e]           # +1 for P, -1 for -P, in the order the lanes read them
            first_o += s[0] + s[1] == 0
            second_o += s[2] + s[3] == 0
        print("[l1-order] halves: first half O in %d buckets, second half O in %d" % (first_o, second_o))
        assert first_o + second_o == 100 and first_o > 0 and second_o > 0
    _case(monkeypatch, "halves", 8, recs, lg, sc, inspect=inspect)


@pytest.mark.parametrize("c,nonzero", [(5, 320), (4, 150)], ids=["mixed_partial_workgroup", "partial_four_lane_workgroup"])
def test_partial_and_mixed_workgroups(c, nonzero, g1, monkeypatch):
    """case 10 (the module docstring says how the two grids come about): `nonzero` uniform scalars, the rest zero"""
    wire, logs = g1
    _case(monkeypatch, "c%d" % c, c, wire, logs, ref.uniform_scalars(nonzero, 10 + c) + [0] * (N - nonzero))


def test_three_runs_give_equal_records(g1, monkeypatch):
    """case 11: which lane group serves which bucket may differ from run to run under the length order (the slots of a
    class are handed out by atomics); the records and the result bytes may not"""
    wire, logs = g1
    _case(monkeypatch, "three runs", 8, wire, logs, ref.uniform_scalars(N, 2), repeat=3)
