"""The stage contracts of the variable-base MSM without a GPU: the layout query is pinned, the host model of the
recoding (tests/msm_stage_ref.py) reconstructs every scalar for every window size and mode and agrees with the host
build of signed_digit_codes, the shape builders give the bins the GPU cases rely on, and the two checkers accept
valid buffers built on the host and reject every corruption, naming the clause."""
import ctypes
import importlib.util
import os
import random

import numpy as np
import pytest

import msm_stage_ref as ref
from multi_msm_ref import LAM
from oracle import bn254 as o
from test_glv_split import codes as host_codes
from test_host_arith import hc  # noqa: F401  (fixture)
from test_msm_plans_gpu import _GLV_EDGE

HERE = os.path.dirname(os.path.abspath(__file__))
UNREDUCED = [o.R, o.R + 1, (1 << 256) - 1, (1 << 256) - 2, 5 * o.R + 7, (1 << 255) + 1, (1 << 256) - o.R]


@pytest.fixture(scope="module")
def L():
    from octopuszk_amd import build, lib
    build.build(verbose=False)
    return lib.load()


def _knobs(L, monkeypatch, env, body):
    try:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        L.ozk_tuning_reload()
        return body()
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)
        L.ozk_tuning_reload()


# ---------------------------------------------------------------------------------------------------- the layout query
def _tool():
    spec = importlib.util.spec_from_file_location("dump_msm_layout", os.path.join(HERE, "..", "tools", "dump_msm_layout.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _check_layout(L, n, t):
    a256 = lambda v: v % 256 == 0
    c, w = ctypes.c_int32(), ctypes.c_int32()
    assert L.ozk_var_msm_plan(n, ctypes.byref(c), ctypes.byref(w)) == 0
    for prepared in (0, 1):
        lay = ref.stage_layout(L, n, t, prepared)
        assert (lay["c"], lay["W"], lay["glv"]) == (c.value, w.value, L.ozk_var_msm_glv(n)), (n, t)
        assert lay["n"] == (2 * n if lay["glv"] else n) and lay["cb"] == lay["c"] - lay["sd"]
        assert lay["NH"] << lay["lo_bits"] == 1 << lay["cb"] and lay["nblk"] == (lay["n"] + 4095) // 4096
        assert lay["big_thresh"] == max(lay["n"] // 64, 1 << 16)
        assert (lay["AFF_WORDS"], lay["REC_WORDS"], lay["REC_TAG"]) == ((16, 40, 36) if t == 1 else (32, 76, 72))
        NB, cap = lay["NB"], lay["n"] * lay["W"]
        arrays = [("hist", 4 * NB), ("total", 16), ("sent", 8 * (cap + 1))]
        if prepared:
            assert lay["aff"] == -1
            assert {k: lay[k] for k in ("hist", "total", "sent")} == {k: ref.stage_layout(L, n, t, 0)[k] for k in ("hist", "total", "sent")}
        else:
            arrays.insert(0, ("aff", 4 * lay["n"] * lay["AFF_WORDS"]))
        for (name, size), nxt in zip(arrays, [lay[a[0]] for a in arrays[1:]] + [lay["sorted_bytes"]]):
            assert a256(lay[name]) and lay[name] >= 0 and lay[name] + size <= nxt, (n, t, prepared, name)
        tail = [("buckets", 4 * NB * lay["REC_WORDS"]), ("hist_t", 4 * NB)]
        for (name, size), nxt in zip(tail, [lay["hist_t"], lay["tail_bytes"]]):
            assert a256(lay[name]) and lay[name] >= 0 and lay[name] + size <= nxt, (n, t, prepared, name)


@pytest.mark.parametrize("type_", [1, 2])
def test_layout_query_is_consistent_at_every_pinned_size(L, type_, monkeypatch):
    tool = _tool()
    for n in tool.SIZES:
        _check_layout(L, n, type_)
    for name, val in tool.KNOBS:
        _knobs(L, monkeypatch, {name: val}, lambda: [_check_layout(L, n, type_) for n in tool.KNOB_SIZES])


def test_layout_query_follows_the_knobs(L, monkeypatch):
    assert ref.stage_layout(L, 4096, 1)["small_sort"] == 1 and ref.stage_layout(L, 4097, 1)["small_sort"] == 0
    lay = lambda: ref.stage_layout(L, 300, 1)
    assert _knobs(L, monkeypatch, {"OZK_MSM_SMALL_SORT": "0"}, lay)["small_sort"] == 0
    got = _knobs(L, monkeypatch, {"OZK_MSM_C": "9", "OZK_MSM_L1": "17", "OZK_MSM_SMALL_SORT": "0", "OZK_MSM_L1_WHOLE": "1"}, lay)
    assert (got["c"], got["cb"], got["L1"], got["NH"], got["l1_whole"]) == (9, 8, 17, 2, 1)
    assert _knobs(L, monkeypatch, {"OZK_MSM_L1_WHOLE": "0"}, lambda: ref.stage_layout(L, 4097, 1))["l1_whole"] == 0
    got = _knobs(L, monkeypatch, {"OZK_MSM_SIGNED": "0"}, lay)
    assert (got["sd"], got["cb"], got["lo_bits"]) == (0, got["c"], min(got["c"], 8))
    got = _knobs(L, monkeypatch, {"OZK_MSM_SIGNED": "0", "OZK_MSM_C": "12"}, lay)
    assert (got["sd"], got["cb"], got["lo_bits"], got["NH"]) == (0, 12, 8, 16)
    got = _knobs(L, monkeypatch, {"OZK_MSM_GLV": "0"}, lay)
    assert (got["glv"], got["n"], got["sd"], got["W"]) == (0, 300, 0, (256 + got["c"] - 1) // got["c"])
    assert ref.stage_layout(L, 300, 1)["small_sort"] == 1


def test_layout_query_rejects_bad_arguments(L):
    out = (ctypes.c_int64 * 22)()
    for n, t, ptr, count in ((0, 1, out, 22), ((1 << 24) + 1, 1, out, 22), (1, 1, None, 22), (1, 1, out, 21), (1, 3, out, 22)):
        assert L.ozk_var_msm_stage_layout(n, t, 0, ptr, count) == -1, (n, t, count)


# ---------------------------------------------------------------------------------------------------- the model
def _model_scalars():
    rng = random.Random(7)
    return _GLV_EDGE + UNREDUCED + [rng.randrange(1 << 256) for _ in range(24)] + [rng.randrange(o.R) for _ in range(24)]


@pytest.mark.parametrize("mode", ["signed", "unsigned", "glv0"])
def test_entries_reconstruct_every_scalar(mode):
    sc = _model_scalars()
    n = len(sc)
    for c in range(1, 17):
        lay = ref.plan_layout(n, c, glv=mode != "glv0", signed=mode == "signed")
        assert lay["sd"] == (1 if mode == "signed" and c >= 2 else 0)
        m = ref.Model(lay, sc)
        assert m.total == len(m.bid) == int(m.counts.sum())
        assert (m.b < (1 << lay["cb"])).all() and (m.w < lay["W"]).all() and (lay["sd"] or (m.b >= 1).all())
        assert lay["sd"] or not m.neg.any()
        for i, s in enumerate(sc):
            if mode == "glv0":
                assert m.reconstruct(i) == s, (c, hex(s))
                continue
            k1, k2 = m.reconstruct(i), m.reconstruct(n + i)
            assert (k1, k2) == (m.halves[i], m.halves[n + i]), (c, hex(s))
            assert (k1 + LAM * k2 - s) % o.R == 0 and abs(k1) < 1 << 127 and abs(k2) < 1 << 127, (c, hex(s))


def test_codes_equal_the_host_build_of_signed_digit_codes(hc):  # noqa: F811
    sc = _model_scalars()
    n = len(sc)
    for c in range(2, 17):
        lay = ref.plan_layout(n, c)
        m = ref.Model(lay, sc)
        for v, h in enumerate(m.halves):
            assert host_codes(hc, abs(h), c, lay["W"], int(h < 0)) == [int(x) for x in m.codes[v]], (c, v)


def test_small_scalars_split_without_the_lattice():
    """the shortcut of half_scalars"""
    from multi_msm_ref import glv_split
    for s in (0, 1, 128, (1 << 63) - 1, 77 << 16):
        assert glv_split(s) == (s, 0)


# ---------------------------------------------------------------------------------------------------- the shapes
@pytest.mark.parametrize("target", [ref.S2_TILE, ref.S2_TILE + 1, 2 * ref.S2_TILE + 1])
def test_shape_one_sort2_bin_of_whole_tiles(L, target):
    lay = ref.stage_layout(L, 1 << 14, 1)
    assert lay["small_sort"] == 0 and lay["sd"] == 1 and target <= lay["big_thresh"]
    # more entries than pairs: 2048 pairs put both halves into the bin (ref.SORT2_CASES, shared with the GPU test)
    _, m, hi = ref.skewed_bin_scalars(lay, target, seed=target, doubles=ref.SORT2_CASES[target])
    bins = m.bin_sizes()
    assert bins[0, hi] == target                      # "bin (window 0, hi 0) holds exactly 8704 / 8705 entries"
    assert hi == 0 or target > lay["n_in"]
    bins[0, hi] = 0
    assert bins.max() <= ref.S2_TILE                  # every other bin is a single tile
    assert -(-target // ref.S2_TILE) == {8704: 1, 8705: 2, 17409: 3}[target]


def test_split_of_r_minus_small():
    from multi_msm_ref import glv_split
    K, k2 = ref.neg_split_constants()
    assert k2 < 0
    for v in (1, 2, 128, 4097, (1 << 20) - 1, 1 << 29):
        assert glv_split(o.R - v) == (K - v, k2)


@pytest.mark.parametrize("over", [0, 1])
def test_shape_one_bin_at_the_big_threshold(L, over):
    lay = ref.stage_layout(L, (1 << 16) + (1 << 12), 1)
    assert lay["big_thresh"] == 1 << 16
    _, m, _ = ref.skewed_bin_scalars(lay, lay["big_thresh"] + over, seed=40 + over)
    bins = m.bin_sizes()
    assert bins[0, 0] == 65536 + over                 # "... exactly 65536 / 65537 entries"
    assert int((bins > lay["big_thresh"]).sum()) == over
    # k_sort2 walks 8 tiles; the big path cuts 65537 entries into 9 work items, the last of one entry
    assert -(-65536 // ref.S2_TILE) == 8 and -(-65537 // ref.SORTBIG_CHUNK) == 9 and 65537 % ref.SORTBIG_CHUNK == 1
    # the scan of the per-block counts takes several blocks of 4096 items
    assert lay["W"] * lay["NH"] * lay["nblk"] > 2 * 4096


def test_shape_two_big_bins_in_different_windows(L):
    lay = ref.stage_layout(L, 1 << 17, 1)
    m = ref.Model(lay, ref.negative_half_scalars(lay, 5))
    big = np.argwhere(m.bin_sizes() > lay["big_thresh"])
    assert len(big) >= 2 and len(set(int(w) for w, _ in big)) >= 2      # "two bins in different windows exceed big_thresh"
    negs = {(int(w), int(h)): int(m.neg[(m.w == w) & ((m.b >> lay["lo_bits"]) == h)].sum()) for w, h in big}
    # the sign bit goes through the big path, set and clear: big bins of mostly negative entries in two windows, and
    # one of mostly positive entries
    assert len({w for (w, h), k in negs.items() if k >= 1 << 15}) >= 2
    assert any(m.bin_sizes()[w, h] - k >= 1 << 15 for (w, h), k in negs.items())


def test_shape_empty_windows(L, monkeypatch):
    def body():
        lay = ref.stage_layout(L, 300, 1)
        assert lay["small_sort"] == 0
        m = ref.Model(lay, ref.low_window_scalars(lay, 3))
        assert not m.counts[3 << lay["cb"]:].any() and m.counts[:3 << lay["cb"]].any()    # "every bucket of window 3 is empty"
        return m
    _knobs(L, monkeypatch, {"OZK_MSM_SMALL_SORT": "0"}, body)
    lay = ref.stage_layout(L, 4097, 1)
    assert lay["nblk"] == 3 and lay["n"] - 2 * 4096 == 2                 # the last chunk of the first two-level size
    m = ref.Model(lay, ref.low_window_scalars(lay, 4))
    assert not m.counts[3 << lay["cb"]:].any()


# ---------------------------------------------------------------------------------------------------- the checkers bite
N_BITE = 300


def _bases(n, seed):
    rng = random.Random(seed)
    pts = [o.G1.mul(o.G1.one, rng.randrange(1, 1 << 64)) for _ in range(n)]     # Jacobian, Z != 1
    pts[3] = o.G1.zero
    pts[5] = (pts[5][0], pts[5][1], o.Q)                                        # a Z that reduces to zero
    pts[7] = o.G1.to_affine(pts[7])
    return pts


@pytest.fixture(scope="module")
def valid(L):
    """valid sorted sets of one input: two-level layout and one-launch layout"""
    sc = ref.uniform_scalars(N_BITE, 11)
    sc[:len(_GLV_EDGE)] = _GLV_EDGE
    bases = _bases(N_BITE, 12)
    out = {}
    # c = 11: 1024 buckets per window for 600 points, so that runs of one, runs of several and empty buckets all occur
    for kind, env in (("two_level", {"OZK_MSM_C": "11", "OZK_MSM_SMALL_SORT": "0"}), ("small", {"OZK_MSM_C": "11"})):
        os.environ.update(env)
        L.ozk_tuning_reload()
        try:
            lay = ref.stage_layout(L, N_BITE, 1)
        finally:
            for k in env:
                del os.environ[k]
            L.ozk_tuning_reload()
        assert lay["small_sort"] == (kind == "small")
        buf, m = ref.build_sorted_set(lay, sc, bases, np.random.default_rng(13))
        out[kind] = lay, buf, m
    return sc, bases, out


def _sent(lay, buf, total):
    return buf[lay["sent"]:lay["sent"] + 8 * total].view("<u4").reshape(total, 2)


def _fails(clause, lay, buf, sc, bases, m):
    with pytest.raises(ref.StageError) as e:
        ref.check_sorted_set(lay, buf, sc, bases, model=m)
    assert e.value.clause == clause, str(e.value)


@pytest.mark.parametrize("kind", ["two_level", "small"])
def test_checker_accepts_a_valid_sorted_set(valid, kind):
    sc, bases, sets = valid
    lay, buf, m = sets[kind]
    ref.check_sorted_set(lay, buf, sc, bases)
    ref.check_sorted_set(lay, buf, sc, bases, model=m)


def test_checker_rejects_every_corruption_of_the_sorted_set(valid):
    sc, bases, sets = valid
    lay, good, m = sets["two_level"]
    T, cb = m.total, lay["cb"]
    u32 = lambda buf, off, k: buf[off:off + 4 * k].view("<u4")

    def corrupt(clause, change):
        buf = good.copy()
        change(buf, _sent(lay, buf, T))
        _fails(clause, lay, buf, sc, bases, m)

    def drop_lower(buf, sent):
        u32(buf, lay["total"], 1)[0] = T - 1
    corrupt("total", drop_lower)

    def drop_keep(buf, sent):     # entry 10 gone, the rest moved up, the last slot keeps its old content
        sent[10:T - 1] = sent[11:T].copy()
    corrupt("multiset", drop_keep)

    def duplicate(buf, sent):
        sent[21] = sent[20]
    corrupt("multiset", duplicate)

    def to_next_bucket(buf, sent):    # the last entry of a run joins the run of the next bucket
        j = int(np.nonzero(sent[1:, 1] == sent[:-1, 1] + 1)[0][0])
        sent[j, 1] += 1
    corrupt("multiset", to_next_bucket)

    def flip_sign(buf, sent):
        sent[33, 0] ^= 0x80000000
    corrupt("multiset", flip_sign)

    empty = int(np.nonzero(m.counts == 0)[0][0])
    full = int(np.nonzero(m.counts > 0)[0][0])

    def hist_poison(buf, sent):
        u32(buf, lay["hist"], lay["NB"])[empty] = 0xFFFFFFFF
    corrupt("hist", hist_poison)

    def hist_off_by_one(buf, sent):
        u32(buf, lay["hist"], lay["NB"])[full] += 1
    corrupt("hist", hist_off_by_one)

    def split_a_run(buf, sent):     # the first entry of a run of several trades places with one behind the next run
        s0 = int(np.nonzero(sent[1:, 1] == sent[:-1, 1])[0][0])
        j = s0 + int(np.nonzero(sent[s0:, 1] != sent[s0, 1])[0][0]) + 1
        sent[[s0, j]] = sent[[j, s0]]
    corrupt("adjacent", split_a_run)

    def swap_pieces(lay_, buf):
        sent = _sent(lay_, buf, T)
        w = sent[:, 1] >> cb
        a, b_ = np.nonzero(w == 1)[0], np.nonzero(w == 2)[0]
        block = np.concatenate([sent[b_], sent[a]])
        sent[a[0]:a[0] + len(block)] = block

    buf = good.copy()
    swap_pieces(lay, buf)
    _fails("prefix sum", lay, buf, sc, bases, m)
    lay_s, good_s, m_s = sets["small"]
    buf = good_s.copy()
    sent = _sent(lay_s, buf, m_s.total)
    w = sent[:, 1] >> lay_s["cb"]
    first, second = int(w[0]), int(w[np.nonzero(w != w[0])[0][0]])
    a, b_ = np.nonzero(w == first)[0], np.nonzero(w == second)[0]
    sent[:len(a) + len(b_)] = np.concatenate([sent[b_], sent[a]])
    ref.check_sorted_set(lay_s, buf, sc, bases, model=m_s)                   # any order of the pieces
    buf = good_s.copy()
    sent = _sent(lay_s, buf, m_s.total)
    sent[:len(a)] = sent[:len(a)][::-1].copy()                               # a piece that is bucket-descending
    _fails("window pieces", lay_s, buf, sc, bases, m_s)
    buf = good_s.copy()
    sent = _sent(lay_s, buf, m_s.total)
    rng = np.random.default_rng(3)
    for s0 in np.nonzero(sent[1:, 1] != sent[:-1, 1])[0][:50] + 1:           # order inside a bucket is free
        e0 = s0 + int(np.argmax(np.append(sent[s0:, 1] != sent[s0, 1], True)))
        sent[s0:e0] = sent[s0:e0][rng.permutation(e0 - s0)]
    ref.check_sorted_set(lay_s, buf, sc, bases, model=m_s)

    def x_plus_q(buf, sent):
        rec = buf[lay["aff"] + 64 * 20:lay["aff"] + 64 * 20 + 32]
        rec[:] = np.frombuffer((int.from_bytes(rec.tobytes(), "little") + o.Q).to_bytes(32, "little"), dtype=np.uint8)
    corrupt("aff", x_plus_q)

    def no_beta(buf, sent):
        a0 = lay["aff"]
        buf[a0 + 64 * (N_BITE + 20):a0 + 64 * (N_BITE + 21)] = buf[a0 + 64 * 20:a0 + 64 * 21]
    corrupt("aff", no_beta)

    def infinity_dropped(buf, sent):      # the sort does not drop the entries of an infinity base
        keep = (sent[:, 0] & 0x7FFFFFFF) != 3
        k = int(keep.sum())
        sent[:k] = sent[keep]
        u32(buf, lay["total"], 1)[0] = k
    corrupt("total", infinity_dropped)


def test_checker_sees_a_sort_that_wrote_over_prepared_bases(L, valid):
    sc, bases, sets = valid
    lay = dict(sets["small"][0], prepared=1)
    buf, m = ref.build_sorted_set(lay, sc, bases)
    ref.check_sorted_set(lay, buf, sc, model=m)
    buf[lay["aff_area"] + 100] = 0
    _fails("aff untouched", lay, buf, sc, None, m)


@pytest.fixture(scope="module")
def valid_buckets(valid):
    """bucket records the test encodes itself over the valid two-level sorted set: bases k_i G, one pair P, -P sharing
    a scalar so that its buckets cancel"""
    sc, _, sets = valid
    lay, _, _ = sets["two_level"]
    rng = random.Random(21)
    logs = [rng.randrange(1, 1 << 64) for _ in range(N_BITE)]
    sc = list(sc)
    cancel = int(np.nonzero(sets["two_level"][2].counts == 0)[0][0])      # an empty bucket of window 0 ...
    assert cancel < 1 << lay["cb"]
    sc[40], sc[41], logs[41] = cancel + 1, cancel + 1, -logs[40]          # ... gets k G and -k G
    sorted_buf, m = ref.build_sorted_set(lay, sc)
    hist, dlogs = ref.bucket_logs(lay, sorted_buf, logs)
    pts = ref.expected_points(1, dlogs)
    assert hist[cancel] == 2 and dlogs[cancel] == 0 and o.G1.is_zero(pts[cancel])
    tail = np.full(lay["tail_bytes"], ref.POISON, dtype=np.uint8)
    recs = tail[lay["buckets"]:lay["buckets"] + 4 * lay["NB"] * lay["REC_WORDS"]].view("<u4").reshape(lay["NB"], -1)
    for b in np.nonzero(hist)[0]:
        P = pts[b]
        if not o.G1.is_zero(P):
            z = rng.randrange(1, o.Q)
            P = (P[0] * z * z % o.Q, P[1] * z * z * z % o.Q, P[2] * z % o.Q)
        else:
            P = (rng.randrange(o.Q), rng.randrange(o.Q), 0)      # infinity is Z = 0, whatever X and Y hold
        recs[b] = ref.encode_record(lay, P, ref.TAG_JAC if b % 3 == 0 else ref.TAG_XYZZ)
    tail[lay["hist_t"]:lay["hist_t"] + 4 * lay["NB"]] = np.frombuffer(hist.astype("<u4").tobytes(), dtype=np.uint8)
    return lay, tail, sorted_buf, logs, pts, cancel


def test_checker_accepts_valid_bucket_records(valid_buckets):
    lay, tail, sorted_buf, logs, pts, _ = valid_buckets
    ref.check_buckets(lay, tail, sorted_buf, logs)


def test_checker_rejects_every_corruption_of_the_bucket_records(valid_buckets):
    lay, good, sorted_buf, logs, pts, cancel = valid_buckets
    hist = ref.read_sorted(lay, sorted_buf)[1]
    live = [int(b) for b in np.nonzero(hist)[0] if b != cancel and b % 3]     # (encoded as XYZZ)

    def corrupt(clause, change):
        tail = good.copy()
        recs = tail[lay["buckets"]:lay["buckets"] + 4 * lay["NB"] * lay["REC_WORDS"]].view("<u4").reshape(lay["NB"], -1)
        change(tail, recs)
        with pytest.raises(ref.StageError) as e:
            ref.check_buckets(lay, tail, sorted_buf, logs, expected=pts)
        assert e.value.clause == clause, str(e.value)

    G = o.G1
    for b, tag in ((live[0], ref.TAG_XYZZ), (live[1], ref.TAG_JAC), (live[2], ref.TAG_XYZZ)):     # (b, tag: used at once)
        corrupt("point", lambda t, r: r.__setitem__(b, ref.encode_record(lay, G.add(pts[b], G.one), tag)))       # a wrong point
        corrupt("point", lambda t, r: r.__setitem__(b, ref.encode_record(lay, G.negate(pts[b]), tag)))           # the negated point
        corrupt("point", lambda t, r: r.__setitem__(b, ref.encode_record(lay, (5, 7, 0), tag)))                  # O where a point belongs
    corrupt("tag", lambda t, r: r[live[3]].__setitem__(lay["REC_TAG"], 0xFFFFFFFF))                              # poison
    corrupt("tag", lambda t, r: r[live[3]].__setitem__(lay["REC_TAG"], 2))
    corrupt("infinity", lambda t, r: r.__setitem__(cancel, ref.encode_record(lay, pts[live[0]], ref.TAG_XYZZ)))
    corrupt("infinity", lambda t, r: r.__setitem__(cancel, ref.encode_record(lay, pts[live[0]], ref.TAG_JAC)))
    corrupt("point", lambda t, r: r[live[4]].__setitem__(30, r[live[4]][30] ^ 1))                                # ZZZ off: ZZ^3 != ZZZ^2

    def hist_t_differs(tail, recs):
        tail[lay["hist_t"]:lay["hist_t"] + 4 * lay["NB"]].view("<u4")[live[5]] += 1
    corrupt("hist_t", hist_t_differs)
    # records of empty buckets are not read: the poison there is accepted (test above), and so is anything else
    tail = good.copy()
    recs = tail[lay["buckets"]:lay["buckets"] + 4 * lay["NB"] * lay["REC_WORDS"]].view("<u4").reshape(lay["NB"], -1)
    recs[np.nonzero(hist == 0)[0]] = 0
    ref.check_buckets(lay, tail, sorted_buf, logs, expected=pts)
