"""The ACCUMULATE stage of the variable-base MSM by itself (ozk_var_msm_accum_dev): the bucket records it leaves in a
poisoned tail buffer, bucket by bucket, against exact integers (tests/msm_stage_ref.py check_buckets).  Bases are
k_i G with known k_i, so a bucket must hold [sum of sign k_i (1 or lambda)] G over its entries of the sorted set,
which the same case has checked against the model first.  Then the tail runs on the same buffer and the final point
is compared with the oracle, so the three staged entries are also checked end to end.

Most cases are the 2^20 workload in miniature, 2^12 pairs with OZK_MSM_C=8 (as test_runmerge_shapes_gpu.py): with the
chunked level 1 (k_segreduce, k_runmerge, k_segreduce_small) that is the one-launch sort's hand-off; the whole-bucket
level 1 (k_bin_sums, k_bucket_items, k_l1_whole) needs the two-level order, so its runs add OZK_MSM_SMALL_SORT=0.
Every case asserts which level-1 path ran (ozk_var_msm_last_l1_path)."""
import numpy as np
import pytest

import msm_stage_ref as ref
import msm_stage_util as util
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

WHOLE, CHUNKED = 1, 0
N = 1 << 12
N_RAGGED = N + 77
N_BIG = (1 << 16) + (1 << 12)
SEED = 53


@pytest.fixture(scope="module")
def g1():
    """bases k_i G (wire, host rows) and the k_i, for the largest n used here"""
    import torch
    from octopuszk_amd import device as dev
    d = dev.gen_g1_bases(N_BIG, SEED)
    torch.cuda.synchronize()
    return d.cpu().numpy().reshape(N_BIG, 96).copy(), dev.gen_base_logs(N_BIG, SEED)


def _final(type_, logs, scalars):
    acc = sum(s * k for s, k in zip(scalars, logs)) % o.R
    if type_ == 1:
        return o.g1_out_le(o.G1.to_affine(o.G1.mul(o.G1.one, acc)))
    return o.g2_out_le(o.G2.to_affine(o.G2.mul(o.G2.one, acc)))


def _stages_case(name, n, wire, logs, scalars, path, type_=1, parts=0, model=None):
    """sort, accumulate and tail over poisoned buffers, each stage's output checked; returns the decoded expectation"""
    t = util.Timer(name)
    st = util.Stages(n, type_)
    lay = st.lay
    sorted0 = st.sort(st.upload(wire[:n]), st.upload(ref.scalar_bytes(scalars)))
    t.lap("sort")
    ref.check_sorted_set(lay, sorted0, scalars, model=model)
    t.lap("model + sorted set")
    tail, sorted1, took = st.accum(parts)
    t.lap("accumulate")
    print("[l1-path] %s: planned l1_whole %d, ran %s" % (name, lay["l1_whole"], {1: "whole buckets", 0: "chunks"}.get(took, took)))
    assert took == path, (took, path)
    same = lambda a, b, off, k: np.array_equal(a[off:off + k], b[off:off + k])
    assert same(sorted0, sorted1, lay["hist"], 4 * lay["NB"]), "ACCUMULATE changed hist"
    assert same(sorted0, sorted1, lay["sent"], 8 * (lay["n"] * lay["W"] + 1)), "ACCUMULATE changed the sorted entries"
    want = ref.check_buckets(lay, tail, sorted0, logs)
    t.lap("buckets")
    assert st.tail(1) == _final(type_, logs, scalars)
    t.lap("tail")
    t.show()
    return st, tail, sorted0, want


C8 = {"OZK_MSM_C": 8}


def _env(l1=None, whole=None, extra=None):
    env = dict(C8)
    if l1 is not None:
        env["OZK_MSM_L1"] = l1
    if whole is not None:
        env["OZK_MSM_L1_WHOLE"] = whole
        if whole:
            env["OZK_MSM_SMALL_SORT"] = 0    # the whole-bucket path reads the two-level order
    env.update(extra or {})
    return env


@pytest.mark.parametrize("whole", [0, 1])
@pytest.mark.parametrize("l1", [52, 8, 4])
def test_workload_shapes(l1, whole, g1, monkeypatch):
    """two- and three-piece runs; runs on both sides of RUN_MAX with survivors for the generic levels; nothing merged.
    By whole buckets the chunk length plays no part: the same buckets must come out."""
    wire, logs = g1
    sc = ref.uniform_scalars(N, 100 + l1)
    util.with_knobs(monkeypatch, _env(l1, whole),
                    lambda: _stages_case("uniform L1=%d whole=%d" % (l1, whole), N, wire, logs, sc, WHOLE if whole else CHUNKED))


def test_ragged_size(g1, monkeypatch):
    """2^12 + 77 pairs: the two-level sort, a partial last block; the default plan takes whole buckets here"""
    wire, logs = g1
    sc = ref.uniform_scalars(N_RAGGED, 7)
    util.with_knobs(monkeypatch, _env(52), lambda: _stages_case("ragged", N_RAGGED, wire, logs, sc, WHOLE))
    util.with_knobs(monkeypatch, _env(52, 0), lambda: _stages_case("ragged, chunks", N_RAGGED, wire, logs, sc, CHUNKED))


def test_half_the_scalars_equal(g1, monkeypatch):
    """one long run per window beside short ones"""
    wire, logs = g1
    sc = ref.uniform_scalars(N, 8)
    sc[::2] = [0x1234567890abcdef1234567890abcdef1234567890abcdef1234567890abcd % o.R] * (N // 2)
    util.with_knobs(monkeypatch, _env(52, 0), lambda: _stages_case("half equal", N, wire, logs, sc, CHUNKED))


@pytest.mark.parametrize("whole", [0, 1])
def test_same_point_groups_of_four(whole, g1, monkeypatch):
    """every base the same point, groups of four pairs sharing a scalar: the doubling branch inside a bucket"""
    wire, logs = g1
    sc = [s for s in ref.uniform_scalars(N // 4, 9) for _ in range(4)]
    same = np.tile(wire[:1], (N, 1))
    util.with_knobs(monkeypatch, _env(2, whole),
                    lambda: _stages_case("same point whole=%d" % whole, N, same, [logs[0]] * N, sc, WHOLE if whole else CHUNKED))


@pytest.mark.parametrize("whole", [0, 1])
def test_plus_minus_every_bucket_cancels(whole, g1, monkeypatch):
    """P and -P alternate and share their scalar; scalars 1..128 first, so that every bucket of window 0 is hit: every
    bucket holds entries (hist > 0) and must decode to O"""
    wire, logs = g1
    rec = wire[0].copy()
    y = int.from_bytes(rec[32:64].tobytes(), "little")
    neg = rec.copy()
    neg[32:64] = np.frombuffer((o.Q - y).to_bytes(32, "little"), dtype=np.uint8)
    recs = np.tile(rec, (N, 1))
    recs[1::2] = neg
    half = list(range(1, 129)) + ref.uniform_scalars(N // 2 - 128, 10)
    sc = [s for s in half for _ in range(2)]

    def body():
        st, tail, sorted0, want = _stages_case("plus minus whole=%d" % whole, N, recs, [logs[0], -logs[0]] * (N // 2), sc,
                                               WHOLE if whole else CHUNKED)
        hist = ref.read_sorted(st.lay, sorted0)[1]
        assert (hist[:128] > 0).all() and all(o.G1.is_zero(P) for P in want if P is not None)
    util.with_knobs(monkeypatch, _env(2, whole), body)


def test_every_seventh_base_infinity(g1, monkeypatch):
    wire, logs = g1
    w = wire[:N].copy()
    w[::7] = np.frombuffer(o.g1_to_wire(o.G1.zero), dtype=np.uint8)
    lg = [0 if i % 7 == 0 else k for i, k in enumerate(logs[:N])]
    sc = ref.uniform_scalars(N, 11)
    util.with_knobs(monkeypatch, _env(52, 0), lambda: _stages_case("seventh base O", N, w, lg, sc, CHUNKED))
    util.with_knobs(monkeypatch, _env(52, 1), lambda: _stages_case("seventh base O, whole", N, w, lg, sc, WHOLE))


@pytest.mark.parametrize("n,path", [(300, CHUNKED), (4097, WHOLE)])
def test_default_plan(n, path, g1):
    """the one-launch sort's hand-off, and the first two-level size (whole buckets by the plan's own choice)"""
    wire, logs = g1
    _stages_case("default plan %d" % n, n, wire, logs, ref.uniform_scalars(n, 12 + n), path)


def test_whole_bucket_fallback_on_a_big_bin(g1, monkeypatch):
    """a coarse bin above big_thresh: k_bucket_items raises its flag, the chunked kernels run, the buckets are right"""
    wire, logs = g1

    def body():
        from octopuszk_amd import lib
        lay = ref.stage_layout(lib.load(), N_BIG, 1)
        assert lay["l1_whole"] == 1
        sc, m, _ = ref.skewed_bin_scalars(lay, lay["big_thresh"] + 1, seed=41)
        _stages_case("big bin, fallback", N_BIG, wire, logs, sc, CHUNKED, model=m)
    util.with_knobs(monkeypatch, {"OZK_MSM_L1_WHOLE": 1}, body)


@pytest.mark.parametrize("whole", [0, 1])
def test_parts_one_then_two(whole, g1, monkeypatch):
    """level 1, then the rest, on one stream: the same decoded buckets as the single call"""
    wire, logs = g1
    sc = ref.uniform_scalars(N, 13)

    def body():
        path = WHOLE if whole else CHUNKED
        st_a, tail_a, _, want = _stages_case("part 0 whole=%d" % whole, N, wire, logs, sc, path)
        st_b, tail_b, sorted_b, _ = _stages_case("parts 1, 2 whole=%d" % whole, N, wire, logs, sc, path, parts=12)
        lay = st_a.lay
        hist = ref.read_sorted(lay, sorted_b)[1]
        recs = lambda t: t[lay["buckets"]:lay["buckets"] + 4 * lay["NB"] * lay["REC_WORDS"]].view("<u4").reshape(lay["NB"], -1)[hist > 0]
        C = o.G1
        for (ta, ca), (tb, cb) in zip(ref.decode_records(lay, recs(tail_a)), ref.decode_records(lay, recs(tail_b))):
            Pa, Pb = ref.record_point(lay, ta, ca), ref.record_point(lay, tb, cb)
            assert (C.is_zero(Pa) and C.is_zero(Pb)) or C.equals(Pa, Pb)
    util.with_knobs(monkeypatch, _env(8, whole), body)


def test_g2(monkeypatch):
    """G2 at 300 pairs with c = 5 (416 buckets): the LDS-accumulator k_segreduce"""
    n = 300
    wire, logs = util.g2_dlog_bases(n, 78)
    sc = ref.uniform_scalars(n, 14)
    util.with_knobs(monkeypatch, {"OZK_MSM_C": 5}, lambda: _stages_case("G2 300 c=5", n, wire, logs, sc, CHUNKED, type_=2))
