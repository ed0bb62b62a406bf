"""The SORT stage of the variable-base MSM by itself (ozk_var_msm_sort_dev): the sorted set it leaves in poisoned
buffers against the exact host model (tests/msm_stage_ref.py check_sorted_set), at the smallest shapes that reach every
sort kernel and branch of csrc/msm_var.cuh:

    k_sort_small                       1, 63 and 4096 pairs (SORTS_MAX_N points exactly); every scalar equal
    k_sort1_*, k_scan_*, k_sort2       4097 pairs (three chunks, the last of two points; a one-block scan); 1 and 300 pairs
                                       with OZK_MSM_SMALL_SORT=0 (nearly every bin empty: zero counts over the poison)
    k_sort2 over several tiles         one coarse bin of S2_TILE, S2_TILE + 1, 2 S2_TILE + 1 entries at 2^14 pairs
    k_sort2 against k_sortbig_*        one coarse bin of big_thresh / big_thresh + 1 entries at 2^16 + 2^12 pairs
    k_sortbig_* with two list rows     2^17 pairs, every second scalar r - small: big bins in every window, both signs
    k_digits, neg_flags, lo_bits = 8   OZK_MSM_GLV=0 and OZK_MSM_SIGNED=0 at 5000 pairs
    NH = 1, 2, 256, c = 1              OZK_MSM_C = 1, 8, 9, 16 at 300 and 5000 pairs
    k_convert_bases                    O, Z = q, Z != 1 and Z = 1 bases; G2 records; prepared bases left alone

The bin sizes these cases rely on are asserted from the model alone in test_msm_stages_cpu.py."""
import numpy as np
import pytest

import msm_stage_ref as ref
import msm_stage_util as util
from oracle import bn254 as o
from test_msm_plans_gpu import _GLV_EDGE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pts():
    return util.g1_points(8, 61)


@pytest.fixture(scope="module")
def pts2():
    return util.g2_points(5, 62)


def _lib():
    from octopuszk_amd import lib
    return lib.load()


def _sort_and_check(name, n_in, scalars, points, type_=1, model=None, expect=None):
    """one SORT over poisoned buffers, checked; `expect` holds layout fields the case relies on"""
    t = util.Timer(name)
    st = util.Stages(n_in, type_)
    for k, v in (expect or {}).items():
        assert st.lay[k] == v, (k, st.lay[k], v)
    bases, wire = util.tiled(points, n_in, type_)
    if model is None:
        model = ref.Model(st.lay, scalars)
    t.lap("model")
    buf = st.sort(st.upload(wire), st.upload(ref.scalar_bytes(scalars)))
    t.lap("device")
    ref.check_sorted_set(st.lay, buf, scalars, bases, model=model)
    t.lap("check")
    t.show()
    return st, buf, model


def _edge_scalars(n, seed):
    """the GLV edge values (unreduced ones among them), zeros, and uniform values"""
    sc = ref.uniform_scalars(n, seed)
    edge = (_GLV_EDGE + [0, 0, 0])[:n]
    sc[:len(edge)] = edge
    return sc


@pytest.mark.parametrize("n", [1, 63, 4096])
def test_small_sort_default_plan(n, pts):
    _sort_and_check("small sort %d" % n, n, _edge_scalars(n, n) if n > 1 else [o.R - 5], pts, expect={"small_sort": 1})


def test_small_sort_every_scalar_equal(pts):
    s = 0x1234567890abcdef1234567890abcdef1234567890abcdef1234567890abcd % o.R
    _sort_and_check("small sort, equal scalars", 4096, [s] * 4096, pts, expect={"small_sort": 1})


def test_first_two_level_size(pts):
    _sort_and_check("two-level 4097", 4097, ref.uniform_scalars(4097, 5), pts, expect={"small_sort": 0, "nblk": 3})


@pytest.mark.parametrize("n", [1, 300])
def test_two_level_sort_with_nearly_every_bin_empty(n, pts, monkeypatch):
    def body():
        lay = ref.stage_layout(_lib(), n, 1)
        sc = ref.low_window_scalars(lay, 3) if n > 1 else [77]
        _, _, m = _sort_and_check("two-level %d, empty bins" % n, n, sc, pts, expect={"small_sort": 0})
        assert not m.counts[3 << lay["cb"]:].any()
    util.with_knobs(monkeypatch, {"OZK_MSM_SMALL_SORT": 0}, body)


@pytest.mark.parametrize("target", sorted(ref.SORT2_CASES))
def test_one_sort2_bin_of_whole_tiles(target, pts):
    n = 1 << 14
    lay = ref.stage_layout(_lib(), n, 1)
    sc, m, hi = ref.skewed_bin_scalars(lay, target, seed=target, doubles=ref.SORT2_CASES[target])
    assert m.bin_sizes()[0, hi] == target <= lay["big_thresh"]
    _sort_and_check("sort2 bin of %d" % target, n, sc, pts, model=m)


@pytest.mark.parametrize("over", [0, 1])
def test_one_bin_at_the_big_threshold(over, pts):
    n = (1 << 16) + (1 << 12)
    lay = ref.stage_layout(_lib(), n, 1)
    sc, m, _ = ref.skewed_bin_scalars(lay, lay["big_thresh"] + over, seed=40 + over)
    assert int((m.bin_sizes() > lay["big_thresh"]).sum()) == over
    _sort_and_check("bin of big_thresh + %d" % over, n, sc, pts, model=m)


def test_two_big_bins_with_negative_entries(pts):
    n = 1 << 17
    lay = ref.stage_layout(_lib(), n, 1)
    sc = ref.negative_half_scalars(lay, 5)
    m = ref.Model(lay, sc)
    big = np.argwhere(m.bin_sizes() > lay["big_thresh"])
    assert len({int(w) for w, _ in big}) >= 2
    _sort_and_check("two big bins 2^17", n, sc, pts, model=m)


@pytest.mark.parametrize("knob", ["OZK_MSM_SIGNED", "OZK_MSM_GLV"])
def test_unsigned_and_plain_plans(knob, pts, monkeypatch):
    n = 5000
    sc = _edge_scalars(n, 9)
    # (without GLV the sort sees 5000 points: the one-launch sort over k_digits' 256-bit windows)
    glv = int(knob != "OZK_MSM_GLV")
    expect = {"sd": 0, "glv": glv, "n": n << glv, "small_sort": 1 - glv, "lo_bits": 8}
    util.with_knobs(monkeypatch, {knob: 0}, lambda: _sort_and_check("%s=0" % knob, n, sc, pts, expect=expect))
    if not glv:   # and the 256-bit windows through the two-level kernels
        expect["small_sort"] = 0
        util.with_knobs(monkeypatch, {knob: 0, "OZK_MSM_SMALL_SORT": 0},
                        lambda: _sort_and_check("%s=0, two-level" % knob, n, sc, pts, expect=expect))


@pytest.mark.parametrize("n", [300, 5000])
@pytest.mark.parametrize("c", [1, 8, 9, 16])
def test_forced_window_sizes(c, n, pts, monkeypatch):
    nh = {1: 1, 8: 1, 9: 2, 16: 256}[c]
    expect = {"c": c, "NH": nh, "small_sort": int(n == 300 and c <= 11)}
    util.with_knobs(monkeypatch, {"OZK_MSM_C": c},
                    lambda: _sort_and_check("c=%d n=%d" % (c, n), n, _edge_scalars(n, 100 + c), pts, expect=expect))


@pytest.mark.parametrize("n", [300, 4097])
def test_edge_scalars_and_edge_bases(n, pts):
    """zero scalars, values >= r, the GLV edges; O, Z = q, Z != 1 and affine bases: the entries of an O base stay"""
    sc = _edge_scalars(n, 17)
    for i in range(len(_GLV_EDGE) + 3, len(_GLV_EDGE) + 40, 2):
        sc[i] = 0
    _, buf, m = _sort_and_check("edges %d" % n, n, sc, pts)
    assert m.half_neg.any() and (~m.half_neg).any()


def test_prepared_bases(pts):
    n = 4097
    sc = ref.uniform_scalars(n, 23)
    st0, buf0, m = _sort_and_check("unprepared 4097", n, sc, pts)
    bases, wire = util.tiled(pts, n)
    st = util.Stages(n, 1, prepared=1)
    prep = st.prepare(st.upload(wire)).cpu().numpy()
    assert np.array_equal(prep[:2 * n * 64], np.frombuffer(ref.expected_aff(st0.lay, bases), dtype=np.uint8))
    buf = st.sort(None, st.upload(ref.scalar_bytes(sc)))
    ref.check_sorted_set(st.lay, buf, sc, model=m)          # the aff area keeps its poison
    a, b = ref.read_sorted(st.lay, buf), ref.read_sorted(st0.lay, buf0)
    assert np.array_equal(a[0][:1], b[0][:1]) and np.array_equal(a[1], b[1]) and np.array_equal(a[4], b[4])


def test_second_call_into_used_buffers(pts):
    """nothing of a call with more entries survives in the buffers: total, the counts of buckets that are now empty"""
    big, n = 1 << 14, 4097
    st = util.Stages(big)
    _, wire = util.tiled(pts, big)
    st.sort(st.upload(wire), st.upload(ref.scalar_bytes(ref.uniform_scalars(big, 29))))
    st2 = util.Stages(n)
    assert st2.lay["sorted_bytes"] <= st.lay["sorted_bytes"] and st2.lay["sort_ws_bytes"] <= st.lay["sort_ws_bytes"]
    st2.sorted, st2.sort_ws = st.sorted, st.sort_ws
    sc = ref.low_window_scalars(st2.lay, 31)
    bases, wire = util.tiled(pts, n)
    buf = st2.sort(st2.upload(wire), st2.upload(ref.scalar_bytes(sc)), poison=False)
    m = ref.check_sorted_set(st2.lay, buf, sc, bases)
    assert not m.counts[3 << st2.lay["cb"]:].any()


@pytest.mark.parametrize("n", [300, 4097])
def test_g2(n, pts2):
    _sort_and_check("G2 %d" % n, n, _edge_scalars(n, 37), pts2, type_=2, expect={"AFF_WORDS": 32})
