"""The fixed-base MSM at every table window, in every form of its gather-add (csrc/msm_fixed.hip).

fb_choose picks the table window wt from n by a cost model, so the shapes of test_fixed_base_gpu.py only ever build the
tables of wt = 1, 2, 3, 6, 8 (and 16 at 2^20); production sizes select 10 and 13.  Here OZK_FB_WS forces every window,
called with window_size = the forced window so that the workspace stays proportionate, and every case first asks
ozk_fixed_batch_msm_plan that the plan it means to run is the plan in force (a forced window above the caller's falls
back silently).

  GLV affine    k_fb_table_affine + k_fb_main_glv_affine (the default form)           G1 wt 1..16, G2 wt 1..10, 16
  GLV Jacobian  k_fb_main_glv, OZK_FB_AFFINE=0                                        the same windows
  plain         k_fb_main, OZK_MSM_GLV=0: window sizes that do not divide 32, last windows that straddle bit 256
                ((24, 11), (20, 13)) or start past it ((30, 9)), and 254 / 255 bits of windows
  truncating    outerc ws in {64, 200, 253}: always the plain form

The base is B = B_LOG g, Jacobian with Z != 1; the expectation is [(s mod r) B_LOG mod r] g from the oracle, computed
once per scalar, as the bytes of BOTH output layouts (64-byte big-endian, 32-byte little-endian compact).  For the
truncating shapes it is (s mod 2^(outerc ws)) B for the word as written (FixedBaseMSM.java:146-164).  The scalars
(fixed_base_util.window_scalars) hold the GLV edge scalars, zeros at the ends of the shared inversion's batches, words
>= r up to 2^256 - 1, and scalars whose GLV halves are patterned for the window under test: every digit 2^wt - 1, a
single bit at and just below every window boundary, bit 126 alone, and the largest all-ones half the split can give.
test_fixed_base_plan_cpu.py asserts that the split realises those halves.

The rule for words >= r: with outerc ws >= 254 every form returns (s mod r) B for every 256-bit word.  Before this
file the plain form dropped the bits of a word at and above 2^(outerc ws) for outerc ws in {254, 255} (2^255 gave O at
(127, 2)); k_fb_main now reduces mod r when its windows cover 254 bits."""
import pytest

import fixed_base_util as fu
from fr_gpu_util import knobs_set

pytestmark = pytest.mark.gpu

G1_WINDOWS = list(range(1, 17))
G2_WINDOWS = list(range(1, 11)) + [16]
GLV_CASES = [(1, w) for w in G1_WINDOWS] + [(2, w) for w in G2_WINDOWS]
# (outerc, ws) of the plain form: ceil(256 / ws) windows; a last window across bit 256; one that starts past it; and
# 254 and 255 bits of windows, where a word >= 2^(outerc ws) must still be reduced, not cut
PLAIN_SHAPES = [((256 + w - 1) // w, w) for w in list(range(1, 14)) + [16]] + [(24, 11), (20, 13), (30, 9)] + \
               [(254, 1), (127, 2), (85, 3), (51, 5)]
TRUNCATING = [(4, 16), (25, 8), (23, 11)]          # 64, 200 and 253 bits
FORM_KNOBS = {fu.FORM_GLV_AFFINE: {}, fu.FORM_GLV_JAC: {"OZK_FB_AFFINE": "0"}, fu.FORM_PLAIN: {"OZK_MSM_GLV": "0"}}


@pytest.fixture(scope="module")
def L():
    from octopuszk_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def oracle():
    return fu.Oracle()


@pytest.fixture(scope="module")
def bases():
    return {bn: fu.base_point(bn) for bn in (1, 2)}


def _check(L, oracle, bn, outerc, ws, base, scalars, run=fu.run_dev, base_log=fu.B_LOG, what=""):
    """both output layouts of one call against the oracle's bytes"""
    for compact in (0, 1):
        got = run(L, bn, outerc, ws, base, scalars, compact)
        want = oracle.expected(bn, scalars, outerc * ws, compact, base_log)
        bad = fu.differing(got, want)
        assert not bad, "%s bn=%d outerc=%d ws=%d compact=%d: scalars %s differ" % (
            what, bn, outerc, ws, compact, [hex(scalars[i]) for i in bad])


def _glv_case(L, monkeypatch, oracle, bases, bn, wt, form, outerc=None):
    outerc = outerc or (254 + wt - 1) // wt
    scalars = fu.window_scalars(wt)
    with knobs_set(L, monkeypatch, dict(FORM_KNOBS[form], OZK_FB_WS=str(wt))):
        assert fu.plan(L, outerc, wt, len(scalars)) == (form, wt, (128 + wt - 1) // wt)
        _check(L, oracle, bn, outerc, wt, bases[bn], scalars)


@pytest.mark.parametrize("bn,wt", GLV_CASES)
def test_glv_affine_at_every_table_window(L, monkeypatch, oracle, bases, bn, wt):
    _glv_case(L, monkeypatch, oracle, bases, bn, wt, fu.FORM_GLV_AFFINE)


@pytest.mark.parametrize("bn,wt", GLV_CASES)
def test_glv_jacobian_at_every_table_window(L, monkeypatch, oracle, bases, bn, wt):
    """k_fb_main_glv: no other test launches it"""
    _glv_case(L, monkeypatch, oracle, bases, bn, wt, fu.FORM_GLV_JAC)


@pytest.mark.parametrize("form", [fu.FORM_GLV_AFFINE, fu.FORM_GLV_JAC])
@pytest.mark.parametrize("bn", [1, 2])
def test_glv_with_510_bits_of_caller_windows(L, monkeypatch, oracle, bases, bn, form):
    """outerc ws = 510: the table still has ceil(128 / wt) windows; the workspace is the caller's 51 windows"""
    _glv_case(L, monkeypatch, oracle, bases, bn, 10, form, outerc=51)


def test_forced_window_above_the_callers_is_the_callers(L, monkeypatch, oracle, bases):
    """what the plan assertions of this file guard against: OZK_FB_WS = 12 with window_size 7 runs window 7"""
    scalars = fu.window_scalars(7)
    with knobs_set(L, monkeypatch, {"OZK_FB_WS": "12"}):
        assert fu.plan(L, 37, 7, len(scalars)) == (fu.FORM_GLV_AFFINE, 7, 19)
        _check(L, oracle, 1, 37, 7, bases[1], scalars)


@pytest.mark.parametrize("outerc,ws", PLAIN_SHAPES)
@pytest.mark.parametrize("bn", [1, 2])
def test_plain_form_windows(L, monkeypatch, oracle, bases, bn, outerc, ws):
    """k_fb_main's digit extraction across 32-bit words, and (s mod r) B for every word once 254 bits are covered"""
    assert outerc * ws >= 254
    scalars = fu.window_scalars(min(ws, 16)) + fu.plain_patterns(ws)
    with knobs_set(L, monkeypatch, FORM_KNOBS[fu.FORM_PLAIN]):
        assert fu.plan(L, outerc, ws, len(scalars)) == (fu.FORM_PLAIN, ws, outerc)
        _check(L, oracle, bn, outerc, ws, bases[bn], scalars)


@pytest.mark.parametrize("outerc,ws", TRUNCATING)
@pytest.mark.parametrize("bn", [1, 2])
def test_truncating_shapes_cut_the_word_as_written(L, oracle, bases, bn, outerc, ws):
    """fewer than 254 bits of windows: (s mod 2^(outerc ws)) B, the reference's rule; no knob decides this"""
    assert outerc * ws in (64, 200, 253)
    scalars = fu.window_scalars(min(ws, 16)) + fu.plain_patterns(ws)
    assert fu.plan(L, outerc, ws, len(scalars)) == (fu.FORM_PLAIN, ws, outerc)
    _check(L, oracle, bn, outerc, ws, bases[bn], scalars)


@pytest.mark.parametrize("cache", ["1", "0"])
@pytest.mark.parametrize("form", [fu.FORM_GLV_AFFINE, fu.FORM_GLV_JAC, fu.FORM_PLAIN])
@pytest.mark.parametrize("bn", [1, 2])
def test_base_as_host_bytes_repeated_calls(L, monkeypatch, oracle, bases, bn, form, cache):
    """ozk_fixed_batch_msm_base_dev three times with one base at each of three windows: the first call builds its table
    in the workspace, the second builds the cached one and gathers from it, the third finds it (the affine form; the
    others, and OZK_FB_TABLE_CACHE=0, build per call from the base copied into the workspace)"""
    windows = (4, 7, 13) if bn == 1 else (4, 7, 10)
    try:
        for wt in windows:
            outerc = (256 + wt - 1) // wt
            scalars = fu.window_scalars(wt)
            with knobs_set(L, monkeypatch, dict(FORM_KNOBS[form], OZK_FB_WS=str(wt), OZK_FB_TABLE_CACHE=cache)):
                want = (form, wt, (128 + wt - 1) // wt) if form != fu.FORM_PLAIN else (form, wt, outerc)
                assert fu.plan(L, outerc, wt, len(scalars)) == want
                for call in range(3):
                    _check(L, oracle, bn, outerc, wt, bases[bn], scalars, run=fu.run_base_dev, what="call %d" % call)
    finally:
        assert L.ozk_host_cache_release() == 0


@pytest.mark.parametrize("form", [fu.FORM_GLV_AFFINE, fu.FORM_GLV_JAC, fu.FORM_PLAIN])
@pytest.mark.parametrize("bn", [1, 2])
def test_infinity_base(L, monkeypatch, oracle, bn, form):
    """every table entry is O: each result is O in both layouts, through the device entry and the host-bytes entry"""
    wt = 5
    outerc = 52
    scalars = fu.window_scalars(wt)
    zero = fu.curve(bn).zero
    with knobs_set(L, monkeypatch, dict(FORM_KNOBS[form], OZK_FB_WS=str(wt))):
        assert fu.plan(L, outerc, wt, len(scalars))[:2] == (form, wt)
        _check(L, oracle, bn, outerc, wt, zero, scalars, base_log=0)
        _check(L, oracle, bn, outerc, wt, zero, scalars, run=fu.run_base_dev, base_log=0)
    assert L.ozk_host_cache_release() == 0
