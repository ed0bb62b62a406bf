"""The fixed-base MSM's plan query (ozk_fixed_batch_msm_plan: what fb_choose of csrc/msm_fixed.hip returns under the
knobs in force, no device work) against the cost model and the knob rules restated in Python (fixed_base_util), and
the scalar list of test_fixed_base_windows_gpu.py against the conditions it is built to meet.  No GPU."""
import pytest

import fixed_base_util as fu
from fr_gpu_util import knobs_set

WS = [1, 5, 8, 11, 17, 22]
NS = [1, 19, 300, 1000, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20]


@pytest.fixture(scope="module")
def L():
    from octopuszk_amd import build, lib
    build.build(verbose=False)
    return lib.load()


def _outerc(ws, bits=254):
    return (bits + ws - 1) // ws


def test_cost_model_windows_named_in_the_suite():
    """the windows the shapes of test_fixed_base_gpu.py and the production sizes select, by the formula"""
    assert [fu.cost_window(w, n) for n, w in ((1, 1), (5, 3), (300, 8), (1000, 11))] == [1, 2, 6, 8]
    assert {fu.cost_window(w, n) for n in (17, 19, 23) for w in (5, 6, 17)} == {3}
    assert [fu.cost_window(17, 1 << k) for k in (14, 16, 18, 20)] == [10, 13, 13, 16]


@pytest.mark.parametrize("ws", WS)
def test_default_plan_is_the_cost_model(L, ws):
    for n in NS:
        want = (fu.FORM_GLV_AFFINE, fu.cost_window(ws, n), (128 + fu.cost_window(ws, n) - 1) // fu.cost_window(ws, n))
        assert fu.plan(L, _outerc(ws), ws, n) == want == fu.plan_model(_outerc(ws), ws, n), (ws, n)
        assert want[1] <= ws
        # more windows than a scalar needs change nothing; one window too few is the plain form
        assert fu.plan(L, 512 // ws, ws, n) == want
        assert (_outerc(ws) - 1) * ws < 254
        assert fu.plan(L, _outerc(ws) - 1, ws, n) == (fu.FORM_PLAIN, ws, _outerc(ws) - 1)


def test_fewer_than_254_bits_of_windows_is_plain(L):
    for outerc, ws in ((4, 16), (8, 8), (64, 1), (25, 8), (23, 11), (11, 22), (253, 1)):
        assert outerc * ws < 254
        assert fu.plan(L, outerc, ws, 1000) == (fu.FORM_PLAIN, ws, outerc)
    for outerc, ws in ((254, 1), (127, 2), (85, 3), (24, 11), (12, 22), (32, 16)):
        assert outerc * ws >= 254
        assert fu.plan(L, outerc, ws, 1000)[0] == fu.FORM_GLV_AFFINE


def test_knobs_move_the_plan_as_documented(L, monkeypatch):
    ws, n = 11, 1 << 14
    outerc = _outerc(ws)
    default = fu.plan(L, outerc, ws, n)
    assert default == (fu.FORM_GLV_AFFINE, 10, 13)
    # OZK_FB_WS: the table window of the GLV forms, 1 .. the caller's
    for forced in range(1, ws + 1):
        with knobs_set(L, monkeypatch, {"OZK_FB_WS": str(forced)}):
            assert fu.plan(L, outerc, ws, n) == (fu.FORM_GLV_AFFINE, forced, (128 + forced - 1) // forced)
            assert fu.plan(L, outerc, ws, n) == fu.plan_model(outerc, ws, n, forced=forced)
    # a forced window above the caller's (or below 1) is the caller's: the workspace was sized for it
    for forced in (ws + 1, 16, 22, 99, -3):
        with knobs_set(L, monkeypatch, {"OZK_FB_WS": str(forced)}):
            assert fu.plan(L, outerc, ws, n) == (fu.FORM_GLV_AFFINE, ws, 12) == fu.plan_model(outerc, ws, n, forced=forced)
    # OZK_FB_AFFINE=0: the Jacobian gather-add over the same table window
    with knobs_set(L, monkeypatch, {"OZK_FB_AFFINE": "0"}):
        assert fu.plan(L, outerc, ws, n) == (fu.FORM_GLV_JAC, 10, 13) == fu.plan_model(outerc, ws, n, affine=0)
    with knobs_set(L, monkeypatch, {"OZK_FB_AFFINE": "0", "OZK_FB_WS": "7"}):
        assert fu.plan(L, outerc, ws, n) == (fu.FORM_GLV_JAC, 7, 19)
    # OZK_MSM_GLV=0: plain windows, the caller's shape; the other two knobs then change nothing
    with knobs_set(L, monkeypatch, {"OZK_MSM_GLV": "0"}):
        assert fu.plan(L, outerc, ws, n) == (fu.FORM_PLAIN, ws, outerc) == fu.plan_model(outerc, ws, n, glv=0)
    with knobs_set(L, monkeypatch, {"OZK_MSM_GLV": "0", "OZK_FB_WS": "4", "OZK_FB_AFFINE": "0"}):
        assert fu.plan(L, outerc, ws, n) == (fu.FORM_PLAIN, ws, outerc)
    # the plain form of a short shape does not look at OZK_FB_WS either
    with knobs_set(L, monkeypatch, {"OZK_FB_WS": "4"}):
        assert fu.plan(L, 8, 8, n) == (fu.FORM_PLAIN, 8, 8)
    assert fu.plan(L, outerc, ws, n) == default                      # the knobs are gone again


def test_bad_shapes_are_rejected(L):
    for outerc, ws, n in ((24, 11, 0), (24, 11, -1), (24, 11, (1 << 24) + 1), (24, 0, 10), (24, 23, 10), (0, 11, 10),
                          (-1, 11, 10), (47, 11, 10), (513, 1, 10), (24, 22, 10)):
        assert fu.plan(L, outerc, ws, n) == fu.E_INVALID, (outerc, ws, n)
        assert L.ozk_fixed_batch_msm_workspace_bytes(outerc, ws, n, 1) == 0
    assert fu.plan(L, 512, 1, 10) == (fu.FORM_GLV_AFFINE, 1, 128)
    assert fu.plan(L, 23, 22, 1 << 24)[0] == fu.FORM_GLV_AFFINE
    # null result pointers are allowed
    assert L.ozk_fixed_batch_msm_plan(24, 11, 10, None, None, None) == 0
    assert L.ozk_fixed_batch_msm_plan(24, 11, 0, None, None, None) == fu.E_INVALID


@pytest.mark.parametrize("wt", range(1, 17))
def test_patterned_scalars_realise_their_halves(wt):
    """the condition the window tests rest on: the split of every patterned scalar gives back the halves it was built
    from, whose digits at table window wt are the intended ones"""
    fu.assert_realised(wt)
    sc = fu.window_scalars(wt)
    assert len(sc) == 39 and all(0 <= s < 1 << 256 for s in sc)
    assert all(s in sc for s in fu.GLV_EDGE + fu.WIDE_WORDS)
