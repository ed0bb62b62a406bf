"""Shared by the tests of the fixed-base MSM's plan and table windows (test_fixed_base_plan_cpu.py,
test_fixed_base_windows_gpu.py): the cost model of fb_choose (octopuszk_amd/csrc/msm_fixed.hip) restated, the plan
query, and the scalar list the window tests run, with the conditions that list is built to meet.

Halves.  The GLV forms split s mod r into s = k1 + k2 lambda (glv.cuh glv_decompose; multi_msm_ref.glv_split is the
same rule in integers) and read ceil(128 / wt) digits of wt bits off each magnitude.  The split rounds DOWN with
reciprocals that are themselves rounded down, so its halves are a (A1, B1) + b (A2, B2) with a and b in [0, 1) or up to
0.19 above it: a large k1 is positive, a large k2 is negative, no magnitude reaches 2^126.97 (tests/test_glv.py), and a
pair (k1, -k2) is certain to come back as written only when both magnitudes lie between 0.19 A2 = 2^124.4 and A2 =
2^126.8.  So 2^127 - 1 is NOT a value a half can take: the largest all-ones pattern here is TOP_ONES = 2^127 - 1 - 2^125
(bit 126 and every bit but 125 below it), and the patterns that would be small carry bit 125 as well.  Whether a pair
is realised is not argued but asserted, scalar by scalar (assert_realised)."""
import ctypes

import multi_msm_ref as ref
from oracle import bn254 as o

R = o.R
LAM = ref.LAM
FORM_PLAIN, FORM_GLV_JAC, FORM_GLV_AFFINE = 0, 1, 2
E_INVALID = -1

# the 17 scalars of test_fixed_base_gpu.test_fixed_base_glv_edge_scalars
GLV_EDGE = [0, 1, 2, R - 1, R - 2, LAM, LAM - 1, LAM + 1, R - LAM, (1 << 127) - 1, 1 << 127, (1 << 127) + 1, 1 << 128,
            1 << 253, R // 2, 9931322734385697763, 147946756881789319010696353538189108491]
# words that are not canonical (>= r), and the largest word below 2^254
WIDE_WORDS = [R, R + 1, 2 * R, (1 << 254) - 1, 1 << 255, (1 << 256) - 1]
# where test_fixed_base_short_batches_with_infinities puts its zeros: first, middle and last of lane 0's batch of the
# shared inversion and first of lane 1's, for n = 19
ZERO_AT = (0, 1, 3, 9, 18)
TOP_ONES = (1 << 127) - 1 - (1 << 125)
FREE_BITS = 126      # the boundary patterns keep to the bits below this one: 2^126 is 0.58 A2


# ---- the plan ------------------------------------------------------------------------------------------------------
def cost_window(ws, n):
    """fb_choose's cost model: the first w in 1..ws with the least 20 o n + 32 o 2^w, o = ceil(128 / w)"""
    best, wt = None, ws
    for w in range(1, ws + 1):
        oc = (128 + w - 1) // w
        cost = 20 * oc * n + 32 * oc * (1 << w)
        if best is None or cost < best:
            best, wt = cost, w
    return wt


def plan_model(outerc, ws, n, glv=1, affine=1, forced=None):
    """(form, table window, windows) as knobs.h documents OZK_MSM_GLV, OZK_FB_AFFINE and OZK_FB_WS"""
    if not glv or outerc * ws < 254:
        return FORM_PLAIN, ws, outerc
    wt = cost_window(ws, n) if forced is None else forced
    if wt < 1 or wt > ws:
        wt = ws
    return (FORM_GLV_AFFINE if affine else FORM_GLV_JAC), wt, (128 + wt - 1) // wt


def plan(L, outerc, ws, n):
    """ozk_fixed_batch_msm_plan -> (form, table window, windows), or the error code for a rejected shape"""
    f, wt, oc = ctypes.c_int32(-7), ctypes.c_int32(-7), ctypes.c_int32(-7)
    rc = L.ozk_fixed_batch_msm_plan(outerc, ws, n, ctypes.byref(f), ctypes.byref(wt), ctypes.byref(oc))
    return (f.value, wt.value, oc.value) if rc == 0 else rc


# ---- patterned halves ----------------------------------------------------------------------------------------------
def digits(mag, wt, count=None):
    """the digits the gather reads: bits [w wt, w wt + wt) of the magnitude, w < ceil(128 / wt)"""
    count = (128 + wt - 1) // wt if count is None else count
    return [(mag >> (w * wt)) & ((1 << wt) - 1) for w in range(count)]


ANCHOR = 1 << 125     # keeps a sparse pattern above 2^124.4


def _boundaries(wt):
    return [w * wt for w in range(1, 128) if w * wt < FREE_BITS]


def half_patterns(wt):
    """name -> magnitude of a half built for table window wt"""
    return {
        "all_ones": (1 << FREE_BITS) - 1,                                     # every digit below bit 126 is 2^wt - 1
        "low_bits": sum(1 << b for b in _boundaries(wt)) | ANCHOR,           # a single bit AT every window boundary
        "high_bits": sum(1 << (b - 1) for b in _boundaries(wt)) | ANCHOR,    # and just BELOW every boundary
        "bit_126": 1 << 126,                                                  # the top bit a half can have, alone
        "top_ones": TOP_ONES,
    }


def check_patterns(wt):
    """the patterns are what their names say, for this window"""
    p = half_patterns(wt)
    full = (1 << wt) - 1
    d = digits(p["all_ones"], wt)
    whole = FREE_BITS // wt                  # windows that lie wholly below bit 126
    assert d[:whole] == [full] * whole and sum(x << (w * wt) for w, x in enumerate(d)) == (1 << FREE_BITS) - 1
    # the window above a boundary holds its lowest bit alone, the window below a boundary its highest bit alone (window
    # 0 has no boundary below it, the last windows none above them); the anchor is the one bit besides
    nb = len(_boundaries(wt))
    low, high = [0] * len(d), [0] * len(d)
    for w in range(1, nb + 1):
        low[w] = 1
        high[w - 1] = 1 << (wt - 1)
    low[125 // wt] |= 1 << (125 % wt)
    high[125 // wt] |= 1 << (125 % wt)
    assert nb == (FREE_BITS - 1) // wt and digits(p["low_bits"], wt) == low and digits(p["high_bits"], wt) == high
    assert p["bit_126"] == 1 << 126
    assert p["top_ones"].bit_length() == 127 and bin(p["top_ones"]).count("1") == 126
    assert all(0.19 * ref.A2 < v < ref.A2 for v in p.values())


def patterned_scalars(wt):
    """[(s, k1, k2)]: s = (k1 + k2 lambda) mod r for pairs of the patterns of window wt, every pattern once as the first
    half (positive) and once as the second (negative), each next to a different pattern"""
    p = half_patterns(wt)
    pairs = [("all_ones", "all_ones"), ("low_bits", "high_bits"), ("high_bits", "low_bits"), ("bit_126", "all_ones"),
             ("all_ones", "bit_126"), ("top_ones", "high_bits"), ("low_bits", "top_ones"), ("top_ones", "top_ones")]
    out = []
    for a, b in pairs:
        k1, k2 = p[a], -p[b]
        out.append(((k1 + k2 * LAM) % R, k1, k2))
    return out


def assert_realised(wt):
    """the split the kernels make (multi_msm_ref.glv_split) gives back exactly the halves the scalars were built
    from, so the digits the gather reads are the intended ones; every pattern occurs in both halves"""
    check_patterns(wt)
    seen = [set(), set()]
    for s, k1, k2 in patterned_scalars(wt):
        assert 0 <= s < R
        got = ref.glv_split(s)
        assert got == (k1, k2), (wt, hex(s), got)
        for h, k in enumerate(got):
            assert digits(abs(k), wt) == digits(abs((k1, k2)[h]), wt)
            seen[h].add(abs(k))
    want = set(half_patterns(wt).values())
    assert seen[0] == want and seen[1] == want


def window_scalars(wt):
    """The list a window test runs, 39 scalars: the GLV edge scalars, the words >= r, the patterned scalars of window
    wt, filler, and zeros at ZERO_AT (n = 39 is five lanes of the shared inversion, the last batch short)."""
    import random
    rng = random.Random(1000)
    body = GLV_EDGE[1:] + WIDE_WORDS + [s for s, _, _ in patterned_scalars(wt)]
    body += [rng.randrange(1 << 256) for _ in range(4)]
    out = []
    it = iter(body)
    for i in range(len(body) + len(ZERO_AT)):
        out.append(0 if i in ZERO_AT else next(it))
    assert [i for i, s in enumerate(out) if s == 0] == list(ZERO_AT)
    return out


def plain_patterns(ws):
    """canonical words (below 2^253 < r, so the plain form reads their digits as written) for the plain form's window
    ws: a single bit at every window boundary, a single bit just below every boundary, and every bit set"""
    bounds = [w * ws for w in range(1, 256) if w * ws < 253]
    out = [sum(1 << b for b in bounds), sum(1 << (b - 1) for b in bounds), (1 << 253) - 1]
    assert all(0 < v < R for v in out)
    return out


# ---- running a case on the device ----------------------------------------------------------------------------------
B_LOG = 0x1234567      # the base is B = B_LOG g


def curve(bn):
    return o.G1 if bn == 1 else o.G2


def base_point(bn):
    """B as the double-and-add leaves it: Jacobian with Z != 1"""
    C = curve(bn)
    B = C.mul(C.one, B_LOG)
    assert not C.F.eq(B[2], C.F.one) and not C.is_zero(B)
    return B


def to_wire(bn, P):
    return o.g1_to_wire(P) if bn == 1 else o.g2_to_wire(P)


class Oracle:
    """[e g] as the bytes of both output layouts, computed once per (curve, e mod r) for all the tests of a module"""

    def __init__(self):
        self._known = {}

    def record(self, bn, e, compact):
        key = (bn, e % R)
        if key not in self._known:
            C = curve(bn)
            P = C.to_affine(C.mul(C.one, key[1]))
            self._known[key] = ((o.g1_out_be if bn == 1 else o.g2_out_be)(P), to_wire(bn, P))
        return self._known[key][1 if compact else 0]

    def expected(self, bn, scalars, bits, compact, base_log=B_LOG):
        """what a call whose windows cover `bits` bits returns: (s mod r) B when they cover a whole scalar, else
        (s mod 2^bits) B for the word as written"""
        return [self.record(bn, (s % R if bits >= 254 else s & ((1 << bits) - 1)) * base_log, compact) for s in scalars]


def record_bytes(bn, compact):
    return (192 if bn == 1 else 384) // (2 if compact else 1)


def _call(L, entry, bn, outerc, ws, scalars, compact):
    """runs `entry` over a poisoned workspace and a poisoned output with a guard tail, waits, and returns the n records
    (the inputs live in the caller's frame until then)"""
    import fr_gpu_util as g
    n = len(scalars)
    per = record_bytes(bn, compact)
    wsb = int(L.ozk_fixed_batch_msm_workspace_bytes(outerc, ws, n, bn))
    assert wsb > 0
    wsp, out = g.poisoned(wsb), g.poisoned(n * per + g.GUARD)
    rc = entry(wsp, wsb, out)
    assert rc == 0, L.ozk_last_error()
    raw = g.host_bytes(out)
    assert raw[n * per:] == bytes([g.POISON]) * g.GUARD, "wrote behind the output"
    return [raw[i * per:(i + 1) * per] for i in range(n)]


def run_dev(L, bn, outerc, ws, base, scalars, compact):
    """ozk_fixed_batch_msm_dev / _compact_dev (the base in device memory, a table per call)"""
    import fr_gpu_util as g
    import numpy as np
    import torch
    d_base = torch.from_numpy(np.frombuffer(to_wire(bn, base), dtype=np.uint8).copy()).cuda()
    d_sc = g.dev_from_ints(scalars)
    fn = L.ozk_fixed_batch_msm_compact_dev if compact else L.ozk_fixed_batch_msm_dev
    return _call(L, lambda wsp, wsb, out: fn(outerc, ws, len(scalars), g.ptr(d_base), g.ptr(d_sc), bn, g.ptr(out),
                                             g.ptr(wsp), wsb, g.stream()),
                 bn, outerc, ws, scalars, compact)


def run_base_dev(L, bn, outerc, ws, base, scalars, compact):
    """ozk_fixed_batch_msm_base_dev (the base as host bytes: the table may come from the cache)"""
    import fr_gpu_util as g
    wire = to_wire(bn, base)
    host = ctypes.create_string_buffer(wire, len(wire))
    d_sc = g.dev_from_ints(scalars)
    return _call(L, lambda wsp, wsb, out: L.ozk_fixed_batch_msm_base_dev(outerc, ws, len(scalars), g.vp(host), g.ptr(d_sc),
                                                                         bn, g.ptr(out), compact, g.ptr(wsp), wsb,
                                                                         g.stream()),
                 bn, outerc, ws, scalars, compact)


def differing(got, want):
    """indices of the records that differ (for the assertion message)"""
    assert len(got) == len(want)
    return [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
