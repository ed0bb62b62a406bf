"""The shared-base batched MSM at every table window (csrc/msm_multi.hip, msm_multi.cuh).

mm_window_bits(n) gives 8 up to n = 1280, 7 up to 2155, 6 up to 3723 and 5 above; test_multi_msm_gpu.py has
n in {1..1024, 4096}, so only the tables of 8 and 5 bits were ever built and evaluated on a device.  The recoding is
host-checked for every window (test_multi_msm_cpu.py); k_mm_chain, k_mm_level and k_mm_eval are not.  Here OZK_MM_WS
forces 4, 5, 6, 7 and 8 (4 shares with 8 the rule oc ws == 128, where the top window takes no carry out), and n = 1281
and 2156 run the windows 7 and 6 at the first sizes that select them, with no knob.  The table is built inside the knob
block, so table and calls see one plan, and ozk_multi_msm_plan is asked for the window that ran.

Scalars: multi_msm_ref.edge_scalars(), the words >= r, and scalars whose GLV halves recode as "raw == half in every
window" (never a carry) and "raw == half + 1 in every window" (always one), for every window size; that the split gives
those halves back is asserted (multi_msm_ref.assert_carry_patterns_realised).  Bases: random ones and the special sets
of test_multi_msm_gpu.test_special_bases.  Reference: oracle.bn254.naive_msm for n <= 3, one ozk_var_msm_dev per row
otherwise, computed once per (shape, bases) and shared by the five windows."""
import ctypes

import pytest

import multi_msm_ref as ref
import test_multi_msm_gpu as mm
from fr_gpu_util import knobs_set
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

WINDOWS = [4, 5, 6, 7, 8]
SHAPES = [(1, 1), (3, 65), (65, 3), (130, 2)]
BASE_KINDS = ["random", "repeated", "negatives", "infinity_at_ends_and_middle", "all_infinity"]


@pytest.fixture(scope="module")
def L():
    from octopuszk_amd import lib
    return lib.load()


@pytest.fixture(scope="module")
def references():
    return {}


def _plan(L, n):
    wb, oc = ctypes.c_int32(), ctypes.c_int32()
    assert L.ozk_multi_msm_plan(n, ctypes.byref(wb), ctypes.byref(oc)) == 0
    return wb.value, oc.value


def _special_scalars(first_ws=None):
    """the scalars every case places; with `first_ws` the patterns of that window lead (the 1 x 1 shape has one slot)"""
    order = ([first_ws] if first_ws else []) + [w for w in WINDOWS if w != first_ws]
    patterned = [s for ws in order for s, _, _ in ref.carry_pattern_scalars(ws)]
    rest = ref.edge_scalars() + mm.EDGES_VAR_ONLY
    return patterned + rest if first_ws else rest + patterned


def _rows(n, k, specials):
    """k x n scalars: two slots of three hold the special scalars in turn, the others random canonical ones"""
    rows = mm._random_rows(k, n, 7000 * n + k)
    t = 0
    for i in range(k):
        for j in range(n):
            if (i * n + j) % 3 != 2:
                mm._put(rows, i, j, specials[t % len(specials)])
                t += 1
    return rows


def _bases(kind, n):
    if kind == "random":
        return mm._random_bases(n, 300 + n)
    return mm._special_base_sets(n + n % 2)[kind][:n]           # (the sets are written for an even n)


def _reference(references, key, n, rows, bases, d_bases):
    if key not in references:
        if n <= 3:
            references[key] = mm._oracle_reference([tuple(c % o.Q for c in P) for P in bases], rows)
        else:
            references[key] = mm._var_reference(d_bases, n, rows)
    return references[key]


def test_patterned_scalars_are_what_they_claim():
    for ws in WINDOWS:
        ref.assert_carry_patterns_realised(ws)
    sp = _special_scalars()
    assert len(sp) == len(set(sp)) == 20 + len(ref.edge_scalars()) + 3
    for n, k in SHAPES[1:]:
        assert 2 * n * k // 3 >= len(sp)                          # every special scalar is placed in these shapes


@pytest.mark.parametrize("kind", BASE_KINDS)
@pytest.mark.parametrize("n,k", SHAPES)
@pytest.mark.parametrize("ws", WINDOWS)
def test_forced_windows(L, monkeypatch, references, ws, n, k, kind):
    from octopuszk_amd.device import SharedBaseMsm
    single = n * k == 1
    rows = _rows(n, k, _special_scalars(ws if single else None))
    bases = _bases(kind, n)
    assert len(bases) == n
    d_bases = mm._dev(mm._wire(bases))
    want = _reference(references, (kind, n, k, ws if single else 0), n, rows, bases, d_bases)
    with knobs_set(L, monkeypatch, {"OZK_MM_WS": str(ws)}):
        assert _plan(L, n) == (ws, ref.windows(ws))
        assert L.ozk_multi_msm_table_bytes(n, 1) == n * ref.records_per_base(ws) * ref.RECORD_BYTES
        msm = SharedBaseMsm(d_bases, n)                          # the table, under the forced plan
        assert (msm.window_bits, msm.windows) == (ws, ref.windows(ws))
        got = mm._run(msm, rows)
        assert _plan(L, n) == (ws, ref.windows(ws))
    mm._assert_rows(got, want, "ws=%d n=%d k=%d %s" % (ws, n, k, kind))
    if kind == "all_infinity":
        assert all(g == mm.INF_RECORD for g in got)
    assert _plan(L, n) == (ref.window_bits(n), ref.windows(ref.window_bits(n)))   # the knob is gone again


@pytest.mark.parametrize("n,ws", [(1281, 7), (2156, 6)])
def test_natural_windows_at_the_first_sizes_that_select_them(L, n, ws):
    from octopuszk_amd.device import SharedBaseMsm
    k = 2
    assert _plan(L, n) == (ws, ref.windows(ws)) and _plan(L, n - 1)[0] == ws + 1
    rows = _rows(n, k, _special_scalars())
    d_bases = mm._dev(mm._wire(mm._random_bases(n, 300 + n)))
    msm = SharedBaseMsm(d_bases, n)
    assert msm.window_bits == ws
    got = mm._run(msm, rows)
    mm._assert_rows(got, mm._var_reference(d_bases, n, rows), "n=%d k=%d (ws=%d) vs ozk_var_msm_dev" % (n, k, ws))
