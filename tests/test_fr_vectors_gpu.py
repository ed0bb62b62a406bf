"""The Fr vector kernels around the transforms (csrc/fft.hip), through the C ABI, against Python integers:
the power-table kernels past the first level of their two-level table (TW_LO = 2048 entries per row), the sparse
products on rows long enough for the strided loop of the long-row reduction to go round more than once, and
ozk_fr_lincomb3_dev with its output aliasing an input.  Every comparison is exact."""
import functools
import random

import numpy as np
import pytest
import torch

import fr_gpu_util as u
from oracle import bn254 as o
from oracle import groth16 as g

pytestmark = pytest.mark.gpu
R = o.R


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------- A. power tables
_rng_a = random.Random(2048)
POWER_PAIRS = {
    "random_1": (_rng_a.randrange(R), 1),
    "random_random": (_rng_a.randrange(R), _rng_a.randrange(R)),
    "r-1_r-1": (R - 1, R - 1),
    "2_0": (2, 0),
    "0_5": (0, 5),          # 0^0 = 1, every later power 0
    "1_r-1": (1, R - 1),
}
LAGRANGE_T = {"random": _rng_a.randrange(R), "0": 0, "2": 2, "mult_gen": o.FR_MULT_GEN}


@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 4096, 4097, 6145])
@pytest.mark.parametrize("pair", list(POWER_PAIRS))
def test_powers_on_every_row_of_the_table(pair, n):
    """ozk_fr_powers_dev: out[i] = base^i k.  k_powers_scaled reads pw[i % 2048] and pw[2048 + i / 2048]; the sizes
    put the last index on both sides of a table row and reach i / 2048 = 1, 2 and 3 (n = m + 1 is the shape the setup
    uses).  Workspace and output start poisoned; the 32 bytes behind the output must stay so."""
    from octopuszk_amd import lib
    L = lib.load()
    base, k = POWER_PAIRS[pair]
    wsb = int(L.ozk_fr_powers_workspace_bytes(n))
    assert wsb > 0
    ws, out = u.poisoned(wsb), u.poisoned(n * 32 + u.GUARD)
    hb, hk = u.host32(base), u.host32(k)
    lib.check(L.ozk_fr_powers_dev(u.vp(hb), u.vp(hk), n, out.data_ptr(), ws.data_ptr(), wsb, _stream()))
    torch.cuda.synchronize()
    want = [pow(base, i, R) * k % R for i in range(n)]
    if base == 0:
        assert want == [k] + [0] * (n - 1)
    bad = u.mismatches(u.ints(out, n), want)
    assert not bad, "%d of %d powers differ, first at %s" % (len(bad), n, bad[:8])
    assert u.tail_untouched(out, n * 32)


@pytest.mark.parametrize("m", [2, 4, 16, 2048, 4096, 8192])
@pytest.mark.parametrize("tname", list(LAGRANGE_T))
def test_lagrange_on_every_row_of_the_table(tname, m):
    """ozk_qap_lagrange_dev against oracle.groth16.lagrange_coefficients and Zt = t^m - 1.  m = 2 and 4 run one lane,
    m = 16 two, m = 8192 four blocks; from m = 4096 on k_lagrange reads the second level of omega's power table at
    i / 2048 > 0.  At t = 0 every coefficient is 1 / m and Zt = r - 1."""
    from octopuszk_amd import lib
    L = lib.load()
    t = LAGRANGE_T[tname]
    assert pow(t, m, R) != 1          # outside the domain: the entry point refuses the others
    wsb = int(L.ozk_qap_lagrange_workspace_bytes(m))
    assert wsb > 0
    ws, out, zt = u.poisoned(wsb), u.poisoned(m * 32 + u.GUARD), u.poisoned(32 + u.GUARD)
    ht, hw = u.host32(t), u.host32(o.fr_root_of_unity(m))
    lib.check(L.ozk_qap_lagrange_dev(u.vp(ht), u.vp(hw), m, out.data_ptr(), zt.data_ptr(), ws.data_ptr(), wsb, _stream()))
    torch.cuda.synchronize()
    got, got_zt = u.ints(out, m), u.ints(zt, 1)[0]
    assert got_zt == (pow(t, m, R) - 1) % R
    if t == 0:
        assert got_zt == R - 1
        assert got == [pow(m, -1, R)] * m
    bad = u.mismatches(got, g.lagrange_coefficients(t, m))
    assert not bad, "%d of %d coefficients differ, first at %s" % (len(bad), m, bad[:8])
    assert u.tail_untouched(out, m * 32) and u.tail_untouched(zt, 32)


# ---------------------------------------------------------------------------------------------- B. long rows
NV = 500
ROWS = 110
# row -> terms.  A row of more than 64 terms is cut into 64 slices of per = ceil(len / 64) terms, each walked by 256
# threads with t += 256: 16384 -> per = 256 (one full sweep), 16385 -> per = 257 (thread 0 goes round twice, the last
# slice is short), 32845 -> per = 514, 40000 -> per = 625 (two to three rounds)
SPECIAL_ROWS = {0: 40000, 10: 0, 11: 1, 12: 64, 13: 65, 40: 16384, 75: 32845, ROWS - 1: 16385}


@functools.lru_cache(maxsize=None)
def _long_row_case():
    """(ptr, idx, random coefficients, random vector): one CSR matrix over NV variables, the longest row first, the
    16385-term row last, about a hundred rows of 0 .. 5 terms between the special ones; index-0 terms planted at the
    ends of the long rows and at the first term of thread 0's second round"""
    nrng = np.random.default_rng(64)
    lens = nrng.integers(0, 6, size=ROWS)
    for row, n in SPECIAL_ROWS.items():
        lens[row] = n
    ptr = np.concatenate(([0], np.cumsum(lens))).astype(np.int64)
    idx = nrng.integers(0, NV, size=int(ptr[-1])).astype(np.int64)
    for row, n in SPECIAL_ROWS.items():
        if n > 64:
            idx[ptr[row]] = idx[ptr[row + 1] - 1] = 0
        if n > 256:
            idx[ptr[row] + 256] = 0
    idx[ptr[11]] = 0            # the one-term row: `one` for the constraint rule, coeff * v[0] for the plain product
    idx[ptr[12] + 5] = 0
    rng = random.Random(65)
    coeff = [rng.randrange(R) for _ in range(int(ptr[-1]))]
    vec = [rng.randrange(R) for _ in range(NV)]
    return ptr, idx, coeff, vec


def _row_sums(ptr, idx, coeff, vec, one0):
    """every row's sum in Python integers; one0: a term with index 0 counts as 1 whatever its coefficient
    (LinearCombination.evaluate), else it is a term like any other"""
    ptr, idx = ptr.tolist(), idx.tolist()
    out = []
    for i in range(len(ptr) - 1):
        s = 0
        for t in range(ptr[i], ptr[i + 1]):
            j = idx[t]
            if one0 and j == 0:
                s += 1
            else:
                s += vec[j] * (coeff[t] if coeff is not None else 1)
        out.append(s % R)
    return out


@pytest.mark.parametrize("mode", ["random", "no_coefficients", "all_r-1"])
@pytest.mark.parametrize("entry", ["ozk_r1cs_evaluate_dev", "ozk_sparse_mat_vec_dev"])
def test_sparse_products_with_long_rows(entry, mode):
    """Both sparse entries (ONE0 = true / false in k_r1cs_eval_long1) on rows of 0 ... 40000 terms, through
    zksnark._CsrDevice as the prover and the setup call them.  all_r-1: coefficients and vector all r - 1, the largest
    terms, partial sums and LDS tree values there are."""
    from octopuszk_amd import lib, zksnark as z
    L = lib.load()
    ptr, idx, coeff, vec = _long_row_case()
    if mode == "no_coefficients":
        coeff = None
    elif mode == "all_r-1":
        coeff, vec = [R - 1] * len(coeff), [R - 1] * NV
    mat = z._CsrDevice(ptr, idx, None if coeff is None else np.array(coeff, dtype=object))
    assert mat.rows == ROWS and mat.n_long == 5
    d_vec = u.dev_from_ints(vec)
    out = u.poisoned(ROWS * 32 + u.GUARD)
    ws = z._CsrDevice.workspace([mat])
    ws.fill_(u.POISON)
    mat.apply(getattr(L, entry), d_vec, out, ws)
    torch.cuda.synchronize()
    want = _row_sums(ptr, idx, coeff, vec, one0=entry == "ozk_r1cs_evaluate_dev")
    bad = u.mismatches(u.ints(out, ROWS), want)
    lens = np.diff(ptr)
    assert not bad, "rows %s differ (their lengths: %s)" % (bad, [int(lens[i]) for i in bad])
    assert u.tail_untouched(out, ROWS * 32)


# ---------------------------------------------------------------------------------------------- D. lincomb3
@pytest.mark.parametrize("alias", ["separate", "a", "b", "c"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_lincomb3_values_and_aliasing(n, alias):
    """ozk_fr_lincomb3_dev: out[i] = (ka a[i] + kb b[i] + c[i]) kk, with `out` a buffer of its own or one of the
    inputs (include/ozk.h allows it; the setup relies on it).  Counts on both sides of a 256-lane block; constants and
    inputs at 0, 1 and r - 1 (all r - 1 is the largest ka a + kb b + c before its reduction).  The expected values come
    from the inputs as they were before the call; inputs that are not the output must come back unchanged."""
    from octopuszk_amd import lib
    L = lib.load()
    rng = random.Random(3000 + n)
    triples = [tuple(rng.randrange(R) for _ in range(3)), (0, 0, 1), (R - 1, R - 1, R - 1), (1, 1, 0)]
    inputs = {
        "random": [[rng.randrange(R) for _ in range(n)] for _ in range(3)],
        "all_r-1": [[R - 1] * n] * 3,
        "zero": [[0] * n] * 3,
    }
    scratch = u.poisoned(96 + u.GUARD)
    for ka, kb, kk in triples:
        for kind, (a, b, c) in inputs.items():
            d = {"a": u.dev_from_ints(a, u.GUARD), "b": u.dev_from_ints(b, u.GUARD), "c": u.dev_from_ints(c, u.GUARD)}
            out = u.poisoned(n * 32 + u.GUARD) if alias == "separate" else d[alias]
            hk = [u.host32(ka), u.host32(kb), u.host32(kk)]
            lib.check(L.ozk_fr_lincomb3_dev(d["a"].data_ptr(), d["b"].data_ptr(), d["c"].data_ptr(), n, u.vp(hk[0]),
                                            u.vp(hk[1]), u.vp(hk[2]), out.data_ptr(), scratch.data_ptr(), _stream()))
            torch.cuda.synchronize()
            what = (kind, "ka kb kk = %d %d %d" % (ka, kb, kk))
            want = [(ka * x + kb * y + w) * kk % R for x, y, w in zip(a, b, c)]
            bad = u.mismatches(u.ints(out, n), want)
            assert not bad, ("%d of %d values differ, first at %s" % (len(bad), n, bad[:8]), what)
            assert u.tail_untouched(out, n * 32), what
            for name, before in zip("abc", (a, b, c)):
                if name != alias:
                    assert u.ints(d[name], n) == before and u.tail_untouched(d[name], n * 32), (name, what)
    assert u.tail_untouched(scratch, 96)
