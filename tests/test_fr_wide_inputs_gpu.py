"""Reduction on load, entry point by entry point (include/ozk.h: the KZG, set-opening, multi-opening, PLONK and lookup
blocks): elements are plain 32-byte words, a word >= r is reduced mod r on load, and every output is canonical.  The
tests of each block write one element as x + r, which is below 2 r and so cannot tell a load that allows any 256-bit
word from one that allows two r.  Here every row, point, weight and host scalar is a full-width word:

  wide   x + k r, k cycling 0..5 by position (2^256 = 5.29 r: the largest k that fits);
  ones   rows, points and scalars of 2^256 - 1 alone, where the model allows it (points of a set stay distinct);
  edges  r, r + 1, 2 r - 1, 2 r, 2 r + 1, 3 r, 4 r, 5 r, 2^255, 2^256 - r, 2^256 - 1 where a row's structure changes
         (first and last element of a lane's piece, of a tile, of the row), and as points, weights and host scalars.

The expected output of every call is the block's integer model on the inputs mod r, compared as integers of the output's
bytes, so a non-canonical output fails; gaps and tails keep their sentinel.  The lengths are the smallest that cross a
tile: T - 1, T + 1, 2 T + 1."""
import random

import pytest

import fr_gpu_util as fu
import kzg_multi_ref as km
import kzg_ref as kr
import kzg_set_ref as ks
import plonk_lookup_ref as lm
import plonk_ref as pm
from fr_gpu_util import ALL_ONES, EDGE_WORDS, POISON_INT, R

pytestmark = pytest.mark.gpu

T = 1024                        # KZG_TILE = PLONK_TILE: the elements one workgroup stages
E_INVALID = -1
LENGTHS = [T - 1, T + 1, 2 * T + 1]
CASES = ["wide", "ones", "edges"]
NE = len(EDGE_WORDS)


def _rows(case, rng, count, length):
    """`count` rows as written for the case, with the conditions on them asserted"""
    if case == "ones":
        rows = [[ALL_ONES] * length for _ in range(count)]
    elif case == "wide":
        rows = [fu.wide_row(rng, length, phase=y) for y in range(count)]
    else:
        rows = [fu.with_edge_words(rng, length, shift=3 * y) for y in range(count)]
    for row in rows:
        fu.assert_wide([row], edges=case == "edges")
    return rows


def _scalars(case, rng, count, turn=0):
    """`count` points, weights or host scalars: turn `turn` of the edge words for the edges case"""
    if case == "ones":
        return [ALL_ONES] * count
    if case == "wide":
        out = fu.wide_scalars(rng, count)
        assert all(v >= 2 * R for v in out)
        return out
    return [EDGE_WORDS[(turn * count + i) % NE] for i in range(count)]


def _turns(case, count):
    """the calls it takes for every edge word to have been a scalar once"""
    return -(-NE // count) if case == "edges" else 1


def _sets(case, rng, count, t, allowed=EDGE_WORDS):
    """`count` sets of t points, pairwise distinct mod r: wide words, led by 2^256 - 1 (ones) or by edge word y (edges)"""
    sets = []
    for y in range(count):
        lead = {"wide": [], "ones": [ALL_ONES], "edges": [allowed[y % len(allowed)]]}[case]
        s = (lead + fu.wide_scalars(rng, t, phase=y))[:t]
        assert len({z % R for z in s}) == t
        sets.append(s)
    return sets


# ---------------------------------------------------------------------------- KZG openings
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("length", LENGTHS)
def test_poly_open(length, case):
    rng = random.Random(5000 + length)
    rows = _rows(case, rng, 3, length)
    # (npolys, poly_stride, points): three rows; for the edges, also ONE row at every edge word
    calls = [(3, length + 3, _scalars("wide" if case == "edges" else case, rng, 3))]
    if case == "edges":
        calls.append((NE, 0, list(EDGE_WORDS)))
        fu.assert_has_edge_words(calls[1][2])
    for npolys, stride, points in calls:
        flat = fu.flat(rows[:npolys if stride else 1], max(stride, length))
        got_q, got_y, gaps = fu.poly_open(flat, npolys, length, stride, points, length + 2)
        for y in range(npolys):
            q, val = kr.div_linear(fu.reduced(rows[y if stride else 0]), points[y] % R)
            assert got_y[y] == val, (length, case, npolys, y)
            assert got_q[y] == q, (length, case, npolys, y)
        assert all(v == POISON_INT for v in gaps)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("n", [64, 2 * T])
def test_evals_open(n, case):
    rng = random.Random(5010 + n)
    omega = kr.root(n)
    omega_written = fu.wide(omega, 5)                  # the host omega as a wide word (it must keep its order)
    assert omega_written >= 4 * R
    rows = _rows(case, rng, 3, n)
    inside = [fu.wide(pow(omega, 1, R), 3), fu.wide(pow(omega, n - 1, R), 5)]
    calls = [(3, n + 1, [_scalars("wide" if case == "edges" else case, rng, 1)[0]] + inside)]
    if case == "edges":
        calls.append((NE, 0, list(EDGE_WORDS)))        # r + 1, 2 r + 1 (the point 1) and 2 r - 1 (the point -1) lie inside
    for npolys, stride, points in calls:
        flat = fu.flat(rows[:npolys if stride else 1], max(stride, n), fill=9)
        got_q, got_y, _, _ = fu.evals_open(flat, npolys, n, stride, omega_written, points, n + 2)
        for y in range(npolys):
            q, val = kr.open_evals(fu.reduced(rows[y if stride else 0]), points[y] % R, omega)
            assert got_y[y] == val, (n, case, npolys, y)
            assert got_q[y] == q, (n, case, npolys, y)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("length", LENGTHS)
def test_rows_combine(length, case):
    rng = random.Random(5020 + length)
    k = NE if case == "edges" else 3
    rows = _rows(case, rng, k, length)
    weights = _scalars(case, rng, k)
    if case == "edges":
        fu.assert_has_edge_words(weights)
    got, tail_ok = fu.rows_combine(fu.flat(rows, length + 1), k, length, length + 1, weights)
    assert got == kr.combine(fu.reduced(rows), fu.reduced(weights)) and tail_ok


# ---------------------------------------------------------------------------- set openings and values at a set
def _set_case(case, rng, length, t, allowed=EDGE_WORDS):
    """(rows, [(npolys, stride, sets)]): three rows at their own sets; for the edges, ONE row at a set per edge word"""
    rows = _rows(case, rng, 3, length)
    calls = [(3, length + 3, _sets("wide" if case == "edges" else case, rng, 3, t))]
    if case == "edges":
        calls.append((len(allowed), 0, _sets(case, rng, len(allowed), t, allowed)))
        assert {s[0] for s in calls[1][2]} == set(allowed)
    return rows, calls


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("t", [1, 3, 32])
def test_poly_open_set(t, length, case):
    rng = random.Random(5030 + 10 * length + t)
    rows, calls = _set_case(case, rng, length, t)
    for npolys, stride, sets in calls:
        flat = fu.flat(rows[:npolys if stride else 1], max(stride, length))
        pts = [z for s in sets for z in s]
        got_q, got_y, gaps, _, _ = fu.poly_open_set(flat, npolys, length, stride, t, pts, length + 2)
        for y in range(npolys):
            q, values = ks.div_set(fu.reduced(rows[y if stride else 0]), fu.reduced(sets[y]))
            assert got_y[t * y:t * (y + 1)] == values, (t, length, case, npolys, y)
            assert got_q[y] == q, (t, length, case, npolys, y)
        assert all(v == POISON_INT for v in gaps)


def test_points_equal_mod_r_are_still_rejected():
    """two points of a set that differ as words and agree mod r: rejected on the host, nothing written"""
    rng = random.Random(5040)
    length = T + 1
    rows = _rows("wide", rng, 1, length)
    x = rng.randrange(R)
    for pts in ([x, x + R], [fu.wide(x, 2), fu.wide(x, 4)], [R, 3 * R], [ALL_ONES, ALL_ONES % R]):
        assert pts[0] != pts[1] and pts[0] % R == pts[1] % R
        _, _, _, quot, vals = fu.poly_open_set(rows[0], 1, length, length, 2, pts, length, expect=E_INVALID)
        assert fu.tail_untouched(quot, 0) and fu.tail_untouched(vals, 0)
        omega = kr.root(64)
        if all(pow(z, 64, R) != 1 for z in pts):
            _, _, quot, vals = fu.evals_open_set(rows[0][:64], 1, 64, 64, omega, 2, pts, 64, expect=E_INVALID)
            assert fu.tail_untouched(quot, 0) and fu.tail_untouched(vals, 0)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("n", [64, 2 * T])
@pytest.mark.parametrize("t", [1, 8])
def test_evals_open_set(t, n, case):
    rng = random.Random(5050 + 10 * n + t)
    omega = kr.root(n)
    omega_written = fu.wide(omega, 5)
    # every point must lie outside the domain: of the edge words, r + 1 and 2 r + 1 (the point 1) and 2 r - 1 (the
    # point -1) lie in every domain, and the model does not allow them here
    allowed = [e for e in EDGE_WORDS if pow(e % R, n, R) != 1]
    assert set(EDGE_WORDS) - set(allowed) == {R + 1, 2 * R + 1, 2 * R - 1}
    rows, calls = _set_case(case, rng, n, t, allowed)
    for npolys, stride, sets in calls:
        assert all(pow(z % R, n, R) != 1 for s in sets for z in s)
        flat = fu.flat(rows[:npolys if stride else 1], max(stride, n), fill=9)
        pts = [z for s in sets for z in s]
        got_q, got_y, _, _ = fu.evals_open_set(flat, npolys, n, stride, omega_written, t, pts, n + 2)
        for y in range(npolys):
            q, values = ks.open_set_evals(fu.reduced(rows[y if stride else 0]), fu.reduced(sets[y]), omega)
            assert got_y[t * y:t * (y + 1)] == values, (t, n, case, npolys, y)
            assert got_q[y] == q, (t, n, case, npolys, y)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("length", LENGTHS)
@pytest.mark.parametrize("t", [1, 3, 32])
def test_poly_eval_set(t, length, case):
    rng = random.Random(5060 + 10 * length + t)
    rows, calls = _set_case(case, rng, length, t)
    for npolys, stride, sets in calls:
        flat = fu.flat(rows[:npolys if stride else 1], max(stride, length))
        got, _ = fu.poly_eval_set(flat, npolys, length, stride, t, [z for s in sets for z in s])
        used = [fu.reduced(rows[y if stride else 0]) for y in range(npolys)]
        assert got == [v for row in km.values_at(used, fu.reduced(sets)) for v in row], (t, length, case, npolys)


# ---------------------------------------------------------------------------- the PLONK rows
def _quotient_scalars(case, rng, count, turn):
    """(k_0, `count` further host scalars) of a quotient call.  The kernel does not read k_0 (column a has the label X
    itself), so the model is given a k_0 that is 1 mod r: 5 r + 1, or for the edges r + 1 and 2 r + 1 in turn.  The
    further scalars are alpha, beta, gamma, k_1, k_2, the four Z_H inverses (then eta, theta): over the two turns they
    hold the nine other edge words, the five that are 0 mod r as gamma, k_1 and k_2 only, since alpha = 0, beta = 0
    or a Z_H inverse of 0 would take whole terms, or the whole value, out of the comparison"""
    if case != "edges":
        return 5 * R + 1, _scalars(case, rng, count)
    a, b, c, d = 2 * R - 1, 1 << 255, (1 << 256) - R, ALL_ONES              # the edge words that are neither 0 nor 1 mod r
    sc = ([a, b, R, 2 * R, 3 * R, c, d, a, b, c, d], [d, c, 4 * R, 5 * R, b, a, d, b, c, b, a])[turn]
    return (R + 1, 2 * R + 1)[turn], sc[:count]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("length", LENGTHS)
def test_rows_coset(length, case):
    rng = random.Random(5070 + length)
    rows = _rows(case, rng, 3, length)
    out_len = length + 5                                                     # (zero-extended)
    seen = []
    for turn in range(_turns(case, 2)):
        s, c = _scalars(case, rng, 2, turn)
        seen += [s, c]
        got, gaps = fu.rows_coset(fu.flat(rows, length + 3), 3, length, length + 3, s, c, out_len, out_len + 2)
        assert got == pm.rows_coset(fu.reduced(rows), s % R, c % R, out_len), (length, case, turn)
        assert all(v == POISON_INT for v in gaps)
    if case == "edges":
        fu.assert_has_edge_words(seen)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("length", LENGTHS)
def test_perm_product(length, case):
    rng = random.Random(5080 + length)
    rows = _rows(case, rng, 6, length)
    wires, sigma = rows[:3], rows[3:]
    seen = []
    for turn in range(_turns(case, 6)):
        omega, k0, k1, k2, beta, gamma = sc = _scalars(case, rng, 6, turn)
        seen += sc
        z, behind, total, zeros = fu.perm_product(wires, sigma, length, length + 3, omega, beta, gamma, ks=(k0, k1, k2))
        want = pm.perm_product(fu.reduced(wires), fu.reduced(sigma), omega % R, fu.reduced([k0, k1, k2]), beta % R, gamma % R)
        assert (z, total, zeros) == want, (length, case, turn)
        assert z[0] == 1 and behind == [POISON_INT] * 2
    if case == "edges":
        fu.assert_has_edge_words(seen)


@pytest.mark.parametrize("length,at", [(T - 1, 0), (T + 1, T - 1), (2 * T + 1, T + 11), (2 * T + 1, 2 * T)])
def test_perm_product_with_a_denominator_that_is_zero_only_mod_r(length, at):
    """w + beta s + gamma = 0 mod r with the wire, the sigma and gamma all written as wide words: the row is counted,
    its factor is 1 and every other row is exact"""
    rng = random.Random(5090 + length + at)
    rows = _rows("wide", rng, 6, length)
    wires, sigma = rows[:3], rows[3:]
    j = at % 3
    wires[j][at], sigma[j][at] = fu.wide(rng.randrange(R), 4), fu.wide(rng.randrange(R), 3)
    omega, beta = fu.wide(kr.root(4 * T), 5), fu.wide(rng.randrange(R), 2)
    gamma = fu.wide(-(wires[j][at] + beta * sigma[j][at]) % R, 5)
    assert min(wires[j][at], sigma[j][at], gamma, beta) >= 2 * R and (wires[j][at] + beta * sigma[j][at] + gamma) % R == 0
    z, _, total, zeros = fu.perm_product(wires, sigma, length, length, omega, beta, gamma)
    want = pm.perm_product(fu.reduced(wires), fu.reduced(sigma), omega % R, pm.KS, beta % R, gamma % R)
    assert want[2] == 1 and zeros == 1 and (z, total) == want[:2]
    if at + 1 < length:
        assert z[at + 1] == z[at]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("n", [4, 256])
def test_plonk_quotient(n, case):
    """the formula on any fifteen rows (no witness is needed for it): alpha, beta, gamma, the k_j and the four Z_H
    inverses are host scalars taken mod r"""
    rng = random.Random(5100 + n)
    rows = _rows(case, rng, 15, 4 * n)
    wit, key = rows[:5], rows[5:]
    seen = []
    for turn in range(_turns(case, 9)):
        k0, sc = _quotient_scalars(case, rng, 9, turn)
        seen += [k0] + sc
        ch, k3, zh = sc[:3], [k0] + sc[3:5], sc[5:]
        got = fu.plonk_quotient(wit, key, n, ch, 4 * n + 3, 4 * n + 1, ks=k3, zh_inv=zh)
        assert got == pm.quotient_on_coset(fu.reduced(wit), fu.reduced(key), n, *fu.reduced(ch), fu.reduced(k3),
                                           fu.reduced(zh)), (n, case, turn)
    if case == "edges":
        fu.assert_has_edge_words(seen)


# ---------------------------------------------------------------------------- the lookup argument
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("length", LENGTHS)
def test_lookup_sum(length, case):
    rng = random.Random(5110 + length)
    rows = _rows(case, rng, 8, length)
    wires, key4, m = rows[:3], rows[3:7], rows[7]
    seen = []
    for turn in range(_turns(case, 2)):
        eta, theta = _scalars(case, rng, 2, turn)
        seen += [eta, theta]
        s, behind, total, zeros = fu.lookup_sum(wires, key4, m, length, length + 3, length + 1, eta, theta)
        want = lm.lookup_sum(fu.reduced(wires), fu.reduced(key4), fu.reduced(m), eta % R, theta % R)
        assert (s, total, zeros) == want, (length, case, turn)
        assert s[0] == 0 and behind == [POISON_INT] * 2
    if case == "edges":
        fu.assert_has_edge_words(seen)


@pytest.mark.parametrize("length,p,q", [(T - 1, 0, T - 2), (T + 1, T - 1, T), (2 * T + 1, 2 * T, T + 11)])
def test_lookup_sum_with_denominators_that_are_zero_only_mod_r(length, p, q):
    """theta + t_p = 0 and theta + f_q = 0 mod r with the table row, the wires, eta and theta written as wide words:
    both are counted, both fractions are 0 and every other row is exact"""
    rng = random.Random(5120 + length + p)
    rows = _rows("wide", rng, 8, length)
    wires, key4, m = rows[:3], rows[3:7], rows[7]
    eta = fu.wide(rng.randrange(R), 3)
    for j in range(3):
        key4[1 + j][p] = fu.wide(rng.randrange(R), 2 + j)
        wires[j][q] = fu.wide(key4[1 + j][p] % R, 5 - j)                     # the same tuple mod r, another word
    theta = fu.wide(-(key4[1][p] + eta * key4[2][p] + eta * eta * key4[3][p]) % R, 4)
    assert min([theta, eta] + [key4[1 + j][p] for j in range(3)] + [wires[j][q] for j in range(3)]) >= 2 * R
    s, _, total, zeros = fu.lookup_sum(wires, key4, m, length, length, length, eta, theta)
    want = lm.lookup_sum(fu.reduced(wires), fu.reduced(key4), fu.reduced(m), eta % R, theta % R)
    assert want[2] == 2 and zeros == 2 and (s, total) == want[:2]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("n", [4, 256])
def test_lookup_quotient(n, case):
    rng = random.Random(5130 + n)
    rows = _rows(case, rng, 21, 4 * n)
    wit, key = rows[:7], rows[7:]
    seen = []
    for turn in range(_turns(case, 9)):
        k0, sc = _quotient_scalars(case, rng, 11, turn)
        seen += [k0] + sc
        ch, k3, zh = sc[:3] + sc[9:], [k0] + sc[3:5], sc[5:9]             # alpha, beta, gamma, eta, theta
        got = fu.plonk_quotient(wit, key, n, ch, 4 * n + 3, 4 * n + 1, ks=k3, zh_inv=zh)
        assert got == lm.quotient_on_coset(fu.reduced(wit), fu.reduced(key), n, *fu.reduced(ch), fu.reduced(k3),
                                           fu.reduced(zh)), (n, case, turn)
    if case == "edges":
        fu.assert_has_edge_words(seen)


def test_lookup_index_and_counts_of_the_widest_words():
    """a table row of 2^256 - 1 three times, its canonical copy, and a copy of row 0 written as 5 r + x: every lookup of
    either tuple, however it is written, lands on the lowest equal row"""
    rng = random.Random(5140)
    x = tuple(rng.randrange(R // 4) for _ in range(3))                          # (5 r + x fits 256 bits)
    ones = (ALL_ONES,) * 3
    table = [x, tuple(rng.randrange(R) for _ in range(3)), tuple(5 * R + v for v in x), ones,
             tuple(v % R for v in ones), tuple(rng.randrange(R) for _ in range(3))]
    assert all(v <= ALL_ONES for row in table for v in row)
    forms = [x, table[2], tuple(v + 3 * R for v in x), ones, table[4], table[1], tuple(v + 2 * R for v in table[5])]
    length = 2 * T + 1
    lookups = [forms[rng.randrange(len(forms))] for _ in range(length)]
    wires = [[row[j] for row in lookups] for j in range(3)]
    qk = [fu.wide(1 + i % 3, i % 6) for i in range(length)]
    m_len = len(table) + 2
    want = lm.multiplicities(wires, qk, table, m_len)
    assert want[1:] == (0, lm.MISSING_NONE) and want[0][2] == 0 and want[0][4] == 0 and want[0][0] > 0 and want[0][3] > 0
    m, behind, missing, first, slots = fu.lookup_counts(wires, qk, table, m_len, length + 3, len(table) + 1)
    assert (m, missing, first) == want and behind == [POISON_INT] * 2
    assert sorted(s for s in slots if s != 0xffffffff) == [0, 1, 3, 5]          # the lowest row of every tuple
