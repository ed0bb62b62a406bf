"""GPU tests of the lookup argument of the PLONK prover: the entry points of
csrc/plonk_lookup.cuh against the integer model (tests/plonk_lookup_ref.py), byte for byte, with sentinel-filled outputs
and gaps, and the protocol of octopuszk_amd/plonk for a circuit with a table over a string of known tau."""
import ctypes
import random

import pytest
import torch

import kzg_ref as kr
import plonk_lookup_ref as lm
import plonk_ref as pm
import srs_gpu_util as u
from fr_gpu_util import lookup_counts as _counts
from fr_gpu_util import lookup_sum as _sum
from fr_gpu_util import plonk_quotient as _plonk_quotient
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

R = o.R
T = 1024                       # PLONK_TILE: the rows one workgroup of the sum handles
BATCH = 8                      # KZG_INV_BATCH: the rows of one lane, inverted together
SCAN = 256                     # PLONK_SCAN_WG: the tile sums one round of the scan takes
E_INVALID = -1
TAU = 0x5eed0123456789abcdef0123456789abcdef0123456789abcdef % R
M = 512                        # 2 M + 1 >= 1024 powers in G1
SENTINEL = 0xA5
SENTINEL_INT = int.from_bytes(bytes([SENTINEL]) * 32, "little")
NONE = lm.MISSING_NONE


def _lib():
    from octopuszk_amd import lib
    return lib.load()


def _ptr(t):
    return ctypes.c_void_p(int(t.data_ptr()))


def _stream():
    return ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))


def _host_ints(values):
    buf = ctypes.create_string_buffer(b"".join(kr.le(v) for v in values), 32 * len(values))
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")


def _columns(table):
    return [[row[j] for row in table] for j in range(3)]


# ---------------------------------------------------------------------------- index and counts
def _special_tuples(rng):
    """one tuple and its near misses: word 7 of the third column, word 0 of the first, two column permutations"""
    x = [rng.getrandbits(220) for _ in range(3)]
    return [tuple(x), (x[0], x[1], x[2] + (1 << 224)), tuple(x), (x[0] ^ 1, x[1], x[2]), (x[1], x[0], x[2]),
            (x[2], x[1], x[0]), (x[0], x[1], x[2] + (2 << 224)), (x[0] ^ 2, x[1], x[2]), (x[0], x[2], x[1])]


def _scenario(n_rows, length, seed):
    """a table of n_rows (row 2 equals row 0, the last row equals row 5 when there are that many) and `length` wire rows:
    three in four look a table row up, written as v + k r; the others hold any tuple, absent ones among them"""
    rng = random.Random(seed)
    special = _special_tuples(rng)
    table = special[:6][:n_rows] + [tuple(rng.randrange(R) for _ in range(3)) for _ in range(n_rows - 6)]
    if n_rows > 6:
        table[-1] = table[5]
    absent = special[6:] + special[n_rows:6]
    rows, qk = [], []
    for i in range(length):
        if rng.randrange(4):
            rows.append(table[rng.randrange(n_rows) if i % 5 else rng.randrange(min(n_rows, 6))])
            qk.append(1 + R * (i % 2) if i % 7 else rng.randrange(1, R))       # any value that is not 0 mod r
        else:
            rows.append(absent[rng.randrange(len(absent))] if i % 2 else table[rng.randrange(n_rows)])
            qk.append(0 if i % 4 else R)                                       # r itself is 0 mod r
    written = [[row[j] + R * ((i + j) % 4) for i, row in enumerate(rows)] for j in range(3)]
    return table, _columns(rows), written, qk


@pytest.mark.parametrize("length", [1, T - 1, T, T + 1, 2 * T + 1])
@pytest.mark.parametrize("n_rows", [1, 2, 3, 255, T, T + 1])
def test_counts_match_the_model(n_rows, length):
    table, wires, written, qk = _scenario(n_rows, length, 3100 + 10 * n_rows + length)
    m_len = n_rows + 3
    want = lm.multiplicities(wires, qk, table, m_len)
    assert want[1] == 0 and sum(want[0]) == sum(1 for v in qk if v % R)
    m, behind, missing, first, slots = _counts(written, qk, table, m_len, length + 3, n_rows + 1)
    assert (m, missing, first) == want and behind == [SENTINEL_INT] * 2
    # padding rows and the later copies of a row stay 0; a tuple's slot holds its lowest row
    assert m[n_rows:] == [0, 0, 0] and (n_rows < 3 or m[2] == 0) and (n_rows <= 6 or m[n_rows - 1] == 0)
    live = sorted(s for s in slots if s != 0xffffffff)
    first_of = {}
    for i, row in enumerate(table):
        first_of.setdefault(row, i)
    assert live == sorted(first_of.values())


def test_every_lookup_on_one_table_row():
    """2049 adds to one address; the table's other rows, near misses of it, stay 0"""
    rng = random.Random(3110)
    table = _special_tuples(rng)[:6]
    length = 2 * T + 1
    wires = _columns([table[3]] * length)
    m, _, missing, first, _ = _counts(wires, [1] * length, table, 8)
    assert (m, missing, first) == ([0, 0, 0, length, 0, 0, 0, 0], 0, NONE)


@pytest.mark.parametrize("at", [[0], [T], [2 * T], [T - 1, T], [5, T - 1, T, T + 70]])
def test_a_miss_is_counted_and_the_first_is_named(at):
    """near misses of table rows with qK = 1, also on both sides of a tile edge"""
    table, wires, written, qk = _scenario(255, 2 * T + 1, 3120 + len(at) + at[0])
    absent = _special_tuples(random.Random(3120 + len(at) + at[0]))[6:]
    for k, i in enumerate(at):
        qk[i] = 1
        for j in range(3):
            written[j][i] = wires[j][i] = absent[k % 3][j]
    want = lm.multiplicities(wires, qk, table, 255)
    assert want[1:] == (len(at), at[0])
    m, _, missing, first, _ = _counts(written, qk, table, 255)
    assert (m, missing, first) == want


def test_two_runs_give_the_same_bytes():
    table, _, written, qk = _scenario(T + 1, 2 * T + 1, 3130)
    first = _counts(written, qk, table, T + 1)
    again = _counts(written, qk, table, T + 1)
    assert first[:4] == again[:4] and sorted(first[4]) == sorted(again[4])


# ---------------------------------------------------------------------------- the running sum
def _consistent(length, seed, n_rows=None):
    """(wires, the rows qK, T1, T2, T3, m) of `length` rows that look up a table of n_rows, padded to `length`"""
    rng = random.Random(seed)
    n_rows = n_rows or min(length, 5)
    table = [tuple(rng.getrandbits(253) for _ in range(3)) for _ in range(n_rows)]
    qk = [rng.randrange(2) for _ in range(length)]
    picks = [rng.randrange(n_rows) for _ in range(length)]
    wires = _columns([table[p] if sel else tuple(rng.getrandbits(253) for _ in range(3)) for p, sel in zip(picks, qk)])
    m = [0] * length
    for p, sel in zip(picks, qk):
        m[p] += sel
    key4 = [qk] + _columns(table + [table[-1]] * (length - n_rows))
    return wires, key4, m


SUM_LENGTHS = [1, BATCH - 1, BATCH, BATCH + 1, T - 1, T, T + 1, 2 * T + 1]


@pytest.mark.parametrize("length", SUM_LENGTHS)
def test_sum_of_a_consistent_witness_closes(length):
    wires, key4, m = _consistent(length, 3140 + length)
    rng = random.Random(3141 + length)
    eta, theta = rng.randrange(R), rng.randrange(R)
    written = [list(row) for row in wires]
    written[1][length // 2] += R                                          # one element written as w + r
    s, behind, total, zeros = _sum(written, key4, m, length, length + 3, length + 1, eta, theta)
    assert (s, total, zeros) == lm.lookup_sum(wires, key4, m, eta, theta)
    assert s[0] == 0 and total == 0 and zeros == 0 and behind == [SENTINEL_INT] * 2


@pytest.mark.parametrize("length", SUM_LENGTHS)
def test_sum_with_m_off_by_one_does_not_close(length):
    wires, key4, m = _consistent(length, 3150 + length)
    rng = random.Random(3151 + length)
    eta, theta = rng.randrange(R), rng.randrange(R)
    m[rng.randrange(min(length, 5))] += 1
    s, _, total, zeros = _sum(wires, key4, m, length, length, length, eta, theta)
    assert (s, total, zeros) == lm.lookup_sum(wires, key4, m, eta, theta) and total != 0 and zeros == 0


@pytest.mark.parametrize("length,p,q", [(BATCH + 1, 0, BATCH), (T + 1, BATCH, T - 1), (2 * T + 1, T, BATCH - 1),
                                        (2 * T + 1, 2 * T, 0), (2 * T + 1, T - 1, T - 1), (2 * T + 1, 0, 2 * T)])
def test_sum_with_zero_denominators(length, p, q):
    """theta + t_p = 0 on the table side and theta + f_q = 0 on the wire side (first row, edge of a batch, edge of a
    tile, last row): both are counted, both fractions are 0, every other row is exact"""
    wires, key4, m = _consistent(length, 3160 + length + p, n_rows=length)
    rng = random.Random(3161 + length + p)
    eta = rng.randrange(R)
    for j in range(3):
        wires[j][q] = key4[1 + j][p]
    key4[0][q] = 1
    theta = -(key4[1][p] + eta * key4[2][p] + eta * eta * key4[3][p]) % R
    m[p] += 1
    s, _, total, zeros = _sum(wires, key4, m, length, length, length, eta, theta)
    want = lm.lookup_sum(wires, key4, m, eta, theta)
    assert want[2] >= 2 and (s, total, zeros) == want         # (and every other row that looks row p up)
    if p + 1 < length and p != q and key4[0][p] == 0:
        assert s[p + 1] == s[p]


def test_sum_past_one_round_of_the_scan():
    """SCAN tiles + 1: the scan of the tile sums takes a second round"""
    length = SCAN * T + T + 1
    wires, key4, m = _consistent(length, 3170, n_rows=300)
    eta, theta = 3 ** 100 % R, 5 ** 100 % R
    s, _, total, zeros = _sum(wires, key4, m, length, length, length, eta, theta)
    assert (s, total, zeros) == lm.lookup_sum(wires, key4, m, eta, theta) and total == 0


# ---------------------------------------------------------------------------- the quotient
def _coset_rows(rows, n):
    w4 = kr.root(4 * n)
    return [kr.ntt(row, w4) for row in pm.rows_coset(rows, pm.G, 1, 4 * n)]


def _lookup_case(n, rng):
    if n == 2:
        table = [tuple(rng.randrange(R) for _ in range(3)) for _ in range(2)]
        return lm.LookupCircuit(2, [[0, 0]] * 5, [[0, 0], [1, 0], [2, 0]], 0, [1, 0], table), list(table[1])
    table = [tuple(rng.randrange(R) for _ in range(3)) for _ in range(min(n - 1, 300))]
    table[-1] = table[0]
    return lm.chain_with_lookups(n, 1, rng, table, n // 2 - 1 if n > 4 else 2)


def _quotient_inputs(n, spoil=None):
    """(the seven witness rows and the fourteen key rows on the coset, the challenges) of a valid witness, or of one
    with m one too high at a row (spoil = "m") or S altered at one row ("S")"""
    rng = random.Random(3180 + n)
    circuit, assignment = _lookup_case(n, rng)
    omega = kr.root(n)
    alpha, beta, gamma, eta, theta = (rng.randrange(R) for _ in range(5))
    wires, key4 = circuit.wire_values(assignment), circuit.key4()
    public = circuit.public_inputs(assignment)
    m, missing, _ = lm.multiplicities(wires, key4[0], circuit.table, n)
    zs, total, _ = pm.perm_product(wires, pm.sigma_labels(circuit), omega, pm.KS, beta, gamma)
    ss, s_total, s_zeros = lm.lookup_sum(wires, key4, m, eta, theta)
    assert missing == 0 and total == 1 and s_total == 0 and s_zeros == 0
    if spoil == "m":
        m[m.index(max(m))] += 1
    if spoil == "S":
        ss[n - 1] = (ss[n - 1] + 1) % R
    wit = ([kr.intt(col, omega) for col in wires] + [kr.intt(zs, omega), kr.intt(pm.pi_evals(n, public), omega)]
           + [kr.intt(m, omega), kr.intt(ss, omega)])
    polys = lm.key_polys(circuit)
    key = polys[:8] + [[pm.inv(n)] * n, [0, 1] + [0] * (n - 2)] + polys[8:]
    return _coset_rows(wit, n), _coset_rows(key, n), (alpha, beta, gamma, eta, theta)


def _quotient(wit, key, n, ch, wit_stride, key_stride, vanilla=False):
    return _plonk_quotient(wit, key, n, ch[:3] if vanilla else ch, wit_stride, key_stride)


def _top_quarter(got, n):
    return pm.rows_coset([kr.intt(got, kr.root(4 * n))], pm.inv(pm.G), 1)[0][3 * n:]


@pytest.mark.parametrize("n", [2, 4, 256, 1024])
def test_quotient_of_a_valid_witness_is_a_polynomial(n):
    wit, key, ch = _quotient_inputs(n)
    written = [list(row) for row in wit]
    written[6][4 * n - 1] += R                                            # S's last value, read again by point 4 n - 5
    written[5][0] += R
    got = _quotient(written, key, n, ch, 4 * n + 3, 4 * n + 1)
    assert got == lm.quotient_on_coset(wit, key, n, *ch, pm.KS, pm.zh_inverses(n))
    assert _top_quarter(got, n) == [0] * n


@pytest.mark.parametrize("spoil", ["m", "S"])
@pytest.mark.parametrize("n", [2, 4, 256, 1024])
def test_quotient_of_a_spoilt_lookup_is_no_polynomial(n, spoil):
    wit, key, ch = _quotient_inputs(n, spoil)
    got = _quotient(wit, key, n, ch, 4 * n, 4 * n)
    assert got == lm.quotient_on_coset(wit, key, n, *ch, pm.KS, pm.zh_inverses(n))
    assert any(_top_quarter(got, n))


@pytest.mark.parametrize("n", [2, 4, 256, 1024])
def test_quotient_without_lookups_is_the_vanilla_quotient(n):
    """qK = 0, m = 0, S = 0, any table: byte for byte what ozk_plonk_quotient_dev writes for the same rows"""
    wit, key, ch = _quotient_inputs(n)
    zero = [0] * (4 * n)
    wit, key = wit[:5] + [zero, zero], key[:10] + [zero] + key[11:]
    got = _quotient(wit, key, n, ch, 4 * n, 4 * n + 2)
    assert got == _quotient(wit[:5], key[:10], n, ch, 4 * n, 4 * n + 2, vanilla=True)
    assert got == pm.quotient_on_coset(wit[:5], key[:10], n, *ch[:3], pm.KS, pm.zh_inverses(n))


# ---------------------------------------------------------------------------- rejections
def test_rejected_shapes_launch_nothing():
    L = _lib()
    n = 8
    buf = torch.full((64 * 4 * n * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    ws = _ws(1 << 20)
    null = ctypes.c_void_p(0)
    stream = _stream()
    keep_one, one = _host_ints([1])
    keep_ks, ks = _host_ints(list(pm.KS))
    keep_zh, zh = _host_ints(pm.zh_inverses(n))
    E = 32
    wires, qk, table = buf[:3 * n * E], buf[3 * n * E:4 * n * E], buf[4 * n * E:7 * n * E]
    index, m = buf[7 * n * E:8 * n * E], buf[8 * n * E:9 * n * E]
    miss, first = buf[9 * n * E:9 * n * E + 4], buf[9 * n * E + 4:9 * n * E + 8]
    ib = L.ozk_plonk_lookup_index_bytes(n)
    assert ib == 4 * 16

    for bad in (0, -1, (1 << 28) + 1):
        assert L.ozk_plonk_lookup_index_bytes(bad) == 0
        assert L.ozk_plonk_lookup_index_dev(null, bad, n, null, 0, stream) == E_INVALID
    assert L.ozk_plonk_lookup_index_dev(_ptr(table), n, n - 1, _ptr(index), ib, stream) == E_INVALID
    assert L.ozk_plonk_lookup_index_dev(null, n, n, _ptr(index), ib, stream) == E_INVALID
    assert L.ozk_plonk_lookup_index_dev(_ptr(table), n, n, null, ib, stream) == E_INVALID
    assert L.ozk_plonk_lookup_index_dev(_ptr(table[8:]), n, n, _ptr(index), ib, stream) == E_INVALID
    assert b"aligned" in L.ozk_last_error()
    assert L.ozk_plonk_lookup_index_dev(_ptr(table), n, n, _ptr(index), ib - 1, stream) == E_INVALID
    assert b"index" in L.ozk_last_error()
    assert L.ozk_plonk_lookup_index_dev(_ptr(table), n, n, _ptr(table[(3 * n - 1) * E:]), ib, stream) == E_INVALID
    assert b"overlap" in L.ozk_last_error()

    def counts(w_, q_, length, stride, t_, rows, tstride, i_, ibytes, m_, m_len, mi, fi):
        return L.ozk_plonk_lookup_counts_dev(w_, q_, length, stride, t_, rows, tstride, i_, ibytes, m_, m_len, mi, fi, stream)

    good = [_ptr(wires), _ptr(qk), n, n, _ptr(table), n, n, _ptr(index), ib, _ptr(m), n, _ptr(miss), _ptr(first)]
    assert counts(null, null, 0, n, null, n, n, null, 0, null, n, null, null) == E_INVALID          # len = 0
    assert counts(null, null, n, n, null, 0, n, null, 0, null, n, null, null) == E_INVALID          # n_rows = 0
    assert counts(null, null, n, n, null, n, n, null, 0, null, n - 1, null, null) == E_INVALID      # n_rows above m_len
    assert counts(*(good[:3] + [n - 1] + good[4:])) == E_INVALID
    assert counts(*(good[:6] + [n - 1] + good[7:])) == E_INVALID
    for i in (0, 1, 4, 7, 9, 11, 12):
        assert counts(*(good[:i] + [null] + good[i + 1:])) == E_INVALID
    for i, off in ((0, wires[8:]), (1, qk[8:]), (4, table[8:]), (9, m[8:])):
        assert counts(*(good[:i] + [_ptr(off)] + good[i + 1:])) == E_INVALID
        assert b"aligned" in L.ozk_last_error()
    assert counts(*(good[:11] + [_ptr(miss[1:])] + good[12:])) == E_INVALID
    assert counts(*(good[:8] + [ib - 4] + good[9:])) == E_INVALID                                    # a short index
    assert b"index" in L.ozk_last_error()
    for i, off in ((9, wires[(3 * n - 1) * E:]), (9, table), (9, index), (11, m[4:]), (12, miss), (11, qk[4:])):
        assert counts(*(good[:i] + [_ptr(off)] + good[i + 1:])) == E_INVALID
        assert b"overlap" in L.ozk_last_error()

    key4, s_out = buf[16 * n * E:20 * n * E], buf[20 * n * E:21 * n * E]
    total, count = buf[21 * n * E:21 * n * E + 32], buf[21 * n * E + 32:21 * n * E + 64]

    def lsum(w_, stride, k_, kstride, m_, length, et, th, s_, t_, c_, w=_ptr(ws), wbytes=1 << 20):
        return L.ozk_plonk_lookup_sum_dev(w_, stride, k_, kstride, m_, length, et, th, s_, t_, c_, w, wbytes, stream)

    good = [_ptr(wires), n, _ptr(key4), n, _ptr(m), n, one, one, _ptr(s_out), _ptr(total), _ptr(count)]
    for bad in (0, -1, (1 << 28) + 1):
        assert L.ozk_plonk_lookup_sum_workspace_bytes(bad) == 0
        assert lsum(null, bad, null, bad, null, bad, null, null, null, null, null, w=null, wbytes=0) == E_INVALID
    assert lsum(*(good[:1] + [n - 1] + good[2:])) == E_INVALID
    assert lsum(*(good[:3] + [n - 1] + good[4:])) == E_INVALID
    for i in (0, 2, 4, 6, 7, 8, 9, 10):
        assert lsum(*(good[:i] + [null] + good[i + 1:])) == E_INVALID
    assert lsum(*good, w=null) == E_INVALID
    for i, off in ((0, wires[8:]), (2, key4[8:]), (4, m[8:]), (8, s_out[8:]), (9, total[8:])):
        assert lsum(*(good[:i] + [_ptr(off)] + good[i + 1:])) == E_INVALID
        assert b"aligned" in L.ozk_last_error()
    assert lsum(*(good[:10] + [_ptr(count[1:])])) == E_INVALID
    for i, off in ((8, wires), (8, key4[(4 * n - 1) * E:]), (8, m), (9, s_out[32:]), (10, total), (9, key4)):
        assert lsum(*(good[:i] + [_ptr(off)] + good[i + 1:])) == E_INVALID
        assert b"overlap" in L.ozk_last_error()
    assert lsum(*good, wbytes=L.ozk_plonk_lookup_sum_workspace_bytes(n) - 1) == E_INVALID
    assert b"workspace" in L.ozk_last_error()
    for inside in (s_out, total, count[:4], wires[(3 * n - 1) * E:], key4, m):    # a workspace that another buffer lies in
        assert lsum(*good, w=_ptr(inside)) == E_INVALID
        assert b"d_workspace overlaps" in L.ozk_last_error()

    n4 = 4 * n
    wit, key, t_out = buf[:7 * n4 * E], buf[7 * n4 * E:21 * n4 * E], buf[21 * n4 * E:22 * n4 * E]

    def quot(w_, ws_, k_, ks_, n_, al, be, ga, kk, zz, et, th, o_):
        return L.ozk_plonk_quotient_lookup_dev(w_, ws_, k_, ks_, n_, al, be, ga, kk, zz, et, th, o_, stream)

    good = [_ptr(wit), n4, _ptr(key), n4, n, one, one, one, ks, zh, one, one, _ptr(t_out)]
    for bad in (0, 1, 6, (1 << 26) + 1, 1 << 27):
        assert quot(null, n4, null, n4, bad, null, null, null, null, null, null, null, null) == E_INVALID
    assert quot(*(good[:1] + [n4 - 1] + good[2:])) == E_INVALID
    assert quot(*(good[:3] + [n4 - 1] + good[4:])) == E_INVALID
    for i in (0, 2, 5, 6, 7, 8, 9, 10, 11, 12):
        assert quot(*(good[:i] + [null] + good[i + 1:])) == E_INVALID
    for i, off in ((0, wit[8:]), (2, key[8:]), (12, t_out[8:])):
        assert quot(*(good[:i] + [_ptr(off)] + good[i + 1:])) == E_INVALID
        assert b"aligned" in L.ozk_last_error()
    for o_bad in (wit[(7 * n4 - 1) * E:], key[(14 * n4 - 1) * E:]):
        assert quot(*(good[:12] + [_ptr(o_bad)])) == E_INVALID
        assert b"overlap" in L.ozk_last_error()
    torch.cuda.synchronize()
    assert u.host(buf) == bytes([SENTINEL]) * buf.numel()


# ---------------------------------------------------------------------------- the protocol
@pytest.fixture(scope="module")
def string():
    from octopuszk_amd import kzg, srs
    s = srs.Srs.from_secrets(M, TAU, 1, 1, generator=1)
    return s, kzg.VerifyKey.from_srs(s)


def _model_string():
    _, (g2, tau_g2) = kr.string(1, TAU)
    return o.G1.to_affine(o.G1.one), g2, tau_g2


def _table(rng, rows):
    """random rows with one duplicate: the last is the first again"""
    table = [tuple(rng.randrange(R) for _ in range(3)) for _ in range(rows - 1)]
    return table + [table[0]]


def _package_circuit(model):
    from octopuszk_amd import plonk
    return plonk.LookupCircuit(model.n, model.selectors, model.wires, model.n_public, model.q_lookup, model.table)


@pytest.fixture(scope="module", params=[(8, 1, 5, 3), (1024, 3, 300, 400)], ids=["n8", "n1024"])
def proved(request, string):
    """one circuit with lookups set up and proved by the package and by the model"""
    from octopuszk_amd import kzg, plonk
    n, n_public, table_rows, lookups = request.param
    s, kvk = string
    rng = random.Random(3190 + n)
    model, assignment = lm.chain_with_lookups(n, n_public, rng, _table(rng, table_rows), lookups)
    pk, vk = plonk.setup(_package_circuit(model), kzg.CommitKey.from_srs(s, n))
    st = lm.setup(model, TAU)
    return {"model": model, "assignment": assignment, "pk": pk, "vk": vk, "kvk": kvk, "st": st,
            "proof": plonk.prove(pk, assignment), "want": lm.prove(model, assignment, TAU, st)}


def test_setup_and_proof_are_the_models(proved):
    from octopuszk_amd import plonk
    vk, proof, want = proved["vk"], proved["proof"], proved["want"]
    assert isinstance(vk, plonk.LookupVerifyingKey) and isinstance(proof, plonk.LookupProof)
    assert vk.to_bytes() == proved["st"]["vk"] and len(vk.to_bytes()) == plonk.LOOKUP_VK_BYTES == 392
    assert list(proof.commitments) == want["commitments"] and list(proof.values) == want["values"]
    assert proof.to_bytes() == want["bytes"] and len(proof.to_bytes()) == plonk.LOOKUP_PROOF_BYTES == 1088
    assert plonk.verify(vk, proved["kvk"], want["public"], proof)
    again = plonk.LookupProof.from_bytes(proof.to_bytes())
    assert plonk.verify(plonk.LookupVerifyingKey.from_bytes(vk.to_bytes()), proved["kvk"], want["public"], again)
    assert plonk.verify(vk, proved["kvk"], want["public"], proof.to_bytes())
    assert lm.verify_bytes(vk.to_bytes(), want["public"], proof.to_bytes(), *_model_string())


def test_the_stages_of_a_lookup_proof(proved):
    from octopuszk_amd import plonk
    timings = {}
    proof = plonk.prove(proved["pk"], wire_values=proved["model"].wire_values(proved["assignment"]), timings=timings)
    assert proof.to_bytes() == proved["want"]["bytes"]
    assert set(timings) == set(plonk.LOOKUP_STAGES) and {"lookup counts", "lookup sum"} <= set(timings)
    assert "lookup sum" not in plonk.protocol.STAGES


def test_a_wrong_public_input_is_refused(proved):
    from octopuszk_amd import plonk
    public = list(proved["want"]["public"])
    public[-1] = (public[-1] + 1) % R
    assert not plonk.verify(proved["vk"], proved["kvk"], public, proved["proof"])
    assert not plonk.verify(proved["vk"], proved["kvk"], public[:-1], proved["proof"])


@pytest.mark.parametrize("section", range(9 + 23 + 2))
def test_a_flipped_bit_is_refused(proved, section):
    from octopuszk_amd import plonk
    raw = bytearray(proved["proof"].to_bytes())
    raw[32 * section + 1] ^= 4
    assert not plonk.verify(proved["vk"], proved["kvk"], proved["want"]["public"], bytes(raw))


def test_a_proof_for_another_table_is_refused(proved, string):
    """the same gates and the same witness over a table with one more row"""
    from octopuszk_amd import plonk
    model = proved["model"]
    other = lm.LookupCircuit(model.n, model.selectors, model.wires, model.n_public, model.q_lookup,
                             model.table + [(1, 2, 3)])
    pk, vk = plonk.setup(_package_circuit(other), proved["pk"].commit_key)
    proof = plonk.prove(pk, proved["assignment"])
    public = proved["want"]["public"]
    assert plonk.verify(vk, proved["kvk"], public, proof)
    assert not plonk.verify(proved["vk"], proved["kvk"], public, proof)


def test_the_two_kinds_of_proof_do_not_mix(proved):
    from octopuszk_amd import plonk
    model, assignment, public = proved["model"], proved["assignment"], proved["want"]["public"]
    plain = plonk.Circuit(model.n, model.selectors, model.wires, model.n_public)
    pk, vk = plonk.setup(plain, proved["pk"].commit_key)
    vanilla = plonk.prove(pk, assignment)
    assert type(vk) is plonk.VerifyingKey and len(vanilla.to_bytes()) == 800 and plonk.verify(vk, proved["kvk"], public, vanilla)
    assert plonk.verify(vk, proved["kvk"], public, proved["proof"].to_bytes()) is False      # 1088 bytes, a vanilla key
    assert plonk.verify(vk, proved["kvk"], public, proved["proof"]) is False
    assert plonk.verify(proved["vk"], proved["kvk"], public, vanilla.to_bytes()) is False     # 800 bytes, a lookup key
    assert plonk.verify(proved["vk"], proved["kvk"], public, vanilla) is False


@pytest.mark.parametrize("tamper", ["tuple", "m", "S"])
def test_the_models_tampered_proofs_are_refused(proved, tamper):
    """each is an honest opening of its commitments: verify_multi passes, the identity does not"""
    from octopuszk_amd import kzg, plonk
    from octopuszk_amd.plonk import protocol
    vk, kvk = proved["vk"], proved["kvk"]
    bad = lm.prove(proved["model"], proved["assignment"], TAU, proved["st"], tamper=tamper)
    proof = plonk.LookupProof.from_bytes(bad["bytes"])
    assert not plonk.verify(vk, kvk, bad["public"], proof)
    cs = list(proof.commitments)
    ch = plonk.lookup_challenges(vk.to_bytes(), bad["public"], cs[:4], cs[4:6], cs[6:])
    assert ch == tuple(bad[k] for k in ("beta", "gamma", "eta", "theta", "alpha", "z"))
    assert not protocol.lookup_identity_holds(vk, bad["public"], proof.values, *ch)
    values = [[v] for v in proof.values[:19]] + [list(proof.values[19:21]), list(proof.values[21:])]
    mo = kzg.MultiOpening(cs[:4] + cs[6:] + list(vk.commitments) + cs[4:6], lm.sets_of(vk.n, ch[5]), values, proof.w,
                          proof.w2)
    assert kzg.verify_multi(kvk, mo)


def test_prove_names_the_row_that_is_not_in_the_table(proved):
    from octopuszk_amd import plonk
    pk, model, assignment = proved["pk"], proved["model"], proved["assignment"]
    rows = [i for i, sel in enumerate(model.q_lookup) if sel]
    at = rows[len(rows) // 2]
    bad = list(assignment)
    bad[model.wires[2][at]] = (bad[model.wires[2][at]] + 1) % R
    named = min(i for i in rows if model.wires[2][i] == model.wires[2][at])
    with pytest.raises(ValueError, match="row %d " % named):
        plonk.prove(pk, bad)
    wires = model.wire_values(assignment)
    wires[0][at] = (wires[0][at] + 1) % R
    with pytest.raises(ValueError, match="row %d " % at):
        plonk.prove(pk, wire_values=wires)
    # the assignment as 32-byte records, a looked-up one of them written as v + r
    records = [kr.le(v) for v in assignment]
    v = model.wires[1][at]
    records[v] = kr.le(assignment[v] + R)
    assert plonk.prove(pk, b"".join(records)).to_bytes() == proved["want"]["bytes"]


def test_a_builder_circuit_with_an_xor_table_proves_and_verifies(string):
    """the public interface from end to end: u xor v = w by one lookup each, a product gate between them; a wrong xor
    is named by its row"""
    from octopuszk_amd import kzg, plonk
    s, kvk = string
    b = plonk.Builder()
    x = b.public()
    u_, v_, w_, p_ = b.var(), b.var(), b.var(), b.var()
    b.table([(i, j, i ^ j) for i in range(4) for j in range(4)])
    b.lookup(u_, v_, w_)
    b.mul(x, w_, p_)
    b.lookup(w_, u_, v_)                                                  # w xor u = v as well
    circuit = b.build()
    assert circuit.n == 16 and circuit.n_table == 16 and circuit.q_lookup[:4] == [0, 1, 0, 1]
    pk, vk = plonk.setup(circuit, kzg.CommitKey.from_srs(s, 16))
    proof = plonk.prove(pk, [7, 2, 3, 1, 7])
    assert plonk.verify(vk, kvk, [7], proof) and not plonk.verify(vk, kvk, [8], proof)
    model = lm.LookupCircuit(16, circuit.selectors, circuit.wires, 1, circuit.q_lookup, circuit.table)
    assert proof.to_bytes() == lm.prove(model, [7, 2, 3, 1, 7], TAU)["bytes"]
    with pytest.raises(ValueError, match="row 1 "):
        plonk.prove(pk, [7, 2, 3, 2, 14])                                 # 2 xor 3 is not 2
    with pytest.raises(ValueError, match="gate"):
        plonk.prove(pk, [7, 2, 3, 1, 8])                                  # in the table, but 7 x 1 is not 8
