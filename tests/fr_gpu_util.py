"""Shared by the GPU tests of the Fr kernels: 32-byte little-endian Fr values between Python integers, host buffers
and device tensors; device buffers filled with a poison byte so that a guard tail shows a write past the end; tuning
knobs set for the length of a block; full-width words (x + k r, the edge words) and the conditions on rows made of
them; and the Fr row entry points of the KZG, PLONK and lookup blocks called on host integers."""
import contextlib
import ctypes

import numpy as np
import torch

from oracle import bn254 as o

R = o.R
POISON = 0xA5
GUARD = 32      # bytes behind every output that the call must leave alone


def host32(v):
    """a 32-byte LE host buffer; the caller keeps it alive until the stream has been synchronised"""
    return ctypes.create_string_buffer(int(v).to_bytes(32, "little"), 32)


def vp(buf):
    return ctypes.cast(buf, ctypes.c_void_p)


def poisoned(nbytes):
    return torch.full((nbytes,), POISON, dtype=torch.uint8, device="cuda")


def zeroed(nbytes):
    return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")


def dev_from_ints(values, guard=0):
    """n x 32 B LE on the device, followed by `guard` poison bytes"""
    raw = b"".join(int(v).to_bytes(32, "little") for v in values) + bytes([POISON]) * guard
    return torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()


def ints(t, n):
    """the first n 32-byte elements of a device tensor as Python integers"""
    raw = bytes(t[:32 * n].cpu().numpy())
    return [int.from_bytes(raw[k:k + 32], "little") for k in range(0, 32 * n, 32)]


def tail_untouched(t, used):
    """everything behind the first `used` bytes still holds the poison"""
    tail = bytes(t[used:].cpu().numpy())
    return len(tail) > 0 and tail == bytes([POISON]) * len(tail)


def host_bytes(t):
    torch.cuda.synchronize()
    return bytes(t.cpu().numpy())


def lib():
    from octopuszk_amd import lib as _lib
    return _lib.load()


def ptr(t):
    return ctypes.c_void_p(int(t.data_ptr()))


def stream():
    return ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))


def host_ints(values):
    """(the buffer, which the caller keeps alive; its address): 32-byte LE words in host memory"""
    buf = ctypes.create_string_buffer(b"".join(int(v).to_bytes(32, "little") for v in values), 32 * len(values))
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def workspace(nbytes):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")


def flat(rows, stride, fill=7):
    """rows laid out at `stride` elements, the gaps holding `fill`"""
    out = []
    for row in rows:
        out += list(row) + [fill] * (stride - len(row))
    return out


# ---- full-width words: every Fr entry point reduces a 256-bit word mod r on load -----------------------------
ALL_ONES = (1 << 256) - 1
EDGE_WORDS = [R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 3 * R, 4 * R, 5 * R, 1 << 255, (1 << 256) - R, ALL_ONES]


def wide(x, k):
    """x + k' r for the largest k' <= min(k, 5) that keeps the word below 2^256 (2^256 = 5.29 r)"""
    k = min(k, 5)
    while x + k * R > ALL_ONES:
        k -= 1
    return x + k * R


def wide_row(rng, length, phase=0):
    """`length` random elements written as wide(x, k), k cycling 0..5 by position"""
    return [wide(rng.randrange(R), (i + phase) % 6) for i in range(length)]


def wide_scalars(rng, count, phase=2):
    return [wide(rng.randrange(R), 2 + (i + phase) % 4) for i in range(count)]


def structure_positions(length, tile=1024, piece=4):
    """where a row's structure changes: the first and last element of a lane's piece (`piece` consecutive elements),
    of a tile, and of the row; at least len(EDGE_WORDS) places when the row has that many elements"""
    want = [0, piece - 1, piece, 2 * piece - 1, length - 1, length - piece]
    for t in range(tile, length + tile, tile):
        want += [t - piece, t - 1, t, t + piece - 1]
    at = sorted({p for p in want if 0 <= p < length})
    spare = (p for p in range(length) if p not in at)
    while len(at) < min(length, len(EDGE_WORDS)):
        at.append(next(spare))
    return sorted(at)


def with_edge_words(rng, length, shift=0, tile=1024, piece=4):
    """a row of wide(x, k) with k cycling 2..5 and the edge words at its structure positions, every edge word at least
    once when the row has len(EDGE_WORDS) elements; `shift` rotates which word lands where"""
    row = [wide(rng.randrange(R), 2 + i % 4) for i in range(length)]
    for n, p in enumerate(structure_positions(length, tile, piece)):
        row[p] = EDGE_WORDS[(n + shift) % len(EDGE_WORDS)]
    return row


def reduced(rows):
    """a list of words, or a list of rows of them, mod r: what the integer models are given"""
    return [reduced(v) if isinstance(v, (list, tuple)) else v % R for v in rows]


def assert_wide(rows, edges=False):
    """the conditions on rows written for the wide cases: every word fits 256 bits, at least half of every row's
    elements as written are >= 2 r, and (edges) every edge word occurs among all the rows' elements"""
    for row in rows:
        assert all(0 <= v <= ALL_ONES for v in row)
        assert 2 * sum(1 for v in row if v >= 2 * R) >= len(row), "fewer than half the elements are >= 2 r"
    if edges:
        seen = {v for row in rows for v in row}
        assert all(e in seen for e in EDGE_WORDS), "an edge word is missing"


def assert_has_edge_words(words):
    assert all(e in set(words) for e in EDGE_WORDS), "an edge word is missing"


def mismatches(got, want):
    """positions where two equally long lists differ (for the assertion message)"""
    assert len(got) == len(want)
    return [i for i, (x, y) in enumerate(zip(got, want)) if x != y]


@contextlib.contextmanager
def knobs_set(L, monkeypatch, knobs):
    """the environment knobs in force (ozk_tuning_reload) inside the block, gone again behind it"""
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    L.ozk_tuning_reload()
    try:
        yield
    finally:
        for k in knobs:
            monkeypatch.delenv(k)
        L.ozk_tuning_reload()


def knob_id(knobs):
    return "_".join("%s%s" % (a[4:], b) for a, b in knobs.items()) or "default"


# ---- the Fr row entry points on host integers --------------------------------------------------------------------
# Shared by the tests of each block (test_kzg_gpu.py, test_kzg_set_gpu.py, test_kzg_multi_gpu.py, test_plonk_gpu.py,
# test_plonk_lookup_gpu.py) and by test_fr_wide_inputs_gpu.py.  Inputs are written as given (any 256-bit word);
# outputs and the gaps between their rows start as POISON bytes.
POISON_INT = int.from_bytes(bytes([POISON]) * 32, "little")


def words(raw):
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def _split(t, count, stride, length):
    """(the `count` rows of `length` elements at `stride`, the elements of the gaps between them)"""
    got = words(host_bytes(t))
    rows = [got[y * stride:y * stride + length] for y in range(count)]
    gaps = [v for y in range(count) for v in got[y * stride + length:(y + 1) * stride]]
    return rows, gaps


def poly_open(coeffs, npolys, length, stride, points, quot_stride):
    """ozk_fr_poly_open_dev: coeffs a flat list laid out at `stride` -> (rows of the quotient, values, the elements of
    the gaps between quotient rows)"""
    L = lib()
    d_c, d_p = dev_from_ints(coeffs), dev_from_ints(points)
    quot, vals = poisoned(npolys * quot_stride * 32), poisoned(npolys * 32)
    wsb = L.ozk_fr_poly_open_workspace_bytes(npolys, length)
    assert wsb > 0
    ws = workspace(wsb)
    rc = L.ozk_fr_poly_open_dev(ptr(d_c), npolys, length, stride, ptr(d_p), ptr(quot), quot_stride, ptr(vals), ptr(ws), wsb,
                                stream())
    assert rc == 0, L.ozk_last_error()
    rows, gaps = _split(quot, npolys, quot_stride, length)
    return rows, words(host_bytes(vals)), gaps


def evals_open(evals, npolys, n, stride, omega, points, quot_stride, expect=0):
    """ozk_fr_evals_open_dev -> (rows of the quotient, values, the two output tensors)"""
    L = lib()
    d_f, d_p = dev_from_ints(evals), dev_from_ints(points)
    quot, vals = poisoned(npolys * quot_stride * 32), poisoned(npolys * 32)
    wsb = L.ozk_fr_evals_open_workspace_bytes(npolys, n)
    assert wsb > 0
    ws = workspace(wsb)
    keep, om = host_ints([omega])
    rc = L.ozk_fr_evals_open_dev(ptr(d_f), npolys, n, stride, om, ptr(d_p), ptr(quot), quot_stride, ptr(vals), ptr(ws), wsb,
                                 stream())
    assert rc == expect, L.ozk_last_error()
    return _split(quot, npolys, quot_stride, n)[0], words(host_bytes(vals)), quot, vals


def rows_combine(flat_rows, k, length, stride, weights):
    """ozk_fr_rows_combine_dev -> (the combination, the GUARD bytes behind it untouched)"""
    L = lib()
    d_r, d_w = dev_from_ints(flat_rows), dev_from_ints(weights)
    out = poisoned(length * 32 + GUARD)
    rc = L.ozk_fr_rows_combine_dev(ptr(d_r), k, length, stride, ptr(d_w), ptr(out), stream())
    assert rc == 0, L.ozk_last_error()
    return ints(out, length), tail_untouched(out, 32 * length)


def poly_open_set(coeffs, npolys, length, stride, t, points, quot_stride, expect=0):
    """ozk_fr_poly_open_set_dev: points npolys t of them (host memory) -> (rows of the quotient, values, the elements of
    the gaps between quotient rows, the two output tensors)"""
    L = lib()
    d_c = dev_from_ints(coeffs)
    keep, p_host = host_ints(points)
    quot, vals = poisoned(npolys * quot_stride * 32), poisoned(npolys * t * 32)
    wsb = L.ozk_fr_poly_open_set_workspace_bytes(npolys, length, t)
    assert wsb > 0
    ws = workspace(wsb)
    rc = L.ozk_fr_poly_open_set_dev(ptr(d_c), npolys, length, stride, t, p_host, ptr(quot), quot_stride, ptr(vals), ptr(ws),
                                    wsb, stream())
    assert rc == expect, L.ozk_last_error()
    rows, gaps = _split(quot, npolys, quot_stride, length)
    return rows, words(host_bytes(vals)), gaps, quot, vals


def evals_open_set(evals, npolys, n, stride, omega, t, points, quot_stride, expect=0):
    """ozk_fr_evals_open_set_dev -> (rows of the quotient, values, the two output tensors)"""
    L = lib()
    d_f = dev_from_ints(evals)
    keep, p_host = host_ints(points)
    quot, vals = poisoned(npolys * quot_stride * 32), poisoned(npolys * t * 32)
    wsb = L.ozk_fr_evals_open_set_workspace_bytes(npolys, n, t)
    assert wsb > 0
    ws = workspace(wsb)
    keep_om, om = host_ints([omega])
    rc = L.ozk_fr_evals_open_set_dev(ptr(d_f), npolys, n, stride, om, t, p_host, ptr(quot), quot_stride, ptr(vals), ptr(ws),
                                     wsb, stream())
    assert rc == expect, L.ozk_last_error()
    return _split(quot, npolys, quot_stride, n)[0], words(host_bytes(vals)), quot, vals


def poly_eval_set(flat_rows, npolys, length, stride, t, points):
    """ozk_fr_poly_eval_set_dev -> (the values, their bytes)"""
    L = lib()
    d_c = dev_from_ints(flat_rows)
    keep, p_host = host_ints(points)
    vals = poisoned(npolys * t * 32)
    wsb = L.ozk_fr_poly_eval_set_workspace_bytes(npolys, length, t)
    assert wsb > 0
    ws = workspace(wsb)
    rc = L.ozk_fr_poly_eval_set_dev(ptr(d_c), npolys, length, stride, t, p_host, ptr(vals), ptr(ws), wsb, stream())
    assert rc == 0, L.ozk_last_error()
    return words(host_bytes(vals)), host_bytes(vals)


def rows_coset(flat_rows, k, length, stride, s, c, out_len, out_stride, in_place=False):
    """ozk_fr_rows_coset_dev -> (the output rows, the elements of the gaps between them)"""
    L = lib()
    d_r = dev_from_ints(flat_rows)
    keep_s, p_s = host_ints([s])
    keep_c, p_c = host_ints([c])
    out = d_r if in_place else poisoned(k * out_stride * 32)
    wsb = L.ozk_fr_rows_coset_workspace_bytes(k, length, out_len)
    assert wsb > 0
    ws = workspace(wsb)
    rc = L.ozk_fr_rows_coset_dev(ptr(d_r), k, length, stride, p_s, p_c, ptr(out), out_len, out_stride, ptr(ws), wsb, stream())
    assert rc == 0, L.ozk_last_error()
    return _split(out, k, out_stride, out_len)


def _tail36(tail):
    """the element and the int32 count of a 64-byte tail; the 28 bytes behind them untouched"""
    t = host_bytes(tail)
    assert t[36:] == bytes([POISON]) * 28
    return int.from_bytes(t[:32], "little"), int.from_bytes(t[32:36], "little", signed=True)


def perm_product(wires, sigma, length, stride, omega, beta, gamma, ks=None):
    """ozk_fr_perm_product_dev -> (z, the elements behind it, the total, the count); ks: plonk_ref.KS unless given"""
    import plonk_ref
    L = lib()
    d_w, d_s = dev_from_ints(flat(wires, stride)), dev_from_ints(flat(sigma, stride))
    keep = [host_ints(v) for v in ([omega], list(plonk_ref.KS if ks is None else ks), [beta], [gamma])]
    z, tail = poisoned((length + 2) * 32), poisoned(64)
    wsb = L.ozk_fr_perm_product_workspace_bytes(length)
    assert wsb > 0
    ws = workspace(wsb)
    rc = L.ozk_fr_perm_product_dev(ptr(d_w), ptr(d_s), length, stride, keep[0][1], keep[1][1], keep[2][1], keep[3][1],
                                   ptr(z), ptr(tail), ptr(tail[32:]), ptr(ws), wsb, stream())
    assert rc == 0, L.ozk_last_error()
    got = words(host_bytes(z))
    return (got[:length], got[length:]) + _tail36(tail)


def plonk_quotient(wit, key, n, challenges, wit_stride, key_stride, ks=None, zh_inv=None):
    """ozk_plonk_quotient_dev for the challenges (alpha, beta, gamma), ozk_plonk_quotient_lookup_dev for (alpha, beta,
    gamma, eta, theta) -> the 4 n values; ks and zh_inv: plonk_ref's unless given"""
    import plonk_ref
    L = lib()
    d_w, d_k = dev_from_ints(flat(wit, wit_stride)), dev_from_ints(flat(key, key_stride))
    scalars = [[c] for c in challenges[:3]] + [list(plonk_ref.KS if ks is None else ks),
                                               list(plonk_ref.zh_inverses(n) if zh_inv is None else zh_inv)]
    keep = [host_ints(v) for v in scalars + [[c] for c in challenges[3:]]]
    out = poisoned((4 * n + 2) * 32)
    entry = L.ozk_plonk_quotient_dev if len(challenges) == 3 else L.ozk_plonk_quotient_lookup_dev
    rc = entry(ptr(d_w), wit_stride, ptr(d_k), key_stride, n, *[k[1] for k in keep], ptr(out), stream())
    assert rc == 0, L.ozk_last_error()
    got = words(host_bytes(out))
    assert got[4 * n:] == [POISON_INT] * 2
    return got[:4 * n]


def lookup_index(d_table, n_rows, table_stride):
    L = lib()
    nbytes = L.ozk_plonk_lookup_index_bytes(n_rows)
    cap = nbytes // 4
    assert cap >= 2 * n_rows and cap & (cap - 1) == 0 and (cap < 4 * n_rows or cap == 2)
    index = poisoned(nbytes + 32)
    rc = L.ozk_plonk_lookup_index_dev(ptr(d_table), n_rows, table_stride, ptr(index), nbytes, stream())
    assert rc == 0, L.ozk_last_error()
    return index, nbytes


def lookup_counts(wires, qk, table, m_len, stride=None, table_stride=None):
    """ozk_plonk_lookup_index_dev and ozk_plonk_lookup_counts_dev; table: n_rows tuples -> (m, the elements behind it,
    missing, first_missing, the index's slots)"""
    L = lib()
    length, n_rows = len(qk), len(table)
    stride, table_stride = stride or length, table_stride or n_rows
    d_w, d_q = dev_from_ints(flat(wires, stride)), dev_from_ints(qk)
    d_t = dev_from_ints(flat([[row[j] for row in table] for j in range(3)], table_stride))
    index, nbytes = lookup_index(d_t, n_rows, table_stride)
    m, tail = poisoned((m_len + 2) * 32), poisoned(16)
    rc = L.ozk_plonk_lookup_counts_dev(ptr(d_w), ptr(d_q), length, stride, ptr(d_t), n_rows, table_stride, ptr(index),
                                       nbytes, ptr(m), m_len, ptr(tail), ptr(tail[4:]), stream())
    assert rc == 0, L.ozk_last_error()
    got, t, slots = words(host_bytes(m)), host_bytes(tail), host_bytes(index)
    assert t[8:] == bytes([POISON]) * 8 and slots[nbytes:] == bytes([POISON]) * 32
    slots = [int.from_bytes(slots[i:i + 4], "little") for i in range(0, nbytes, 4)]
    return (got[:m_len], got[m_len:], int.from_bytes(t[:4], "little", signed=True),
            int.from_bytes(t[4:8], "little", signed=True), slots)


def lookup_sum(wires, key4, m, length, stride, key_stride, eta, theta):
    """ozk_plonk_lookup_sum_dev -> (S, the elements behind it, the total, the count)"""
    L = lib()
    d_w, d_k, d_m = dev_from_ints(flat(wires, stride)), dev_from_ints(flat(key4, key_stride)), dev_from_ints(m)
    keep = [host_ints([eta]), host_ints([theta])]
    s, tail = poisoned((length + 2) * 32), poisoned(64)
    wsb = L.ozk_plonk_lookup_sum_workspace_bytes(length)
    assert wsb > 0
    ws = workspace(wsb)
    rc = L.ozk_plonk_lookup_sum_dev(ptr(d_w), stride, ptr(d_k), key_stride, ptr(d_m), length, keep[0][1], keep[1][1], ptr(s),
                                    ptr(tail), ptr(tail[32:]), ptr(ws), wsb, stream())
    assert rc == 0, L.ozk_last_error()
    got = words(host_bytes(s))
    return (got[:length], got[length:]) + _tail36(tail)
