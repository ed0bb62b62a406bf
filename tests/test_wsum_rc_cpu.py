"""The index arithmetic of the row / column window sums (octopuszk_amd/csrc/wsum_rc.h), compiled for the host with the
address and undefined-behaviour sanitizers and compared with a Python model: the row parts and the column parts each
partition the 2^cb buckets of a window, every partial slot is written once and read once, and with integer stand-ins
for the buckets  2^s sum_r r R_r + sum_q (q + 1) C_q  equals  sum_b (b + 1) B_b.

Geometries: the kernels' own (s = ceil(cb / 2), parts of 16) for cb = 1 .. 16 — below cb = 8 a row or a column is
shorter than one part — and ragged ones: parts of 5, 7 and 12 buckets, which divide no row length, and lopsided
splits (s = 0, s = cb, s = cb - 1)."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "wsum_rc_hostcheck.cpp")
BIN = os.path.join(HERE, "native", "_wsum_rc_hostcheck")
HDR = os.path.join(HERE, "..", "octopuszk_amd", "csrc", "wsum_rc.h")


@pytest.fixture(scope="module")
def prog():
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in (SRC, HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", BIN, SRC])
    return BIN


def _run(prog, cb, s, chunk):
    out = subprocess.run([prog, str(cb), str(s), str(chunk)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    rows = [l.split() for l in out.stdout.splitlines()]
    return {k: [[int(x) for x in r[1:]] for r in rows if r[0] == k] for k in "GRCD"}


CASES = [(cb, (cb + 1) // 2, 16) for cb in range(1, 17)]
CASES += [(cb, (cb + 1) // 2, ch) for cb in (3, 6, 9, 10, 13) for ch in (5, 7, 12)]
CASES += [(7, 0, 16), (7, 7, 16), (9, 8, 16), (10, 3, 7), (1, 0, 16), (1, 1, 1)]


@pytest.mark.parametrize("cb,s,chunk", CASES)
def test_parts_slots_and_the_weighted_identity(prog, cb, s, chunk):
    got = _run(prog, cb, s, chunk)
    NB = 1 << cb
    rows, cols, row_parts, col_parts, row_slots, col_slots, lanes, reduce_lanes = got["G"][0]
    assert (rows, cols) == (1 << (cb - s), 1 << s) and rows * cols == NB
    assert (row_parts, col_parts) == (-(-cols // chunk), -(-rows // chunk))
    assert (row_slots, col_slots, lanes, reduce_lanes) == (rows * row_parts, cols * col_parts, max(rows * row_parts, cols * col_parts), rows + cols)
    rng = np.random.default_rng(100 * cb + s)
    B = [int(x) for x in rng.integers(1, 1 << 40, size=NB)]          # integer stand-ins for the bucket sums

    # stage 1: every bucket is in exactly one row part and one column part, inside its own row / column
    row_slot, col_slot = {}, {}
    seen_r, seen_c = np.zeros(NB, dtype=np.int64), np.zeros(NB, dtype=np.int64)
    assert [r[0] for r in got["R"]] == list(range(row_slots)) and [c[0] for c in got["C"]] == list(range(col_slots))
    for t, first, n in got["R"]:
        assert 1 <= n <= chunk
        idx = [first + k for k in range(n)]
        assert idx[-1] < NB and len({b >> s for b in idx}) == 1
        seen_r[idx] += 1
        row_slot[t] = (idx[0] >> s, sum(B[b] for b in idx))
    for t, first, n, stride in got["C"]:
        assert 1 <= n <= chunk and stride == cols
        idx = [first + k * stride for k in range(n)]
        assert idx[-1] < NB and len({b & (cols - 1) for b in idx}) == 1
        seen_c[idx] += 1
        col_slot[t] = (idx[0] & (cols - 1), sum(B[b] for b in idx))
    assert (seen_r == 1).all() and (seen_c == 1).all()
    # lanes adjacent in t take adjacent columns (adjacent records in the column pass)
    assert all(col_slot[t][0] == t % cols for t in range(col_slots))

    # stage 2: every slot is read once, by the lane of its own row / column
    read_r, read_c = np.zeros(row_slots, dtype=np.int64), np.zeros(col_slots, dtype=np.int64)
    R, C = [0] * rows, [0] * cols
    assert [d[0] for d in got["D"]] == list(range(rows + cols))
    for u, col, first, stride, n in got["D"]:
        slots = [first + k * stride for k in range(n)]
        if col == 0:
            assert u < rows and slots[-1] < row_slots and all(row_slot[x][0] == u for x in slots)
            read_r[slots] += 1
            R[u] = sum(row_slot[x][1] for x in slots)
        else:
            assert col == 1 and u >= rows and slots[-1] < col_slots and all(col_slot[x][0] == u - rows for x in slots)
            read_c[slots] += 1
            C[u - rows] = sum(col_slot[x][1] for x in slots)
    assert (read_r == 1).all() and (read_c == 1).all()
    assert R == [sum(B[r * cols:(r + 1) * cols]) for r in range(rows)]
    assert C == [sum(B[q::cols]) for q in range(cols)]

    # the identity the tail rests on (signed digits: bucket b weighs b + 1; unsigned: b)
    for sd in (1, 0):
        want = sum((b + sd) * B[b] for b in range(NB))
        assert (1 << s) * sum(r * R[r] for r in range(rows)) + sum((q + sd) * C[q] for q in range(cols)) == want
