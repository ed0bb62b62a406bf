#!/usr/bin/env python3
"""The workspace sizes of the FFT, witness-map, QAP-instance, constraint-evaluation and BACE entry points as the
library reports them, for a fixed list of shapes: what tests/test_fft_layout_cpu.py pins against
tests/golden/fft_layout_sizes.json.  No device is needed.

    python tools/dump_fft_layout.py > tests/golden/fft_layout_sizes.json     # at the commit whose layout is the yardstick
"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

# every power of two the entry points accept, and sizes both transforms refuse (0 bytes)
DOMAINS = [1 << k for k in range(29)] + [0, -4, 3, 4097, 2050, (1 << 28) + 1]
# powers-up-to-n tables: around the first-level length (2048), a second-level step (4096), and the maximum
POWERS = [1, 2, 2047, 2048, 2049, 4096, 4097, 1 << 20, 1 << 28, (1 << 28) + 1]
LONG_ROWS = [0, 1, 7]
# (n, N, D, n_ops, n_slots, n_consts): the shapes of tests/test_bace_gpu.py (programs of a few records, and one of
# 2000 records whose slots spill past the LDS cap), the evaluators' layouts (D = N, no program), and D = 1, 2, 4096, 8192
BACE = [(4, 2, 8, 9, 5, 0), (1, 16, 16, 3, 3, 1), (2, 1, 2, 4, 4, 0), (1, 8, 256, 6, 2, 0), (2, 4, 16, 5, 5, 0),
        (8, 64, 256, 2000, 40, 100), (2, 1024, 2048, 4, 4, 0), (1, 256, 2048, 3, 2, 0), (2, 2048, 4096, 4, 4, 0),
        (1, 512, 4096, 3, 2, 0), (3, 4096, 8192, 40, 12, 0), (6, 32, 128, 2000, 40, 100), (5, 64, 256, 300, 20, 15),
        (3, 16, 32, 5, 5, 0), (4, 128, 512, 500, 30, 25), (4, 1 << 16, 1 << 18, 200, 17, 10), (6, 256, 1024, 400, 29, 20),
        (3, 16, 16, 0, 0, 0), (1, 16, 16, 0, 0, 0), (4, 1 << 16, 1 << 16, 0, 0, 0),
        (1, 1, 1, 1, 1, 0), (2, 2, 2, 1, 1, 0), (1, 4096, 4096, 1, 1, 0), (1, 8192, 8192, 1, 1, 0),
        (4, 3, 8, 1, 1, 0), (4, 8, 4, 1, 1, 0)]
# (rows, n_ops, n_slots, n_consts)
BACE_EVAL = [(1, 1, 1, 0), (32, 2000, 40, 100), (128, 500, 30, 25), (1 << 16, 200, 17, 10), (65537, 200, 17, 10),
             (1 << 28, 3, 2, 0), (0, 1, 1, 0)]


def layout_rows(L):
    """every row of the table: {"fn": entry point, "args": its arguments, "bytes": what it returns}"""
    rows = []

    def add(fn, *args):
        rows.append({"fn": fn, "args": list(args), "bytes": int(getattr(L, fn)(*args))})

    for n in DOMAINS:
        add("ozk_fft_workspace_bytes", n)
        add("ozk_qap_witness_workspace_bytes", n)
    for n in POWERS:
        add("ozk_qap_lagrange_workspace_bytes", n)
        add("ozk_fr_powers_workspace_bytes", n)
    for n in LONG_ROWS:
        add("ozk_r1cs_evaluate_workspace_bytes", n)
    for shape in BACE:
        add("ozk_bace_workspace_bytes", *shape)
    for shape in BACE_EVAL:
        add("ozk_bace_evaluate_workspace_bytes", *shape)
    return rows


if __name__ == "__main__":
    from octopuszk_amd import lib
    assert "OZK_BACE_LDS_SLOTS" not in os.environ, "OZK_BACE_LDS_SLOTS is set in the caller's environment"
    print("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in layout_rows(lib.load())) + "\n]")
