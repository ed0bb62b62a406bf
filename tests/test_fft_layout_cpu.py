"""The workspace sizes of the FFT, the witness map, the QAP instance's vector entries, constraint evaluation and BACE,
pinned: tests/golden/fft_layout_sizes.json was recorded with tools/dump_fft_layout.py at the commit before the domain
tables got one carving function (DomainTables, csrc/fr_tables.cuh), and the library must report every row of it
exactly — every power of two up to 2^28 for the two transforms, the sizes around the power table's first level, and
the BACE shapes of tests/test_bace_gpu.py.  The size queries need no device.  (Positions INSIDE a workspace are
checked on the GPU: test_fft_tables_gpu.py::test_workspace_shows_which_path_built_the_tables.)"""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _tool():
    spec = importlib.util.spec_from_file_location("dump_fft_layout", os.path.join(ROOT, "tools", "dump_fft_layout.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tables():
    from octopuszk_amd import lib
    with open(os.path.join(HERE, "golden", "fft_layout_sizes.json")) as f:
        want = json.load(f)
    return want, _tool().layout_rows(lib.load())


def _args(want, fn):
    return [tuple(r["args"]) for r in want if r["fn"] == fn]


def test_golden_table_covers_the_cases(tables):
    want, _ = tables
    tool = _tool()
    for fn in ("ozk_fft_workspace_bytes", "ozk_qap_witness_workspace_bytes"):
        assert _args(want, fn) == [(n,) for n in tool.DOMAINS]
        assert {(1 << k,) for k in range(29)} | {(3,), (4097,)} <= set(_args(want, fn))
    for fn in ("ozk_qap_lagrange_workspace_bytes", "ozk_fr_powers_workspace_bytes"):
        assert _args(want, fn) == [(n,) for n in tool.POWERS]
        assert {(1,), (2,), (2047,), (2048,), (2049,), (4096,), (4097,), (1 << 20,), (1 << 28,)} <= set(_args(want, fn))
    assert _args(want, "ozk_r1cs_evaluate_workspace_bytes") == [(0,), (1,), (7,)]
    assert _args(want, "ozk_bace_workspace_bytes") == tool.BACE
    assert {1, 2, 4096, 8192} <= {a[2] for a in tool.BACE}
    assert _args(want, "ozk_bace_evaluate_workspace_bytes") == tool.BACE_EVAL


def test_refused_sizes_are_zero(tables):
    want, _ = tables
    by = {(r["fn"], tuple(r["args"])): r["bytes"] for r in want}
    for n in (0, -4, 3, 4097, (1 << 28) + 1):
        assert by[("ozk_fft_workspace_bytes", (n,))] == 0
        assert by[("ozk_qap_witness_workspace_bytes", (n,))] == 0
    assert by[("ozk_qap_witness_workspace_bytes", (1,))] == 0 and by[("ozk_fft_workspace_bytes", (1,))] > 0
    assert by[("ozk_bace_workspace_bytes", (4, 3, 8, 1, 1, 0))] == 0
    assert by[("ozk_bace_workspace_bytes", (4, 8, 4, 1, 1, 0))] == 0


def test_every_row_is_reproduced_exactly(tables):
    want, got = tables
    assert len(got) == len(want)
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, "first of %d differing rows: golden %r, library %r" % (len(diff), diff[0][0], diff[0][1])
