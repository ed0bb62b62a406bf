"""The variable-base MSM's plan and buffer layout, pinned: tests/golden/msm_layout_sizes.json was recorded with
tools/dump_msm_layout.py at the commit before the plan got one home (plan_for, msm_var_driver.cuh), and the library
must report every row of it exactly — window bits, windows, GLV, the three stage regions, the tail, the prepared
records and both workspaces, for both point types, at every size where the plan changes and under every kept knob
that shapes it.  The size queries need no device."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _tool():
    spec = importlib.util.spec_from_file_location("dump_msm_layout", os.path.join(ROOT, "tools", "dump_msm_layout.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tables():
    from octopuszk_amd import lib
    with open(os.path.join(HERE, "golden", "msm_layout_sizes.json")) as f:
        want = json.load(f)
    return want, _tool().layout_rows(lib.load())


def test_golden_table_covers_the_cases(tables):
    want, _ = tables
    tool = _tool()
    for t in tool.TYPES:
        assert [r["n"] for r in want if r["type"] == t and r["knob"] == ""] == tool.SIZES
        for name, val in tool.KNOBS:
            assert [r["n"] for r in want if r["type"] == t and r["knob"] == "%s=%s" % (name, val)] == tool.KNOB_SIZES
    assert {1 << 23, (1 << 23) + 1, 1 << 24, 4096, 4097} <= set(tool.SIZES)


def test_every_row_is_reproduced_exactly(tables):
    want, got = tables
    assert len(got) == len(want)
    diff = [(w, g) for w, g in zip(want, got) if w != g]
    assert not diff, "first of %d differing rows: golden %r, library %r" % (len(diff), diff[0][0], diff[0][1])
