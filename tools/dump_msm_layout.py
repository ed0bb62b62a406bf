#!/usr/bin/env python3
"""The variable-base MSM's plan and buffer sizes as the library reports them, for a fixed list of sizes and knob
settings: what tests/test_msm_layout_cpu.py pins against tests/golden/msm_layout_sizes.json.  No device is needed
(the size queries fall back to 256 compute units, the MI355X's count).

    python tools/dump_msm_layout.py > tests/golden/msm_layout_sizes.json     # at the commit whose layout is the yardstick
"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

# the pinned plan changes of tests/test_msm_plans_gpu.py, the sort switch, the GLV limit and the maximum
SIZES = [1, 45, 46, 277, 278, 2611, 2612, 4096, 4097, 13491, 13492, 14079, 14080, 112639, 112640, 1 << 17, 1 << 18,
         1 << 20, 1 << 21, 1 << 22, 1 << 23, (1 << 23) + 1, 1 << 24]
KNOB_SIZES = [278, 4097, 1 << 16, 1 << 20]
KNOBS = [("OZK_MSM_GLV", "0"), ("OZK_MSM_SIGNED", "0"), ("OZK_MSM_C", "7"), ("OZK_MSM_L1", "16"),
         ("OZK_MSM_L1_ROUNDS", "0")]
TYPES = [1, 2]   # OZK_G1, OZK_G2


def _row(L, n, t):
    c, w = ctypes.c_int32(), ctypes.c_int32()
    assert L.ozk_var_msm_plan(n, ctypes.byref(c), ctypes.byref(w)) == 0
    st = [ctypes.c_size_t() for _ in range(3)]
    assert L.ozk_var_msm_stage_bytes(n, t, *[ctypes.byref(x) for x in st]) == 0
    return {"n": n, "type": t, "c": c.value, "W": w.value, "glv": L.ozk_var_msm_glv(n),
            "stage": [x.value for x in st],
            "tail": L.ozk_var_msm_tail_bytes(n, t), "prepared": L.ozk_var_msm_prepared_bytes(n, t),
            "head_ws": L.ozk_var_msm_head_workspace_bytes(n, t), "ws": L.ozk_var_msm_workspace_bytes(n, t)}


def layout_rows(L):
    """every row of the table, each with the knob setting ("" for the defaults) it was taken under"""
    rows = []
    for t in TYPES:
        for n in SIZES:
            rows.append(dict(_row(L, n, t), knob=""))
    for name, val in KNOBS:
        assert name not in os.environ, "%s is set in the caller's environment" % name
        os.environ[name] = val
        L.ozk_tuning_reload()
        try:
            for t in TYPES:
                for n in KNOB_SIZES:
                    rows.append(dict(_row(L, n, t), knob="%s=%s" % (name, val)))
        finally:
            del os.environ[name]
            L.ozk_tuning_reload()
    return rows


if __name__ == "__main__":
    from octopuszk_amd import lib
    rows = layout_rows(lib.load())
    print("[\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]")
