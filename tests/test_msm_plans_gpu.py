"""VariableBaseMSM at every window size and at every change of the window plan.

The cost model (msm_var_driver.cuh make_plan) picks the window size c from n, and c is not monotonic in n.  The plan
is pinned here: a scan of ozk_var_msm_plan over every n <= 2^18 must find exactly PLAN_CHANGES, so that a change to
the cost model shows up as a failure instead of silently moving which windows the suite exercises.  At every change
n - 1 and n run against the oracle (G1: the C oracle's Pippenger; G2: the discrete-log identity with bases k_i G2 from
the fixed-base path), as do 4096 / 4097 where the single-launch sort gives way to the two-level one.  Then every c in
1..16 is forced with OZK_MSM_C, under the default plan, OZK_MSM_SIGNED=0 and OZK_MSM_GLV=0, with scalars at the GLV
decomposition's edges (unreduced values up to 2^256 - 1 among them): k_digits / k_digits_glv, the top-window carry of
the signed digits and the bucket counts of every window size."""
import ctypes
import random

import numpy as np
import pytest

from oracle import bn254 as o
from oracle import coracle

pytestmark = pytest.mark.gpu

# (n, c below n, c from n on) for every n <= 2^18 where the default plan (GLV and signed digits on) changes c
PLAN_CHANGES = [(46, 4, 5), (123, 5, 6), (220, 6, 5), (278, 5, 8), (2612, 8, 10), (13492, 10, 12), (14080, 12, 13),
                (112640, 13, 16)]
SORT_SWITCH = 4097   # first n of the two-level sort

_LAM = 4407920970296243842393367215006156084916469457145843978461   # the G1 endomorphism's eigenvalue (glv.cuh)
_GLV_EDGE = [0, 1, 2, o.R - 1, o.R - 2, _LAM, _LAM - 1, _LAM + 1, o.R - _LAM, o.R - _LAM - 1,
             (1 << 127) - 1, 1 << 127, (1 << 127) + 1, 1 << 128, 1 << 253, o.R // 2, o.R // 3,
             9931322734385697763, 147946756881789319010696353538189108491,
             o.R, o.R + 1, (1 << 256) - 1, 5 * o.R + 7, (1 << 256) - o.R, (1 << 255) + 1]


def _plan(L, n):
    c, w = ctypes.c_int32(), ctypes.c_int32()
    from octopuszk_amd import lib
    lib.check(L.ozk_var_msm_plan(n, ctypes.byref(c), ctypes.byref(w)))
    return c.value, w.value


def test_window_plan_changes_where_pinned():
    from octopuszk_amd import lib
    L = lib.load()
    found, prev = [], None
    for n in range(1, (1 << 18) + 1):
        c, _ = _plan(L, n)
        if prev is not None and c != prev:
            found.append((n, prev, c))
        prev = c
    assert found == PLAN_CHANGES


def _sizes():
    return sorted({m for n, _, _ in PLAN_CHANGES for m in (n - 1, n)} | {SORT_SWITCH - 1, SORT_SWITCH})


def _expected_c(n):
    if n == SORT_SWITCH or n == SORT_SWITCH - 1:
        return None
    for m, before, after in PLAN_CHANGES:
        if n == m - 1:
            return before
        if n == m:
            return after
    return None


@pytest.mark.parametrize("n", _sizes())
def test_g1_at_every_plan_change_vs_oracle(n):
    import torch
    from octopuszk_amd import device as dev, lib
    L = lib.load()
    want_c = _expected_c(n)
    if want_c is not None:
        assert _plan(L, n)[0] == want_c, n
    bases = dev.gen_g1_bases(n, seed=1000 + n)
    rng = np.random.default_rng(n)
    sc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sc[:, 31] &= 0x1F
    sc[:8] = np.frombuffer(b"".join(int(s % o.R).to_bytes(32, "little") for s in _GLV_EDGE[:8]), dtype=np.uint8).reshape(8, 32)
    ws = dev.VarMsmWorkspace(n, 1)
    out = ws.run(bases, torch.from_numpy(sc.reshape(-1)).cuda())
    torch.cuda.synchronize()
    want = coracle.pippenger_g1(bytes(bases.cpu().numpy()), bytes(sc.reshape(-1)), n)
    assert bytes(out.cpu().numpy()) == want, (n, _plan(L, n))


@pytest.fixture(scope="module")
def g2_dlog():
    """n_max G2 bases k_i G2 (k_i < 2^64) from the fixed-base path, on the device, and the k_i"""
    import torch
    from octopuszk_amd import lib
    L = lib.load()
    n = max(_sizes())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(77)
    ks = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    ks[:, 8:] = 0
    base = torch.from_numpy(np.frombuffer(o.g2_to_wire(o.G2.one), dtype=np.uint8).copy()).cuda()
    out_be = torch.empty(n * 384, dtype=torch.uint8, device="cuda")
    wsb = int(L.ozk_fixed_batch_msm_workspace_bytes(4, 16, n, 2))
    wsf = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    lib.check(L.ozk_fixed_batch_msm_dev(4, 16, n, p(base), p(torch.from_numpy(ks.reshape(-1)).cuda()), 2, p(out_be),
                                        p(wsf), wsb, st))
    torch.cuda.synchronize()
    be = out_be.cpu().numpy().reshape(n, 6, 64)
    assert not be[:, :, :32].any()
    wire = np.ascontiguousarray(be[:, :, ::-1][:, :, :32]).reshape(n, -1).copy()
    return wire, [int.from_bytes(k.tobytes(), "little") for k in ks]


@pytest.mark.parametrize("n", _sizes())
def test_g2_at_every_plan_change_discrete_log_identity(n, g2_dlog):
    import torch
    from octopuszk_amd import device as dev, lib
    L = lib.load()
    want_c = _expected_c(n)
    if want_c is not None:
        assert _plan(L, n)[0] == want_c, n
    wire, ks = g2_dlog
    rng = np.random.default_rng(500 + n)
    sc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sc[:, 31] &= 0x1F
    ws = dev.VarMsmWorkspace(n, 2)
    out = ws.run(torch.from_numpy(wire[:n].reshape(-1).copy()).cuda(), torch.from_numpy(sc.reshape(-1)).cuda())
    torch.cuda.synchronize()
    acc = sum(int.from_bytes(sc[i].tobytes(), "little") * ks[i] for i in range(n)) % o.R
    assert bytes(out.cpu().numpy()) == o.g2_out_le(o.G2.to_affine(o.G2.mul(o.G2.one, acc))), (n, _plan(L, n))


def _rand_points(C, n, rng):
    return [C.to_affine(C.mul(C.one, rng.randrange(1, 1 << 64))) for _ in range(n)]


@pytest.mark.parametrize("mode", ["default", "signed0", "glv0"])
@pytest.mark.parametrize("type_", [1, 2])
def test_every_forced_window_size(type_, mode, monkeypatch):
    from octopuszk_amd import lib, variable_base_msm as vb
    L = lib.load()
    G = o.G1 if type_ == 1 else o.G2
    n = 300 if type_ == 1 else 64
    rng = random.Random(40 + type_)
    bases = _rand_points(G, n, rng)
    bases[3] = G.zero
    scalars = (_GLV_EDGE + [rng.randrange(1 << 256) for _ in range(n)])[:n]
    want = (o.g1_out_le if type_ == 1 else o.g2_out_le)(G.to_affine(o.pippenger_msm(G, [s % o.R for s in scalars], bases)))
    marshal = vb.marshal_g1 if type_ == 1 else vb.marshal_g2
    raw_bases = marshal(bases)
    raw_scalars = b"".join(int(s).to_bytes(32, "little") for s in scalars)
    c0 = _plan(L, n)
    env = {"signed0": {"OZK_MSM_SIGNED": "0"}, "glv0": {"OZK_MSM_GLV": "0"}}.get(mode, {})
    try:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for c in range(1, 17):
            monkeypatch.setenv("OZK_MSM_C", str(c))
            L.ozk_tuning_reload()
            assert _plan(L, n)[0] == c
            assert L.ozk_var_msm_glv(n) == (0 if mode == "glv0" else 1)
            got = vb.variable_base_serial_msm_native_helper(raw_bases, raw_scalars, n, type_, 0)
            assert got == want, (mode, c)
    finally:
        for k in list(env) + ["OZK_MSM_C"]:
            monkeypatch.delenv(k, raising=False)
        L.ozk_tuning_reload()
    assert _plan(L, n) == c0 and L.ozk_var_msm_glv(n) == 1
