"""k_runmerge (msm_var.cuh) at the run shapes of the 2^20 workload, in miniature.

The run merge sums the pieces that level 1 leaves of every bucket cut by a lane boundary: in rounds, one addition per
run and round, over a work list in LDS; the partial sum of a run waits in its bucket record between rounds.  At
n = 2^12 with OZK_MSM_C=8 (signed: 128 buckets x 16 windows, ~64 entries per bucket, as at 2^20) the level-1 chunk
length OZK_MSM_L1 sets the shapes: 52 gives the workload's own (two- and three-piece runs, one left-over round), 8 gives
runs of 14-24 slots (many rounds, both sides of RUN_MAX, survivors for the generic levels), 4 only runs longer than
RUN_MAX (nothing merged).  Bases are k_i G with known k_i (gen_g1_bases / gen_base_logs), so the expected point is
(sum s_i k_i) G from exact integers and the oracle's group law; G2 the same with bases from the fixed-base path."""
import ctypes

import numpy as np
import pytest

from oracle import bn254 as o

pytestmark = pytest.mark.gpu

N = 1 << 12
N_RAGGED = N + 77
SEED = 31


@pytest.fixture(scope="module")
def g1():
    """bases k_i G (wire, on the device) and the k_i, for the largest n used here"""
    from octopuszk_amd import device as dev
    return dev.gen_g1_bases(N_RAGGED, SEED), dev.gen_base_logs(N_RAGGED, SEED)


_CASES = {}


def _uniform_case(l1, ks):
    """uniform scalars and the expected point of cases 1-3 (and 8), computed once"""
    if l1 not in _CASES:
        sc = _uniform(N, 100 + l1)
        _CASES[l1] = sc, _g1_point(sum(s * k for s, k in zip(_ints(sc), ks)))
    return _CASES[l1]


def _uniform(n, seed):
    rng = np.random.default_rng(seed)
    sc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sc[:, 31] &= 0x1F
    return sc


def _ints(sc):
    return [int.from_bytes(row.tobytes(), "little") for row in sc]


def _g1_point(acc):
    return o.g1_out_le(o.G1.to_affine(o.G1.mul(o.G1.one, acc % o.R)))


def _assert_eq(got, want):
    assert got == want


def _with_plan(monkeypatch, l1, body):
    from octopuszk_amd import lib
    L = lib.load()
    try:
        monkeypatch.setenv("OZK_MSM_C", "8")
        monkeypatch.setenv("OZK_MSM_L1", str(l1))
        L.ozk_tuning_reload()
        body()
    finally:
        monkeypatch.delenv("OZK_MSM_C", raising=False)
        monkeypatch.delenv("OZK_MSM_L1", raising=False)
        L.ozk_tuning_reload()


def _run_g1(d_bases, sc, n, poison=None):
    import torch
    from octopuszk_amd import device as dev
    ws = dev.VarMsmWorkspace(n, 1)
    if poison is not None:
        ws.ws.fill_(poison)
    out = ws.run(d_bases[:n * 96], torch.from_numpy(np.ascontiguousarray(sc).reshape(-1)).cuda())
    torch.cuda.synchronize()
    return bytes(out.cpu().numpy())


@pytest.mark.parametrize("l1", [52, 8, 4])
def test_workload_shapes(l1, g1, monkeypatch):
    """cases 1-3: the workload's two- and three-piece runs; runs around RUN_MAX with survivors; nothing to merge"""
    d_bases, ks = g1
    sc, want = _uniform_case(l1, ks)
    _with_plan(monkeypatch, l1, lambda: _assert_eq(_run_g1(d_bases, sc, N), want))


def test_ragged_size(g1, monkeypatch):
    """case 4: n = 2^12 + 77, a partial last block and chunk"""
    d_bases, ks = g1
    sc = _uniform(N_RAGGED, 7)
    want = _g1_point(sum(s * k for s, k in zip(_ints(sc), ks)))
    _with_plan(monkeypatch, 52, lambda: _assert_eq(_run_g1(d_bases, sc, N_RAGGED), want))


def test_skew_beside_short_runs(g1, monkeypatch):
    """case 5: half the scalars equal — one run of ~160 slots per window among two-piece runs in the same blocks"""
    d_bases, ks = g1
    sc = _uniform(N, 8)
    c = 0x1234567890abcdef1234567890abcdef1234567890abcdef1234567890abcd % o.R
    sc[::2] = np.frombuffer(c.to_bytes(32, "little"), dtype=np.uint8)
    want = _g1_point(sum(s * k for s, k in zip(_ints(sc), ks)))
    _with_plan(monkeypatch, 52, lambda: _assert_eq(_run_g1(d_bases, sc, N), want))


@pytest.mark.parametrize("arrangement", ["same_point", "plus_minus"])
def test_group_law_corners_inside_the_merge(arrangement, g1, monkeypatch):
    """case 6, chunks of two entries: every base is the same point P and groups of four pairs share a scalar, so a
    bucket's pieces are 2P and 2P (the doubling branch of xyzz_add); with bases P, -P alternating a piece is P + (-P),
    the point at infinity, and every bucket sums to infinity."""
    import torch
    d_bases, ks = g1
    n = 320
    rec = d_bases[:96].cpu().numpy().copy()
    recs = np.tile(rec, (n, 1))
    signs = [1] * n
    if arrangement == "plus_minus":
        y = int.from_bytes(rec[32:64].tobytes(), "little")
        neg = rec.copy()
        neg[32:64] = np.frombuffer((o.Q - y).to_bytes(32, "little"), dtype=np.uint8)
        recs[1::2] = neg
        signs = [1, -1] * (n // 2)
    group = _uniform(n // 4, 9)
    sc = np.repeat(group, 4, axis=0)
    want = _g1_point(sum(sg * s * ks[0] for sg, s in zip(signs, _ints(sc))))
    if arrangement == "plus_minus":
        assert want == o.g1_out_le(o.G1.zero_affine)
    bases = torch.from_numpy(recs.reshape(-1)).cuda()
    _with_plan(monkeypatch, 2, lambda: _assert_eq(_run_g1(bases, sc, n), want))


def test_g2_workload_shape(monkeypatch):
    """case 7: G2 at the geometry of case 1 (n = 2^11), bases k_i G2 with k_i < 2^64 from the fixed-base path"""
    import torch
    from octopuszk_amd import device as dev, lib
    L = lib.load()
    n = 1 << 11
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ks = np.random.default_rng(78).integers(0, 256, size=(n, 32), dtype=np.uint8)
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
    wire = np.ascontiguousarray(be[:, :, ::-1][:, :, :32]).reshape(-1).copy()
    sc = _uniform(n, 10)
    acc = sum(s * k for s, k in zip(_ints(sc), _ints(ks))) % o.R
    want = o.g2_out_le(o.G2.to_affine(o.G2.mul(o.G2.one, acc)))

    def body():
        ws = dev.VarMsmWorkspace(n, 2)
        out = ws.run(torch.from_numpy(wire).cuda(), torch.from_numpy(sc.reshape(-1)).cuda())
        torch.cuda.synchronize()
        assert bytes(out.cpu().numpy()) == want

    _with_plan(monkeypatch, 52, body)


@pytest.mark.parametrize("poison", [0xFF, 0x00])
@pytest.mark.parametrize("l1", [52, 8])
def test_over_a_poisoned_workspace(l1, poison, g1, monkeypatch):
    """case 8: a read of a stale intermediate record (a bucket slot or a list entry not written this run) shows"""
    d_bases, ks = g1
    sc, want = _uniform_case(l1, ks)
    _with_plan(monkeypatch, l1, lambda: _assert_eq(_run_g1(d_bases, sc, N, poison), want))
