"""The shared-base batched MSM on hardware (ozk_multi_msm_*, device.SharedBaseMsm): all 192 bytes of every output
against two references that are already trusted — oracle.bn254's naive MSM for small shapes and one
ozk_var_msm_dev call per row (bit-exact with the oracle since the first round) for the larger ones."""
import ctypes
import random

import numpy as np
import pytest
import torch

import multi_msm_ref as ref
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

INF_RECORD = bytes(64) + (1).to_bytes(64, "little") + bytes(64)
EDGES_VAR_ONLY = [o.R, (1 << 254) - 1, (1 << 256) - 1]      # not canonical: compared with ozk_var_msm_dev only


def _dev(b):
    return torch.from_numpy(np.frombuffer(bytes(b), dtype=np.uint8).copy()).cuda()


def _random_bases(n, seed):
    """n random multiples of the generator, affine: a doubling-and-adding walk from a random start (the walk's
    discrete logs are as unknown to the MSM as independent draws, and 4096 of them take a second on the host)"""
    rng = random.Random(seed)
    p = o.G1.mul(o.G1.one, rng.randrange(1, o.R))
    q = o.G1.mul(o.G1.one, rng.randrange(1, o.R))
    out = []
    for _ in range(n):
        out.append(o.G1.to_affine(p))
        p = o.G1.add(o.G1.twice(p), q)
    return out


def _wire(bases):
    return b"".join(o.g1_to_wire(tuple(c % o.Q for c in P)) for P in bases)


def _random_rows(k, n, seed):
    """k x n canonical scalars as a uint8 array [k, n, 32]: uniform below 0x30 << 248 (< r)"""
    a = np.random.default_rng(seed).integers(0, 256, size=(k, n, 32), dtype=np.uint8)
    a[:, :, 31] %= 0x30
    return a


def _put(rows, i, j, s):
    rows[i, j, :] = np.frombuffer(int(s).to_bytes(32, "little"), dtype=np.uint8)


def _place_edges(rows, edges):
    """the edge scalars in the first / last column and the first / last row, cycling"""
    k, n = rows.shape[:2]
    for t, s in enumerate(edges):
        _put(rows, t % k, 0, s)
        _put(rows, (t * 7 + 1) % k, n - 1, s)
        _put(rows, 0, t % n, s)
        _put(rows, k - 1, (t * 5 + 2) % n, s)


def _var_reference(d_bases, n, rows, which=None):
    """one ozk_var_msm_dev call per row (of the rows listed in `which`): {row: 192 bytes}"""
    from octopuszk_amd.device import VarMsmWorkspace
    w = VarMsmWorkspace(n, 1)
    out = {}
    for i in (range(rows.shape[0]) if which is None else which):
        d_s = torch.from_numpy(np.ascontiguousarray(rows[i]).reshape(-1)).cuda()
        out[i] = bytes(w.run(d_bases, d_s).cpu().numpy())
    return out


def _oracle_reference(bases, rows):
    out = {}
    for i in range(rows.shape[0]):
        sc = [int.from_bytes(bytes(rows[i, j]), "little") % o.R for j in range(rows.shape[1])]
        out[i] = o.g1_out_le(o.G1.to_affine(o.naive_msm(o.G1, sc, bases)))
    return out


def _run(msm, rows):
    k = rows.shape[0]
    d_s = torch.from_numpy(np.ascontiguousarray(rows).reshape(-1)).cuda()
    raw = bytes(msm.run(d_s, k).cpu().numpy())
    assert len(raw) == 192 * k
    return [raw[192 * i:192 * (i + 1)] for i in range(k)]


def _assert_rows(got, want, what):
    for i, w in want.items():
        assert got[i] == w, "%s: output %d differs" % (what, i)


SHAPES = [(1, 1), (1, 2), (2, 63), (2, 64), (3, 65), (3, 1000), (15, 64), (15, 1000), (16, 1), (16, 65), (63, 2),
          (63, 63), (1023, 64), (1023, 65), (1024, 1), (1024, 2), (4096, 1), (4096, 63)]


@pytest.mark.parametrize("n,k", SHAPES)
def test_shapes_against_var_msm(n, k):
    from octopuszk_amd.device import SharedBaseMsm
    bases = _random_bases(n, 100 + n)
    d_bases = _dev(_wire(bases))
    rows = _random_rows(k, n, 1000 * n + k)
    _place_edges(rows, ref.edge_scalars() + EDGES_VAR_ONLY)
    msm = SharedBaseMsm(d_bases, n)
    got = _run(msm, rows)
    _assert_rows(got, _var_reference(d_bases, n, rows), "n=%d k=%d vs ozk_var_msm_dev" % (n, k))
    if n <= 3 and k <= 65:
        _assert_rows(got, _oracle_reference(bases, rows), "n=%d k=%d vs oracle" % (n, k))


def test_plan_matches_model():
    from octopuszk_amd import lib as _lib
    L = _lib.load()
    for n in (1, 15, 1023, 1280, 1281, 2156, 3724, 4096):
        wb, oc = ctypes.c_int32(), ctypes.c_int32()
        assert L.ozk_multi_msm_plan(n, ctypes.byref(wb), ctypes.byref(oc)) == 0
        assert (wb.value, oc.value) == (ref.window_bits(n), ref.windows(ref.window_bits(n)))
        assert L.ozk_multi_msm_table_bytes(n, 1) == n * ref.records_per_base(wb.value) * 64


def test_profiler_shape_sampled_and_repeatable():
    """n = 1023, K = 4096: 64 sampled outputs against ozk_var_msm_dev, all outputs against a second run"""
    from octopuszk_amd.device import SharedBaseMsm
    n, k = 1023, 4096
    d_bases = _dev(_wire(_random_bases(n, 77)))
    rows = _random_rows(k, n, 4242)
    _place_edges(rows, ref.edge_scalars())
    msm = SharedBaseMsm(d_bases, n)
    got = _run(msm, rows)
    sample = sorted(set([0, 1, k - 1] + random.Random(1).sample(range(k), 61)))
    _assert_rows(got, _var_reference(d_bases, n, rows, sample), "n=1023 k=4096 sample")
    assert _run(msm, rows) == got


def _special_base_sets(n):
    P = _random_bases(2, 9)
    z = 0x1234567890abcdef1234567
    scaled = [(Q[0] * z * z % o.Q, Q[1] * z * z * z % o.Q, z) for Q in _random_bases(n, 10)]
    rnd = _random_bases(n, 12)
    with_inf = list(rnd)
    for j in (0, n // 2, n - 1):
        with_inf[j] = (0, 1, 0)
    return {
        "repeated": [P[0]] * n,                                        # P + P and P - P inside one output
        "negatives": [P[0], o.G1.negate(P[0])] * (n // 2),
        "infinity_at_ends_and_middle": with_inf,
        "all_infinity": [(0, 1, 0)] * n,
        "infinity_other_form": [(5, 7, 0)] + rnd[1:],                # Z = 0 with arbitrary X, Y
        "z_not_one": scaled,
    }


@pytest.mark.parametrize("name", ["repeated", "negatives", "infinity_at_ends_and_middle", "all_infinity",
                                  "infinity_other_form", "z_not_one"])
def test_special_bases(name):
    from octopuszk_amd.device import SharedBaseMsm
    n, k = 16, 24
    bases = _special_base_sets(n)[name]
    d_bases = _dev(_wire(bases))
    rows = _random_rows(k, n, 31)
    _place_edges(rows, ref.edge_scalars() + EDGES_VAR_ONLY)
    rows[3] = 0                                                         # all-zero row
    cancel = {3}
    if name in ("repeated", "negatives"):
        rows[5] = 0
        rows[6] = 0
        if name == "repeated":
            _put(rows, 5, 0, 1), _put(rows, 5, n - 1, o.R - 1)          # P - P
            _put(rows, 6, 2, 9), _put(rows, 6, 3, o.R - 4), _put(rows, 6, 9, o.R - 5)
        else:
            _put(rows, 5, 0, 5), _put(rows, 5, 1, 5)                    # 5 P + 5 (-P)
            _put(rows, 6, 0, 7), _put(rows, 6, 3, 3), _put(rows, 6, 4, o.R - 4)
        cancel |= {5, 6}
    got = _run(SharedBaseMsm(d_bases, n), rows)
    for i in cancel:
        assert got[i] == INF_RECORD, (name, i)
    if name == "all_infinity":
        assert all(g == INF_RECORD for g in got)
    _assert_rows(got, _var_reference(d_bases, n, rows), name + " vs ozk_var_msm_dev")
    small = np.ascontiguousarray(rows[:8])
    _assert_rows(got, _oracle_reference([tuple(c % o.Q for c in P) for P in bases], small), name + " vs oracle")


def test_infinity_outputs_at_the_ends_of_the_normalising_batches():
    """k = 11 outputs are two lanes of the shared inversion of k_mm_norm (lane 0 holds 0, 2, .., 10, lane 1 holds 1, ..,
    9: a short batch); all-zero rows 0, 5 and 10 put O first and last in lane 0's batch and in the middle of lane 1's"""
    from octopuszk_amd.device import SharedBaseMsm
    n, k = 5, 11
    d_bases = _dev(_wire(_random_bases(n, 55)))
    rows = _random_rows(k, n, 56)
    for i in (0, 5, 10):
        rows[i] = 0
    got = _run(SharedBaseMsm(d_bases, n), rows)
    assert [i for i in range(k) if got[i] == INF_RECORD] == [0, 5, 10]
    _assert_rows(got, _var_reference(d_bases, n, rows), "n=5 k=11 vs ozk_var_msm_dev")


def test_edge_scalars_against_oracle():
    """every edge scalar alone and in company, n = 3, against the oracle's naive MSM"""
    from octopuszk_amd.device import SharedBaseMsm
    bases = _random_bases(3, 5)
    edges = ref.edge_scalars()
    k = 2 * len(edges)
    rows = np.zeros((k, 3, 32), dtype=np.uint8)
    for t, s in enumerate(edges):
        _put(rows, t, t % 3, s)
        for j in range(3):
            _put(rows, len(edges) + t, j, edges[(t + 3 * j) % len(edges)])
    got = _run(SharedBaseMsm(_dev(_wire(bases)), 3), rows)
    _assert_rows(got, _oracle_reference(bases, rows), "edge scalars")
    assert got[0] == INF_RECORD                                         # the scalar 0


def test_table_reuse_and_two_objects():
    from octopuszk_amd.device import SharedBaseMsm
    n = 15
    d1, d2 = _dev(_wire(_random_bases(n, 1))), _dev(_wire(_random_bases(n, 2)))
    a = SharedBaseMsm(d1, n)
    rows_small, rows_big = _random_rows(5, n, 50), _random_rows(700, n, 51)
    first = _run(a, rows_small)
    b = SharedBaseMsm(d2, n)
    got_b = _run(b, rows_small)
    big = _run(a, rows_big)                                             # same table, another k (workspace grows)
    assert _run(a, rows_small) == first                                 # ... and back, undisturbed by b
    _assert_rows(first, _var_reference(d1, n, rows_small), "first object")
    _assert_rows(got_b, _var_reference(d2, n, rows_small), "second object")
    _assert_rows(big, _var_reference(d1, n, rows_big, range(0, 700, 13)), "first object, k = 700")
    assert got_b != first


def test_host_mirror():
    from octopuszk_amd.variable_base_msm import batched_serial_msm
    bases = _random_bases(4, 21)
    rng = random.Random(2)
    rows = [[rng.randrange(o.R) for _ in bases] for _ in range(3)] + [[0, 0, 0, 0]]
    got = batched_serial_msm(rows, bases)
    for row, g in zip(rows, got):
        assert g == o.G1.to_affine(o.naive_msm(o.G1, row, bases))


def test_argument_checks():
    from octopuszk_amd import lib as _lib
    L = _lib.load()
    E_INVALID = -1
    assert L.ozk_multi_msm_table_bytes(15, 2) == 0 and L.ozk_multi_msm_table_bytes(0, 1) == 0
    assert L.ozk_multi_msm_table_bytes(4097, 1) == 0
    assert L.ozk_multi_msm_workspace_bytes(15, 0, 1) == 0 and L.ozk_multi_msm_workspace_bytes(15, 4, 2) == 0
    assert L.ozk_multi_msm_workspace_bytes(4096, (1 << 16) + 1, 1) == 0       # k * n > 2^28
    assert L.ozk_multi_msm_workspace_bytes(4096, 1 << 16, 1) > 0
    assert L.ozk_multi_msm_plan(0, None, None) == E_INVALID and L.ozk_multi_msm_plan(4097, None, None) == E_INVALID
    n, k = 15, 4
    tb, wb = L.ozk_multi_msm_table_bytes(n, 1), L.ozk_multi_msm_workspace_bytes(n, k, 1)
    d_bases = _dev(_wire(_random_bases(n, 3)))
    table = torch.zeros(tb, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(wb, dtype=torch.uint8, device="cuda")
    sc = torch.zeros(k * n * 32, dtype=torch.uint8, device="cuda")
    out = torch.full((k * 192,), 0xA5, dtype=torch.uint8, device="cuda")
    p = lambda t: int(t.data_ptr())
    st = int(torch.cuda.current_stream().cuda_stream)
    prep = lambda nn, ty, tbytes, wbytes: L.ozk_multi_msm_prepare_dev(p(d_bases), nn, ty, p(table), tbytes, p(ws), wbytes, st)
    run = lambda nn, kk, ty, wbytes: L.ozk_multi_msm_dev(p(table), p(sc), nn, kk, ty, p(out), p(ws), wbytes, st)
    assert prep(n, 2, tb, wb) == E_INVALID and prep(0, 1, tb, wb) == E_INVALID and prep(4097, 1, tb, wb) == E_INVALID
    assert prep(n, 1, tb - 1, wb) == E_INVALID and prep(n, 1, tb, 1024) == E_INVALID
    assert run(n, k, 2, wb) == E_INVALID and run(0, k, 1, wb) == E_INVALID and run(4097, k, 1, wb) == E_INVALID
    assert run(n, 0, 1, wb) == E_INVALID and run(4096, (1 << 16) + 1, 1, wb) == E_INVALID
    assert run(n, k, 1, 16) == E_INVALID
    torch.cuda.synchronize()
    assert bool((table == 0).all()) and bool((out == 0xA5).all())            # nothing was launched
    assert prep(n, 1, tb, wb) == 0 and run(n, k, 1, wb) == 0
    torch.cuda.synchronize()
    assert bytes(out.cpu().numpy()) == INF_RECORD * k                          # zero scalars
