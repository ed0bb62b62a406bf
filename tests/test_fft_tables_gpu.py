"""The transforms with their tables built per call in the caller's workspace (csrc/fft.hip fft_layout, qap_layout,
qap_build_tables; csrc/bace.hip bace_twiddles), and the knobs beside them: OZK_FFT_PLAN_CACHE=0, the byte-budget
fallback OZK_FFT_PLAN_CACHE_MB (a plan larger than the budget is not cached: production domains above 4 GiB),
OZK_FFT_TW_PYRAMID=0 and OZK_QAP_FOLD_SCALE=0 (k_coset_scale as a kernel of its own, at sizes where it reads the
second level of its power table).  Every result is compared byte for byte with the oracle.

Which path ran is observable: both layouts take omega first, so on the per-call path the first 32 bytes of the
workspace hold omega after the call, and on the plan path they keep the zeros the test put there.  The rest of the
workspace starts poisoned.  ozk_host_cache_release() goes before every call: a plan cached by an earlier test would be
a hit (the cache looks a key up before it looks at the byte budget), and the per-call path would not run.  The one
exception is test_transform_and_witness_map_share_a_domain, which releases once and then keeps the cache across its
three calls (release=False): what it checks is two kinds of plan living side by side."""
import ctypes
import functools
import random

import numpy as np
import pytest
import torch

import fr_gpu_util as u
from oracle import bn254 as o
from oracle import coracle
from test_qap_witness_gpu import _oracle_with_c_fft

pytestmark = pytest.mark.gpu
R = o.R


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _per_call(knobs):
    return knobs.get("OZK_FFT_PLAN_CACHE") == "0" or knobs.get("OZK_FFT_PLAN_CACHE_MB") == "0"


def _workspace(nbytes):
    """poison, except the 256 bytes where a per-call build puts omega"""
    ws = u.poisoned(nbytes)
    ws[:256] = 0
    return ws


def _upload(raw):
    return torch.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()


# ---------------------------------------------------------------------------------------------- forward transform
@functools.lru_cache(maxsize=None)
def _fft_case(n):
    """(input bytes, omega bytes, the oracle's 64-byte elements, their low halves)"""
    a = np.random.default_rng(n).integers(0, 256, size=(n, 32), dtype=np.uint8)
    a[:, 31] &= 0x1F
    a[0] = 0
    a[n // 2] = np.frombuffer(o.to_le32(R - 1), dtype=np.uint8)
    w = o.to_le32(o.fr_root_of_unity(n))
    want64 = coracle.fft_fr(a.tobytes(), n, w)
    want32 = np.frombuffer(want64, dtype=np.uint8).reshape(n, 64)[:, :32].tobytes()
    return a.tobytes(), w, want64, want32


def _fft_compact(L, n, release=True):
    """ozk_fft_compact_dev on _fft_case(n): (output tensor with its guard, workspace) after the call"""
    from octopuszk_amd import lib
    data, w, _, _ = _fft_case(n)
    wsb = int(L.ozk_fft_workspace_bytes(n))
    assert wsb > 0
    ws, d_in, out = _workspace(wsb), _upload(data), u.poisoned(n * 32 + u.GUARD)
    hw = ctypes.create_string_buffer(w, 32)
    if release:
        L.ozk_host_cache_release()
    lib.check(L.ozk_fft_compact_dev(d_in.data_ptr(), n, u.vp(hw), out.data_ptr(), ws.data_ptr(), wsb, _stream()))
    torch.cuda.synchronize()
    return out, ws


def _check_fft_compact(L, n, per_call, release=True):
    _, w, _, want32 = _fft_case(n)
    out, ws = _fft_compact(L, n, release)
    assert bytes(out[:n * 32].cpu().numpy()) == want32
    assert u.tail_untouched(out, n * 32)
    # (a transform of one element has no plan: its omega always lands in the workspace)
    assert bytes(ws[:32].cpu().numpy()) == (w if per_call or n == 1 else bytes(32))


@pytest.mark.parametrize("n", [1, 2, 512, 1024, 4096, 1 << 14, 1 << 17])
@pytest.mark.parametrize("knobs", [{"OZK_FFT_PLAN_CACHE": "0"}, {"OZK_FFT_PLAN_CACHE_MB": "0"}, {"OZK_FFT_TW_PYRAMID": "0"},
                                   {"OZK_FFT_PLAN_CACHE": "0", "OZK_FFT_TW_PYRAMID": "0"}], ids=u.knob_id)
def test_fft_with_tables_in_the_workspace(knobs, n, monkeypatch):
    """ozk_fft_compact_dev (32-byte elements) below the tile (1, 2, 512), at one pass (1024), two (4096, 2^14) and
    three (2^17): twiddles built into the workspace (fft_layout, fft_build_twiddles) with and without the pyramid's
    levels, and the plan's table read with a stride."""
    from octopuszk_amd import lib
    L = lib.load()
    with u.knobs_set(L, monkeypatch, knobs):
        _check_fft_compact(L, n, _per_call(knobs))


def test_fft_host_with_tables_in_the_workspace(monkeypatch):
    """ozk_fft_host under OZK_FFT_PLAN_CACHE=0: the 64-byte format, upper halves zero, from a poisoned output"""
    from octopuszk_amd import lib
    L = lib.load()
    with u.knobs_set(L, monkeypatch, {"OZK_FFT_PLAN_CACHE": "0"}):
        for n in (2, 4096):
            data, w, want64, _ = _fft_case(n)
            out = ctypes.create_string_buffer(bytes([u.POISON]) * (64 * n), 64 * n)
            L.ozk_host_cache_release()
            lib.check(L.ozk_fft_host(ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p), n,
                                     ctypes.cast(ctypes.c_char_p(w), ctypes.c_void_p), 0, ctypes.cast(out, ctypes.c_void_p)))
            assert not np.frombuffer(out.raw, dtype=np.uint8).reshape(n, 64)[:, 32:].any(), n
            assert out.raw == want64, n


# ---------------------------------------------------------------------------------------------- witness map
@functools.lru_cache(maxsize=None)
def _qap_case(m):
    """(a, b, c as device-ready bytes, omega, the m + 1 expected coefficients of H)"""
    rng = random.Random(700 + m)
    a = [rng.randrange(R) for _ in range(m)]
    b = [rng.randrange(R) for _ in range(m)]
    a[0], b[1] = 0, R - 1
    c = [x * y % R for x, y in zip(a, b)]
    c[7 % m] = (c[7 % m] + 1) % R     # one violated constraint: still the same function
    want = o.qap_witness_coefficients_h(a, b, c) if m <= 4096 else _oracle_with_c_fft(a, b, c)
    assert len(want) == m + 1 and want[m] == 0
    raw = tuple(b"".join(o.to_le32(x) for x in v) for v in (a, b, c))
    return raw, o.to_le32(o.fr_root_of_unity(m)), want


def _check_qap_witness(L, m, per_call, release=True):
    from octopuszk_amd import lib
    raw, w, want = _qap_case(m)
    wsb = int(L.ozk_qap_witness_workspace_bytes(m))
    assert wsb > 0
    ws, d_h = _workspace(wsb), u.poisoned((m + 1) * 32 + u.GUARD)
    d_abc = [_upload(v) for v in raw]
    hw, hg = ctypes.create_string_buffer(w, 32), u.host32(o.FR_MULT_GEN)
    if release:
        L.ozk_host_cache_release()
    lib.check(L.ozk_qap_witness_dev(d_abc[0].data_ptr(), d_abc[1].data_ptr(), d_abc[2].data_ptr(), m, u.vp(hw), u.vp(hg),
                                    d_h.data_ptr(), ws.data_ptr(), wsb, _stream()))
    torch.cuda.synchronize()
    bad = u.mismatches(u.ints(d_h, m + 1), want)
    assert not bad, "%d of %d coefficients of H differ, first at %s" % (len(bad), m + 1, bad[:8])
    assert u.tail_untouched(d_h, (m + 1) * 32)
    assert bytes(ws[:32].cpu().numpy()) == (w if per_call else bytes(32))


@pytest.mark.parametrize("m", [2, 512, 1024, 4096, 8192])
@pytest.mark.parametrize("knobs", [{"OZK_FFT_PLAN_CACHE": "0"}, {"OZK_FFT_PLAN_CACHE_MB": "0"}, {"OZK_QAP_FOLD_SCALE": "0"},
                                   {"OZK_FFT_PLAN_CACHE": "0", "OZK_QAP_FOLD_SCALE": "0"}, {}], ids=u.knob_id)
def test_qap_witness_with_tables_in_the_workspace(knobs, m, monkeypatch):
    """ozk_qap_witness_dev with its constants, twiddles, coset powers and scale tables built into the workspace
    (qap_layout, qap_build_tables), and with the coset scaling as a kernel of its own: below 1024 it always is, at 4096
    and 8192 with the fold off k_coset_scale reads the second level of its power table.  Against
    oracle.bn254.qap_witness_coefficients_h (the C oracle's transforms at 8192), trailing zero included."""
    from octopuszk_amd import lib
    L = lib.load()
    with u.knobs_set(L, monkeypatch, knobs):
        _check_qap_witness(L, m, _per_call(knobs))


@pytest.mark.parametrize("knob", ["OZK_FFT_PLAN_CACHE", "OZK_FFT_PLAN_CACHE_MB"])
def test_workspace_shows_which_path_built_the_tables(knob, monkeypatch):
    """Both directions of the observable the tests above rely on, in one process state: with the knob at 0 omega
    appears at the head of the workspace, without it the same call leaves the zeros there (and both give the oracle's
    result)."""
    from octopuszk_amd import lib
    L = lib.load()
    with u.knobs_set(L, monkeypatch, {knob: "0"}):
        _check_fft_compact(L, 4096, True)
        _check_qap_witness(L, 1024, True)
    _check_fft_compact(L, 4096, False)
    _check_qap_witness(L, 1024, False)


@pytest.mark.parametrize("n", [2, 1024])
@pytest.mark.parametrize("knobs", [{}, {"OZK_FFT_PLAN_CACHE_MB": "0"}], ids=u.knob_id)
def test_transform_and_witness_map_share_a_domain(knobs, n, monkeypatch):
    """The plan cache's two kinds of key on ONE domain, interleaved with nothing released in between: a transform, the
    witness map, the transform again, all with the same omega (_fft_case and _qap_case both take fr_root_of_unity(n)).
    Both kinds of plan are carved by one function and looked up in one cache: same_key must keep (n, omega) apart from
    (n, omega, g), or the witness map would find a plan without its coset tables and the second transform one that
    is not its own.  n = 2 is the smallest plan, n = 1024 the smallest tiled transform (the witness map's last passes
    fold the scalings in).  With the byte budget at 0 the same three calls build their tables in their workspaces."""
    from octopuszk_amd import lib
    L = lib.load()
    assert _fft_case(n)[1] == _qap_case(n)[1]
    with u.knobs_set(L, monkeypatch, knobs):
        L.ozk_host_cache_release()
        _check_fft_compact(L, n, _per_call(knobs), release=False)
        _check_qap_witness(L, n, _per_call(knobs), release=False)
        _check_fft_compact(L, n, _per_call(knobs), release=False)


# ---------------------------------------------------------------------------------------------- BACE
@pytest.mark.parametrize("case", ["n1", "bace_test", "degree1"])
def test_bace_with_tables_in_the_workspace(case, monkeypatch):
    """The small cases of test_bace_gpu.py once more with bace_twiddles building its tables per call, against
    bace_ref: n1 (N = 1, D = 2) is the smallest that reaches it with a size of two, but a table of one entry says
    little, so the BaceTest circuit (D = 8) and degree1 (N = D = 16) follow.  ozk_bace_prove_dev is called as
    bace.Prover.compute_proof calls it, with a workspace of the test's own: bace_layout puts the root of unity handed to
    the per-call build behind its 256-byte constant block, so those 32 bytes hold a primitive D-th root of unity after a
    per-call run and stay zero when the plan cache served the tables."""
    import bace_ref as ref
    import bace_util as bu
    from octopuszk_amd import bace, lib
    from octopuszk_amd.device import _ptr
    L = lib.load()
    x, y = bace.InputGate(0), bace.InputGate(1)
    if case == "n1":
        circ, N, inputs = bace.Circuit([x, y], x * y + y), 1, [3, 9]
    elif case == "degree1":
        circ, N = bace.Circuit([x], x + bace.ConstantGate(5)), 16
        rng = random.Random(3)
        inputs = [rng.randrange(R) for _ in range(N)]
    else:
        circ, inputs, N = bu.bace_test_circuit()
    D_ref, want = ref.prove(bu.to_ref(circ), inputs, circ.input_size, N)
    p = bace.Prover(circ, inputs, N)
    assert p.D == D_ref >= 2
    prog, n_slots, cb, n_consts = bace._program_args(circ)
    n_ops = prog.shape[0]
    wsb = int(L.ozk_bace_workspace_bytes(p.n, p.N, p.D, n_ops, n_slots, n_consts))
    assert wsb > 512
    for knobs in ({"OZK_FFT_PLAN_CACHE": "0"}, {}):
        ws = u.poisoned(wsb)
        ws[256:512] = 0
        proof = u.poisoned(p.D * 32 + u.GUARD)
        L.ozk_host_cache_release()
        with u.knobs_set(L, monkeypatch, knobs):
            lib.check(L.ozk_bace_prove_dev(_ptr(p.inputs), p.n, p.N, prog.ctypes.data, n_ops, n_slots, bace._vp(cb), n_consts,
                                           p.D, _ptr(proof), _ptr(ws), wsb, _stream()))
            torch.cuda.synchronize()
        assert u.ints(proof, p.D) == want, knobs
        assert u.tail_untouched(proof, p.D * 32), knobs
        root = u.ints(ws[256:288], 1)[0]
        if _per_call(knobs):
            assert pow(root, p.D, R) == 1 and pow(root, p.D // 2, R) == R - 1, knobs
        else:
            assert root == 0, knobs
