"""BACE on the GPU against tests/bace_ref.py: proof bytes, inputs taken mod r, the HBM slot path and the LDS slot caps,
the interpreter past one launch of lanes, the verifier, getResult and the naive evaluator, a D = 2^18 consistency
check, repeatability."""
import os
import random
import secrets

import pytest
import torch

import bace_ref as ref
import bace_util as bu
from octopuszk_amd import bace
from octopuszk_amd import lib as _lib
from octopuszk_amd.zksnark import fr_random

pytestmark = pytest.mark.gpu
R = bace.FR


def _ints(t):
    torch.cuda.synchronize()
    raw = bytes(t.cpu().numpy().tobytes())
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(raw) // 32)]


def _dev_words(values):
    """32-byte LE words on the device as written (a list of ints goes through the package mod r)"""
    return torch.tensor(list(b"".join(v.to_bytes(32, "little") for v in values)), dtype=torch.uint8).cuda()


def _check_against_oracle(circ, inputs, N):
    n = circ.input_size
    as_written = _dev_words(inputs) if any(v >= R for v in inputs) else inputs
    D, proof = bace.Prover(circ, as_written, N).compute_proof()
    D_ref, want = ref.prove(bu.to_ref(circ), [v % R for v in inputs], n, N)
    assert D == D_ref
    assert _ints(proof) == want
    return D, proof


def _random_inputs(n, N, seed):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(n * N)]


def test_bace_test_case_bit_exact():
    circ, inputs, N = bu.bace_test_circuit()
    D, proof = _check_against_oracle(circ, inputs, N)
    assert D == 8
    v = bace.Verifier(circ, (D, proof), inputs, N)
    assert v.verify_proof(seed=57)
    assert _ints(v.get_result()) == [circ.compute(inputs[4 * i:4 * i + 4]) for i in range(N)]


@pytest.mark.parametrize("case", ["degree1", "n1", "chain32", "edges"])
def test_small_cases_bit_exact(case):
    x = bace.InputGate(0)
    if case == "degree1":                # D = N
        circ, N = bace.Circuit([x], x + bace.ConstantGate(5)), 16
        inputs = _random_inputs(1, N, 3)
    elif case == "n1":                   # one instance
        y = bace.InputGate(1)
        circ, N = bace.Circuit([x, y], x * y + y), 1
        inputs = [3, 9]
    elif case == "chain32":              # x^32: D = 32 N
        circ, N = bu.power_chain(5), 8
        inputs = _random_inputs(1, N, 4)
    else:                                # inputs 0, 1, r - 1 and r, r + 1, 2^256 - 1: taken mod r
        y = bace.InputGate(1)
        circ, N = bace.Circuit([x, y], (x * y) * (x + y)), 4
        inputs = [0, 1, R - 1, R, R + 1, (1 << 256) - 1, R - 1, R - 1]
    _check_against_oracle(circ, inputs, N)


def test_random_dag_bit_exact():
    circ = bu.random_dag(8, 2000, 4, seed=7, const_rate=0.05)
    assert circ.total_degree() == 4
    _check_against_oracle(circ, _random_inputs(8, 64, 8), 64)


@pytest.mark.parametrize("D", [2048, 4096])
def test_lds_multipass_boundary(D):
    # D = 2048: every transform in LDS; D = 4096: the forward and final transforms take the tiled passes
    x, y = bace.InputGate(0), bace.InputGate(1)
    circ = bace.Circuit([x, y], x * y + x)
    N = D // 2
    _check_against_oracle(circ, _random_inputs(2, N, D), N)
    circ3 = bu.power_chain(3)              # N = D / 8: the column transforms in LDS, the others tiled at 4096
    _check_against_oracle(circ3, _random_inputs(1, D // 8, D + 1), D // 8)


def test_tiled_columns_bit_exact():
    # N = 4096: the batched column transforms themselves take the tiled passes (several columns on blockIdx.y)
    circ = bu.random_dag(3, 40, 2, seed=11)
    _check_against_oracle(circ, _random_inputs(3, 4096, 12), 4096)


def test_hbm_slot_path_same_bytes():
    circ = bu.random_dag(6, 2000, 4, seed=9, const_rate=0.05)
    _, n_slots, _ = circ.compile()
    assert n_slots > 4
    inputs = _random_inputs(6, 32, 10)
    _, a = bace.Prover(circ, inputs, 32).compute_proof()
    L = _lib.load()
    old = os.environ.get("OZK_BACE_LDS_SLOTS")
    try:
        for cap in ("0", "3", "28", "64"):   # all in HBM, three in LDS, the most LDS a workgroup may take, clamped to it
            os.environ["OZK_BACE_LDS_SLOTS"] = cap
            L.ozk_tuning_reload()
            _, b = bace.Prover(circ, inputs, 32).compute_proof()
            assert torch.equal(a, b)
            assert _ints(bace.NaiveEvaluator(circ, inputs, 32).get_result()) == ref.naive(bu.to_ref(circ), inputs, 6, 32)
    finally:
        if old is None:
            os.environ.pop("OZK_BACE_LDS_SLOTS", None)
        else:
            os.environ["OZK_BACE_LDS_SLOTS"] = old
        L.ozk_tuning_reload()


def test_interpreter_past_one_launch_of_lanes():
    """65536 + 65 rows: a launch has 65536 lanes, and 65 of them (one whole wave and one lane) take a second trip of the
    loop over points; with three slots in LDS the spilled slots of that trip are indexed by the lane, not the row"""
    rows, n = 65536 + 65, 2
    circ = bu.random_dag(n, 70, 4, seed=25, const_rate=0.05)        # (34 of its gates reach the result)
    prog, n_slots, _ = circ.compile()
    assert n_slots > 3 and 30 <= prog.shape[0] <= 60
    inputs = _random_inputs(n, rows, 24)
    for k, row in enumerate((0, 65535, 65536, rows - 1)):          # written as x + k r, k = 2 .. 5 where it fits
        for j in range(n):
            v, m = inputs[n * row + j], 2 + k
            while v + m * R >= 1 << 256:
                m -= 1
            inputs[n * row + j] = v + m * R
    assert all(inputs[n * row] >= 2 * R for row in (0, 65535, 65536, rows - 1))
    want = [circ.compute(inputs[n * i:n * i + n]) for i in range(rows)]
    d_inputs = _dev_words(inputs)
    assert _ints(bace.NaiveEvaluator._evaluate(circ, d_inputs, rows)) == want
    L = _lib.load()
    old = os.environ.get("OZK_BACE_LDS_SLOTS")
    try:
        os.environ["OZK_BACE_LDS_SLOTS"] = "3"
        L.ozk_tuning_reload()
        assert _ints(bace.NaiveEvaluator._evaluate(circ, d_inputs, rows)) == want
    finally:
        if old is None:
            os.environ.pop("OZK_BACE_LDS_SLOTS", None)
        else:
            os.environ["OZK_BACE_LDS_SLOTS"] = old
        L.ozk_tuning_reload()


def test_verifier_accepts_and_rejects():
    circ = bu.random_dag(5, 300, 3, seed=13, const_rate=0.05)
    N = 64
    inputs = _random_inputs(5, N, 14)
    D, proof = bace.Prover(circ, inputs, N).compute_proof()
    v = bace.Verifier(circ, (D, proof), inputs, N)
    assert v.verify_proof(seed=57)
    assert v.verify_proof()                                     # r from secrets
    omega = pow(ref.bn254.fr_root_of_unity(N), 5, R)            # r inside the N-point domain
    assert v.verify_proof(challenge=omega)
    assert v.verify_proof(challenge=1)
    for pos in (0, D // 2, D - 1):
        bad = proof.clone()
        c = _ints(proof[32 * pos:32 * pos + 32])[0]
        bad[32 * pos:32 * pos + 32] = torch.tensor(list(((c + 1) % R).to_bytes(32, "little")), dtype=torch.uint8)
        vb = bace.Verifier(circ, (D, bad), inputs, N)
        assert not vb.verify_proof(seed=57)
        assert not vb.verify_proof()


def test_columns_at_matches_oracle():
    n, N = 3, 16
    inputs = _random_inputs(n, N, 15)
    circ = bace.Circuit([bace.InputGate(j) for j in range(n)], bace.InputGate(0))
    circ.result_gate = circ.input_gates[0] * circ.input_gates[1] + circ.input_gates[2]
    v = bace.Verifier(circ, bace.Prover(circ, inputs, N).compute_proof(), inputs, N)
    r = secrets.randbelow(R)
    got = _ints(v.columns_at(r))
    want = [ref.horner(ref.ifft(col), r) for col in ref.columns(inputs, n, N)]
    assert got == want
    w = ref.bn254.fr_root_of_unity(N)
    assert _ints(v.columns_at(pow(w, 3, R))) == [inputs[3 * n + j] for j in range(n)]   # r in the domain: the value


def test_result_and_naive_equal_host_circuit():
    circ = bu.random_dag(4, 500, 4, seed=17, const_rate=0.05)
    N = 128
    inputs = _random_inputs(4, N, 18)
    host = [circ.compute(inputs[4 * i:4 * i + 4]) for i in range(N)]
    proof = bace.Prover(circ, inputs, N).compute_proof()
    assert _ints(bace.Verifier(circ, proof, inputs, N).get_result()) == host
    assert _ints(bace.NaiveEvaluator(circ, inputs, N).get_result()) == host
    dev_inputs = torch.tensor(list(b"".join(v.to_bytes(32, "little") for v in inputs)), dtype=torch.uint8).cuda()
    assert _ints(bace.NaiveEvaluator(circ, dev_inputs, N).get_result()) == host


def test_large_d_consistency():
    n, N = 4, 1 << 16
    circ = bu.random_dag(n, 200, 4, seed=19, const_rate=0.05)
    assert circ.total_degree() == 4
    inputs = _random_inputs(n, N, 20)
    D, proof = bace.Prover(circ, inputs, N).compute_proof()
    assert D == 1 << 18
    host = [circ.compute(inputs[n * i:n * i + n]) for i in range(N)]
    v = bace.Verifier(circ, (D, proof), inputs, N)
    assert _ints(v.get_result()) == host
    r = secrets.randbelow(R)
    assert v.claim(r) == ref.horner(_ints(proof), r)
    assert v.verify_proof(challenge=r)


def test_repeatable():
    circ = bu.random_dag(6, 400, 4, seed=21, const_rate=0.05)
    inputs = _random_inputs(6, 256, 22)
    _, a = bace.Prover(circ, inputs, 256).compute_proof()
    _, b = bace.Prover(circ, inputs, 256).compute_proof()
    assert torch.equal(a, b)


def test_invalid_arguments_rejected():
    circ, inputs, N = bu.bace_test_circuit()
    with pytest.raises(ValueError):
        bace.Prover(circ, inputs, 3)
    x = bace.InputGate(0)
    with pytest.raises(ValueError):
        bace.Prover(bace.Circuit([x], bace.ConstantGate(2)), [1, 2, 3, 4], 4)
    L = _lib.load()
    assert L.ozk_bace_workspace_bytes(4, 3, 8, 1, 1, 0) == 0
    assert L.ozk_bace_workspace_bytes(4, 8, 4, 1, 1, 0) == 0
