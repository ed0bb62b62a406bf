"""BACE on the host: gate semantics, total_degree, the compiled program (through a Python interpreter of the
program format), the oracle on the reference's BaceTest case, and argument validation.  No GPU."""
import random

import pytest

from octopuszk_amd import bace
from tests import bace_ref as ref
from tests import bace_util as bu

R = bace.FR


def test_gate_semantics_and_degree():
    x, y = bace.InputGate(0), bace.InputGate(1)
    c = bace.ConstantGate(7)
    s = x * y                         # shared subgate: counted once per path by total_degree
    circ = bace.Circuit([x, y], (s + c) * s)
    assert circ.total_degree() == 4
    assert circ.compute([3, 5]) == (15 + 7) * 15
    sq = bace.Circuit([x], x * x)
    assert sq.total_degree() == 2 and sq.compute([R - 1]) == 1
    assert bace.Circuit([x], x + bace.ConstantGate(1)).total_degree() == 1
    assert bace.Circuit([x], bace.ConstantGate(3) * bace.ConstantGate(4)).total_degree() == 0
    assert bace.Circuit([x, y], x.add(y).mul(x)).compute([2, 3]) == 10
    assert circ.is_valid()


def test_is_valid_detects_a_loop():
    x = bace.InputGate(0)
    g = x + x
    h = g * x
    g.right = h                       # g -> h -> g
    assert not bace.Circuit([x], h).is_valid()


def test_chain_degree():
    assert bu.power_chain(5).total_degree() == 32
    assert bu.power_chain(5).compute([3]) == pow(3, 32, R)


@pytest.mark.parametrize("seed", [1, 2])
def test_compiled_program_matches_compute(seed):
    circ = bu.random_dag(12, 2000, 6, seed, const_rate=0.05)
    prog, n_slots, consts = circ.compile()
    assert prog.shape[1] == 4 and prog[-1][0] in (bace.OP_ADD, bace.OP_MUL)
    order_len = len(bace._post_order(circ.result_gate))
    assert prog.shape[0] == order_len                   # each gate once
    assert n_slots < order_len // 2                     # liveness: slots are reused
    rng = random.Random(seed)
    gates = bu.to_ref(circ)
    for _ in range(5):
        x = [rng.randrange(R) for _ in range(12)]
        want = circ.compute(x)
        assert bu.run_program(prog, n_slots, consts, x) == want
        assert ref.evaluate(gates, x) == want
    assert ref.degree(gates) == circ.total_degree()


def test_bace_test_case_on_the_oracle():
    circ, inputs, N = bu.bace_test_circuit()
    gates = bu.to_ref(circ)
    D, coeffs = ref.prove(gates, inputs, 4, N)
    assert D == 8 and len(coeffs) == 8
    from octopuszk_amd.zksnark import fr_random
    assert ref.verify(gates, (D, coeffs), inputs, 4, N, fr_random(57))
    res = ref.result((D, coeffs), N)
    assert res == [circ.compute(inputs[4 * i:4 * i + 4]) for i in range(N)] == ref.naive(gates, inputs, 4, N)
    bad = [100] + coeffs[1:]
    assert not ref.verify(gates, (D, bad), inputs, 4, N, fr_random(57))


def test_argument_validation():
    circ, inputs, N = bu.bace_test_circuit()
    with pytest.raises(ValueError):
        bace.proof_size(circ, 3)                         # N not a power of two
    with pytest.raises(ValueError):
        bace.Prover(circ, inputs[:-1], N)                # wrong input length
    x = bace.InputGate(0)
    with pytest.raises(ValueError):
        bace.proof_size(bace.Circuit([x], bace.ConstantGate(5)), 4)   # deg = 0: D = 1 < N
    with pytest.raises(ValueError):
        bace.proof_size(bu.power_chain(8), 1 << 21)      # D = 2^29 > 2^28
    with pytest.raises(ValueError):
        bace.Circuit([x], x + x).compute([1, 2])
