"""CPU tests of the import of an R1CS into PLONK: plonk.from_r1cs against the arithmetic of
zksnark.is_satisfied constraint by constraint, and against the second compiler of tests/plonk_r1cs_ref.py row by
row."""
import random

import numpy as np
import pytest

import plonk_r1cs_ref as rm
import plonk_ref as pm

R = pm.R


def _zksnark_relation(rel):
    from octopuszk_amd import zksnark as z
    sides = [z.LinearCombinations(s.ptr, s.index, s.value) for s in (rel.A, rel.B, rel.C)]
    return z.R1CSRelation(*sides, rel.num_inputs, rel.num_auxiliary)


def _gates(circuit):
    """(selectors, cells) of every row"""
    return [([col[i] for col in circuit.selectors], [col[i] for col in circuit.wires]) for i in range(circuit.n)]


def _constraint_rows(rel):
    """the row of every constraint's own gate, from the pinned order: the public rows, then per constraint its chain
    gates and its gate"""
    at, rows = rel.num_inputs, []
    for i in range(rel.num_constraints):
        for side in (rel.A, rel.B, rel.C):
            at += max(sum(1 for v, _ in side.terms[i] if v != 0) - 1, 0)
        rows.append(at)
        at += 1
    return rows, at


# ---------------------------------------------------------------------------- equivalence
def test_a_constraint_gate_holds_exactly_when_the_constraint_does():
    from octopuszk_amd import plonk
    from octopuszk_amd import zksnark as z
    rel, good = rm.mixed_relation()
    assert max(len(row) for row in rel.A.terms) == rm.LONG > 64
    zrel = _zksnark_relation(rel)
    circuit = plonk.from_r1cs(zrel)
    gates = _gates(circuit)
    own, used = _constraint_rows(rel)
    rng = random.Random(3601)
    assignments = [good] + [[1] + [rng.randrange(R) for _ in range(rm.NV - 1)] for _ in range(19)]
    assignments[1] = good[:-1] + [(good[-1] + 1) % R]
    assert z.is_satisfied(zrel, good[:rm.NI], good[rm.NI:])
    seen = set()
    for w in assignments:
        values = circuit.extend(w)
        assert values == rm.extend(rel, w) and len(values) == circuit.n_vars
        ev, _ = z.constraint_evaluations(zrel, w)
        holds = [(int(ev[0][i]) * int(ev[1][i]) - int(ev[2][i])) % R == 0 for i in range(rel.num_constraints)]
        assert holds == [rm.constraint_holds(rel, i, w) for i in range(rel.num_constraints)]
        for i, (q, cells) in enumerate(gates):
            if i in own:
                assert rm.gate_holds(q, cells, values) == holds[own.index(i)], (i, own.index(i))
            elif i >= circuit.n_public:                                   # (a public row holds with its PI term)
                assert rm.gate_holds(q, cells, values), i                 # chain gates and empty gates
        seen.update(holds)
    assert seen == {True, False}


@pytest.mark.parametrize("nc,ni", [(6, 2), (30, 3)])
def test_the_synthetic_circuit_and_its_witness(nc, ni):
    from octopuszk_amd import plonk
    from octopuszk_amd import zksnark as z
    r1cs, primary, auxiliary = z.serial_construct(nc, ni)
    circuit = plonk.from_r1cs(r1cs)
    assert circuit.term_coeff is None
    values = circuit.extend(primary + auxiliary)
    for i, (q, cells) in enumerate(_gates(circuit)):
        if i >= circuit.n_public:
            assert rm.gate_holds(q, cells, values), i
    assert [values[v] for v in circuit.wires[0][:ni]] == primary


# ---------------------------------------------------------------------------- layout
def test_layout_is_the_pinned_one():
    from octopuszk_amd import plonk
    rel, w = rm.mixed_relation()
    circuit = plonk.from_r1cs(rel)
    rows, stream = rm.compile_rows(rel)
    own, used = _constraint_rows(rel)
    nv, terms = rel.num_variables, len(stream)
    chained = sum(max(sum(1 for v, _ in side.terms[i] if v != 0) - 1, 0) for side in (rel.A, rel.B, rel.C)
                  for i in range(rel.num_constraints))
    assert len(rows) == used == rel.num_inputs + rel.num_constraints + chained
    n, want = rm.padded(rows)
    assert (circuit.n, circuit.n_public) == (n, rel.num_inputs) and n >= len(rows) > n // 2
    assert _gates(circuit) == [(list(q), list(cells)) for q, cells in want]
    assert isinstance(circuit, plonk.R1CSCircuit) and isinstance(circuit, plonk.Circuit)
    assert circuit.num_variables == nv and circuit.n_vars == nv + terms
    assert circuit.term_index == [v for v, _, _ in stream] and circuit.term_coeff == [c for _, c, _ in stream]
    starts = sorted({t0 for _, _, t0 in stream})
    assert circuit.chain_start == starts
    assert circuit.chain_length == [sum(1 for _, _, t0 in stream if t0 == s) for s in starts]
    # the slot of a chain's first term is in no cell; every other accumulator is
    cells = {v for col in circuit.wires for v in col}
    assert all(nv + s not in cells for s in starts)
    assert {v - nv for v in cells if v >= nv} == set(range(terms)) - set(starts)
    # public rows as Builder.build writes them, empty rows behind
    for i in range(rel.num_inputs):
        assert _gates(circuit)[i] == ([1, 0, 0, 0, 0], [i, i, i])
    assert all(g == ([0] * 5, [0] * 3) for g in _gates(circuit)[used:])


def test_two_calls_agree_and_unit_coefficients_are_ones():
    from octopuszk_amd import plonk
    from octopuszk_amd import zksnark as z
    rel, _ = rm.mixed_relation()
    one, two = plonk.from_r1cs(rel), plonk.from_r1cs(rel)
    for name in ("n", "n_public", "n_vars", "selectors", "wires", "term_index", "term_coeff", "chain_start", "chain_length"):
        assert getattr(one, name) == getattr(two, name), name
    r1cs, _, _ = z.serial_construct(30, 3)
    ones = [z.LinearCombinations(lc.ptr, lc.index, np.array([1] * len(lc.index), dtype=object)) for lc in (r1cs.A, r1cs.B, r1cs.C)]
    explicit = plonk.from_r1cs(z.R1CSRelation(*ones, r1cs.num_inputs, r1cs.num_auxiliary))
    unit = plonk.from_r1cs(r1cs)
    assert explicit.selectors == unit.selectors and explicit.wires == unit.wires
    assert unit.term_coeff is None and explicit.term_coeff == [1] * len(unit.term_index)


def test_row_count_of_the_synthetic_circuit():
    """about ni + 3.5 nc rows: nc / 2 chains of two terms and, in the last constraint, two chains of nc"""
    from octopuszk_amd import plonk
    from octopuszk_amd import zksnark as z
    nc, ni = 30, 3
    r1cs, _, _ = z.serial_construct(nc, ni)
    circuit = plonk.from_r1cs(r1cs)
    used = ni + nc + nc // 2 + 2 * nc                                    # (the last constraint's combinations have nc + 1 terms)
    assert circuit.n == 128 and used == 108
    assert all(any(col[i] for col in circuit.selectors) for i in range(used))
    assert not any(col[i] for col in circuit.selectors for i in range(used, circuit.n))


# ---------------------------------------------------------------------------- rejections
def test_rejections(monkeypatch):
    from octopuszk_amd import plonk
    from octopuszk_amd.plonk import circuit as pc
    rel, _ = rm.mixed_relation()
    short = rm.Relation(rel.A, rm.Side(rel.B.terms[:-1]), rel.C, rel.num_inputs, rel.num_auxiliary)
    with pytest.raises(ValueError):
        plonk.from_r1cs(short)
    for bad in (rm.NV, -1):
        outside = rm.Relation(rel.A, rel.B, rm.Side(rel.C.terms[:-1] + [[(bad, 1)]]), rel.num_inputs, rel.num_auxiliary)
        with pytest.raises(ValueError):
            plonk.from_r1cs(outside)
    rows = plonk.from_r1cs(rel).n
    monkeypatch.setattr(pc, "N_MAX", rows)
    assert plonk.from_r1cs(rel).n == rows
    monkeypatch.setattr(pc, "N_MAX", rows // 2)                          # fewer rows than the circuit has
    with pytest.raises(ValueError):
        plonk.from_r1cs(rel)


def test_extend_takes_the_r1cs_assignment_alone():
    from octopuszk_amd import plonk
    rel, w = rm.mixed_relation()
    circuit = plonk.from_r1cs(rel)
    for bad in (w[:-1], w + [0], w[:-1] + [R], w[:-1] + [-1]):
        with pytest.raises(ValueError):
            circuit.extend(bad)
