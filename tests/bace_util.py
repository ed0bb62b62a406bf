"""Circuits for the BACE tests and tools: the reference's BaceTest circuit, chains and random DAGs, and their
translation into the gate tuples of tests/bace_ref.py."""
import random

from octopuszk_amd import bace


def bace_test_circuit():
    """BaceTest.setUp: (x1 x2) + (x3 x4), inputs 1..16, N = 4."""
    x = [bace.InputGate(i) for i in range(4)]
    return bace.Circuit(x, (x[0] * x[1]) + (x[2] * x[3])), list(range(1, 17)), 4


def power_chain(k):
    """x^(2^k) by k squarings of one input."""
    x = bace.InputGate(0)
    g = x
    for _ in range(k):
        g = g * g
    return bace.Circuit([x], g)


def random_dag(n, gates, max_degree, seed, const_rate=0.05, recent=None):
    """A random DAG over n inputs: sums and products of earlier gates (products only while the degree stays within
    max_degree), some constants; operands uniform over all earlier gates, or over the last `recent` ones.  The result
    adds the last gate of every degree, so the circuit has degree exactly max_degree when one was reached."""
    rng = random.Random(seed)
    xs = [bace.InputGate(j) for j in range(n)]
    pool, deg = list(xs), [1] * n

    def pick():
        lo = 0 if recent is None else max(0, len(pool) - recent)
        return rng.randrange(lo, len(pool))

    while len(pool) < n + gates:
        if rng.random() < const_rate:
            pool.append(bace.ConstantGate(rng.randrange(bace.FR)))
            deg.append(0)
            continue
        a, b = pick(), pick()
        if rng.random() < 0.5 and deg[a] + deg[b] <= max_degree:
            pool.append(pool[a] * pool[b])
            deg.append(deg[a] + deg[b])
        else:
            pool.append(pool[a] + pool[b])
            deg.append(max(deg[a], deg[b]))
    res = None
    for d in range(max_degree, 0, -1):
        idx = [i for i in range(len(pool)) if deg[i] == d]
        if idx:
            res = pool[idx[-1]] if res is None else res + pool[idx[-1]]
    return bace.Circuit(xs, res)


def to_ref(circuit):
    """The circuit as tests/bace_ref.py gate tuples (evaluation order, result last)."""
    order = bace._post_order(circuit.result_gate)
    col = {id(g): j for j, g in enumerate(circuit.input_gates)}
    pos, out = {}, []
    for g in order:
        if isinstance(g, bace.InputGate):
            out.append(("in", col[id(g)]))
        elif isinstance(g, bace.ConstantGate):
            out.append(("const", g.value))
        else:
            out.append(("add" if isinstance(g, bace.SumGate) else "mul", pos[id(g.left)], pos[id(g.right)]))
        pos[id(g)] = len(out) - 1
    return out


def run_program(prog, n_slots, consts, x):
    """A Python interpreter of the program format of include/ozk.h ("BACE programs")."""
    R = bace.FR
    slots = [None] * n_slots
    last = None
    for op, dst, a, b in prog.tolist():
        if op == bace.OP_INPUT:
            v = x[a] % R
        elif op == bace.OP_CONST:
            v = consts[a]
        elif op == bace.OP_ADD:
            v = (slots[a] + slots[b]) % R
        else:
            v = slots[a] * slots[b] % R
        slots[dst] = v
        last = v
    return last
