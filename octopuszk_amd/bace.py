"""BACE: Williams' Merlin-Arthur proof for batch arithmetic-circuit evaluation (the reference's bace/ package) on the
GPU, through the C ABI of libozk_hip.so (include/ozk.h, "BACE").  There is no CPU path.

A circuit has n input gates; N instances (a power of two) are given row-major: value i*n + j is input j of instance i,
either as a list of ints or as a uint8 CUDA tensor of N*n x 32-byte little-endian values.  The prover interpolates
every column over the N-point domain (beta_j), evaluates the circuit on the beta_j at the D = lowestPowerOfTwo(deg*N)
points of the larger domain and returns the D coefficients of R(z) = C(beta(z)).  The verifier checks R(r) ==
C(beta(r)) at one random r.  Field: BN254 Fr (the reference's test uses a 180-bit field).

Tensors live on the current device and work on the current stream.
"""
import secrets

import numpy as np
import torch

from . import lib as _lib
from .device import _ptr, _stream
from .fft import FR, fr_random, lowest_power_of_two
from .vectors import fr_poly_eval
from .wire import host_bytes, ints32, le32
from .wire import vp as _vp

MAX_D = 1 << 28     # the 2-adicity of Fr
OP_INPUT, OP_CONST, OP_ADD, OP_MUL = 0, 1, 2, 3


# ---------------------------------------------------------------------------------------------- gates
class Gate:
    """bace.circuit.Gate: a node of the circuit DAG; shared subgates are evaluated once."""

    left = None
    right = None

    def add(self, other):
        return SumGate(self, other)

    def mul(self, other):
        return ProductGate(self, other)

    __add__ = add
    __mul__ = mul

    def children(self):
        return [g for g in (self.left, self.right) if g is not None]


class InputGate(Gate):
    """bace.circuit.InputGate(value, index): `index` names the variable; the COLUMN is the gate's position in the
    circuit's input_gates list.  `value` is what compute() loads into it."""

    def __init__(self, index=0, value=0):
        self.index = index
        self.value = value % FR


class ConstantGate(Gate):
    def __init__(self, value):
        self.value = value % FR


class SumGate(Gate):
    def __init__(self, left, right):
        self.left, self.right = left, right


class ProductGate(Gate):
    def __init__(self, left, right):
        self.left, self.right = left, right


def _post_order(root):
    """Each gate reachable from root once, children (left, then right) before parents: the order of
    Circuit.evaluate's stack traversal.  Iterative, so that deep circuits do not hit the recursion limit."""
    order, seen, stack = [], set(), [(root, False)]
    while stack:
        g, expanded = stack.pop()
        if expanded:
            order.append(g)
            continue
        if id(g) in seen:
            continue
        seen.add(id(g))
        stack.append((g, True))
        for c in reversed(g.children()):   # left is popped first
            if id(c) not in seen:
                stack.append((c, False))
    return order


class Circuit:
    """bace.circuit.Circuit(inputGates, resultGate)."""

    def __init__(self, input_gates, result_gate):
        self.input_gates = list(input_gates)
        self.result_gate = result_gate
        self.input_size = len(self.input_gates)
        self._compiled = None
        self._degree = None

    def compute(self, inputs):
        """Circuit.compute: the circuit on one instance (a list of input_size ints), on the host."""
        inputs = list(inputs)
        if len(inputs) != self.input_size:
            raise ValueError("Assignment size must match circuit size")
        for g, v in zip(self.input_gates, inputs):
            g.value = int(v) % FR
        val = {}
        for g in _post_order(self.result_gate):
            if isinstance(g, (InputGate, ConstantGate)):
                val[id(g)] = g.value
            elif isinstance(g, SumGate):
                val[id(g)] = (val[id(g.left)] + val[id(g.right)]) % FR
            else:
                val[id(g)] = val[id(g.left)] * val[id(g.right)] % FR
        return val[id(self.result_gate)]

    def total_degree(self):
        """Circuit.totalDegree over the gate TREE (input 1, constant 0, sum max, product sum), memoised per gate: a
        gate's degree does not depend on the path to it, so the memo gives the Java recursion's value."""
        if self._degree is None:
            deg = {}
            for g in _post_order(self.result_gate):
                if isinstance(g, InputGate):
                    deg[id(g)] = 1
                elif isinstance(g, ConstantGate):
                    deg[id(g)] = 0
                elif isinstance(g, SumGate):
                    deg[id(g)] = max(deg[id(g.left)], deg[id(g.right)])
                else:
                    deg[id(g)] = deg[id(g.left)] + deg[id(g.right)]
            self._degree = deg[id(self.result_gate)]
        return self._degree

    def is_valid(self):
        """Circuit.isValid: no gate reaches itself."""
        WHITE, GREY, BLACK = 0, 1, 2
        colour = {}
        stack = [(self.result_gate, iter(self.result_gate.children()))]
        colour[id(self.result_gate)] = GREY
        while stack:
            g, it = stack[-1]
            c = next(it, None)
            if c is None:
                colour[id(g)] = BLACK
                stack.pop()
                continue
            st = colour.get(id(c), WHITE)
            if st == GREY:
                return False
            if st == WHITE:
                colour[id(c)] = GREY
                stack.append((c, iter(c.children())))
        return True

    def compile(self):
        """The straight-line program of include/ozk.h ("BACE programs"): (program int32 n_ops x 4, n_slots, constants).
        Every reachable gate is one record, in evaluation order, the result last; a slot is freed after the last
        record that reads it (liveness) and reused by later records."""
        if self._compiled is not None:
            return self._compiled
        order = _post_order(self.result_gate)
        column = {}
        for j, g in enumerate(self.input_gates):
            column[id(g)] = j   # (a gate listed twice takes its last column, as compute()'s loads do)
        last_use = {}
        for t, g in enumerate(order):
            for c in g.children():
                last_use[id(c)] = t
        consts, const_idx = [], {}
        slot_of, free, n_slots = {}, [], 0
        prog = np.zeros((len(order), 4), dtype=np.int32)
        for t, g in enumerate(order):
            if isinstance(g, InputGate):
                if id(g) not in column:
                    raise ValueError("input gate (index %d) is not in the circuit's input_gates" % g.index)
                rec = [OP_INPUT, 0, column[id(g)], 0]
            elif isinstance(g, ConstantGate):
                if g.value not in const_idx:
                    const_idx[g.value] = len(consts)
                    consts.append(g.value)
                rec = [OP_CONST, 0, const_idx[g.value], 0]
            else:
                rec = [OP_ADD if isinstance(g, SumGate) else OP_MUL, 0, slot_of[id(g.left)], slot_of[id(g.right)]]
                for c in {id(g.left), id(g.right)}:   # operands read for the last time: their slots are free again
                    if last_use[c] == t:
                        free.append(slot_of[c])
            if free:
                s = free.pop()
            else:
                s, n_slots = n_slots, n_slots + 1
            rec[1] = s
            slot_of[id(g)] = s
            prog[t] = rec
        self._compiled = (prog, n_slots, consts)
        return self._compiled


# ---------------------------------------------------------------------------------------------- device helpers
def _check_shape(circuit, num_inputs):
    n, N = circuit.input_size, int(num_inputs)
    if n <= 0:
        raise ValueError("the circuit has no input gates")
    if N <= 0 or N & (N - 1):
        raise ValueError("num_inputs = %d is not a power of two" % N)
    return n, N


def proof_size(circuit, num_inputs):
    """D = MathUtils.lowestPowerOfTwo(totalDegree * N) (Prover.computeProof), checked."""
    n, N = _check_shape(circuit, num_inputs)
    deg = circuit.total_degree()
    if deg <= 0:
        raise ValueError("a constant circuit (degree 0) has no proof: D = 1 < N")
    D = lowest_power_of_two(deg * N)
    if D > MAX_D:
        raise ValueError("D = %d exceeds 2^28, the 2-adicity of Fr" % D)
    return D


def _inputs_dev(inputs, count):
    if isinstance(inputs, torch.Tensor):
        if not (inputs.is_cuda and inputs.dtype == torch.uint8):
            raise TypeError("inputs must be a uint8 CUDA tensor or a list of ints")
        if inputs.numel() != count * 32:
            raise ValueError("inputs: %d bytes, expected %d values of 32 bytes" % (inputs.numel(), count))
        return inputs.contiguous().view(-1)
    inputs = list(inputs)
    if len(inputs) != count:
        raise ValueError("inputs: %d values, expected %d" % (len(inputs), count))
    return torch.from_numpy(np.frombuffer(le32(int(v) % FR for v in inputs), dtype=np.uint8).copy()).cuda()


def _program_args(circuit):
    prog, n_slots, consts = circuit.compile()
    cb = le32(c % FR for c in consts) if consts else b"\x00" * 32
    return np.ascontiguousarray(prog), n_slots, cb, len(consts)


# ---------------------------------------------------------------------------------------------- prover / verifier
class Prover:
    """bace.Prover(circuit, input, numInputs)."""

    def __init__(self, circuit, inputs, num_inputs):
        self.circuit = circuit
        self.n, self.N = _check_shape(circuit, num_inputs)
        self.D = proof_size(circuit, num_inputs)
        self.inputs = _inputs_dev(inputs, self.n * self.N)

    def compute_proof(self):
        """Prover.computeProof: (D, the D coefficients of R as a D x 32-byte uint8 CUDA tensor)."""
        L = _lib.load()
        prog, n_slots, cb, n_consts = _program_args(self.circuit)
        n_ops = prog.shape[0]
        wsb = int(L.ozk_bace_workspace_bytes(self.n, self.N, self.D, n_ops, n_slots, n_consts))
        if wsb == 0:
            raise ValueError("shape rejected: n = %d, N = %d, D = %d" % (self.n, self.N, self.D))
        ws = torch.empty(wsb, dtype=torch.uint8, device=self.inputs.device)
        proof = torch.empty(self.D * 32, dtype=torch.uint8, device=self.inputs.device)
        _lib.check(L.ozk_bace_prove_dev(_ptr(self.inputs), self.n, self.N, prog.ctypes.data, n_ops, n_slots, _vp(cb),
                                        n_consts, self.D, _ptr(proof), _ptr(ws), wsb, _stream()))
        return self.D, proof


class Verifier:
    """bace.Verifier(circuit, proof, input, numInputs); proof = (D, D x 32-byte tensor or list of ints)."""

    def __init__(self, circuit, proof, inputs, num_inputs):
        self.circuit = circuit
        self.n, self.N = _check_shape(circuit, num_inputs)
        D, coeffs = proof
        D = int(D)
        if D < self.N or D & (D - 1) or D > MAX_D:
            raise ValueError("proof size D = %d is not a power of two in [N, 2^28]" % D)
        self.D = D
        self.proof = _inputs_dev(coeffs, D)
        self.inputs = _inputs_dev(inputs, self.n * self.N)

    def columns_at(self, r):
        """beta_j(r) for every column j: a CUDA tensor of n x 32 bytes."""
        L = _lib.load()
        wsb = int(L.ozk_bace_workspace_bytes(self.n, self.N, self.N, 0, 0, 0))
        ws = torch.empty(wsb, dtype=torch.uint8, device=self.inputs.device)
        out = torch.empty(self.n * 32, dtype=torch.uint8, device=self.inputs.device)
        rb = (int(r) % FR).to_bytes(32, "little")
        _lib.check(L.ozk_bace_columns_at_dev(_ptr(self.inputs), self.n, self.N, _vp(rb), _ptr(out), _ptr(ws), wsb,
                                             _stream()))
        return out

    def claim(self, r):
        """The proof polynomial at r (NaiveEvaluation.parallelEvaluatePolynomial)."""
        return ints32(host_bytes(fr_poly_eval(self.proof, r)))[0]

    def verify_proof(self, seed=None, challenge=None):
        """Verifier.verifyProof: accept exactly when proof(r) == C(beta_1(r), ..., beta_n(r)), comparing field values
        (the Java compares object identity).  r = fr_random(seed) when a seed is given (reproduces the Java run; a
        prover who knows the seed can forge, so only for tests and replays), the exact `challenge` when given, else
        uniform from `secrets`."""
        if seed is not None and challenge is not None:
            raise ValueError("give a seed or a challenge, not both")
        if challenge is not None:
            r = int(challenge) % FR
        elif seed is not None:
            r = fr_random(seed)
        else:
            r = secrets.randbelow(FR)
        beta = self.columns_at(r)
        want = ints32(host_bytes(NaiveEvaluator._evaluate(self.circuit, beta, 1)))[0]
        return self.claim(r) == want

    def get_result(self):
        """Verifier.getResult: the proof evaluated at omega_N^i, i < N = C on instance i: an N x 32-byte tensor."""
        L = _lib.load()
        wsb = int(L.ozk_bace_workspace_bytes(1, self.N, self.N, 0, 0, 0))
        ws = torch.empty(wsb, dtype=torch.uint8, device=self.proof.device)
        out = torch.empty(self.N * 32, dtype=torch.uint8, device=self.proof.device)
        _lib.check(L.ozk_bace_result_dev(_ptr(self.proof), self.D, self.N, _ptr(out), _ptr(ws), wsb, _stream()))
        return out


class NaiveEvaluator:
    """bace.NaiveEvaluator(circuit, input, numInputs): the circuit on every instance row, one GPU lane per row."""

    def __init__(self, circuit, inputs, num_inputs):
        self.circuit = circuit
        self.n, self.N = _check_shape(circuit, num_inputs)
        self.inputs = _inputs_dev(inputs, self.n * self.N)

    @staticmethod
    def _evaluate(circuit, d_inputs, rows):
        L = _lib.load()
        prog, n_slots, cb, n_consts = _program_args(circuit)
        n_ops = prog.shape[0]
        wsb = int(L.ozk_bace_evaluate_workspace_bytes(rows, n_ops, n_slots, n_consts))
        ws = torch.empty(wsb, dtype=torch.uint8, device=d_inputs.device)
        out = torch.empty(rows * 32, dtype=torch.uint8, device=d_inputs.device)
        _lib.check(L.ozk_bace_evaluate_dev(_ptr(d_inputs), circuit.input_size, rows, prog.ctypes.data, n_ops, n_slots,
                                           _vp(cb), n_consts, _ptr(out), _ptr(ws), wsb, _stream()))
        return out

    def get_result(self):
        """NaiveEvaluator.getResult: an N x 32-byte tensor, C on instance i at record i."""
        return self._evaluate(self.circuit, self.inputs, self.N)
