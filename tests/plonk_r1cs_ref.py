"""Exact-integer model of the import of an R1CS into PLONK, beside tests/plonk_ref.py: the
semantics of a linear combination (a term with index 0 contributes one whatever its coefficient), a second compiler
written from the section's normal form and row order, the two kernels of csrc/plonk_r1cs.cuh on host integers (the
running sums of a term stream, the gather of the wires from cell descriptors), and the R1CS the tests share: twelve
constraints over nine variables with every shape of combination, and a witness that satisfies it.  Written from the
description, not from octopuszk_amd/plonk/circuit.py, which the tests compare with it."""
import random

import numpy as np

import plonk_ref as pm

R = pm.R
MONT_R = 1 << 261          # a coefficient of the term stream is stored as c MONT_R mod r
NONE = 0xFFFFFFFF


# ---------------------------------------------------------------------------- linear combinations
class Side:
    """one of A, B, C in CSR form, as zksnark.LinearCombinations holds it"""

    def __init__(self, rows, unit=False):
        """rows: a list of rows of (index, coefficient); unit: value is None (every coefficient must be 1)"""
        self.ptr = np.cumsum([0] + [len(row) for row in rows]).astype(np.int64)
        self.index = np.array([v for row in rows for v, _ in row], dtype=np.int64)
        self.value = None if unit else np.array([c for row in rows for _, c in row] + [None], dtype=object)[:-1]
        self.terms = [list(row) for row in rows]


class Relation:
    def __init__(self, a, b, c, num_inputs, num_auxiliary):
        self.A, self.B, self.C = a, b, c
        self.num_inputs, self.num_auxiliary = num_inputs, num_auxiliary
        self.num_variables = num_inputs + num_auxiliary
        self.num_constraints = len(a.terms)


def lc_value(terms, w):
    return sum(1 if v == 0 else c * w[v] for v, c in terms) % R


def constraint_holds(rel, i, w):
    return (lc_value(rel.A.terms[i], w) * lc_value(rel.B.terms[i], w) - lc_value(rel.C.terms[i], w)) % R == 0


# ---------------------------------------------------------------------------- the shared R1CS
NV, NI, LONG = 9, 3, 70     # LONG: past the 64 terms at which the Groth16 side's CSR kernels change path


def mixed_relation(seed=3600):
    """(relation, a full assignment that satisfies it): 12 constraints over 9 variables with explicit coefficients.
    Empty, single-term and constant-only combinations, index-0 terms with a coefficient other than 1, a variable
    repeated inside one combination and one combination of LONG terms; C ends on a term whose coefficient makes the
    constraint hold under the assignment."""
    rng = random.Random(seed)
    w = [1] + [rng.randrange(1, R) for _ in range(NV - 1)]
    term = lambda: (rng.randrange(1, NV), rng.randrange(R))
    shapes = [
        ([], [term(), term(), term()], None),                                     # 0 = 0: A and C are empty
        ([term()], [(0, 5)], []),                                                 # one term times a constant alone
        ([(0, 7), (0, 1)], [term()], [term(), (0, 9), term()]),                   # constants whose coefficients are not 1
        ([(4, rng.randrange(R)), (4, rng.randrange(R)), (6, 3)], [(0, 3), term()], [term()]),   # variable 4 twice
        ([term() if j % 9 else (0, j) for j in range(LONG)], [term()], [(0, 2)]),  # 70 terms, index 0 among them
    ]
    while len(shapes) < 12:
        a = [term() for _ in range(rng.randrange(5))] + [(0, rng.randrange(R)) for _ in range(rng.randrange(3))]
        b = [term() for _ in range(rng.randrange(4))]
        rng.shuffle(a)
        shapes.append((a, b, [term() for _ in range(rng.randrange(4))]))
    rows = [[], [], []]
    for a, b, c in shapes:
        if c is None:
            c = []
        else:
            v = rng.randrange(1, NV)
            c = c + [(v, (lc_value(a, w) * lc_value(b, w) - lc_value(c, w)) * pm.inv(w[v]) % R)]
        for side, terms in zip(rows, (a, b, c)):
            side.append(terms)
    rel = Relation(Side(rows[0]), Side(rows[1]), Side(rows[2]), NI, NV - NI)
    assert all(constraint_holds(rel, i, w) for i in range(12))
    return rel, w


# ---------------------------------------------------------------------------- the compiler, a second time
def compile_rows(rel):
    """(rows as ((qL, qR, qO, qM, qC), (a, b, c)) before padding, the term stream as (index, coefficient, chain start))
    by the normal form of section 36"""
    nv, rows, stream = rel.num_variables, [], []
    for v in range(rel.num_inputs):
        rows.append(((1, 0, 0, 0, 0), (v, v, v)))
    for i in range(rel.num_constraints):
        forms = []
        for side in (rel.A, rel.B, rel.C):
            terms = side.terms[i]
            k = sum(1 for v, _ in terms if v == 0)
            rest = [(v, c % R) for v, c in terms if v != 0]
            if not rest:
                forms.append((0, 0, k))
            elif len(rest) == 1:
                forms.append((rest[0][1], rest[0][0], k))
            else:
                t0 = len(stream)
                stream += [(v, c, t0) for v, c in rest]
                for j in range(1, len(rest)):
                    left = (rest[0][1], rest[0][0]) if j == 1 else (1, nv + t0 + j - 1)
                    rows.append(((left[0], rest[j][1], R - 1, 0, 0), (left[1], rest[j][0], nv + t0 + j)))
                forms.append((1, nv + t0 + len(rest) - 1, k))
        (sa, xa, ka), (sb, xb, kb), (sc, xc, kc) = forms
        rows.append(((sa * kb % R, sb * ka % R, -sc % R, sa * sb % R, (ka * kb - kc) % R), (xa, xb, xc)))
    return rows, stream


def padded(rows):
    n = 2
    while n < len(rows):
        n *= 2
    return n, rows + [((0, 0, 0, 0, 0), (0, 0, 0))] * (n - len(rows))


def model_circuit(rel):
    """the compiled circuit as a plonk_ref.Circuit"""
    n, rows = padded(compile_rows(rel)[0])
    return pm.Circuit(n, [[q[k] for q, _ in rows] for k in range(5)], [[w[k] for _, w in rows] for k in range(3)],
                      rel.num_inputs)


def extend(rel, w):
    """the assignment, then the accumulator after every position of the term stream"""
    out, acc = list(w), 0
    for t, (v, c, t0) in enumerate(compile_rows(rel)[1]):
        acc = (0 if t == t0 else acc) + c * w[v]
        out.append(acc % R)
    return out


def gate_holds(q, cells, values):
    a, b, c = (values[v] for v in cells)
    return (q[0] * a + q[1] * b + q[2] * c + q[3] * a * b + q[4]) % R == 0


# ---------------------------------------------------------------------------- the two kernels
def term_sums(index, coeff_words, vec_words, n_vec):
    """(the inclusive running sums, the number of indices >= n_vec) over words as written: a coefficient word stands
    for (word mod r) / MONT_R, an index >= n_vec for a zero term"""
    unmont = pm.inv(MONT_R)
    out, acc, bad = [], 0, 0
    for t, v in enumerate(index):
        if v >= n_vec:
            bad += 1
        else:
            c = 1 if coeff_words is None else coeff_words[t] % R * unmont
            acc = (acc + c * (vec_words[v] % R)) % R
        out.append(acc)
    return out, bad


def wires(src_words, cells):
    """(rows of src[hi] - src[lo], or src[hi] where lo is NONE; the number of descriptors pointing outside src, whose
    cells are zero)"""
    n_src, bad, out = len(src_words), 0, []
    for row in cells:
        new = []
        for hi, lo in row:
            if hi >= n_src or (lo != NONE and lo >= n_src):
                bad += 1
                new.append(0)
            else:
                new.append((src_words[hi] - (0 if lo == NONE else src_words[lo])) % R)
        out.append(new)
    return out, bad
