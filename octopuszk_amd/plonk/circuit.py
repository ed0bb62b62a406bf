"""Circuits of the PLONK prover: gates over variables, host only."""
import numpy as np

from ..fft import FR, FR_MULT_GEN, root_of_unity

K = (1, FR_MULT_GEN, FR_MULT_GEN * FR_MULT_GEN)      # the cosets of the three wire columns' identity labels
N_MAX = 1 << 26                                      # the quotient's coset has 4 n <= 2^28 points


class Circuit:
    """n = 2^k >= 2 gates.  selectors: the five columns qL, qR, qO, qM, qC of n ints; wires: the three columns a, b, c of
    n variable numbers (two cells naming one variable are copy-constrained); the first n_public rows are the public
    inputs: qL = 1, every other selector 0, the input in column a."""

    def __init__(self, n, selectors, wires, n_public=0):
        n, n_public = int(n), int(n_public)
        if n < 2 or n & (n - 1) or n > N_MAX:
            raise ValueError("n = %d: a power of two in [2, 2^26]" % n)
        selectors, wires = [list(col) for col in selectors], [list(col) for col in wires]
        if len(selectors) != 5 or len(wires) != 3 or any(len(col) != n for col in selectors + wires):
            raise ValueError("five selector columns and three wire columns of n = %d rows" % n)
        if not 0 <= n_public <= n:
            raise ValueError("n_public = %d: at most n = %d" % (n_public, n))
        self.n, self.n_public = n, n_public
        self.selectors = [[int(v) % FR for v in col] for col in selectors]
        self.wires = [[int(v) for v in col] for col in wires]
        if any(v < 0 for col in self.wires for v in col):
            raise ValueError("a variable number is negative")
        self.n_vars = 1 + max(v for col in self.wires for v in col)
        self._index = None
        for i in range(n_public):
            if [col[i] for col in self.selectors] != [1, 0, 0, 0, 0]:
                raise ValueError("row %d is a public input: qL = 1 and every other selector 0" % i)

    def permutation(self):
        """sigma over the cells j n + i: the cells of one variable, in increasing order, form one cycle"""
        n = self.n
        cells = {}
        for j, col in enumerate(self.wires):
            for i, v in enumerate(col):
                cells.setdefault(v, []).append(j * n + i)
        sigma = [0] * (3 * n)
        for members in cells.values():
            for at, cell in enumerate(members):
                sigma[cell] = members[(at + 1) % len(members)]
        return sigma

    def sigma_labels(self):
        """the three rows s1, s2, s3: cell (j, i) carries the identity label k_j' omega^i' of the cell sigma maps it to"""
        n, powers = self.n, [1]
        omega = root_of_unity(n)
        for _ in range(n - 1):
            powers.append(powers[-1] * omega % FR)
        sigma = self.permutation()
        return [[K[sigma[j * n + i] // n] * powers[sigma[j * n + i] % n] % FR for i in range(n)] for j in range(3)]

    def checked_assignment(self, assignment):
        """one int in [0, r) per variable"""
        values = [int(v) for v in assignment]
        if len(values) != self.n_vars:
            raise ValueError("%d values for %d variables" % (len(values), self.n_vars))
        if any(not 0 <= v < FR for v in values):
            raise ValueError("a value does not lie in [0, r)")
        return values

    def wire_values(self, assignment):
        """the three columns of values under one Fr value per variable"""
        values = self.checked_assignment(assignment)
        return [[values[v] for v in col] for col in self.wires]

    def wire_index(self):
        """the three wire columns as one [3, n] index array, built once"""
        if self._index is None:
            self._index = np.array(self.wires, dtype=np.int64)
        return self._index


class LookupCircuit(Circuit):
    """A Circuit with one lookup table.  q_lookup: a column of n values in {0, 1}; table:
    1 <= n_table <= n rows (T1, T2, T3) of ints, taken mod r.  In a row with q_lookup = 1 the tuple (a, b, c) must be a
    row of the table; the row's arithmetic gate holds as in any other row."""

    def __init__(self, n, selectors, wires, n_public, q_lookup, table):
        super().__init__(n, selectors, wires, n_public)
        self.q_lookup = [int(v) for v in q_lookup]
        if len(self.q_lookup) != self.n or any(v not in (0, 1) for v in self.q_lookup):
            raise ValueError("q_lookup: n = %d values in {0, 1}" % self.n)
        rows = [tuple(row) for row in table]
        if not 1 <= len(rows) <= self.n:
            raise ValueError("the table has %d rows: at least 1 and at most n = %d" % (len(rows), self.n))
        if any(len(row) != 3 for row in rows):
            raise ValueError("a table row is three values")
        self.table = [tuple(int(v) % FR for v in row) for row in rows]
        self.n_table = len(self.table)

    def table_columns(self):
        """the three columns T1, T2, T3 of n values: the table, then its last row repeated"""
        rows = self.table + [self.table[-1]] * (self.n - self.n_table)
        return [[row[j] for row in rows] for j in range(3)]


class Builder:
    """Collects variables and gates; build() puts the public inputs first and pads with empty gates to a power of two.
    A variable used in several cells is copy-constrained by that alone.  table() and lookup() make it a circuit with
    lookups: build() then returns a LookupCircuit."""

    def __init__(self):
        self._n_vars, self._public, self._gates = 0, [], []
        self._table, self._lookups = None, set()

    def var(self) -> int:
        self._n_vars += 1
        return self._n_vars - 1

    def public(self) -> int:
        v = self.var()
        self._public.append(v)
        return v

    def _known(self, *vs):
        for v in vs:
            if not (isinstance(v, int) and 0 <= v < self._n_vars):
                raise ValueError("%r is no variable of this builder" % (v,))

    def gate(self, ql, qr, qo, qm, qc, a, b, c):
        """ql a + qr b + qo c + qm a b + qc = 0"""
        self._known(a, b, c)
        self._gates.append(((ql, qr, qo, qm, qc), (a, b, c)))

    def mul(self, x, y, out):
        self.gate(0, 0, -1, 1, 0, x, y, out)

    def add(self, x, y, out):
        self.gate(1, 1, -1, 0, 0, x, y, out)

    def constant(self, x, value):
        """x = value"""
        self.gate(1, 0, 0, 0, -int(value), x, x, x)

    def assert_equal(self, u, v):
        """u = v, as the gate u - v = 0"""
        self.gate(1, -1, 0, 0, 0, u, v, u)

    def table(self, rows):
        """the circuit's lookup table: rows of three ints, once per builder"""
        if self._table is not None:
            raise ValueError("the table is already set")
        rows = [tuple(int(v) for v in row) for row in rows]
        if not rows or any(len(row) != 3 for row in rows):
            raise ValueError("a table is at least one row of three values")
        self._table = rows

    def lookup(self, a, b, c):
        """(a, b, c) is a row of the table: a row with every selector 0"""
        if self._table is None:
            raise ValueError("lookup needs a table: call table(rows) first")
        self._known(a, b, c)
        self._lookups.add(len(self._gates))
        self._gates.append(((0, 0, 0, 0, 0), (a, b, c)))

    def build(self) -> Circuit:
        rows = [((1, 0, 0, 0, 0), (v, v, v)) for v in self._public] + self._gates
        if self._n_vars == 0:
            raise ValueError("a circuit needs a variable")
        n = 2
        while n < len(rows) or (self._table is not None and n < len(self._table)):
            n *= 2
        rows += [((0, 0, 0, 0, 0), (0, 0, 0))] * (n - len(rows))
        selectors, wires = [[q[k] for q, _ in rows] for k in range(5)], [[w[k] for _, w in rows] for k in range(3)]
        if self._table is None:
            circuit = Circuit(n, selectors, wires, len(self._public))
        else:
            q_lookup = [int(i - len(self._public) in self._lookups) for i in range(n)]
            circuit = LookupCircuit(n, selectors, wires, len(self._public), q_lookup, self._table)
        if circuit.n_vars != self._n_vars:
            raise ValueError("variable %d is in no gate" % circuit.n_vars)
        return circuit


class R1CSCircuit(Circuit):
    """The circuit that from_r1cs compiles of an R1CS.  Variables 0 .. num_variables - 1 are the
    R1CS's own, variable 0 the constant one; variable num_variables + t is the accumulator after position t of the term
    stream: term_index (T variable numbers) and term_coeff (T ints in [0, r), or None when every one is 1) hold the
    non-constant terms of every chained combination in row order, chain_start and chain_length where each chain lies
    in the stream.  The slot of a chain's first term is in no cell.  n_vars = num_variables + T."""

    def __init__(self, n, selectors, wires, n_public, num_variables, term_index, term_coeff, chain_start, chain_length):
        super().__init__(n, selectors, wires, n_public)
        self.num_variables = int(num_variables)
        self.term_index, self.term_coeff = list(term_index), None if term_coeff is None else list(term_coeff)
        self.chain_start, self.chain_length = list(chain_start), list(chain_length)
        self.n_vars = self.num_variables + len(self.term_index)

    def extend(self, full):
        """the n_vars values of an R1CS assignment (num_variables ints in [0, r), full[0] = 1): the assignment, then
        the running sum of every chain"""
        values = [int(v) for v in full]
        if len(values) != self.num_variables:
            raise ValueError("%d values for %d variables" % (len(values), self.num_variables))
        if any(not 0 <= v < FR for v in values):
            raise ValueError("a value does not lie in [0, r)")
        index, coeff = self.term_index, self.term_coeff
        for start, length in zip(self.chain_start, self.chain_length):
            acc = 0
            for t in range(start, start + length):
                acc = (acc + (values[index[t]] if coeff is None else coeff[t] * values[index[t]])) % FR
                values.append(acc)
        return values


def _column_terms(lc, nv):
    """(the number of rows, a function row -> its (index, coefficient) pairs) of one side of an R1CS"""
    ptr, index = [int(p) for p in lc.ptr], [int(v) for v in lc.index]
    value = None if lc.value is None else [int(c) % FR for c in lc.value]
    if not ptr or ptr[0] != 0 or ptr[-1] != len(index) or any(a > b for a, b in zip(ptr, ptr[1:])):
        raise ValueError("ptr does not split the %d terms into rows" % len(index))
    if value is not None and len(value) != len(index):
        raise ValueError("%d coefficients for %d terms" % (len(value), len(index)))
    if any(not 0 <= v < nv for v in index):
        raise ValueError("a term names a variable outside [0, %d)" % nv)
    return len(ptr) - 1, lambda i: [(index[t], 1 if value is None else value[t]) for t in range(ptr[i], ptr[i + 1])]


def from_r1cs(r1cs) -> R1CSCircuit:
    """An R1CS as a vanilla circuit.  r1cs has A, B, C with ptr, index, value (CSR; value None: every coefficient is
    one), num_inputs and num_auxiliary.  A term with index 0 contributes one whatever its coefficient, every other
    term coefficient * variable; terms are neither merged nor reordered.  With k index-0 terms and p others a
    combination is s x + k: s = 0 (p = 0), its one coefficient and variable (p = 1), or 1 and the last accumulator of
    a chain of p - 1 addition gates (qL = c_1 or 1, qR = c_j, qO = -1).  The constraint is then the one gate
    qM = sA sB, qL = sA kB, qR = sB kA, qO = -sC, qC = kA kB - kC over (xA, xB, xC).  Rows: the num_inputs public rows,
    then per constraint the chains of A, B, C and its gate, then empty gates to a power of two."""
    ni, nv = int(r1cs.num_inputs), int(r1cs.num_inputs) + int(r1cs.num_auxiliary)
    if not 0 <= ni <= nv or nv < 1:
        raise ValueError("num_inputs = %d of %d variables" % (ni, nv))
    sides = [_column_terms(lc, nv) for lc in (r1cs.A, r1cs.B, r1cs.C)]
    nc = sides[0][0]
    if any(rows != nc for rows, _ in sides):
        raise ValueError("A, B and C have %s rows" % ", ".join(str(rows) for rows, _ in sides))
    unit = all(lc.value is None for lc in (r1cs.A, r1cs.B, r1cs.C))
    sel, wires = [[1] * ni, [0] * ni, [0] * ni, [0] * ni, [0] * ni], [list(range(ni)) for _ in range(3)]
    term_index, term_coeff, chain_start, chain_length = [], [], [], []

    def gate(q, cells):
        for col, v in zip(sel, q):
            col.append(v)
        for col, v in zip(wires, cells):
            col.append(v)

    def normal_form(terms):
        """(s, x, k) with the combination = s x + k, after the chain gates it needs"""
        k = sum(1 for v, _ in terms if v == 0)
        rest = [(v, c) for v, c in terms if v != 0]
        if len(rest) < 2:
            return (rest[0][1], rest[0][0], k) if rest else (0, 0, k)
        start = len(term_index)
        chain_start.append(start)
        chain_length.append(len(rest))
        term_index.extend(v for v, _ in rest)
        term_coeff.extend(c for _, c in rest)
        gate((rest[0][1], rest[1][1], -1, 0, 0), (rest[0][0], rest[1][0], nv + start + 1))
        for j in range(2, len(rest)):
            gate((1, rest[j][1], -1, 0, 0), (nv + start + j - 1, rest[j][0], nv + start + j))
        return 1, nv + start + len(rest) - 1, k

    for i in range(nc):
        (sa, xa, ka), (sb, xb, kb), (sc, xc, kc) = (normal_form(terms(i)) for _, terms in sides)
        gate((sa * kb, sb * ka, -sc, sa * sb, ka * kb - kc), (xa, xb, xc))
        if len(sel[0]) > N_MAX:
            raise ValueError("the circuit has more than N_MAX = 2^26 rows")
    if nv + len(term_index) >= (1 << 32) - 1:
        raise ValueError("%d variables and %d chain terms: their sum must stay below 2^32 - 1" % (nv, len(term_index)))
    if len(sel[0]) > N_MAX:
        raise ValueError("the circuit has more than N_MAX = 2^26 rows")
    n = 2
    while n < len(sel[0]):
        n *= 2
    for _ in range(n - len(sel[0])):
        gate((0, 0, 0, 0, 0), (0, 0, 0))
    return R1CSCircuit(n, sel, wires, ni, nv, term_index, None if unit else term_coeff, chain_start, chain_length)
