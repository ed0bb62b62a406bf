"""Exact-integer model of the PLONK prover and verifier with one lookup table, on top of
tests/plonk_ref.py: the multiplicities of a witness against a table with the first-occurrence rule, the running sum
of fractions with its zero-denominator rule, the quotient with the two lookup terms pointwise on the coset, setup, the
prover with a known tau (and three ways to cheat), the transcript, the bytes, and the verifier in the exponent and on
bytes alone.  Written from the scheme's description (Haboeck, "Multivariate lookups based on logarithmic derivatives",
in its univariate running-sum form), not from octopuszk_amd/plonk or csrc/plonk_lookup.cuh, which the tests compare
with it."""
import hashlib

import kzg_multi_ref as km
import kzg_ref as kr
import plonk_ref as pm

R = pm.R
KS = pm.KS
inv = pm.inv
TAGS = {name: b"OZK-plookup-" + name for name in (b"beta", b"gamma", b"eta", b"theta", b"alpha", b"z")}
PROOF_BYTES = 9 * 32 + 23 * 32 + 64
VK_BYTES = 8 + 12 * 32
MISSING_NONE = 0x7fffffff


# ---------------------------------------------------------------------------- the kernels
def multiplicities(wires, qk, table, m_len):
    """(m of m_len counts, the number of rows with qK != 0 whose tuple is in no table row, the first of them or
    MISSING_NONE).  table: n_rows tuples; a tuple that several rows hold is counted at the FIRST of them; values are
    compared mod r."""
    first = {}
    for i, row in enumerate(table):
        first.setdefault(tuple(v % R for v in row), i)
    m, missing, first_missing = [0] * m_len, 0, MISSING_NONE
    for i, sel in enumerate(qk):
        if sel % R == 0:
            continue
        at = first.get(tuple(col[i] % R for col in wires))
        if at is None:
            missing += 1
            first_missing = min(first_missing, i)
        else:
            m[at] += 1
    return m, missing, first_missing


def batch_inverses(values):
    """1 / v for every nonzero v, 0 for zero: one modular inversion"""
    prefix, run = [], 1
    for v in values:
        prefix.append(run)
        if v % R:
            run = run * v % R
    back, out = inv(run), [0] * len(values)
    for i in range(len(values) - 1, -1, -1):
        if values[i] % R:
            out[i] = back * prefix[i] % R
            back = back * values[i] % R
    return out


def lookup_sum(wires, key4, m, eta, theta):
    """(S with S[0] = 0, the sum over all rows, the number of zero denominators among the 2 len): a fraction whose
    denominator is zero counts as 0.  key4: the rows qK, T1, T2, T3."""
    qk, t1, t2, t3 = key4
    length = len(qk)
    dt = [(theta + t1[i] + eta * t2[i] + eta * eta * t3[i]) % R for i in range(length)]
    df = [(theta + wires[0][i] + eta * wires[1][i] + eta * eta * wires[2][i]) % R for i in range(length)]
    it, jf = batch_inverses(dt), batch_inverses(df)
    s, acc = [], 0
    for i in range(length):
        s.append(acc)
        acc = (acc + m[i] * it[i] - qk[i] * jf[i]) % R
    return s, acc, sum(1 for v in dt + df if v == 0)


def quotient_on_coset(wit, key, n, alpha, beta, gamma, eta, theta, ks, zh_inv):
    """t at the 4 n points of the coset from the rows a, b, c, Z, PI, m, S and qL .. s3, L_1, x, qK, T1, T2, T3"""
    a, b, c, _, _, m, s = wit
    l1, qk, t1, t2, t3 = key[8], key[10], key[11], key[12], key[13]
    vanilla = pm.quotient_on_coset(wit[:5], key[:10], n, alpha, beta, gamma, ks, [1] * 4)
    out = []
    for i in range(4 * n):
        df = theta + a[i] + eta * b[i] + eta * eta * c[i]
        dt = theta + t1[i] + eta * t2[i] + eta * eta * t3[i]
        lk1 = (s[(i + 4) % (4 * n)] - s[i]) * dt * df - m[i] * df + qk[i] * dt
        lk2 = s[i] * l1[i]
        out.append((vanilla[i] + alpha ** 3 * lk1 + alpha ** 4 * lk2) * zh_inv[i % 4] % R)
    return out


# ---------------------------------------------------------------------------- circuits
class LookupCircuit(pm.Circuit):
    """a Circuit plus the selector column q_lookup and a table of 1 <= n_table <= n rows (T1, T2, T3)"""

    def __init__(self, n, selectors, wires, n_public, q_lookup, table):
        super().__init__(n, selectors, wires, n_public)
        self.q_lookup, self.table = list(q_lookup), [tuple(v % R for v in row) for row in table]
        assert 1 <= len(self.table) <= n and len(self.q_lookup) == n

    def table_columns(self):
        rows = self.table + [self.table[-1]] * (self.n - len(self.table))
        return [[row[j] for row in rows] for j in range(3)]

    def key4(self):
        return [list(self.q_lookup)] + self.table_columns()


def chain_with_lookups(n, n_public, rng, table, lookups):
    """(circuit, assignment) of n rows: plonk_ref.chain over the first n / 2 rows, then `lookups` rows that each look
    a random table row up through three fresh variables (every third reuses the variables of the row before it), then
    padding"""
    base, values = pm.chain(n // 2, n_public, rng, constant=n // 2 >= 4)
    assert lookups <= n // 2
    sel, wires = [list(col) for col in base.selectors], [list(col) for col in base.wires]
    qk = [0] * (n // 2)
    last = None
    for k in range(lookups):
        if k % 3 == 2 and last is not None:
            cells = last
        else:
            row = table[rng.randrange(len(table))]
            cells = tuple(range(len(values), len(values) + 3))
            values += [v % R for v in row]
        last = cells
        for col in sel:
            col.append(0)
        for col, v in zip(wires, cells):
            col.append(v)
        qk.append(1)
    while len(qk) < n:
        for col in sel:
            col.append(0)
        for col in wires:
            col.append(0)
        qk.append(0)
    return LookupCircuit(n, sel, wires, n_public, qk, table), values


def key_polys(circuit):
    """the twelve coefficient rows qL, qR, qO, qM, qC, s1, s2, s3, qK, T1, T2, T3"""
    omega = kr.root(circuit.n)
    return pm.key_polys(circuit) + [kr.intt([v % R for v in row], omega) for row in circuit.key4()]


# ---------------------------------------------------------------------------- the protocol in the exponent
def setup(circuit, tau):
    polys = key_polys(circuit)
    logs = [kr.horner(p, tau) for p in polys]
    encs = [pm.enc(v) for v in logs]
    return {"polys": polys, "logs": logs, "commitments": encs, "vk": pm.vk_bytes(circuit, encs)}


def _c128(d):
    return int.from_bytes(d[:16], "little") or 1


def challenges(vk, public, abcm, zs_commits=None, t_commits=None):
    """(beta, gamma, eta, theta[, alpha[, z]]): D1 = SHA-256("OZK-plookup-beta" | vk | public inputs | [a] [b] [c] [m]),
    beta from D1, gamma, eta, theta from SHA-256(their tag | D1), alpha from D2 = SHA-256("OZK-plookup-alpha" | D1 | [Z]
    [S]), z from SHA-256("OZK-plookup-z" | D2 | [t_lo] [t_mid] [t_hi])"""
    d1 = hashlib.sha256(TAGS[b"beta"] + vk + b"".join(kr.le(x) for x in public) + b"".join(abcm)).digest()
    out = [_c128(d1)] + [_c128(hashlib.sha256(TAGS[name] + d1).digest()) for name in (b"gamma", b"eta", b"theta")]
    if zs_commits is not None:
        d2 = hashlib.sha256(TAGS[b"alpha"] + d1 + b"".join(zs_commits)).digest()
        out.append(_c128(d2))
        if t_commits is not None:
            out.append(_c128(hashlib.sha256(TAGS[b"z"] + d2 + b"".join(t_commits)).digest()))
    return tuple(out)


def quotient(circuit, key_coeffs, wire_coeffs, z_coeffs, m_coeffs, s_coeffs, public, alpha, beta, gamma, eta, theta):
    """the 4 n coefficients of the quotient through the coset of 4 n points"""
    n = circuit.n
    w4 = kr.root(4 * n)
    pi = kr.intt(pm.pi_evals(n, public), kr.root(n))
    extra = [[inv(n)] * n, [0, 1] + [0] * (n - 2)]
    rows = wire_coeffs + [z_coeffs, pi, m_coeffs, s_coeffs] + key_coeffs[:8] + extra + key_coeffs[8:]
    on = [kr.ntt(row, w4) for row in pm.rows_coset(rows, pm.G, 1, 4 * n)]
    t = quotient_on_coset(on[:7], on[7:], n, alpha, beta, gamma, eta, theta, KS, pm.zh_inverses(n))
    return pm.rows_coset([kr.intt(t, w4)], inv(pm.G), 1)[0]


def sets_of(n, z):
    return [[z]] * 19 + [[z, z * kr.root(n) % R]] * 2


def prove(circuit, assignment, tau, st=None, tamper=None):
    """The prover with a known tau; a dict as plonk_ref.prove returns.  tamper: None, or one way to cheat, each proved
    as far as an honest opening of what was committed goes (t keeps its low 3 n coefficients):
      "tuple"  the first lookup row holds a tuple that is in no table row, and m is the honest one's (forced)
      "m"      m is one too high at the row of the first lookup
      "S"      S is shifted by the constant 1"""
    st = st or setup(circuit, tau)
    n, omega = circuit.n, kr.root(circuit.n)
    public = circuit.public_inputs(assignment)
    wires = circuit.wire_values(assignment)
    key4 = circuit.key4()
    m, missing, _ = multiplicities(wires, key4[0], circuit.table, n)
    assert missing == 0
    at = key4[0].index(1)
    if tamper == "tuple":
        # the variables of that row are in lookup rows only; every cell of them moves, so the copy constraints hold
        moved = {circuit.wires[j][at] for j in range(3)}
        assignment = [(v + 1) % R if k in moved else v for k, v in enumerate(assignment)]
        wires = circuit.wire_values(assignment)
        assert multiplicities(wires, key4[0], circuit.table, n)[1] > 0
    if tamper == "m":
        m = list(m)
        m[multiplicities([[col[at]] for col in wires], [1], circuit.table, n)[0].index(1)] += 1
    wire_coeffs = [kr.intt(col, omega) for col in wires]
    m_coeffs = kr.intt(m, omega)
    logs = [kr.horner(p, tau) for p in wire_coeffs + [m_coeffs]]
    abcm = [pm.enc(v) for v in logs]
    beta, gamma, eta, theta = challenges(st["vk"], public, abcm)
    zs, total, zeros = pm.perm_product(wires, pm.sigma_labels(circuit), omega, KS, beta, gamma)
    ss, s_total, s_zeros = lookup_sum(wires, key4, m, eta, theta)
    if tamper == "S":
        ss = [(v + 1) % R for v in ss]
    z_coeffs, s_coeffs = kr.intt(zs, omega), kr.intt(ss, omega)
    logs += [kr.horner(z_coeffs, tau), kr.horner(s_coeffs, tau)]
    zs_commits = [pm.enc(v) for v in logs[4:6]]
    alpha = challenges(st["vk"], public, abcm, zs_commits)[4]
    t = quotient(circuit, st["polys"], wire_coeffs, z_coeffs, m_coeffs, s_coeffs, public, alpha, beta, gamma, eta, theta)
    parts = [t[:n], t[n:2 * n], t[2 * n:3 * n]]
    logs += [kr.horner(p, tau) for p in parts]
    t_commits = [pm.enc(v) for v in logs[6:9]]
    z = challenges(st["vk"], public, abcm, zs_commits, t_commits)[5]
    rows = wire_coeffs + [m_coeffs] + parts + st["polys"] + [z_coeffs, s_coeffs]
    commitments = abcm + t_commits + st["commitments"] + zs_commits
    multi = km.prove(rows, sets_of(n, z), tau, commitments)
    values = [v for row in multi["values"] for v in row]
    proof = b"".join(abcm + zs_commits + t_commits) + b"".join(kr.le(v) for v in values) + multi["w"] + multi["w2"]
    return {"bytes": proof, "commitments": abcm + zs_commits + t_commits, "values": values, "w": multi["w"],
            "w2": multi["w2"], "logs": logs + [multi["w_log"], multi["w2_log"]], "beta": beta, "gamma": gamma, "eta": eta,
            "theta": theta, "alpha": alpha, "z": z, "total": total, "zeros": zeros, "s_total": s_total, "s_zeros": s_zeros,
            "t": t, "m": m, "s": ss, "public": public, "assignment": assignment}


def parse_proof(b):
    assert len(b) == PROOF_BYTES
    return [b[32 * i:32 * i + 32] for i in range(9)], kr.ints(b[288:1024]), b[1024:1056], b[1056:]


def identity_holds(n, public, values, beta, gamma, eta, theta, alpha, z) -> bool:
    """the identity with the two lookup terms on the 23 opened values"""
    a, b, c, m, t_lo, t_mid, t_hi, ql, qr, qo, qm, qc, s1, s2, s3, qk, t1, t2, t3, zz, zw, ss, sw = values
    zn = pow(z, n, R)
    if zn == 1:
        return False
    omega = kr.root(n)
    lag = [pow(omega, i, R) * (zn - 1) * inv(n * (z - pow(omega, i, R))) % R for i in range(max(1, len(public)))]
    pi = -sum(x * l for x, l in zip(public, lag)) % R
    gate = ql * a + qr * b + qo * c + qm * a * b + qc + pi
    p1 = (zz * (a + beta * z + gamma) * (b + beta * KS[1] * z + gamma) * (c + beta * KS[2] * z + gamma)
          - zw * (a + beta * s1 + gamma) * (b + beta * s2 + gamma) * (c + beta * s3 + gamma))
    p2 = (zz - 1) * lag[0]
    df = theta + a + eta * b + eta * eta * c
    dt = theta + t1 + eta * t2 + eta * eta * t3
    lk1 = (sw - ss) * dt * df - m * df + qk * dt
    lk2 = ss * lag[0]
    t = t_lo + zn * t_mid + zn * zn * t_hi
    return (gate + alpha * p1 + alpha ** 2 * p2 + alpha ** 3 * lk1 + alpha ** 4 * lk2 - t * (zn - 1)) % R == 0


def _statement(vk, public, proof):
    """(n, the challenges, the multi-opening's commitments, sets and rows) of a parsed proof"""
    n = int.from_bytes(vk[:4], "little")
    cs, values, w, w2 = proof
    ch = challenges(vk, public, cs[:4], cs[4:6], cs[6:])
    key = [vk[8 + 32 * i:40 + 32 * i] for i in range(12)]
    commitments = cs[:4] + cs[6:] + key + cs[4:6]
    rows = [[v] for v in values[:19]] + [values[19:21], values[21:]]
    return n, ch, commitments, sets_of(n, ch[5]), rows


def verify_exponent(st, circuit, public, proof, tau) -> bool:
    """the verifier where every point is known by its logarithm (proof: the dict of prove())"""
    if len(public) != circuit.n_public or any(not 0 <= v < R for v in proof["values"]):
        return False
    parsed = (proof["commitments"], proof["values"], proof["w"], proof["w2"])
    n, ch, commitments, sets, rows = _statement(st["vk"], public, parsed)
    if not identity_holds(n, public, proof["values"], *ch):
        return False
    logs = proof["logs"]
    row_logs = logs[:4] + logs[6:9] + st["logs"] + logs[4:6]
    w_log, w2_log = logs[9], logs[10]
    g, u = km.challenges(commitments, sets, rows, proof["w"])
    weights, total, z_t = km.at_z(sets, rows, g, u)
    f = (sum(wt * c for wt, c in zip(weights, row_logs)) - total - z_t * w_log) % R
    return (f + u * w2_log - tau * w2_log) % R == 0


def verify_bytes(vk, public, proof: bytes, g1, g2, tau_g2) -> bool:
    """the verifier on bytes alone, over the model pairing"""
    if len(vk) != VK_BYTES or len(proof) != PROOF_BYTES:
        return False
    n_public = int.from_bytes(vk[4:8], "little")
    parsed = parse_proof(proof)
    if len(public) != n_public or any(v >= R for v in parsed[1]):
        return False
    n, ch, commitments, sets, rows = _statement(vk, public, parsed)
    if not identity_holds(n, public, parsed[1], *ch):
        return False
    return km.verify(g1, g2, tau_g2, km.opening_bytes(commitments, sets, rows, parsed[2], parsed[3]))
