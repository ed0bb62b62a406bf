"""Exact-integer model of the PLONK prover and verifier, on top of tests/kzg_ref.py and
tests/kzg_multi_ref.py: the three kernels in host integers (rows by the powers of a coset shift, the permutation grand
product with its zero-denominator rule, the quotient pointwise on the coset), the prover with a known tau (every
commitment is [p(tau)] g1, kept beside its logarithm), the transcript, the bytes of proof and verifying key, and the
verifier twice: in the exponent, where the pairing check is an identity of scalars, and over the model pairing on the
bytes alone.  Written from the scheme's description (Gabizon, Williamson, Ciobotaru, without the linearisation
polynomial and without blinding), not from octopuszk_amd/plonk or csrc/plonk.cuh, which the tests compare with it."""
import hashlib

import codec_ref as ref
import kzg_multi_ref as km
import kzg_ref as kr
from oracle import bn254 as o

R = o.R
G = 5                                   # the multiplicative generator: coset shift, and k1 = G, k2 = G^2
KS = (1, G, G * G)
BETA_TAG, GAMMA_TAG, ALPHA_TAG, Z_TAG = b"OZK-plonk-beta", b"OZK-plonk-gamma", b"OZK-plonk-alpha", b"OZK-plonk-z"
PROOF_BYTES = 7 * 32 + 16 * 32 + 64


def inv(v):
    return pow(v % R, -1, R)


# ---------------------------------------------------------------------------- the three kernels
def rows_coset(rows, s, c, out_len=None):
    """out[y][i] = c s^i rows[y][i], zero up to out_len"""
    out = []
    for row in rows:
        length = len(row) if out_len is None else out_len
        acc, new = c % R, []
        for v in row:
            new.append(v * acc % R)
            acc = acc * s % R
        out.append(new + [0] * (length - len(row)))
    return out


def perm_product(wires, sigma, omega, ks, beta, gamma):
    """(z with z[0] = 1, the product over all rows, the number of rows with a zero denominator): a row whose
    denominator is zero has the factor 1.  The nonzero denominators are inverted together (one modular inversion and
    three products a row), which is exact and keeps long rows quick."""
    length = len(wires[0])
    nums, dens, x = [], [], 1
    for i in range(length):
        num = den = 1
        for j in range(3):
            num = num * (wires[j][i] + beta * ks[j] * x + gamma) % R
            den = den * (wires[j][i] + beta * sigma[j][i] + gamma) % R
        nums.append(num)
        dens.append(den)
        x = x * omega % R
    prefix, run = [], 1
    for den in dens:
        prefix.append(run)
        if den:
            run = run * den % R
    back, invs = inv(run), [0] * length
    for i in range(length - 1, -1, -1):
        if dens[i]:
            invs[i] = back * prefix[i] % R
            back = back * dens[i] % R
    z, acc, zeros = [], 1, 0
    for num, den, di in zip(nums, dens, invs):
        z.append(acc)
        if den == 0:
            zeros += 1
        else:
            acc = acc * num % R * di % R
    return z, acc, zeros


def quotient_on_coset(wit, key, n, alpha, beta, gamma, ks, zh_inv):
    """t at the 4 n points of the coset from the rows a, b, c, Z, PI and qL, qR, qO, qM, qC, s1, s2, s3, L_1, x"""
    a, b, c, zz, pi = wit
    ql, qr, qo, qm, qc, s1, s2, s3, l1, xs = key
    out = []
    for i in range(4 * n):
        x = xs[i]
        gate = ql[i] * a[i] + qr[i] * b[i] + qo[i] * c[i] + qm[i] * a[i] * b[i] + qc[i] + pi[i]
        p1 = (zz[i] * (a[i] + beta * ks[0] * x + gamma) * (b[i] + beta * ks[1] * x + gamma) * (c[i] + beta * ks[2] * x + gamma)
              - zz[(i + 4) % (4 * n)] * (a[i] + beta * s1[i] + gamma) * (b[i] + beta * s2[i] + gamma)
              * (c[i] + beta * s3[i] + gamma))
        p2 = (zz[i] - 1) * l1[i]
        out.append((gate + alpha * p1 + alpha * alpha * p2) * zh_inv[i % 4] % R)
    return out


def zh_inverses(n):
    """1 / (g^n i4^m - 1), m < 4, for i4 = omega_4n^n"""
    i4 = pow(kr.root(4 * n), n, R)
    return [inv(pow(G, n, R) * pow(i4, m, R) - 1) for m in range(4)]


# ---------------------------------------------------------------------------- circuits
class Circuit:
    """n = 2^k gates: five selector columns and three columns of variable numbers; the first n_public rows are the
    public inputs (qL = 1, the input in column a)"""

    def __init__(self, n, selectors, wires, n_public):
        self.n, self.selectors, self.wires, self.n_public = n, [list(s) for s in selectors], [list(w) for w in wires], n_public

    def wire_values(self, assignment):
        return [[assignment[v] % R for v in col] for col in self.wires]

    def public_inputs(self, assignment):
        return [assignment[v] % R for v in self.wires[0][:self.n_public]]


def sigma_labels(circuit, omega=None):
    """The three label rows of the permutation: the cells of one variable, in the order of j n + i, form one cycle,
    each cell carrying the identity label of the next.  omega: the domain's generator unless given (any element whose
    first n powers differ serves a grand product)"""
    n = len(circuit.wires[0])
    omega = kr.root(n) if omega is None else omega
    cells = {}
    for j in range(3):
        for i in range(n):
            cells.setdefault(circuit.wires[j][i], []).append((j, i))
    powers = [1]
    for _ in range(n - 1):
        powers.append(powers[-1] * omega % R)
    rows = [[0] * n for _ in range(3)]
    for members in cells.values():
        for at, (j, i) in enumerate(members):
            nj, ni = members[(at + 1) % len(members)]
            rows[j][i] = KS[nj] * powers[ni] % R
    return rows


def key_polys(circuit):
    """the eight coefficient rows qL, qR, qO, qM, qC, s1, s2, s3"""
    omega = kr.root(circuit.n)
    return [kr.intt([v % R for v in row], omega) for row in circuit.selectors + sigma_labels(circuit)]


def chain(n, n_public, rng, shared=True, constant=True):
    """(circuit, assignment) of n gates: the public inputs, then a chain of multiplications and additions in which one
    variable (the first public input) feeds many gates, a gate with a constant, and padding rows"""
    values = [rng.randrange(R) for _ in range(n_public)]
    sel, wires = [[] for _ in range(5)], [[], [], []]

    def gate(q, a, b, c):
        for col, v in zip(sel, q):
            col.append(v % R)
        for col, v in zip(wires, (a, b, c)):
            col.append(v)

    for v in range(n_public):
        gate((1, 0, 0, 0, 0), v, v, v)
    prev = 0
    body = n - n_public - (2 if constant else 0) - 1
    for k in range(body):
        other = 0 if shared and k % 3 == 0 else prev
        new = len(values)
        if k % 2:
            values.append(values[prev] * values[other] % R)
            gate((0, 0, -1, 1, 0), prev, other, new)
        else:
            values.append((values[prev] + values[other]) % R)
            gate((1, 1, -1, 0, 0), prev, other, new)
        prev = new
    if constant:
        new = len(values)
        values.append((3 * values[prev] + 7) % R)                       # 3 prev + 7 - new = 0
        gate((3, 0, -1, 0, 7), prev, prev, new)
        values.append(11)                                               # new2 = 11: a constant alone
        gate((0, 0, -1, 0, 11), new, new, new + 1)
    while len(sel[0]) < n:
        gate((0, 0, 0, 0, 0), 0, 0, 0)
    return Circuit(n, sel, wires, n_public), values


# ---------------------------------------------------------------------------- the protocol in the exponent
def enc(log):
    return ref.encode_g1(kr.g1_mul(o.G1.one, log))


def vk_bytes(circuit, commitments) -> bytes:
    return circuit.n.to_bytes(4, "little") + circuit.n_public.to_bytes(4, "little") + b"".join(commitments)


def setup(circuit, tau):
    polys = key_polys(circuit)
    logs = [kr.horner(p, tau) for p in polys]
    encs = [enc(v) for v in logs]
    return {"polys": polys, "logs": logs, "commitments": encs, "vk": vk_bytes(circuit, encs)}


def _c128(d):
    return int.from_bytes(d[:16], "little") or 1


def challenges(vk, public, abc, z_commit=None, t_commits=None):
    """(beta, gamma[, alpha[, z]]): beta is drawn from D1 = SHA-256("OZK-plonk-beta" | the verifying key | the public
    inputs | [a] [b] [c]), gamma from SHA-256("OZK-plonk-gamma" | D1), alpha from D2 = SHA-256("OZK-plonk-alpha" | D1 |
    [Z]) and z from SHA-256("OZK-plonk-z" | D2 | [t_lo] [t_mid] [t_hi]); each is the first 16 bytes, little-endian, 1
    if they are zero"""
    d1 = hashlib.sha256(BETA_TAG + vk + b"".join(kr.le(x) for x in public) + b"".join(abc)).digest()
    out = [_c128(d1), _c128(hashlib.sha256(GAMMA_TAG + d1).digest())]
    if z_commit is not None:
        d2 = hashlib.sha256(ALPHA_TAG + d1 + z_commit).digest()
        out.append(_c128(d2))
        if t_commits is not None:
            out.append(_c128(hashlib.sha256(Z_TAG + d2 + b"".join(t_commits)).digest()))
    return tuple(out)


def pi_evals(n, public):
    return [(-x) % R for x in public] + [0] * (n - len(public))


def poly_mul(a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % R
    return out


def quotient(circuit, key_coeffs, wire_coeffs, z_coeffs, public, alpha, beta, gamma):
    """the 4 n coefficients of (gate + alpha P1 + alpha^2 P2) / Z_H through the coset of 4 n points; the top n are
    zero exactly when Z_H divides the numerator"""
    n = circuit.n
    w4 = kr.root(4 * n)
    l1 = [inv(n)] * n
    rows = wire_coeffs + [z_coeffs, kr.intt(pi_evals(n, public), kr.root(n))] + key_coeffs + [l1, [0, 1] + [0] * (n - 2)]
    on = [kr.ntt(row, w4) for row in rows_coset(rows, G, 1, 4 * n)]
    t = quotient_on_coset(on[:5], on[5:], n, alpha, beta, gamma, KS, zh_inverses(n))
    return rows_coset([kr.intt(t, w4)], inv(G), 1)[0]


def sets_of(n, z):
    return [[z]] * 14 + [[z, z * kr.root(n) % R]]


def prove(circuit, assignment, tau, st=None, tamper_t=False):
    """The prover with a known tau.  Returns a dict: the proof's bytes, its parts, the logarithms of its nine points,
    the challenges and the polynomials.  tamper_t: t_lo is committed and opened with 1 added to its constant term, an
    honest opening of a statement the identity does not hold for."""
    st = st or setup(circuit, tau)
    n, omega = circuit.n, kr.root(circuit.n)
    public = circuit.public_inputs(assignment)
    wires = circuit.wire_values(assignment)
    wire_coeffs = [kr.intt(col, omega) for col in wires]
    logs = [kr.horner(p, tau) for p in wire_coeffs]
    abc = [enc(v) for v in logs]
    beta, gamma = challenges(st["vk"], public, abc)
    zs, total, zeros = perm_product(wires, sigma_labels(circuit), omega, KS, beta, gamma)
    z_coeffs = kr.intt(zs, omega)
    logs.append(kr.horner(z_coeffs, tau))
    z_commit = enc(logs[-1])
    _, _, alpha = challenges(st["vk"], public, abc, z_commit)
    t = quotient(circuit, st["polys"], wire_coeffs, z_coeffs, public, alpha, beta, gamma)
    parts = [t[:n], t[n:2 * n], t[2 * n:3 * n]]
    if tamper_t:
        parts[0] = [(parts[0][0] + 1) % R] + parts[0][1:]
    logs += [kr.horner(p, tau) for p in parts]
    t_commits = [enc(v) for v in logs[4:]]
    _, _, _, z = challenges(st["vk"], public, abc, z_commit, t_commits)
    rows = wire_coeffs + parts + st["polys"] + [z_coeffs]
    commitments = abc + t_commits + st["commitments"] + [z_commit]
    multi = km.prove(rows, sets_of(n, z), tau, commitments)
    values = [v for row in multi["values"] for v in row]
    proof = b"".join(abc + [z_commit] + t_commits) + b"".join(kr.le(v) for v in values) + multi["w"] + multi["w2"]
    return {"bytes": proof, "commitments": abc + [z_commit] + t_commits, "values": values, "w": multi["w"], "w2": multi["w2"],
            "logs": logs + [multi["w_log"], multi["w2_log"]], "beta": beta, "gamma": gamma, "alpha": alpha, "z": z,
            "total": total, "zeros": zeros, "t": t, "wire_coeffs": wire_coeffs, "z_coeffs": z_coeffs, "public": public}


def parse_proof(b):
    assert len(b) == PROOF_BYTES
    return [b[32 * i:32 * i + 32] for i in range(7)], kr.ints(b[224:736]), b[736:768], b[768:]


def identity_holds(n, public, values, beta, gamma, alpha, z) -> bool:
    """the PLONK identity on the 16 opened values"""
    a, b, c, t_lo, t_mid, t_hi, ql, qr, qo, qm, qc, s1, s2, s3, zz, zw = values
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
    t = t_lo + zn * t_mid + zn * zn * t_hi
    return (gate + alpha * p1 + alpha * alpha * p2 - t * (zn - 1)) % R == 0


def _statement(vk, public, proof):
    """(the challenges, the multi-opening's rows) of a parsed proof"""
    n = int.from_bytes(vk[:4], "little")
    cs, values, w, w2 = proof
    beta, gamma, alpha, z = challenges(vk, public, cs[:3], cs[3], cs[4:])
    key = [vk[8 + 32 * i:40 + 32 * i] for i in range(8)]
    commitments = cs[:3] + cs[4:] + key + [cs[3]]
    sets = sets_of(n, z)
    rows = [[v] for v in values[:14]] + [values[14:]]
    return n, (beta, gamma, alpha, z), commitments, sets, rows


def verify_exponent(st, circuit, public, proof, tau) -> bool:
    """The verifier where every point is known by its logarithm: proof is the dict of prove(), whose values, points and
    logarithms the caller may have altered together.  The pairing check of the multi-opening becomes F + z W' = tau W'
    over the scalars."""
    if len(public) != circuit.n_public or any(not 0 <= v < R for v in proof["values"]):
        return False
    parsed = (proof["commitments"], proof["values"], proof["w"], proof["w2"])
    n, (beta, gamma, alpha, z), commitments, sets, rows = _statement(st["vk"], public, parsed)
    if not identity_holds(n, public, proof["values"], beta, gamma, alpha, z):
        return False
    logs = proof["logs"]
    row_logs = logs[:3] + logs[4:7] + st["logs"] + [logs[3]]
    w_log, w2_log = logs[7], logs[8]
    g, u = km.challenges(commitments, sets, rows, proof["w"])
    weights, total, z_t = km.at_z(sets, rows, g, u)
    f = (sum(wt * c for wt, c in zip(weights, row_logs)) - total - z_t * w_log) % R
    return (f + u * w2_log - tau * w2_log) % R == 0


def verify_bytes(vk, public, proof: bytes, g1, g2, tau_g2) -> bool:
    """the verifier on bytes alone, over the model pairing"""
    n_public = int.from_bytes(vk[4:8], "little")
    parsed = parse_proof(proof)
    if len(public) != n_public or any(v >= R for v in parsed[1]):
        return False
    n, (beta, gamma, alpha, z), commitments, sets, rows = _statement(vk, public, parsed)
    if not identity_holds(n, public, parsed[1], beta, gamma, alpha, z):
        return False
    return km.verify(g1, g2, tau_g2, km.opening_bytes(commitments, sets, rows, parsed[2], parsed[3]))
