"""Exact-integer model of zero-knowledge PLONK proofs, on top of tests/plonk_ref.py and
tests/plonk_lookup_ref.py (an imported R1CS is tests/plonk_r1cs_ref.py's compiled circuit under the vanilla prover): the
two kernels of csrc/plonk_zk.cuh on host integers (the blinders of coefficient rows, the split of the quotient into its
three blinded parts) and the two provers with a known tau and a given list of blinders, whose proofs the verifiers of
the models below take unchanged.  Every row of a proof has N = n + ZK_PAD coefficients.  Written from the section's
description, not from octopuszk_amd/plonk or csrc/plonk_zk.cuh, which the tests compare with it."""
import kzg_multi_ref as km
import kzg_ref as kr
import plonk_lookup_ref as lm
import plonk_ref as pm

R = pm.R
ZK_PAD = 8
T_COEFFS = 6                 # t has at most 3 n + T_COEFFS coefficients
BLINDERS = 13                # a0 a1 b0 b1 c0 c1 Z0 Z1 Z2 u0 u1 v0 v1
LOOKUP_BLINDERS = 18         # a0 a1 b0 b1 c0 c1 m0 m1 Z0 Z1 Z2 S0 S1 S2 u0 u1 v0 v1


# ---------------------------------------------------------------------------- the two kernels
def rows_blind(rows, n, blinders):
    """rows as written (words of any size, at any stride >= n + 4) -> the rows after ozk_fr_rows_blind_dev: row[j]
    becomes (row[j] - r_j) mod r and row[n + j] becomes r_j mod r for the blinders r_0 .. of that row; every other word
    stays as it was written"""
    out = []
    for row, rs in zip(rows, blinders):
        assert len(rs) <= 4 <= n and len(row) >= n + 4
        new = list(row)
        for j, r in enumerate(rs):
            new[j] = (row[j] - r) % R
            new[n + j] = r % R
        out.append(new)
    return out


def quotient_split(t, n, out_stride, blinders):
    """the 4 n coefficients of t as written -> (the rows t_lo', t_mid', t_hi' of out_stride elements, how many of the
    coefficients from 3 n + T_COEFFS are not zero mod r)"""
    assert len(t) == 4 * n and out_stride >= n + ZK_PAD and len(blinders) == 4
    u, v = blinders[:2], blinders[2:]
    t = [x % R for x in t]
    lo = t[:n] + list(u)
    mid = [(x - (u[i] if i < 2 else 0)) % R for i, x in enumerate(t[n:2 * n])] + list(v)
    hi = [(x - (v[i] if i < 2 else 0)) % R for i, x in enumerate(t[2 * n:3 * n + T_COEFFS])]
    rows = [[x % R for x in row] + [0] * (out_stride - len(row)) for row in (lo, mid, hi)]
    return rows, sum(1 for x in t[3 * n + T_COEFFS:] if x)


# ---------------------------------------------------------------------------- polynomials
def padded(row, n):
    return list(row) + [0] * (n + ZK_PAD - len(row))


def blinded(coeffs, n, rs):
    """the n coefficients of w -> the N of w + (r_0 + r_1 X + ..)(X^n - 1)"""
    return rows_blind([padded(coeffs, n)], n, [list(rs)])[0]


def zh_at(n, x):
    return (pow(x, n, R) - 1) % R


def recombined(parts, n):
    """the coefficients of t_lo' + X^n t_mid' + X^2n t_hi'"""
    out = [0] * (2 * n + len(parts[2]))
    for k, part in enumerate(parts):
        for i, x in enumerate(part):
            out[k * n + i] = (out[k * n + i] + x) % R
    return out


# ---------------------------------------------------------------------------- the provers
def prove(circuit, assignment, tau, blinders, st=None):
    """plonk_ref.prove with the 13 blinders of a vanilla (or imported R1CS) proof; a dict of the same keys"""
    assert len(blinders) == BLINDERS
    st = st or pm.setup(circuit, tau)
    n, omega = circuit.n, kr.root(circuit.n)
    public = circuit.public_inputs(assignment)
    wires = circuit.wire_values(assignment)
    wire_coeffs = [blinded(kr.intt(col, omega), n, blinders[2 * j:2 * j + 2]) for j, col in enumerate(wires)]
    logs = [kr.horner(p, tau) for p in wire_coeffs]
    abc = [pm.enc(v) for v in logs]
    beta, gamma = pm.challenges(st["vk"], public, abc)
    zs, total, zeros = pm.perm_product(wires, pm.sigma_labels(circuit), omega, pm.KS, beta, gamma)
    z_coeffs = blinded(kr.intt(zs, omega), n, blinders[6:9])
    logs.append(kr.horner(z_coeffs, tau))
    z_commit = pm.enc(logs[-1])
    _, _, alpha = pm.challenges(st["vk"], public, abc, z_commit)
    t = pm.quotient(circuit, st["polys"], wire_coeffs, z_coeffs, public, alpha, beta, gamma)
    parts, nonzero = quotient_split(t, n, n + ZK_PAD, blinders[9:])
    logs += [kr.horner(p, tau) for p in parts]
    t_commits = [pm.enc(v) for v in logs[4:]]
    _, _, _, z = pm.challenges(st["vk"], public, abc, z_commit, t_commits)
    rows = wire_coeffs + parts + [padded(p, n) for p in st["polys"]] + [z_coeffs]
    commitments = abc + t_commits + st["commitments"] + [z_commit]
    multi = km.prove(rows, pm.sets_of(n, z), tau, commitments)
    values = [v for row in multi["values"] for v in row]
    proof = b"".join(abc + [z_commit] + t_commits) + b"".join(kr.le(v) for v in values) + multi["w"] + multi["w2"]
    return {"bytes": proof, "commitments": abc + [z_commit] + t_commits, "values": values, "w": multi["w"], "w2": multi["w2"],
            "logs": logs + [multi["w_log"], multi["w2_log"]], "beta": beta, "gamma": gamma, "alpha": alpha, "z": z,
            "total": total, "zeros": zeros, "t": t, "parts": parts, "nonzero": nonzero, "wire_coeffs": wire_coeffs,
            "z_coeffs": z_coeffs, "wires": wires, "zs": zs, "public": public}


def prove_lookup(circuit, assignment, tau, blinders, st=None):
    """plonk_lookup_ref.prove (no tampering) with the 18 blinders of a proof with lookups"""
    assert len(blinders) == LOOKUP_BLINDERS
    st = st or lm.setup(circuit, tau)
    n, omega = circuit.n, kr.root(circuit.n)
    public = circuit.public_inputs(assignment)
    wires = circuit.wire_values(assignment)
    key4 = circuit.key4()
    m, missing, _ = lm.multiplicities(wires, key4[0], circuit.table, n)
    assert missing == 0
    wire_coeffs = [blinded(kr.intt(col, omega), n, blinders[2 * j:2 * j + 2]) for j, col in enumerate(wires)]
    m_coeffs = blinded(kr.intt(m, omega), n, blinders[6:8])
    logs = [kr.horner(p, tau) for p in wire_coeffs + [m_coeffs]]
    abcm = [pm.enc(v) for v in logs]
    beta, gamma, eta, theta = lm.challenges(st["vk"], public, abcm)
    zs, total, zeros = pm.perm_product(wires, pm.sigma_labels(circuit), omega, pm.KS, beta, gamma)
    ss, s_total, s_zeros = lm.lookup_sum(wires, key4, m, eta, theta)
    z_coeffs = blinded(kr.intt(zs, omega), n, blinders[8:11])
    s_coeffs = blinded(kr.intt(ss, omega), n, blinders[11:14])
    logs += [kr.horner(z_coeffs, tau), kr.horner(s_coeffs, tau)]
    zs_commits = [pm.enc(v) for v in logs[4:6]]
    alpha = lm.challenges(st["vk"], public, abcm, zs_commits)[4]
    t = lm.quotient(circuit, st["polys"], wire_coeffs, z_coeffs, m_coeffs, s_coeffs, public, alpha, beta, gamma, eta, theta)
    parts, nonzero = quotient_split(t, n, n + ZK_PAD, blinders[14:])
    logs += [kr.horner(p, tau) for p in parts]
    t_commits = [pm.enc(v) for v in logs[6:9]]
    z = lm.challenges(st["vk"], public, abcm, zs_commits, t_commits)[5]
    rows = wire_coeffs + [m_coeffs] + parts + [padded(p, n) for p in st["polys"]] + [z_coeffs, s_coeffs]
    commitments = abcm + t_commits + st["commitments"] + zs_commits
    multi = km.prove(rows, lm.sets_of(n, z), tau, commitments)
    values = [v for row in multi["values"] for v in row]
    proof = b"".join(abcm + zs_commits + t_commits) + b"".join(kr.le(v) for v in values) + multi["w"] + multi["w2"]
    return {"bytes": proof, "commitments": abcm + zs_commits + t_commits, "values": values, "w": multi["w"],
            "w2": multi["w2"], "logs": logs + [multi["w_log"], multi["w2_log"]], "beta": beta, "gamma": gamma, "eta": eta,
            "theta": theta, "alpha": alpha, "z": z, "total": total, "zeros": zeros, "s_total": s_total, "s_zeros": s_zeros,
            "t": t, "parts": parts, "nonzero": nonzero, "m": m, "s": ss, "wires": wires, "zs": zs,
            "wire_coeffs": wire_coeffs, "m_coeffs": m_coeffs, "z_coeffs": z_coeffs, "s_coeffs": s_coeffs, "public": public}
