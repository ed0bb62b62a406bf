"""Exact-integer model of the setup from a powers-of-tau string, in the exponent, over
oracle.bn254: every group element is its discrete logarithm to the generator of its group.  Written from the
protocol's description, not from octopuszk_amd/srs.py, which the tests compare with it."""
import ceremony_ref as cref
from oracle import bn254 as o
from oracle import groth16 as g

R = o.R


# ---------------------------------------------------------------------------- transforms of scalars
def dft(vals, omega):
    """out[j] = sum_i omega^(i j) vals[i]: the definition up to 64 values, an even / odd split above"""
    n = len(vals)
    if n <= 64:
        pw = [pow(omega, k, R) for k in range(n)]
        return [sum(v * pw[i * j % n] for i, v in enumerate(vals)) % R for j in range(n)]
    even, odd = dft(vals[0::2], omega * omega % R), dft(vals[1::2], omega * omega % R)
    out, w = [0] * n, 1
    for j in range(n // 2):
        t = w * odd[j] % R
        out[j], out[j + n // 2] = (even[j] + t) % R, (even[j] - t) % R
        w = w * omega % R
    return out


def inverse_dft(vals, omega=None):
    """the inverse over the domain of omega (default: the root of unity of the size): omega^-1 and 1 / n"""
    n = len(vals)
    omega = o.fr_root_of_unity(n) if omega is None else omega
    ninv = pow(n, -1, R)
    return [v * ninv % R for v in dft(vals, pow(omega, -1, R))]


# ---------------------------------------------------------------------------- the string and the key
def srs_exp(m, tau, alpha, beta):
    return dict(m=m, tau_g1=[pow(tau, i, R) for i in range(2 * m + 1)], tau_g2=[pow(tau, i, R) for i in range(m)],
                alpha_tau_g1=[alpha * pow(tau, i, R) % R for i in range(m)],
                beta_tau_g1=[beta * pow(tau, i, R) % R for i in range(m)], beta_g2=beta)


def _products(r1cs, lag):
    """(At, Bt, Ct) of the transposed matrices times one Lagrange vector, with the input_i rows of A"""
    nc, ni, nv = r1cs.num_constraints, r1cs.num_inputs, r1cs.num_variables
    out = [[0] * nv for _ in range(3)]
    for i in range(ni):
        out[0][i] = lag[nc + i]
    for i, sides in enumerate(r1cs.constraints):
        for acc, terms in zip(out, sides):
            for index, value in terms:
                acc[index] = (acc[index] + lag[i] * value) % R
    return out


def setup_exp(r1cs, srs):
    """the key of r1cs (an oracle.groth16.R1CS) from a string in the exponent: gamma = delta = 1"""
    m = g.lowest_power_of_two(r1cs.num_constraints + r1cs.num_inputs)
    if m != srs["m"]:
        raise ValueError("m")
    ni = r1cs.num_inputs
    l1, la = inverse_dft(srs["tau_g1"][:m]), inverse_dft(srs["alpha_tau_g1"])
    lb, l2 = inverse_dft(srs["beta_tau_g1"]), inverse_dft(srs["tau_g2"])
    at, bt, ct = _products(r1cs, l1)
    abc = [(x + y + z) % R for x, y, z in zip(_products(r1cs, lb)[0], _products(r1cs, la)[1], ct)]
    tg1 = srs["tau_g1"]
    return dict(alpha_g1=srs["alpha_tau_g1"][0], beta_g1=srs["beta_tau_g1"][0], beta_g2=srs["beta_g2"],
                delta_g1=tg1[0], delta_g2=srs["tau_g2"][0], gamma_g2=srs["tau_g2"][0],
                query_a=at, query_b_g1=bt, query_b_g2=_products(r1cs, l2)[1],
                gamma_abc_g1=abc[:ni], delta_abc_g1=abc[ni:],
                query_h=[(tg1[i + m] - tg1[i]) % R for i in range(m + 1)])


def as_oracle_crs(r1cs, key):
    """the model key as the object oracle.groth16.proof_scalars / verify_in_the_exponent read"""
    crs = g.CRS()
    crs.r1cs = r1cs
    crs.qap = g.QAPRelation(key["query_a"], key["query_b_g1"], None, None, None, None, r1cs.num_inputs,
                            r1cs.num_variables, None)
    crs.secrets = dict(alpha=key["alpha_g1"], beta=key["beta_g1"], gamma=key["gamma_g2"], delta=key["delta_g1"])
    crs.delta_abc_scalars, crs.ht_scalars = key["delta_abc_g1"], key["query_h"]
    crs.gamma_abc_scalars = key["gamma_abc_g1"]
    return crs


G1_FIELDS = ("alpha_g1", "beta_g1", "delta_g1", "query_a", "query_b_g1", "delta_abc_g1", "query_h", "gamma_abc_g1")
G2_FIELDS = ("beta_g2", "delta_g2", "query_b_g2", "gamma_g2")


def encodings(exps, type_, gen):
    """the compressed encodings (section 13) of [e] gen for the logarithms `exps` (one or a list), concatenated"""
    exps = exps if isinstance(exps, list) else [exps]
    return b"".join(cref.encode(type_, cref.scale(type_, gen, e % R)) for e in exps)


# ---------------------------------------------------------------------------- a small circuit with real coefficients
def handmade_r1cs(seed=5):
    """(r1cs, primary, auxiliary): 12 constraints over 3 inputs (the constant and two values) with coefficients in
    {1, r - 1, 2, random}; variable 0 only ever carries the coefficient 1 (LinearCombination.evaluate gives a term of
    index 0 the value one whatever its coefficient)."""
    import random
    rng = random.Random(seed)
    k = [rng.randrange(3, R) for _ in range(4)]
    full = [1, rng.randrange(R), rng.randrange(R)]
    cons = []

    def lc(terms):
        return sum(1 if i == 0 else full[i] * v for i, v in terms) % R

    def constraint(A, B):
        full.append(lc(A) * lc(B) % R)
        cons.append((A, B, [(len(full) - 1, 1)]))

    constraint([(1, 1), (2, R - 1)], [(0, 1)])                          # x1 - x2
    constraint([(1, 2), (0, 1)], [(2, 1)])                              # (2 x1 + 1) x2
    constraint([(3, k[0])], [(4, R - 1), (1, 1)])
    constraint([(5, 1), (5, 1)], [(0, 1), (3, k[1])])                   # the same variable twice in a row
    constraint([(1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1)], [(0, 1)])
    constraint([(7, R - 1), (7, 1), (2, 2)], [(6, 2)])                  # a variable and its negative
    constraint([(8, k[2]), (4, R - 1)], [(8, 1)])
    constraint([(0, 1), (9, 1)], [(0, 1), (9, R - 1)])
    constraint([(10, 2)], [(10, 2), (1, k[3])])
    constraint([(11, 1)], [(2, R - 1)])
    constraint([(12, 1), (3, R - 1)], [(12, 1), (3, 1)])
    constraint([(i, 1) for i in range(1, 14)], [(13, 1)])
    r1cs = g.R1CS(cons, 3, len(full) - 3)
    assert len(cons) == 12 and g.is_satisfied(r1cs, full[:3], full[3:])
    return r1cs, full[:3], full[3:]
