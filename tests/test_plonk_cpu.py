"""The integer model of the PLONK prover and verifier (tests/plonk_ref.py) against itself at n = 4 and n = 8, and what
of octopuszk_amd/plonk needs no device: the Builder's permutation and the strict byte formats."""
import random

import pytest

import kzg_ref as kr
import plonk_ref as pm

R = pm.R
TAU = 0x5eed0123456789abcdef0123456789abcdef0123456789abcdef % R


def _case(n):
    circuit, assignment = pm.chain(n, 1, random.Random(290 + n), constant=n >= 8)
    return circuit, assignment, pm.setup(circuit, TAU)


@pytest.fixture(scope="module", params=[4, 8])
def proved(request):
    circuit, assignment, st = _case(request.param)
    return circuit, assignment, st, pm.prove(circuit, assignment, TAU, st)


def test_an_honest_proof_verifies(proved):
    circuit, assignment, st, proof = proved
    assert proof["total"] == 1 and proof["zeros"] == 0
    assert proof["t"][3 * circuit.n:] == [0] * circuit.n
    assert len(proof["bytes"]) == pm.PROOF_BYTES == 800
    assert pm.verify_exponent(st, circuit, proof["public"], proof, TAU)


def test_a_wrong_public_input_fails(proved):
    circuit, _, st, proof = proved
    assert not pm.verify_exponent(st, circuit, [(proof["public"][0] + 1) % R], proof, TAU)
    assert not pm.verify_exponent(st, circuit, [], proof, TAU)


@pytest.mark.parametrize("which", range(16))
def test_every_value_altered_by_one_fails(proved, which):
    circuit, _, st, proof = proved
    bad = dict(proof)
    bad["values"] = list(proof["values"])
    bad["values"][which] = (bad["values"][which] + 1) % R
    assert not pm.verify_exponent(st, circuit, proof["public"], bad, TAU)


def test_an_honest_opening_of_another_statement_fails_the_identity_alone(proved):
    circuit, assignment, st, _ = proved
    bad = pm.prove(circuit, assignment, TAU, st, tamper_t=True)
    n, ch, commitments, sets, rows = pm._statement(st["vk"], bad["public"], pm.parse_proof(bad["bytes"]))
    assert not pm.identity_holds(n, bad["public"], bad["values"], *ch)
    assert not pm.verify_exponent(st, circuit, bad["public"], bad, TAU)
    # the opening itself is sound: the scalar form of the pairing check
    import kzg_multi_ref as km
    g, u = km.challenges(commitments, sets, rows, bad["w"])
    weights, total, z_t = km.at_z(sets, rows, g, u)
    logs = bad["logs"]
    row_logs = logs[:3] + logs[4:7] + st["logs"] + [logs[3]]
    f = (sum(w * c for w, c in zip(weights, row_logs)) - total - z_t * logs[7]) % R
    assert (f + u * logs[8] - TAU * logs[8]) % R == 0


def _quotient_of(circuit, assignment, st):
    """t's 4 n coefficients under fixed challenges, with the polynomials it is made of"""
    n, omega = circuit.n, kr.root(circuit.n)
    beta, gamma, alpha = 3 + n, 5 + n, 7 + n
    wires = circuit.wire_values(assignment)
    public = circuit.public_inputs(assignment)
    zs, total, _ = pm.perm_product(wires, pm.sigma_labels(circuit), omega, pm.KS, beta, gamma)
    wire_coeffs, z_coeffs = [kr.intt(col, omega) for col in wires], kr.intt(zs, omega)
    t = pm.quotient(circuit, st["polys"], wire_coeffs, z_coeffs, public, alpha, beta, gamma)
    return t, total, (wire_coeffs, z_coeffs, public, alpha, beta, gamma)


@pytest.mark.parametrize("n", [4, 8])
def test_a_violated_gate_gives_a_non_polynomial_quotient(n):
    circuit, assignment, st = _case(n)
    t, total, _ = _quotient_of(circuit, assignment, st)
    assert total == 1 and t[3 * n:] == [0] * n
    bad = list(assignment)
    bad[-1] = (bad[-1] + 1) % R                      # the output of the last gate: in one cell, so no copy breaks
    t, total, _ = _quotient_of(circuit, bad, st)
    assert total == 1 and any(t[3 * n:])


@pytest.mark.parametrize("n", [4, 8])
def test_a_violated_copy_gives_a_product_other_than_one(n):
    circuit, assignment, _ = _case(n)
    wires = circuit.wire_values(assignment)
    wires[1][circuit.n_public] = (wires[1][circuit.n_public] + 1) % R       # one cell of a variable in many cells
    _, total, zeros = pm.perm_product(wires, pm.sigma_labels(circuit), kr.root(n), pm.KS, 11, 13)
    assert total != 1 and zeros == 0


def _add(a, b):
    out = [0] * max(len(a), len(b))
    for i, v in enumerate(a):
        out[i] = v
    for i, v in enumerate(b):
        out[i] = (out[i] + v) % R
    return out


def _scale(a, k):
    return [v * k % R for v in a]


@pytest.mark.parametrize("n", [4, 8])
def test_the_three_parts_of_t_times_z_h_are_the_numerator(n):
    circuit, assignment, st = _case(n)
    t, _, ((a, b, c), z, public, alpha, beta, gamma) = _quotient_of(circuit, assignment, st)
    ql, qr, qo, qm, qc, s1, s2, s3 = st["polys"]
    omega = kr.root(n)
    pi = kr.intt(pm.pi_evals(n, public), omega)
    x = [0, 1]
    mul = pm.poly_mul
    gate = _add(_add(_add(mul(ql, a), mul(qr, b)), _add(mul(qo, c), mul(qm, mul(a, b)))), _add(qc, pi))

    def factor(w, label, k):
        return _add(_add(w, _scale(label, beta * k % R)), [gamma])

    left = mul(mul(mul(z, factor(a, x, 1)), factor(b, x, pm.KS[1])), factor(c, x, pm.KS[2]))
    z_shift = [v * pow(omega, i, R) % R for i, v in enumerate(z)]
    right = mul(mul(mul(z_shift, factor(a, s1, 1)), factor(b, s2, 1)), factor(c, s3, 1))
    p2 = mul(_add(z, [R - 1]), [pm.inv(n)] * n)
    numerator = _add(_add(gate, _scale(_add(left, _scale(right, R - 1)), alpha)), _scale(p2, alpha * alpha % R))
    t_lo, t_mid, t_hi = t[:n], t[n:2 * n], t[2 * n:3 * n]
    whole = t_lo + t_mid + t_hi                                       # t_lo + X^n t_mid + X^2n t_hi
    z_h = [R - 1] + [0] * (n - 1) + [1]
    product = mul(whole, z_h)
    width = max(len(product), len(numerator))
    assert product + [0] * (width - len(product)) == numerator + [0] * (width - len(numerator))
    assert any(numerator)


def test_the_kernels_models_at_their_edges():
    rng = random.Random(291)
    rows = [[rng.randrange(R) for _ in range(5)] for _ in range(2)]
    out = pm.rows_coset(rows, 5, 3, 8)
    assert [len(r) for r in out] == [8, 8] and out[1][5:] == [0, 0, 0]
    assert out[0][2] == rows[0][2] * 3 * 25 % R
    # a zero denominator: the row's factor is 1, it is counted, the rows around it are exact
    wires = [[rng.randrange(R) for _ in range(6)] for _ in range(3)]
    sigma = [[rng.randrange(R) for _ in range(6)] for _ in range(3)]
    beta = 9
    gamma = (-(wires[2][3] + beta * sigma[2][3])) % R
    z, total, zeros = pm.perm_product(wires, sigma, 7, pm.KS, beta, gamma)
    assert zeros == 1 and z[4] == z[3] and z[0] == 1 and total != 0


# ---------------------------------------------------------------------------- the package, without a device
def test_the_builder_wires_one_cycle_per_variable():
    from octopuszk_amd import plonk
    b = plonk.Builder()
    x, y = b.public(), b.public()
    u, v, w = b.var(), b.var(), b.var()
    b.mul(x, y, u)
    b.add(u, x, v)
    b.gate(2, 0, -1, 0, 5, v, v, w)
    b.assert_equal(w, w)
    b.constant(u, 12)
    circuit = b.build()
    assert circuit.n == 8 and circuit.n_public == 2 and circuit.n_vars == 5
    assert [col[:2] for col in circuit.selectors] == [[1, 1], [0, 0], [0, 0], [0, 0], [0, 0]]
    assert circuit.selectors[2][2] == R - 1 and circuit.selectors[4][6] == R - 12
    n, sigma = circuit.n, circuit.permutation()
    assert sorted(sigma) == list(range(3 * n))
    flat = [v_ for col in circuit.wires for v_ in col]
    for var in range(circuit.n_vars):
        cells = [i for i, v_ in enumerate(flat) if v_ == var]
        seen, at = [], cells[0]
        for _ in cells:
            seen.append(at)
            at = sigma[at]
        assert at == cells[0] and sorted(seen) == cells          # one cycle through exactly the variable's cells
    # the labels are the model's
    model = pm.Circuit(n, circuit.selectors, circuit.wires, circuit.n_public)
    assert circuit.sigma_labels() == pm.sigma_labels(model)
    with pytest.raises(ValueError):
        b.mul(x, y, 99)
    with pytest.raises(ValueError):
        plonk.Circuit(6, [[0] * 6] * 5, [[0] * 6] * 3)
    with pytest.raises(ValueError):
        plonk.Circuit(4, [[0] * 4] * 5, [[0] * 4] * 3, n_public=1)          # row 0 is no public-input row


def test_the_challenges_are_the_models(proved):
    from octopuszk_amd import plonk
    _, _, st, proof = proved
    cs = proof["commitments"]
    got = plonk.challenges(st["vk"], proof["public"], cs[:3], cs[3], cs[4:])
    assert got == (proof["beta"], proof["gamma"], proof["alpha"], proof["z"])
    assert plonk.challenges(st["vk"], proof["public"], cs[:3]) == got[:2]


def test_proof_bytes_round_trip_and_are_parsed_strictly(proved):
    from octopuszk_amd import plonk
    _, _, _, proof = proved
    raw = proof["bytes"]
    p = plonk.Proof.from_bytes(raw)
    assert p.to_bytes() == raw and list(p.values) == proof["values"] and list(p.commitments) == proof["commitments"]
    for bad in (raw[:-1], raw + b"\0", b""):
        with pytest.raises(ValueError, match="length"):
            plonk.Proof.from_bytes(bad)
    for i in range(16):                                                    # a value written as y + r, or as r itself
        at = 224 + 32 * i
        for v in (proof["values"][i] + R, R):
            if v < 1 << 256:
                with pytest.raises(ValueError, match="below r"):
                    plonk.Proof.from_bytes(raw[:at] + kr.le(v) + raw[at + 32:])
    for at in list(range(0, 224, 32)) + [736, 768]:                       # every point: an x that is no field element
        with pytest.raises(ValueError, match="decode"):
            plonk.Proof.from_bytes(raw[:at] + b"\xff" * 31 + b"\x3f" + raw[at + 32:])
    with pytest.raises(ValueError):
        plonk.Proof(proof["commitments"], proof["values"][:15], proof["w"], proof["w2"])


def test_verifying_key_bytes_round_trip_and_are_parsed_strictly(proved):
    from octopuszk_amd import plonk
    circuit, _, st, _ = proved
    raw = st["vk"]
    vk = plonk.VerifyingKey.from_bytes(raw)
    assert vk.to_bytes() == raw and (vk.n, vk.n_public) == (circuit.n, 1) and list(vk.commitments) == st["commitments"]
    for bad in (raw[:-1], raw + b"\0"):
        with pytest.raises(ValueError, match="length"):
            plonk.VerifyingKey.from_bytes(bad)
    for n in (0, 1, 6, (1 << 26) + 1, 1 << 27):
        with pytest.raises(ValueError, match="power of two"):
            plonk.VerifyingKey.from_bytes(n.to_bytes(4, "little") + raw[4:])
    with pytest.raises(ValueError, match="n_public"):
        plonk.VerifyingKey.from_bytes(raw[:4] + (circuit.n + 1).to_bytes(4, "little") + raw[8:])
    for i in range(8):
        at = 8 + 32 * i
        with pytest.raises(ValueError, match="decode"):
            plonk.VerifyingKey.from_bytes(raw[:at] + b"\xff" * 31 + b"\x3f" + raw[at + 32:])
