"""CPU tests of zero-knowledge PLONK proofs: the integer model (tests/plonk_zk_ref.py) checked
against the properties that make the scheme work, and what of octopuszk_amd/plonk's zero-knowledge interface needs no
device: the argument checks of setup(zk=True) and of prove(blinders=...), which are made before any device call."""
import random

import pytest

import kzg_ref as kr
import plonk_lookup_ref as lm
import plonk_r1cs_ref as rm
import plonk_ref as pm
import plonk_zk_ref as zm

R = pm.R
TAU = 0x5eed0123456789abcdef0123456789abcdef0123456789abcdef % R


def _blinders(rng, count):
    return [rng.randrange(1, R) for _ in range(count)]


def _eval(coeffs, x):
    return kr.horner(coeffs, x % R)


# ---------------------------------------------------------------------------- the two kernels' models
def test_rows_blind_touches_two_elements_a_blinder():
    n = 8
    rows = [[100 + 20 * y + i for i in range(n + 5)] for y in range(3)]
    rows[0][0], rows[0][1] = 0, R - 1
    got = zm.rows_blind(rows, n, [[1, R - 1], [], [5, 6, 7, 8]])
    assert got[0][:2] == [R - 1, 0] and got[0][n:n + 2] == [1, R - 1]           # 0 - 1 and (r - 1) - (r - 1)
    assert got[1] == rows[1]
    assert got[2][:4] == [135, 135, 135, 135] and got[2][n:n + 4] == [5, 6, 7, 8]
    for y, touched in enumerate(([0, 1, n, n + 1], [], [0, 1, 2, 3, n, n + 1, n + 2, n + 3])):
        assert all(got[y][i] == rows[y][i] for i in range(n + 5) if i not in touched)


def test_quotient_split_with_zero_blinders_is_plain_slices():
    n = 8
    rng = random.Random(3700)
    t = [rng.randrange(R) for _ in range(3 * n + 6)] + [0] * (n - 6)
    rows, nonzero = zm.quotient_split(t, n, n + 9, [0] * 4)
    assert nonzero == 0
    assert rows == [t[:n] + [0] * 9, t[n:2 * n] + [0] * 9, t[2 * n:3 * n + 6] + [0] * 3]
    for at, want in ((3 * n + 6, 1), (4 * n - 1, 1), (3 * n + 5, 0)):
        planted = list(t)
        planted[at] = (planted[at] + 1) % R
        assert zm.quotient_split(planted, n, n + 8, [0] * 4)[1] == want
    u0, u1, v0, v1 = blinders = _blinders(rng, 4)
    rows, _ = zm.quotient_split(t, n, n + 8, blinders)
    assert rows[0][n:n + 2] == [u0, u1] and rows[1][n:n + 2] == [v0, v1] and rows[0][n + 2:] == [0] * 6
    assert rows[1][:2] == [(t[n] - u0) % R, (t[n + 1] - u1) % R] and rows[2][:2] == [(t[2 * n] - v0) % R, (t[2 * n + 1] - v1) % R]
    assert zm.recombined(rows, n)[:3 * n + 6] == t[:3 * n + 6]


# ---------------------------------------------------------------------------- the model's proofs
@pytest.fixture(scope="module", params=[8, 16], ids=["n8", "n16"])
def vanilla(request):
    n = request.param
    rng = random.Random(3710 + n)
    circuit, assignment = pm.chain(n, 2, rng)
    st = pm.setup(circuit, TAU)
    blinders = _blinders(rng, zm.BLINDERS)
    return {"n": n, "circuit": circuit, "assignment": assignment, "st": st, "blinders": blinders,
            "plain": pm.prove(circuit, assignment, TAU, st), "zk": zm.prove(circuit, assignment, TAU, blinders, st)}


def test_blinded_rows_agree_with_the_witness_on_the_domain(vanilla):
    n, proof = vanilla["n"], vanilla["zk"]
    omega = kr.root(n)
    for coeffs, evals in zip(proof["wire_coeffs"] + [proof["z_coeffs"]], proof["wires"] + [proof["zs"]]):
        assert len(coeffs) == n + zm.ZK_PAD
        assert [_eval(coeffs, pow(omega, i, R)) for i in range(n)] == evals


def test_a_blinded_row_moves_by_its_blinders_times_zh(vanilla):
    n, plain, proof, blinders = vanilla["n"], vanilla["plain"], vanilla["zk"], vanilla["blinders"]
    x = 0x1234567 + n
    for j in range(3):
        r0, r1 = blinders[2 * j:2 * j + 2]
        moved = (_eval(proof["wire_coeffs"][j], x) - _eval(plain["wire_coeffs"][j], x)) % R
        assert moved == (r0 + r1 * x) * zm.zh_at(n, x) % R != 0
    r0, r1, r2 = blinders[6:9]                                            # Z is another under the blinded [a] [b] [c]
    moved = (_eval(proof["z_coeffs"], x) - _eval(kr.intt(proof["zs"], kr.root(n)), x)) % R
    assert moved == (r0 + r1 * x + r2 * x * x) * zm.zh_at(n, x) % R != 0


def test_the_quotient_parts_recombine_and_t_ends_at_3n_plus_6(vanilla):
    n, proof = vanilla["n"], vanilla["zk"]
    t = proof["t"]
    assert len(t) == 4 * n and t[3 * n + 6:] == [0] * (n - 6) and proof["nonzero"] == 0
    assert t[3 * n + 5] != 0                                             # the bound is reached: Z' a' b' c' / Z_H
    assert all(len(p) == n + zm.ZK_PAD for p in proof["parts"])
    assert zm.recombined(proof["parts"], n)[:3 * n + 6] == t[:3 * n + 6]
    assert not any(zm.recombined(proof["parts"], n)[3 * n + 6:])
    x = 0x7654321
    parts_at = [_eval(p, x) for p in proof["parts"]]
    xn = pow(x, n, R)
    assert (parts_at[0] + xn * parts_at[1] + xn * xn * parts_at[2]) % R == _eval(t, x)
    plain_parts = [t[:n], t[n:2 * n], t[2 * n:3 * n + 6]]
    assert all(_eval(p, x) != _eval(q, x) for p, q in zip(proof["parts"], plain_parts))


def test_the_models_zk_proof_verifies_under_the_unchanged_verifier(vanilla):
    circuit, st, proof = vanilla["circuit"], vanilla["st"], vanilla["zk"]
    assert len(proof["bytes"]) == pm.PROOF_BYTES == 800
    assert pm.verify_exponent(st, circuit, proof["public"], proof, TAU)
    assert proof["public"] == vanilla["plain"]["public"]
    spoilt = dict(proof, values=[(proof["values"][0] + 1) % R] + proof["values"][1:])
    assert not pm.verify_exponent(st, circuit, proof["public"], spoilt, TAU)


def test_zero_blinders_give_the_proof_without_zk(vanilla):
    circuit, assignment, st = vanilla["circuit"], vanilla["assignment"], vanilla["st"]
    assert zm.prove(circuit, assignment, TAU, [0] * zm.BLINDERS, st)["bytes"] == vanilla["plain"]["bytes"]
    zk, plain = vanilla["zk"], vanilla["plain"]
    assert all(a != b for a, b in zip(zk["commitments"], plain["commitments"]))
    assert all(zk["values"][i] != plain["values"][i] for i in (0, 1, 2, 3, 4, 5, 14, 15))


def test_a_violated_gate_shows_past_3n_plus_6():
    n = 8
    rng = random.Random(3720)
    circuit, assignment = pm.chain(n, 1, rng)
    bad = assignment[:-1] + [(assignment[-1] + 1) % R]                   # the last gate's output: in one cell only
    assert zm.prove(circuit, bad, TAU, _blinders(rng, zm.BLINDERS))["nonzero"] > 0


def test_the_bytes_verifier_takes_a_zk_proof():
    """the model pairing on the bytes alone, once: the verifier sees nothing but a proof"""
    n = 8
    rng = random.Random(3730)
    circuit, assignment = pm.chain(n, 1, rng)
    st = pm.setup(circuit, TAU)
    proof = zm.prove(circuit, assignment, TAU, _blinders(rng, zm.BLINDERS), st)
    _, (g2, tau_g2) = kr.string(1, TAU)
    assert pm.verify_bytes(st["vk"], proof["public"], proof["bytes"], pm.o.G1.to_affine(pm.o.G1.one), g2, tau_g2)


@pytest.mark.parametrize("n", [8, 16])
def test_the_lookup_model(n):
    rng = random.Random(3740 + n)
    table = [tuple(rng.randrange(R) for _ in range(3)) for _ in range(5)]
    circuit, assignment = lm.chain_with_lookups(n, 1, rng, table, n // 2 - 1)
    st = lm.setup(circuit, TAU)
    blinders = _blinders(rng, zm.LOOKUP_BLINDERS)
    plain, proof = lm.prove(circuit, assignment, TAU, st), zm.prove_lookup(circuit, assignment, TAU, blinders, st)
    omega = kr.root(n)
    for coeffs, evals in ((proof["m_coeffs"], proof["m"]), (proof["s_coeffs"], proof["s"]), (proof["z_coeffs"], proof["zs"])):
        assert [_eval(coeffs, pow(omega, i, R)) for i in range(n)] == evals
    assert proof["t"][3 * n + 6:] == [0] * (n - 6) and proof["nonzero"] == 0
    assert zm.recombined(proof["parts"], n)[:3 * n + 6] == proof["t"][:3 * n + 6]
    assert len(proof["bytes"]) == lm.PROOF_BYTES == 1088
    assert lm.verify_exponent(st, circuit, proof["public"], proof, TAU)
    assert zm.prove_lookup(circuit, assignment, TAU, [0] * zm.LOOKUP_BLINDERS, st)["bytes"] == plain["bytes"]
    assert all(a != b for a, b in zip(proof["commitments"], plain["commitments"]))
    assert all(proof["values"][i] != plain["values"][i] for i in (0, 1, 2, 3, 4, 5, 6, 19, 20, 21, 22))


def test_the_r1cs_model():
    rel, w = rm.mixed_relation()
    circuit = rm.model_circuit(rel)
    assignment = rm.extend(rel, w)
    rng = random.Random(3750)
    st = pm.setup(circuit, TAU)
    proof = zm.prove(circuit, assignment, TAU, _blinders(rng, zm.BLINDERS), st)
    assert circuit.n >= 8 and proof["nonzero"] == 0
    assert pm.verify_exponent(st, circuit, proof["public"], proof, TAU)
    assert zm.prove(circuit, assignment, TAU, [0] * zm.BLINDERS, st)["bytes"] == pm.prove(circuit, assignment, TAU, st)["bytes"]


# ---------------------------------------------------------------------------- the package's argument checks
def _package_circuit(n):
    from octopuszk_amd import plonk
    model, _ = pm.chain(n, 1, random.Random(3760 + n), constant=n >= 8)
    return plonk.Circuit(n, model.selectors, model.wires, 1)


@pytest.mark.parametrize("n,bases", [(8, 8), (8, 15), (8, 17), (16, 16), (4, 12), (2, 10)])
def test_setup_zk_names_the_two_sizes(n, bases):
    """n below 8 or a commit key of other than n + ZK_PAD bases: refused before any device call"""
    from octopuszk_amd import kzg, plonk
    assert plonk.ZK_PAD == zm.ZK_PAD == 8
    with pytest.raises(ValueError) as e:
        plonk.setup(_package_circuit(n), kzg.CommitKey(None, bases, 64), zk=True)
    assert "n = %d" % n in str(e.value) and "n = %d" % bases in str(e.value)


def test_setup_without_zk_still_takes_n_bases_only():
    from octopuszk_amd import kzg, plonk
    with pytest.raises(ValueError, match="n = 8 gates, the commit key n = 16 bases"):
        plonk.setup(_package_circuit(8), kzg.CommitKey(None, 16, 64))
    with pytest.raises(ValueError, match="n = 8 gates, the commit key n = 16 bases"):
        plonk.setup(_package_circuit(8), kzg.CommitKey(None, 16, 64), zk=False)


def _bare_keys():
    """(a vanilla and a lookup proving key with nothing on the device, the number of blinders each takes)"""
    from octopuszk_amd import kzg, plonk
    circuit = _package_circuit(8)
    ck = kzg.CommitKey(None, 16, 64)
    model = lm.chain_with_lookups(8, 1, random.Random(3770), [(1, 2, 3), (4, 5, 6)], 2)[0]
    lookup = plonk.LookupCircuit(8, model.selectors, model.wires, 1, model.q_lookup, model.table)
    return ((plonk.ProvingKey(circuit, ck, None, None, None, None), plonk.ZK_BLINDERS),
            (plonk.LookupProvingKey(lookup, ck, None, None, None, None, None, None), plonk.ZK_LOOKUP_BLINDERS))


def test_prove_checks_the_blinders_before_anything_else():
    from octopuszk_amd import plonk
    assert (plonk.ZK_BLINDERS, plonk.ZK_LOOKUP_BLINDERS) == (zm.BLINDERS, zm.LOOKUP_BLINDERS) == (13, 18)
    for pk, count in _bare_keys():
        assert pk.zk is False
        with pytest.raises(ValueError, match="zk=True"):
            plonk.prove(pk, [0] * 4, blinders=[0] * count)
        with pytest.raises(ValueError, match="zk=True"):
            plonk.prove(pk, [0] * 4, blinders=[])
        pk.zk = True
        for wrong in ([0] * (count - 1), [0] * (count + 1), [], [0] * (31 - count)):
            with pytest.raises(ValueError, match="%d blinders" % len(wrong)):
                plonk.prove(pk, [0] * 4, blinders=wrong)
        for bad in (R, -1, 1 << 256, 0.5, None):
            with pytest.raises(ValueError, match="ints in"):
                plonk.prove(pk, [0] * 4, blinders=[0] * (count - 1) + [bad])
        with pytest.raises(ValueError, match="ints in"):
            plonk.prove(pk, [0] * 4, blinders=[R - 1] * (count - 1) + [R])
