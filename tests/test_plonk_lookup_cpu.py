"""The integer model of the PLONK prover and verifier with lookups (tests/plonk_lookup_ref.py) against itself at n = 4
and n = 8, the logUp identity on small random cases, and what of octopuszk_amd/plonk needs no device: the Builder's rules
for tables, the two strict byte formats, the transcript and the verifier's identity, which every proof of the model,
honest or not, is also put to."""
import random

import pytest

import kzg_ref as kr
import plonk_lookup_ref as lm
import plonk_ref as pm
from octopuszk_amd import plonk
from octopuszk_amd.plonk import LookupCircuit, lookup_challenges, protocol      # (this file is about them: no lookups, no tests)

R = pm.R
TAU = 0x5eed0123456789abcdef0123456789abcdef0123456789abcdef % R


def _table(rng, rows):
    """random rows, the last a copy of the first"""
    table = [tuple(rng.randrange(R) for _ in range(3)) for _ in range(rows - 1)]
    return table + [table[0]] if rows > 1 else [tuple(rng.randrange(R) for _ in range(3))]


def _case(n):
    rng = random.Random(310 + n)
    circuit, assignment = lm.chain_with_lookups(n, 1, rng, _table(rng, n - 1), n // 2 - 1 if n > 4 else 2)
    return circuit, assignment, lm.setup(circuit, TAU)


def _package_identity(st, proof):
    """the package's verifier up to the pairing, host only: the strict parsers, its transcript, its identity"""
    vk = plonk.LookupVerifyingKey.from_bytes(st["vk"])
    parsed = plonk.LookupProof(proof["commitments"], proof["values"], proof["w"], proof["w2"])
    cs = list(parsed.commitments)
    ch = lookup_challenges(vk.to_bytes(), proof["public"], cs[:4], cs[4:6], cs[6:])
    return protocol.lookup_identity_holds(vk, proof["public"], parsed.values, *ch)


@pytest.fixture(scope="module", params=[4, 8])
def proved(request):
    circuit, assignment, st = _case(request.param)
    return circuit, assignment, st, lm.prove(circuit, assignment, TAU, st)


def test_an_honest_proof_verifies(proved):
    circuit, _, st, proof = proved
    assert proof["total"] == 1 and proof["zeros"] == 0 and proof["s_total"] == 0 and proof["s_zeros"] == 0
    assert proof["t"][3 * circuit.n:] == [0] * circuit.n
    assert len(proof["bytes"]) == lm.PROOF_BYTES == 1088 and len(st["vk"]) == lm.VK_BYTES == 392
    assert sum(proof["m"]) == sum(circuit.q_lookup) > 0
    assert lm.verify_exponent(st, circuit, proof["public"], proof, TAU)
    assert _package_identity(st, proof)


def test_a_wrong_public_input_fails(proved):
    circuit, _, st, proof = proved
    assert not lm.verify_exponent(st, circuit, [(proof["public"][0] + 1) % R], proof, TAU)
    assert not _package_identity(st, dict(proof, public=[(proof["public"][0] + 1) % R]))


@pytest.mark.parametrize("which", range(23))
def test_every_value_altered_by_one_fails(proved, which):
    circuit, _, st, proof = proved
    bad = dict(proof)
    bad["values"] = list(proof["values"])
    bad["values"][which] = (bad["values"][which] + 1) % R
    assert not lm.verify_exponent(st, circuit, proof["public"], bad, TAU)
    assert not _package_identity(st, bad)


@pytest.mark.parametrize("tamper", ["tuple", "m", "S"])
def test_a_tampered_proof_is_refused(proved, tamper):
    """an out-of-table tuple with m forced, m off by one, S shifted by a constant: the quotient is no polynomial, and
    the honest opening of its low three quarters fails the identity"""
    circuit, assignment, st, _ = proved
    bad = lm.prove(circuit, assignment, TAU, st, tamper=tamper)
    assert any(bad["t"][3 * circuit.n:])
    n, ch, _, _, _ = lm._statement(st["vk"], bad["public"], lm.parse_proof(bad["bytes"]))
    assert not lm.identity_holds(n, bad["public"], bad["values"], *ch)
    assert not lm.verify_exponent(st, circuit, bad["public"], bad, TAU)
    assert not _package_identity(st, bad)


def test_a_vanilla_proof_and_a_lookup_proof_do_not_share_a_transcript(proved):
    _, _, st, proof = proved
    cs = proof["commitments"]
    assert pm.challenges(st["vk"], proof["public"], cs[:3])[0] != proof["beta"]
    assert plonk.challenges(st["vk"], proof["public"], cs[:3])[0] != lookup_challenges(st["vk"], proof["public"], cs[:4])[0]
    assert len({proof[k] for k in ("beta", "gamma", "eta", "theta", "alpha", "z")}) == 6


@pytest.mark.parametrize("seed", range(6))
def test_the_logup_identity_on_random_small_cases(seed):
    """sum_i m_i / (theta + t_i) = sum_i qK_i / (theta + f_i) exactly when every looked-up tuple is in the table, with
    m counted at the first of equal rows; the padded table's copies carry 0"""
    rng = random.Random(3100 + seed)
    length, n_rows = rng.choice([5, 8, 13]), rng.choice([1, 2, 4])
    table = [tuple(rng.randrange(4) for _ in range(3)) for _ in range(n_rows)]
    table.append(table[0])                                                # a duplicate of the first row
    qk = [rng.randrange(2) for _ in range(length)]
    rows = [table[rng.randrange(len(table))] for _ in range(length)]
    wires = [[row[j] + R * (i % 2) for i, row in enumerate(rows)] for j in range(3)]     # every other one as v + r
    m, missing, first = lm.multiplicities(wires, qk, table, length + 2)
    assert missing == 0 and first == lm.MISSING_NONE and sum(m) == sum(qk)
    seen = set()
    for i, row in enumerate(table):
        assert row not in seen or m[i] == 0
        seen.add(row)
    assert m[len(table):] == [0] * (length + 2 - len(table))
    padded = table + [table[-1]] * (length + 2 - len(table))
    held = LookupCircuit(8, [[0] * 8] * 5, [[0] * 8] * 3, 0, (qk + [0] * 8)[:8], table)     # the package pads alike
    assert held.table_columns() == [[row[j] for row in (table + [table[-1]] * 8)[:8]] for j in range(3)] and held.n_table == len(table)
    key4 = [qk + [0, 0]] + [[row[j] for row in padded] for j in range(3)]
    wide = [col + [9, 9] for col in wires]
    eta, theta = rng.randrange(R), rng.randrange(R)
    s, total, zeros = lm.lookup_sum(wide, key4, m, eta, theta)
    assert s[0] == 0 and total == 0 and zeros == 0
    # one count too many, or one tuple outside the table: the sum does not close
    at = m.index(max(m)) if sum(m) else 0
    assert lm.lookup_sum(wide, key4, m[:at] + [m[at] + 1] + m[at + 1:], eta, theta)[1] != 0
    if sum(qk):
        i = qk.index(1)
        off = [col[:i] + [col[i] + 7] + col[i + 1:] for col in wide]
        assert lm.multiplicities(off, key4[0], table, length + 2)[1:] == (1, i)
        assert lm.lookup_sum(off, key4, m, eta, theta)[1] != 0


def test_a_zero_denominator_counts_as_zero_and_is_counted():
    rng = random.Random(3190)
    table = [(1, 2, 3), (4, 5, 6)]
    wires, qk = [[1, 4, 1], [2, 5, 2], [3, 6, 3]], [1, 1, 0]
    key4 = [qk, [1, 4, 4], [2, 5, 5], [3, 6, 6]]
    m = lm.multiplicities(wires, qk, table, 3)[0]
    eta = rng.randrange(R)
    theta = -(1 + 2 * eta + 3 * eta * eta) % R                           # theta + t_0 = theta + f_0 = theta + f_2 = 0
    s, total, zeros = lm.lookup_sum(wires, key4, m, eta, theta)
    assert zeros == 3 and s[:2] == [0, 0] and total == 0
    assert s[2] == (pm.inv(theta + 4 + 5 * eta + 6 * eta * eta) * (m[1] - 1)) % R


# ---------------------------------------------------------------------------- the package, host only
def test_the_builder_rules_for_tables():
    b = plonk.Builder()
    x, y, w = b.public(), b.var(), b.var()
    b.mul(x, y, w)
    with pytest.raises(ValueError, match="table"):
        b.lookup(x, y, w)
    with pytest.raises(ValueError):
        b.table([])
    with pytest.raises(ValueError):
        b.table([(1, 2)])
    b.table([(i, i + 1, 2 * i + R) for i in range(5)])
    with pytest.raises(ValueError, match="already"):
        b.table([(1, 2, 3)])
    with pytest.raises(ValueError):
        b.lookup(x, y, 99)
    b.lookup(x, y, w)
    circuit = b.build()
    assert isinstance(circuit, plonk.LookupCircuit) and isinstance(circuit, plonk.Circuit)
    assert circuit.n == 8 and circuit.n_table == 5                       # 3 rows, but a table of 5
    assert circuit.q_lookup == [0, 0, 1, 0, 0, 0, 0, 0]
    assert [col[2] for col in circuit.selectors] == [0] * 5 and [col[2] for col in circuit.wires] == [x, y, w]
    assert circuit.table[4] == (4, 5, 8) and [col[7] for col in circuit.table_columns()] == [4, 5, 8]
    assert [col[4] for col in circuit.table_columns()] == [4, 5, 8]


def test_a_vanilla_builder_still_builds_a_plain_circuit():
    b = plonk.Builder()
    x, y, w = b.public(), b.var(), b.var()
    b.mul(x, y, w)
    circuit = b.build()
    assert type(circuit) is plonk.Circuit and circuit.n == 2 and not hasattr(circuit, "q_lookup")


def test_the_lookup_circuit_validates_its_columns():
    sel, wires = [[0, 0]] * 5, [[0, 1], [0, 1], [0, 1]]
    assert plonk.LookupCircuit(2, sel, wires, 0, [0, 1], [(R + 1, 2, 3)]).table == [(1, 2, 3)]
    for q_lookup, table in (([0, 2], [(1, 2, 3)]), ([0], [(1, 2, 3)]), ([0, 1], []), ([0, 1], [(1, 2, 3)] * 3),
                            ([0, 1], [(1, 2)])):
        with pytest.raises(ValueError):
            plonk.LookupCircuit(2, sel, wires, 0, q_lookup, table)


def test_the_challenges_are_the_models(proved):
    _, _, st, proof = proved
    cs = proof["commitments"]
    got = lookup_challenges(st["vk"], proof["public"], cs[:4], cs[4:6], cs[6:])
    assert got == tuple(proof[k] for k in ("beta", "gamma", "eta", "theta", "alpha", "z"))
    assert lookup_challenges(st["vk"], proof["public"], cs[:4]) == got[:4]


def test_proof_bytes_round_trip_and_are_parsed_strictly(proved):
    _, _, _, proof = proved
    raw = proof["bytes"]
    p = plonk.LookupProof.from_bytes(raw)
    assert p.to_bytes() == raw and list(p.values) == proof["values"] and len(raw) == plonk.LOOKUP_PROOF_BYTES == 1088
    for bad in (raw[:-1], raw + b"\0", raw[:800]):
        with pytest.raises(ValueError, match="length"):
            plonk.LookupProof.from_bytes(bad)
    for which, name in ((3, "m"), (15, "qK"), (22, "S at z omega")):
        at = 288 + 32 * which
        with pytest.raises(ValueError, match="value %s " % name):
            plonk.LookupProof.from_bytes(raw[:at] + kr.le(R) + raw[at + 32:])
    for which, name in ((3, r"\[m\]"), (5, r"\[S\]"), (33, "W'")):
        at = 32 * which if which < 9 else 1056
        with pytest.raises(ValueError, match=name):
            plonk.LookupProof.from_bytes(raw[:at] + b"\xff" * 32 + raw[at + 32:])
    with pytest.raises(ValueError):
        plonk.Proof.from_bytes(raw)


def test_verifying_key_bytes_round_trip_and_are_parsed_strictly(proved):
    circuit, _, st, _ = proved
    raw = st["vk"]
    vk = plonk.LookupVerifyingKey.from_bytes(raw)
    assert vk.to_bytes() == raw and (vk.n, vk.n_public) == (circuit.n, 1) and len(raw) == plonk.LOOKUP_VK_BYTES == 392
    for bad in (raw[:-1], raw + b"\0", raw[:264]):
        with pytest.raises(ValueError, match="length"):
            plonk.LookupVerifyingKey.from_bytes(bad)
    with pytest.raises(ValueError, match="power of two"):
        plonk.LookupVerifyingKey.from_bytes((6).to_bytes(4, "little") + raw[4:])
    with pytest.raises(ValueError, match="n_public"):
        plonk.LookupVerifyingKey.from_bytes(raw[:4] + (circuit.n + 1).to_bytes(4, "little") + raw[8:])
    at = 8 + 32 * 9
    with pytest.raises(ValueError, match=r"\[T1\]"):
        plonk.LookupVerifyingKey.from_bytes(raw[:at] + b"\xff" * 32 + raw[at + 32:])
    with pytest.raises(ValueError):
        plonk.VerifyingKey.from_bytes(raw)
