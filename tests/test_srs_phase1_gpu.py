"""Phase-1 contributions to a powers-of-tau string and the string file on hardware (octopuszk_amd/srs.py, DESIGN.md
section 21): the contributed string against the string of the multiplied secrets, acceptance of honest steps and chains,
every tamper class of tests/test_srs_phase1_cpu.py by the name of its check, the file's round trip and refusals, and a
key built at the end of a chain."""
import functools
import hashlib
import random

import pytest
import torch

import codec_cases as cases
import srs_gpu_util as u
from oracle import bn254 as o

pytestmark = pytest.mark.gpu
R = o.R
T, AL, BE = 0x1234567890ABCDEF % R, 0xABCDEF0123456789ABCDEF % R, pow(7, 100, R)
S, A, B = 0x1234567890ABCDEF1234567890ABCDEF % R, 0xFEDCBA0987654321 % R, pow(5, 77, R)
NONCES = (77, 1 << 200, R - 5)
SEED = b"seed of the phase-1 tests"
SIZES = (2, 8, 64)
ARRAYS = (("tau_g1", 1), ("tau_g2", 2), ("alpha_tau_g1", 1), ("beta_tau_g1", 1), ("beta_g2", 2))


@functools.lru_cache(maxsize=None)
def _before(m):
    from octopuszk_amd import srs
    return srs.Srs.from_secrets(m, T, AL, BE)


@functools.lru_cache(maxsize=None)
def _step(m):
    """(the string after, the receipt bytes)"""
    return _before(m).contribute(S, A, B, nonces=NONCES)


def _encodings(s):
    return {name: u.compress(getattr(s, name), type_) for name, type_ in ARRAYS}


@pytest.mark.parametrize("m", SIZES)
def test_contribution_gives_the_string_of_the_multiplied_secrets(m):
    from octopuszk_amd import srs
    after, receipt = _step(m)
    want = srs.Srs.from_secrets(m, T * S % R, AL * A % R, BE * B % R)
    got, exp = _encodings(after), _encodings(want)
    for name, type_ in ARRAYS:
        assert got[name] == exp[name], name
        assert getattr(after, name).numel() == getattr(_before(m), name).numel()
    assert len(receipt) == 432 and after.m == m
    assert got["tau_g1"][:32] == _encodings(_before(m))["tau_g1"][:32]


@pytest.mark.parametrize("m", SIZES)
def test_honest_contribution_and_chain_are_accepted(m):
    from octopuszk_amd import srs
    after, receipt = _step(m)
    why = []
    assert srs.verify_contribution(_before(m), after, receipt, seed=SEED, why=why), why
    s0 = srs.Srs.initial(m)
    s1, r1 = s0.contribute(S, A, B, nonces=NONCES)
    s2, r2 = s1.contribute(previous=r1)                                  # secrets and nonces drawn inside
    assert srs.verify_chain([s0, s1, s2], [r1, r2], seed=SEED, why=why), why
    assert srs.verify_chain([s0, s1, s2], [r1, r2])                      # unseeded weights
    assert _encodings(s1) == _encodings(srs.Srs.from_secrets(m, S, A, B))
    # a broken link
    s2b, r2b = s1.contribute(5, 6, 7, nonces=NONCES, previous=b"not the receipt before")
    assert not srs.verify_chain([s0, s1, s2b], [r1, r2b], seed=SEED, why=why) and why == ["chain"]


# ---------------------------------------------------------------------------- tampers, m = 8
M = 8


def _altered(s, **changes):
    from octopuszk_amd import srs
    fields = dict(tau_g1=s.tau_g1, tau_g2=s.tau_g2, alpha_tau_g1=s.alpha_tau_g1, beta_tau_g1=s.beta_tau_g1, beta_g2=s.beta_g2)
    fields.update(changes)
    return srs.Srs(s.m, **fields)


def _other(t, type_, index, source=None):
    """the array with the point at `index` replaced by the one at `source` (default: its neighbour below): a valid
    point of the group, the wrong one"""
    n = 96 * type_
    source = index - 1 if source is None else source
    out = t.reshape(-1).clone()
    out[n * index:n * (index + 1)] = t.reshape(-1)[n * source:n * (source + 1)]
    return out


def _wrong_base_receipt():
    """alpha's proof of knowledge taken over tau's base: R = u tau_g1[1], z answering the challenge that R gets"""
    from octopuszk_amd import ceremony, srs
    rec = srs.Receipt.from_bytes(_step(M)[1])
    base = _before(M).tau_g1.reshape(-1)[96:192]
    r_enc = u.compress(ceremony.scale_points(base, NONCES[1], 1), 1)
    before, after, _, _ = rec.blocks[1]
    rec.blocks[1] = (before, after, r_enc, 0)
    rec.blocks[1] = (before, after, r_enc, (NONCES[1] + rec.challenge(1) * A) % R)
    return rec.to_bytes()


TAMPERS = ("generator g1", "generator g2", "tau_g1 point", "tau_g2 point", "alpha_tau_g1 point", "beta_tau_g1 point",
           "beta_g2", "tau_g2 by other powers", "pok over the wrong base", "swapped h", "receipt m")


def _tamper(label):
    """(after, receipt, the check that must fail)"""
    from octopuszk_amd import srs
    after, receipt = _step(M)
    if label == "generator g1":
        return _altered(after, tau_g1=_other(after.tau_g1, 1, 0, 2)), receipt, "generators"
    if label == "generator g2":
        return _altered(after, tau_g2=_other(after.tau_g2, 2, 0, 1)), receipt, "generators"
    if label == "tau_g1 point":
        return _altered(after, tau_g1=_other(after.tau_g1, 1, 2 * M)), receipt, "wellformed"
    if label == "tau_g2 point":
        return _altered(after, tau_g2=_other(after.tau_g2, 2, M - 1)), receipt, "wellformed"
    if label == "alpha_tau_g1 point":
        return _altered(after, alpha_tau_g1=_other(after.alpha_tau_g1, 1, 2)), receipt, "wellformed"
    if label == "beta_tau_g1 point":
        return _altered(after, beta_tau_g1=_other(after.beta_tau_g1, 1, 1)), receipt, "wellformed"
    if label == "beta_g2":
        return _altered(after, beta_g2=after.tau_g2.reshape(-1)[192:384].clone()), receipt, "wellformed"
    if label == "tau_g2 by other powers":
        other = srs.Srs.from_secrets(M, T * (S + 1) % R, AL, BE)
        return _altered(after, tau_g2=other.tau_g2), receipt, "wellformed"
    if label == "pok over the wrong base":
        return after, _wrong_base_receipt(), "pok"
    if label == "swapped h":
        return after, receipt[:16] + hashlib.sha256(b"another").digest() + receipt[48:], "pok"
    if label == "receipt m":
        return after, receipt[:8] + (2 * M).to_bytes(8, "little") + receipt[16:], "receipt_points"
    raise KeyError(label)


@pytest.mark.parametrize("label", TAMPERS)
def test_each_tamper_class_fails_by_the_name_of_its_check(label):
    from octopuszk_amd import srs
    after, receipt, check = _tamper(label)
    why = []
    assert not srs.verify_contribution(_before(M), after, receipt, seed=SEED, why=why)
    assert why == [check]


# ---------------------------------------------------------------------------- the file
@pytest.mark.parametrize("m", SIZES)
def test_save_and_load_round_trip(m, tmp_path):
    from octopuszk_amd import srs
    after, _ = _step(m)
    path = str(tmp_path / "string.ozksrs")
    after.save(path)
    with open(path, "rb") as f:
        raw = f.read()
    assert len(raw) == srs.string_file_size(m) == 48 + 32 * (4 * m + 1) + 64 * (m + 1)
    back = srs.Srs.load(path)
    assert back.m == m and _encodings(back) == _encodings(after)
    assert _encodings(srs.Srs.load(raw)) == _encodings(after)            # bytes are accepted too
    parsed_m, sections = srs.parse_string_file(raw)
    assert parsed_m == m and all(sections[name] == enc for name, enc in _encodings(after).items())
    assert u.host(back.tau_g1)[64:96] == (1).to_bytes(32, "little")     # decoded with Z = 1


def test_load_refuses_a_flipped_byte_and_a_non_point(tmp_path):
    from octopuszk_amd import srs
    m = 8
    after, _ = _step(m)
    path = str(tmp_path / "string.ozksrs")
    after.save(path)
    with open(path, "rb") as f:
        raw = f.read()
    with pytest.raises(ValueError, match="digest"):
        srs.Srs.load(raw[:500] + bytes([raw[500] ^ 0x10]) + raw[501:])
    _, sections = srs.parse_string_file(raw)
    rng = random.Random(11)
    for name, type_, index in (("alpha_tau_g1", 1, 1), ("tau_g2", 2, m - 1), ("tau_g1", 1, 2 * m)):
        n = 32 * type_
        bad = dict(sections)
        bad[name] = sections[name][:n * index] + cases.non_residue_x(type_, rng) + sections[name][n * (index + 1):]
        with pytest.raises(ValueError, match="section %s: point %d " % (name, index)):
            srs.Srs.load(srs.string_file_bytes(m, bad))
    # the first of two bad points, in file order, is the one reported
    bad = dict(sections)
    bad["beta_tau_g1"] = cases.non_residue_x(1, rng) + sections["beta_tau_g1"][32:]
    bad["tau_g2"] = cases.non_residue_x(2, rng) + sections["tau_g2"][64:]
    with pytest.raises(ValueError, match="section beta_tau_g1: point 0 "):
        srs.Srs.load(srs.string_file_bytes(m, bad))


# ---------------------------------------------------------------------------- end to end
def test_a_key_from_the_end_of_a_chain_proves_and_verifies(tmp_path):
    from octopuszk_amd import ceremony, srs
    from octopuszk_amd import zksnark as z
    m = 8
    s0 = srs.Srs.initial(m)
    s1, r1 = s0.contribute()
    s2, r2 = s1.contribute(previous=r1)
    assert srs.verify_chain([s0, s1, s2], [r1, r2])
    path = str(tmp_path / "final.ozksrs")
    s2.save(path)
    final = srs.Srs.load(path)
    assert final.check()
    r1cs, primary, auxiliary = z.serial_construct(5, 3)
    assert z.lowest_power_of_two(5 + 3) == m
    crs = z.setup_from_srs(r1cs, final)
    pk, vk = crs.proving_key, z.verification_key(crs)
    pk2, vk2, rec = pk.contribute(vk)
    assert ceremony.verify_chain([pk, pk2], [rec], vks=[vk, vk2])
    prover = z.SerialProver(pk2)
    proof = prover.prove(primary, auxiliary, seed=5)
    prover.close()
    assert z.Verifier.verify(vk2, primary, proof)
    assert not z.Verifier.verify(vk, primary, proof)                     # the final key only
    assert not z.Verifier.verify(vk2, [primary[0], (primary[1] + 1) % R] + list(primary[2:]), proof)
