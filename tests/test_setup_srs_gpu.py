"""The Groth16 setup from a powers-of-tau string on hardware (octopuszk_amd/srs.py): the key
against the integer model point for point, proofs under it, contributions on top of it, the key file, a circuit with
real coefficients, and every way a malformed string fails its check."""
import functools

import pytest
import torch

import ceremony_ref as cref
import codec_cases as cases
import srs_gpu_util as u
import srs_setup_ref as sref
from oracle import bn254 as o
from oracle import groth16 as g

pytestmark = pytest.mark.gpu
R = o.R
TAU, ALPHA, BETA = 0x1234567890ABCDEF % R, 0xABCDEF0123456789ABCDEF % R, pow(7, 100, R)
SEED = b"seed of the srs tests"
SHAPES = [(100, 3), (13, 3)]        # m = 128 and m = 16


@functools.lru_cache(maxsize=None)
def _gen():
    from octopuszk_amd import zksnark as z
    return z.fr_random(z.SEED)


@functools.lru_cache(maxsize=None)
def _srs(m, tau=TAU):
    from octopuszk_amd import srs
    return srs.Srs.from_secrets(m, tau, ALPHA, BETA)


@functools.lru_cache(maxsize=None)
def _made(nc, ni, tau=TAU):
    from octopuszk_amd import zksnark as z
    r1cs, primary, auxiliary = z.serial_construct(nc, ni)
    m = z.lowest_power_of_two(nc + ni)
    crs = z.setup_from_srs(r1cs, _srs(m, tau))
    return dict(crs=crs, pk=crs.proving_key, vk=z.verification_key(crs), primary=primary, auxiliary=auxiliary, m=m)


def _compare(crs, key):
    pk = crs.proving_key
    for names, type_ in ((sref.G1_FIELDS, 1), (sref.G2_FIELDS, 2)):
        for name in names:
            t = getattr(crs, name) if name in ("gamma_g2", "gamma_abc_g1") else getattr(pk, name)
            exps = key[name] if isinstance(key[name], list) else [key[name]]
            assert t.numel() == 96 * type_ * len(exps), name
            assert u.compress(t, type_) == u.expected(type_, exps, _gen()), name


@pytest.mark.parametrize("nc,ni", SHAPES)
def test_string_is_well_formed_and_the_key_is_the_model_key(nc, ni):
    made = _made(nc, ni)
    assert _srs(made["m"]).check(seed=SEED)
    assert _srs(made["m"]).check()
    r1cs, _, _ = g.serial_construct(nc, ni)
    _compare(made["crs"], sref.setup_exp(r1cs, sref.srs_exp(made["m"], TAU, ALPHA, BETA)))
    assert made["crs"].secrets is None and made["pk"].r1cs is not None and made["crs"].timing


def _prove(pk, primary, auxiliary):
    from octopuszk_amd import zksnark as z
    p = z.SerialProver(pk)
    proof = p.prove(primary, auxiliary, seed=5)
    p.close()
    return proof


@pytest.mark.parametrize("nc,ni", SHAPES)
def test_proofs_verify_under_the_key_and_only_under_it(nc, ni):
    from octopuszk_amd import zksnark as z
    made = _made(nc, ni)
    primary, auxiliary = made["primary"], made["auxiliary"]
    proof = _prove(made["pk"], primary, auxiliary)
    assert z.Verifier.verify(made["vk"], primary, proof)
    assert not z.Verifier.verify(made["vk"], [primary[0], (primary[1] + 1) % R] + list(primary[2:]), proof)
    assert not z.Verifier.verify(_made(nc, ni, TAU + 1)["vk"], primary, proof)


def test_contributions_and_the_key_file(tmp_path):
    from octopuszk_amd import ceremony
    from octopuszk_amd import zksnark as z
    made = _made(100, 3)
    pk, vk, primary, auxiliary = made["pk"], made["vk"], made["primary"], made["auxiliary"]
    pk2, vk2, rec = pk.contribute(vk, 0x1234567890ABCDEF1234567890ABCDEF % R, nonce=77)
    pk3, vk3, rec3 = pk2.contribute(vk2, 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % R, nonce=78, previous=rec.to_bytes())
    assert ceremony.verify_chain([pk, pk2, pk3], [rec, rec3], vks=[vk, vk2, vk3], seed=SEED)
    proof = _prove(pk3, primary, auxiliary)
    assert z.Verifier.verify(vk3, primary, proof)
    assert not z.Verifier.verify(vk, primary, proof)
    path = str(tmp_path / "from_srs.ozkpk")
    pk.save(path)
    back = z.ProvingKey.load(path)
    for name in z._PK_G1 + z._PK_G2:
        type_ = 1 if name in z._PK_G1 else 2
        assert u.compress(getattr(back, name), type_) == u.compress(getattr(pk, name), type_), name
    pf = z.SerialProver.from_key_file(path)
    assert z.Verifier.verify(vk, primary, pf.prove(primary, auxiliary, seed=5))
    pf.close()


def test_circuit_with_real_coefficients():
    from octopuszk_amd import zksnark as z
    r1cs, primary, auxiliary = sref.handmade_r1cs()
    rel = u.relation(r1cs)
    assert z.is_satisfied(rel, primary, auxiliary)
    crs = z.setup_from_srs(rel, _srs(16))
    _compare(crs, sref.setup_exp(r1cs, sref.srs_exp(16, TAU, ALPHA, BETA)))
    vk = z.verification_key(crs)
    proof = _prove(crs.proving_key, primary, auxiliary)
    assert z.Verifier.verify(vk, primary, proof)
    assert not z.Verifier.verify(vk, [primary[0], primary[1], (primary[2] + 1) % R], proof)


# ---------------------------------------------------------------------------- malformed strings
def _altered(**changes):
    from octopuszk_amd import srs
    s = _srs(16)
    fields = dict(tau_g1=s.tau_g1, tau_g2=s.tau_g2, alpha_tau_g1=s.alpha_tau_g1, beta_tau_g1=s.beta_tau_g1, beta_g2=s.beta_g2)
    fields.update(changes)
    return srs.Srs(16, **fields)


def _put(t, type_, index, point_bytes):
    n = 96 * type_
    out = t.reshape(-1).clone()
    out[n * index:n * (index + 1)] = point_bytes if isinstance(point_bytes, torch.Tensor) else u.dev(point_bytes)
    return out


def _other(t, type_, index):
    """the array with the point at `index` replaced by its neighbour below: a valid point of the group, the wrong one"""
    n = 96 * type_
    return _put(t, type_, index, t.reshape(-1)[n * (index - 1):n * index].clone())


TAMPERS = [("tau_g1", 1, 1, "powers_g1"), ("tau_g1", 1, 32, "powers_g1"),
           ("tau_g2", 2, 1, "powers_g1"), ("tau_g2", 2, 15, "powers_g2"),      # tau_g2[1] anchors the G1 shift test
           ("alpha_tau_g1", 1, 1, "alpha_powers"), ("alpha_tau_g1", 1, 15, "alpha_powers"),
           ("beta_tau_g1", 1, 1, "beta_powers"), ("beta_tau_g1", 1, 15, "beta_powers")]


@pytest.mark.parametrize("name,type_,index,check", TAMPERS)
def test_one_altered_point_fails_its_check(name, type_, index, check):
    s = _srs(16)
    why = []
    assert not _altered(**{name: _other(getattr(s, name), type_, index)}).check(seed=SEED, why=why)
    assert why == [check]


def test_other_malformed_strings_fail_by_name():
    s = _srs(16)
    C2 = cases.curve(2)
    cases_ = [
        (dict(beta_g2=s.tau_g2.reshape(-1)[192:384].clone()), "beta_g2"),
        (dict(tau_g1=_put(s.tau_g1, 1, 1, cref.wire(1, o.G1.zero))), "shape"),
        (dict(tau_g2=_put(s.tau_g2, 2, 1, cref.wire(2, cref.twist_point_outside_the_subgroup()))), "shape"),
        (dict(beta_g2=u.dev(cref.wire(2, C2.to_affine(C2.zero)))), "shape"),
        (dict(tau_g1=s.tau_g1.reshape(-1)[:-96].clone()), "shape"),
        (dict(tau_g2=s.tau_g2.reshape(-1)[:-192].clone()), "shape"),
        (dict(alpha_tau_g1=s.alpha_tau_g1.reshape(-1)[:-96].clone()), "shape"),
        (dict(beta_tau_g1=s.beta_tau_g1.reshape(-1)[:-96].clone()), "shape"),
    ]
    for changes, check in cases_:
        why = []
        assert not _altered(**changes).check(seed=SEED, why=why), changes.keys()
        assert why == [check], (list(changes), why)
    assert s.check(seed=SEED)


def test_setup_refuses_a_string_of_another_size_and_a_tau_in_the_domain():
    from octopuszk_amd import srs
    from octopuszk_amd import zksnark as z
    r1cs, _, _ = z.serial_construct(13, 3)
    with pytest.raises(ValueError, match="16.*128|128.*16"):
        z.setup_from_srs(r1cs, _srs(128))
    inside = srs.Srs.from_secrets(16, pow(o.fr_root_of_unity(16), 3, R), ALPHA, BETA)
    with pytest.raises(ValueError, match="domain"):
        z.setup_from_srs(r1cs, inside)
