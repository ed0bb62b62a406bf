"""The setup from a powers-of-tau string without a GPU: the integer model
(tests/srs_setup_ref.py) against the code that exists, the per-lane functions of the point kernels
(octopuszk_amd/csrc/ec_fft.cuh, built for the host) against the model, and the argument errors that need no device."""
import ctypes
import os
import random
import subprocess

import pytest

import ceremony_ref as cref
import codec_cases as cases
import srs_setup_ref as sref
from oracle import bn254 as o
from oracle import groth16 as g

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "ecfft_hostcheck.cpp")
LIB = os.path.join(HERE, "native", "_ecfft_hostcheck.so")
CSRC = os.path.join(HERE, "..", "octopuszk_amd", "csrc")
R, Q = o.R, o.Q
TAU, ALPHA, BETA = 0x1234567 % R, 0xABCDEF0123456789ABCDEF % R, pow(7, 100, R)


@pytest.fixture(scope="module")
def efhc():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("ec_fft.cuh", "points_scale.cuh", "glv.cuh", "fq2.cuh", "fp29.cuh",
                                                    "ec.cuh", "curve.cuh", "consts_gen.h")]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


def _words(b):
    return (ctypes.c_uint32 * (len(b) // 4)).from_buffer_copy(b)


def _le(v):
    return int(v).to_bytes(32, "little")


# ---------------------------------------------------------------------------- the model
@pytest.mark.parametrize("m", [2, 4, 8, 16, 32, 64])
def test_inverse_dft_of_the_powers_is_the_lagrange_basis(m):
    """pins omega and 1 / n to the code that exists: L_j(tau) = inverse DFT of (tau^i)"""
    for tau in (TAU, 5, R - 1):
        assert sref.inverse_dft([pow(tau, i, R) for i in range(m)]) == g.lagrange_coefficients(tau, m)


def test_model_transform_splits_as_the_definition():
    rng = random.Random(3)
    vals = [rng.randrange(R) for _ in range(256)]
    omega = o.fr_root_of_unity(256)
    assert sref.dft(vals, omega) == o.naive_dft(vals, omega)
    assert sref.inverse_dft(sref.dft(vals, omega)) == vals


@pytest.mark.parametrize("circuit", ["serial", "handmade"])
def test_model_key_satisfies_groth16_in_the_exponent(circuit):
    r1cs, primary, auxiliary = g.serial_construct(8, 3) if circuit == "serial" else sref.handmade_r1cs()
    m = g.lowest_power_of_two(r1cs.num_constraints + r1cs.num_inputs)
    key = sref.setup_exp(r1cs, sref.srs_exp(m, TAU, ALPHA, BETA))
    crs = sref.as_oracle_crs(r1cs, key)
    full, H, _, _ = g.r1cs_to_qap_witness(r1cs, primary, auxiliary)
    abc = g.proof_scalars(crs, full, H, 11, 13)
    assert g.verify_in_the_exponent(crs, primary, abc)
    assert not g.verify_in_the_exponent(crs, [primary[0], (primary[1] + 1) % R] + primary[2:], abc)
    # a wrong witness: H no longer is the quotient
    wrong = list(auxiliary)
    wrong[1] = (wrong[1] + 1) % R
    assert not g.is_satisfied(r1cs, primary, wrong)
    full_w, H_w, _, _ = g.r1cs_to_qap_witness(r1cs, primary, wrong)
    assert not g.verify_in_the_exponent(crs, primary, g.proof_scalars(crs, full_w, H_w, 11, 13))
    # and the key of another tau does not take the proof
    other = sref.as_oracle_crs(r1cs, sref.setup_exp(r1cs, sref.srs_exp(m, TAU + 1, ALPHA, BETA)))
    assert not g.verify_in_the_exponent(other, primary, abc)


def test_model_refuses_a_string_of_another_size():
    r1cs, _, _ = g.serial_construct(8, 3)
    with pytest.raises(ValueError):
        sref.setup_exp(r1cs, sref.srs_exp(8, TAU, ALPHA, BETA))


# ---------------------------------------------------------------------------- the kernels' pieces on the host
@pytest.mark.parametrize("type_", [1, 2])
def test_twiddle_recoding_reconstructs_the_twiddle(efhc, type_):
    rng = random.Random(21)
    omega = o.fr_root_of_unity(1 << 20)
    cases_ = [(omega, 1, i) for i in (0, 1, 2, 3, 1 << 19, (1 << 19) - 1, (1 << 21) - 1)]
    cases_ += [(pow(omega, -1, R), pow(1 << 20, -1, R), i) for i in (0, 1, 77, (1 << 19) - 1)]
    cases_ += [(rng.randrange(R), rng.randrange(R), rng.randrange(1 << 22)) for _ in range(40)]
    cases_ += [(0, 5, 0), (0, 5, 1), (R - 1, R - 1, 3)]
    for base, k, i in cases_:
        want = k * pow(base, i, R) % R
        out = (ctypes.c_uint32 * 8)()
        efhc.efhc_twiddle(_words(_le(base)), _words(_le(k)), i, out)
        assert int.from_bytes(bytes(out), "little") == want, (base, k, i)
        steps = (ctypes.c_uint8 * 256)()
        n = efhc.efhc_schedule(_words(_le(base)), _words(_le(k)), i, type_, steps)
        assert 0 <= n <= (130 if type_ == 1 else 255)
        assert cref.schedule_value(list(steps[:n]), type_) == want


def _points(type_):
    C = cases.curve(type_)
    rng = random.Random(50 + type_)
    P = C.to_affine(C.mul(C.one, rng.randrange(1, R)))
    S = C.to_affine(C.mul(C.one, rng.randrange(1, R)))
    J = cases.rescale(type_, S, rng.randrange(2, Q))
    return C, P, S, J, C.zero


def _sum(C, A, B, negate=False):
    return C.to_affine(C.add(A, C.negate(B) if negate and not C.is_zero(B) else B))


@pytest.mark.parametrize("type_", [1, 2])
def test_butterfly_matches_the_model(efhc, type_):
    """every pair the exceptional inputs of a transform produce: a == [w] b, a == -[w] b, O on either side, Z != 1"""
    C, P, S, J, O = _points(type_)
    n = 24 * type_
    w = pow(o.fr_root_of_unity(64), 5, R)
    wP = C.to_affine(C.mul(P, w))
    pairs = [(P, S), (P, P), (wP, P), (C.to_affine(C.negate(wP)), P), (O, P), (P, O), (O, O), (J, P), (P, J)]
    for ka, kb in ((None, None), (None, w), (pow(64, -1, R), w), (None, 0), (None, 1), (None, R - 1)):
        for A, B in pairs:
            oa, ob = (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
            efhc.efhc_butterfly(_words(cases.wire(type_, A, 0)), _words(cases.wire(type_, B, 0)), type_,
                                None if ka is None else _words(_le(ka)), None if kb is None else _words(_le(kb)), oa, ob)
            a = cref.scale(type_, A, 1 if ka is None else ka)
            v = cref.scale(type_, B, 1 if kb is None else kb)
            assert bytes(oa) == cref.wire(type_, _sum(C, a, v)), (ka, kb, A, B)
            assert bytes(ob) == cref.wire(type_, _sum(C, a, v, True)), (ka, kb, A, B)


@pytest.mark.parametrize("type_", [1, 2])
def test_sum_and_sparse_term_match_the_model(efhc, type_):
    C, P, S, J, O = _points(type_)
    n = 24 * type_
    rng = random.Random(8)
    for A, B in ((P, S), (P, P), (O, P), (P, O), (O, O), (J, S), (S, J)):
        for negate in (0, 1):
            out = (ctypes.c_uint32 * n)()
            efhc.efhc_add(_words(cases.wire(type_, A, 0)), _words(cases.wire(type_, B, 0)), type_, negate, out)
            assert bytes(out) == cref.wire(type_, _sum(C, A, B, bool(negate))), (A, B, negate)
        for c in (None, 0, 1, R - 1, 2, rng.randrange(1 << 253, R), R, R + 1, (1 << 256) - 1):
            out = (ctypes.c_uint32 * n)()
            efhc.efhc_term(_words(cases.wire(type_, A, 0)), _words(cases.wire(type_, B, 0)),
                           None if c is None else _words(_le(c)), type_, out)
            want = _sum(C, C.to_affine(A), cref.scale(type_, B, 1 if c is None else c % R))
            assert bytes(out) == cref.wire(type_, want), (A, B, c)


@pytest.mark.parametrize("type_", [1, 2])
def test_wire_point_reader_and_writer_round_trip(efhc, type_):
    """CurveIO::aff_from_wire then write<WireIn> (curve.cuh), the reader and writer every point kernel shares: Z = 0
    (in both spellings), Z = 1, a random Z, and Z = q given as raw words, which reads as O; byte for byte against
    the oracle's affine point"""
    C, P, S, J, O = _points(type_)
    n = 24 * type_
    flat = (lambda A: list(A)) if type_ == 1 else (lambda A: [c for xy in A for c in xy])
    raw = lambda A: b"".join(_le(c) for c in flat(A))
    zq = Q if type_ == 1 else (Q, 0)
    z0 = 0 if type_ == 1 else (0, 0)
    zqq = Q if type_ == 1 else (Q, Q)
    for A, want in ((O, O), ((P[0], P[1], z0), O), (P, P), (S, S), (J, S), ((J[0], J[1], zq), O), ((P[0], P[1], zqq), O)):
        out = (ctypes.c_uint32 * n)()
        efhc.efhc_roundtrip(_words(raw(A)), type_, out)
        assert bytes(out) == cref.wire(type_, C.to_affine(want)), A


def test_sparse_term_is_exact_outside_the_subgroup(efhc):
    """the per-lane ladder of a general coefficient assumes no subgroup: [r] P of such a twist point is not O"""
    P = cref.twist_point_outside_the_subgroup()
    c = random.Random(4).randrange(1 << 253, R)
    out = (ctypes.c_uint32 * 48)()
    efhc.efhc_term(_words(cases.wire(2, o.G2.zero, 0)), _words(cases.wire(2, P, 0)), _words(_le(c)), 2, out)
    assert bytes(out) == cref.wire(2, cref.scale(2, P, c))


# ---------------------------------------------------------------------------- arguments
def test_the_library_mirror_lists_the_new_entry_points():
    from octopuszk_amd import lib
    for name in ("ozk_ec_fft_dev", "ozk_ec_fft_workspace_bytes", "ozk_sparse_mat_points_dev",
                 "ozk_sparse_mat_points_workspace_bytes", "ozk_points_add_dev"):
        assert name in lib.exported_symbols()
    header = open(os.path.join(HERE, "..", "include", "ozk.h")).read()
    for name in ("ozk_ec_fft_dev(", "ozk_sparse_mat_points_dev(", "ozk_points_add_dev("):
        assert name in header


def test_argument_errors_without_a_device():
    from octopuszk_amd import srs
    for m in (0, 1, 3, 12):
        with pytest.raises(ValueError):
            srs.Srs.from_secrets(m, TAU, ALPHA, BETA)
    assert srs.CHECKS == ("shape", "powers_g1", "powers_g2", "alpha_powers", "beta_powers", "beta_g2")
    # the weight stream has its own tag: it is not the stream of a phase-2 check over the same seed
    from octopuszk_amd import ceremony, transcript
    assert transcript.weights(b"s", 3, srs._RHO_TAG) != transcript.weights(b"s", 3, ceremony._RHO_TAG)
    w = transcript.weights(b"s", 3, srs._RHO_TAG)
    assert len(w) == 96 and all(w[32 * i + 16:32 * i + 32] == bytes(16) and any(w[32 * i:32 * i + 16]) for i in range(3))
