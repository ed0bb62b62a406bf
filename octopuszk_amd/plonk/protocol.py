"""Setup, prover and verifier of the PLONK package: the transcript, the byte formats and the order
of the device calls.  The group side is CommitKey.commit, CommitKey.open_multi and verify_multi; the field side is the
transform and the three kernels of csrc/plonk.cuh."""
import time

import numpy as np
import torch

from .. import kzg as _kzg
from .. import transcript as _transcript
from ..fft import FR, FR_MULT_GEN, root_of_unity
from ..vectors import fr_fft, fr_perm_product, fr_rows_coset, plonk_quotient
from ..wire import dev_bytes, ints32, le32, upload
from .circuit import K, N_MAX, Circuit

PROOF_BYTES = 7 * 32 + 16 * 32 + 64
VK_BYTES = 8 + 8 * 32
_BETA_TAG, _GAMMA_TAG, _ALPHA_TAG, _Z_TAG = b"OZK-plonk-beta", b"OZK-plonk-gamma", b"OZK-plonk-alpha", b"OZK-plonk-z"
_COMMITMENTS = ("[a]", "[b]", "[c]", "[Z]", "[t_lo]", "[t_mid]", "[t_hi]")
_KEY_COMMITMENTS = ("[qL]", "[qR]", "[qO]", "[qM]", "[qC]", "[s1]", "[s2]", "[s3]")
_VALUES = ("a", "b", "c", "t_lo", "t_mid", "t_hi", "qL", "qR", "qO", "qM", "qC", "s1", "s2", "s3", "Z", "Z at z omega")
STAGES = ("witness upload", "witness transforms", "grand product", "coset transforms", "quotient kernel", "commitments",
          "multi-opening")
_UPLOAD, _WITNESS, _PRODUCT, _COSET, _QUOTIENT, _COMMIT, _OPEN = STAGES


def _inv(v):
    return pow(v % FR, -1, FR)


# ---------------------------------------------------------------------------- bytes
class VerifyingKey:
    """n uint32 LE | n_public uint32 LE | [qL] [qR] [qO] [qM] [qC] [s1] [s2] [s3], compressed: 264 bytes"""

    def __init__(self, n, n_public, commitments):
        self.n, self.n_public = int(n), int(n_public)
        if self.n < 2 or self.n & (self.n - 1) or self.n > N_MAX:
            raise ValueError("verifying key: n = %d is not a power of two in [2, 2^26]" % self.n)
        if not 0 <= self.n_public <= self.n:
            raise ValueError("verifying key: n_public = %d, not in [0, n = %d]" % (self.n_public, self.n))
        self.commitments = tuple(bytes(c) for c in commitments)
        if len(self.commitments) != 8 or any(len(c) != 32 for c in self.commitments):
            raise ValueError("verifying key: eight commitments of 32 bytes")

    def to_bytes(self) -> bytes:
        return self.n.to_bytes(4, "little") + self.n_public.to_bytes(4, "little") + b"".join(self.commitments)

    @staticmethod
    def from_bytes(b) -> "VerifyingKey":
        """Strict and host-only: ValueError naming the field for a wrong length, n no power of two in [2, 2^26],
        n_public above n, a point that does not decode."""
        b = bytes(b)
        if len(b) != VK_BYTES:
            raise ValueError("verifying key: length %d, not %d" % (len(b), VK_BYTES))
        cs = [b[8 + 32 * i:40 + 32 * i] for i in range(8)]
        vk = VerifyingKey(int.from_bytes(b[:4], "little"), int.from_bytes(b[4:8], "little"), cs)
        _kzg.require_g1(zip(_KEY_COMMITMENTS, cs), "verifying key")
        return vk


class Proof:
    """[a] [b] [c] [Z] [t_lo] [t_mid] [t_hi] | the 16 values a, b, c, t_lo, t_mid, t_hi, qL, qR, qO, qM, qC, s1, s2, s3,
    Z at z, then Z at z omega | W | W': 800 bytes"""

    def __init__(self, commitments, values, w, w2):
        self.commitments = tuple(bytes(c) for c in commitments)
        self.values = tuple(int(v) for v in values)
        self.w, self.w2 = bytes(w), bytes(w2)
        if len(self.commitments) != 7 or any(len(c) != 32 for c in self.commitments + (self.w, self.w2)):
            raise ValueError("proof: seven commitments, W and W' of 32 bytes")
        if len(self.values) != 16 or any(not 0 <= v < FR for v in self.values):
            raise ValueError("proof: sixteen values in [0, r)")

    def to_bytes(self) -> bytes:
        return b"".join(self.commitments) + le32(self.values) + self.w + self.w2

    @staticmethod
    def from_bytes(b) -> "Proof":
        """Strict and host-only: ValueError naming the field for a wrong length, a value >= r, a point that does not
        decode."""
        b = bytes(b)
        if len(b) != PROOF_BYTES:
            raise ValueError("proof: length %d, not %d" % (len(b), PROOF_BYTES))
        values = ints32(b[224:736])
        for name, v in zip(_VALUES, values):
            if v >= FR:
                raise ValueError("proof: the value %s is not below r" % name)
        cs = [b[32 * i:32 * i + 32] for i in range(7)]
        _kzg.require_g1(list(zip(_COMMITMENTS, cs)) + [("W", b[736:768]), ("W'", b[768:])], "proof")
        return Proof(cs, values, b[736:768], b[768:])


# ---------------------------------------------------------------------------- the transcript
def challenges(vk_bytes, public_inputs, abc, z_commitment=None, t_commitments=None) -> tuple:
    """(beta, gamma[, alpha[, z]]), as far as the commitments given reach.  With D1 = SHA-256("OZK-plonk-beta" | the
    verifying key's bytes | the public inputs, 32 bytes each | [a] [b] [c]) and D2 = SHA-256("OZK-plonk-alpha" | D1 |
    [Z]): beta is drawn from D1, gamma from SHA-256("OZK-plonk-gamma" | D1), alpha from D2 and z from
    SHA-256("OZK-plonk-z" | D2 | [t_lo] [t_mid] [t_hi]); each is the first 16 bytes, little-endian, 1 if they are zero."""
    parts = (bytes(vk_bytes), le32(public_inputs), b"".join(abc))
    d1 = _transcript.digest(_BETA_TAG, *parts)
    out = [_transcript.challenge128(_BETA_TAG, *parts), _transcript.challenge128(_GAMMA_TAG, d1)]
    if z_commitment is not None:
        d2 = _transcript.digest(_ALPHA_TAG, d1, z_commitment)
        out.append(_transcript.challenge128(_ALPHA_TAG, d1, z_commitment))
        if t_commitments is not None:
            out.append(_transcript.challenge128(_Z_TAG, d2, b"".join(t_commitments)))
    return tuple(out)


# ---------------------------------------------------------------------------- transforms of rows
def _rows(values):
    """rows of host ints -> [k, 32 n] on the device"""
    return dev_bytes(le32(v for row in values for v in row)).view(len(values), -1)


def _interpolate(evals, k, n):
    """k rows of values on the domain of omega_n -> their coefficient rows (a new tensor)"""
    out = torch.empty_like(evals)
    w_inv = _inv(root_of_unity(n))
    for y in range(k):
        fr_fft(evals[y], n, w_inv, out[y])
    return fr_rows_coset(out, k, n, n, 1, _inv(n), out)


def _onto_coset(coeffs, k, n):
    """k coefficient rows of n -> their values at g omega_4n^i, i < 4 n (a new tensor)"""
    scaled = fr_rows_coset(coeffs, k, n, n, FR_MULT_GEN, 1, None, 4 * n)
    out = torch.empty_like(scaled)
    w4 = root_of_unity(4 * n)
    for y in range(k):
        fr_fft(scaled[y], 4 * n, w4, out[y])
    return out


def _off_coset(evals, n):
    """one row of 4 n values on the coset -> its 4 n coefficients (a new tensor)"""
    out = fr_fft(evals, 4 * n, _inv(root_of_unity(4 * n)))
    return fr_rows_coset(out, 1, 4 * n, 4 * n, _inv(FR_MULT_GEN), _inv(4 * n), out)


def zh_inverses(n):
    """1 / (g^n i4^m - 1), m < 4, i4 = omega_4n^n: all that 1 / Z_H takes on the coset"""
    i4 = pow(root_of_unity(4 * n), n, FR)
    return [_inv(pow(FR_MULT_GEN, n, FR) * pow(i4, m, FR) - 1) for m in range(4)]


# ---------------------------------------------------------------------------- setup
class ProvingKey:
    """What the prover keeps of one circuit: the circuit, the CommitKey, the eight coefficient rows qL .. s3 and the
    three rows of sigma labels on the device, the table of qL, qR, qO, qM, qC, s1, s2, s3, L_1 and the points
    themselves on the coset of 4 n points (10 x 4 n x 32 bytes on the device), and the verifying key."""

    def __init__(self, circuit, commit_key, coeffs, sigma, table, vk):
        self.circuit, self.commit_key, self.coeffs, self.sigma, self.table, self.vk = circuit, commit_key, coeffs, sigma, table, vk


def setup(circuit, commit_key):
    """(ProvingKey, VerifyingKey) of a circuit over a CommitKey of n bases: eight commitments, no secret"""
    if not isinstance(circuit, Circuit):
        raise TypeError("setup takes a plonk.Circuit")
    n = circuit.n
    if commit_key.n != n:
        raise ValueError("the circuit has n = %d gates, the commit key n = %d bases" % (n, commit_key.n))
    sigma = _rows(circuit.sigma_labels())
    coeffs = _interpolate(torch.cat([_rows(circuit.selectors), sigma]), 8, n)
    vk = VerifyingKey(n, circuit.n_public, commit_key.commit(coeffs))
    # L_1 = (X^n - 1) / (n (X - 1)) has every coefficient 1 / n; the points of the coset are the values of X
    extra = _rows([[_inv(n)] * n, [0, 1] + [0] * (n - 2)])
    table = _onto_coset(torch.cat([coeffs, extra]), 10, n)
    return ProvingKey(circuit, commit_key, coeffs, sigma, table, vk), vk


# ---------------------------------------------------------------------------- the prover
class _Clock:
    """seconds per stage into `into` (device work included: a stage ends with a synchronisation), or nothing"""

    def __init__(self, into):
        self.into, self.at = into, None
        if into is not None:
            torch.cuda.synchronize()
            self.at = time.perf_counter()

    def lap(self, stage):
        if self.into is None:
            return
        torch.cuda.synchronize()
        now = time.perf_counter()
        self.into[stage] = self.into.get(stage, 0.0) + now - self.at
        self.at = now


def prove(pk, assignment=None, timings=None, wire_values=None) -> Proof:
    """The proof of one assignment (one Fr value per variable: a list of ints, or their 32-byte little-endian records
    back to back as bytes, which are taken mod r), or of a witness produced elsewhere and given cell by cell
    (wire_values: the three columns a, b, c of n values).  ValueError, before any commitment to t, when the
    grand product does not close (a copy constraint is violated) or the quotient is no polynomial (a gate is violated,
    seen as a nonzero top quarter of its 4 n coefficients by one reduction on the device); RuntimeError when a
    denominator of the grand product is zero.  timings: a dict that receives the seconds of every stage of STAGES."""
    circuit, ck, n = pk.circuit, pk.commit_key, pk.circuit.n
    omega = root_of_unity(n)
    vk_bytes = pk.vk.to_bytes()
    if (assignment is None) == (wire_values is None):
        raise ValueError("prove takes an assignment or the three columns of wire values")
    clock = _Clock(timings)
    if wire_values is None:
        # one 32-byte record per variable, gathered into the three columns by the circuit's index
        if isinstance(assignment, (bytes, bytearray)):
            if len(assignment) != 32 * circuit.n_vars:
                raise ValueError("%d bytes for %d variables of 32 bytes" % (len(assignment), circuit.n_vars))
            raw = bytes(assignment)
        else:
            raw = le32(circuit.checked_assignment(assignment))
        records = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 32)
        host = records[circuit.wire_index()].reshape(3, 32 * n)
        public = [int.from_bytes(raw[32 * v:32 * v + 32], "little") % FR for v in circuit.wires[0][:circuit.n_public]]
    else:
        values = [[int(v) for v in col] for col in wire_values]
        if len(values) != 3 or any(len(col) != n or any(not 0 <= v < FR for v in col) for col in values):
            raise ValueError("wire_values: three columns of n = %d values in [0, r)" % n)
        host = np.frombuffer(le32(v for col in values for v in col), dtype=np.uint8).reshape(3, 32 * n)
        public = values[0][:circuit.n_public]
    wires = upload(host)
    clock.lap(_UPLOAD)
    wire_coeffs = _interpolate(wires, 3, n)
    clock.lap(_WITNESS)
    abc = ck.commit(wire_coeffs)
    clock.lap(_COMMIT)
    beta, gamma = challenges(vk_bytes, public, abc)
    z_evals, total, zero_dens = fr_perm_product(wires, pk.sigma, n, n, omega, K, beta, gamma)
    if zero_dens:
        raise RuntimeError("the grand product met %d zero denominator(s) under these challenges" % zero_dens)
    if total != 1:
        raise ValueError("a copy constraint is violated: the grand product does not close")
    clock.lap(_PRODUCT)
    z_coeffs = _interpolate(z_evals.unsqueeze(0), 1, n)
    pi_evals = torch.zeros((1, 32 * n), dtype=torch.uint8, device=wires.device)
    if public:
        pi_evals[0, :32 * len(public)] = dev_bytes(le32((FR - x) % FR for x in public))
    pi_coeffs = _interpolate(pi_evals, 1, n)
    clock.lap(_WITNESS)
    z_commitment = ck.commit(z_coeffs)[0]
    clock.lap(_COMMIT)
    alpha = challenges(vk_bytes, public, abc, z_commitment)[2]
    wit = _onto_coset(torch.cat([wire_coeffs, z_coeffs, pi_coeffs]), 5, n)
    clock.lap(_COSET)
    t_evals = plonk_quotient(wit, 4 * n, pk.table, 4 * n, n, alpha, beta, gamma, K, zh_inverses(n))
    clock.lap(_QUOTIENT)
    t = _off_coset(t_evals, n)
    if bool(t[32 * 3 * n:].any().item()):
        raise ValueError("a gate is violated: the quotient is no polynomial")
    clock.lap(_COSET)
    t_rows = t[:32 * 3 * n].view(3, 32 * n)
    t_commitments = ck.commit(t_rows)
    clock.lap(_COMMIT)
    z = challenges(vk_bytes, public, abc, z_commitment, t_commitments)[3]
    if pow(z, n, FR) == 1:
        raise RuntimeError("the evaluation challenge fell into the domain")
    rows = torch.cat([wire_coeffs, t_rows, pk.coeffs, z_coeffs])
    mo = ck.open_multi(rows, _point_sets(n, z), abc + t_commitments + list(pk.vk.commitments) + [z_commitment])
    clock.lap(_OPEN)
    return Proof(abc + [z_commitment] + t_commitments, [y for row in mo.values for y in row], mo.w, mo.w2)


def _point_sets(n, z):
    return [[z]] * 14 + [[z, z * root_of_unity(n) % FR]]


# ---------------------------------------------------------------------------- the verifier
def identity_holds(vk, public_inputs, values, beta, gamma, alpha, z) -> bool:
    """gate + alpha P1 + alpha^2 (Z - 1) L_1 = t Z_H at z, on the 16 opened values"""
    a, b, c, t_lo, t_mid, t_hi, ql, qr, qo, qm, qc, s1, s2, s3, zz, zw = values
    n = vk.n
    zn = pow(z, n, FR)
    if zn == 1:
        return False
    omega, w, lagrange = root_of_unity(n), 1, []
    for _ in range(max(1, len(public_inputs))):
        lagrange.append(w * (zn - 1) * _inv(n * (z - w)) % FR)
        w = w * omega % FR
    pi = -sum(x * l for x, l in zip(public_inputs, lagrange)) % FR
    gate = ql * a + qr * b + qo * c + qm * a * b + qc + pi
    p1 = (zz * (a + beta * z + gamma) * (b + beta * K[1] * z + gamma) * (c + beta * K[2] * z + gamma)
          - zw * (a + beta * s1 + gamma) * (b + beta * s2 + gamma) * (c + beta * s3 + gamma))
    p2 = (zz - 1) * lagrange[0]
    t = t_lo + zn * (t_mid + zn * t_hi)
    return (gate + alpha * p1 + alpha * alpha * p2 - t * (zn - 1)) % FR == 0


def verify(vk, kzg_vk, public_inputs, proof) -> bool:
    """Whether `proof` (a Proof or its 800 bytes) proves the circuit of `vk` on these public inputs: the proof's form,
    then the identity on the opened values, then verify_multi over the MultiOpening rebuilt from the verifying key, the
    proof and z.  False, never an exception, for a malformed proof of the right size."""
    try:
        proof = proof if isinstance(proof, Proof) else Proof.from_bytes(proof)
        public = [int(x) for x in public_inputs]
    except (ValueError, TypeError):
        return False
    if len(public) != vk.n_public or any(not 0 <= x < FR for x in public):
        return False
    cs = list(proof.commitments)
    beta, gamma, alpha, z = challenges(vk.to_bytes(), public, cs[:3], cs[3], cs[4:])
    if not identity_holds(vk, public, proof.values, beta, gamma, alpha, z):
        return False
    values = [[v] for v in proof.values[:14]] + [list(proof.values[14:])]
    try:
        mo = _kzg.MultiOpening(cs[:3] + cs[4:] + list(vk.commitments) + [cs[3]], _point_sets(vk.n, z), values, proof.w,
                               proof.w2)
    except ValueError:
        return False
    return _kzg.verify_multi(kzg_vk, mo)
