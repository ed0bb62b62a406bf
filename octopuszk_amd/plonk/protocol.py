"""Setup, prover and verifier of the PLONK package: the transcript, the byte formats and the order
of the device calls.  The group side is CommitKey.commit, CommitKey.open_multi and verify_multi; the field side is the
transform and the three kernels of csrc/plonk.cuh.  A circuit with a lookup table has its own key,
proof and transcript tags; its field side adds the kernels of csrc/plonk_lookup.cuh.  An imported R1CS (DESIGN.md section
36) is a vanilla circuit with a key of its own kind, which holds what builds the witness on the device
(csrc/plonk_r1cs.cuh).  A key of setup(zk=True) makes zero-knowledge proofs: its rows have
ZK_PAD coefficients more, the prover blinds what it commits to (csrc/plonk_zk.cuh), and the verifier is the same.
verify_all and verify_each check K proofs under one key with one pairing product: the
transcripts and the per-proof arithmetic of verify run on the device (csrc/plonk_verify.cuh, csrc/sha256.cuh)."""
import secrets
import time

import numpy as np
import torch

from .. import kzg as _kzg
from .. import lib as _lib
from .. import transcript as _transcript
from ..fft import FR, FR_MULT_GEN, root_of_unity
from ..vectors import (fr_fft, fr_perm_product, fr_rows_blind, fr_rows_coset, fr_term_sums, msm, plonk_lookup_counts,
                       plonk_lookup_index, plonk_lookup_sum, plonk_quotient, plonk_quotient_lookup, plonk_quotient_split,
                       plonk_verify_challenges, plonk_verify_scalars, plonk_wires)
from ..wire import dev_bytes, host_bytes, ints32, is_inf_out, le32, upload, wire_out_to_in
from .circuit import K, N_MAX, Circuit, LookupCircuit, R1CSCircuit

PROOF_BYTES = 7 * 32 + 16 * 32 + 64
VK_BYTES = 8 + 8 * 32
_BETA_TAG, _GAMMA_TAG, _ALPHA_TAG, _Z_TAG = b"OZK-plonk-beta", b"OZK-plonk-gamma", b"OZK-plonk-alpha", b"OZK-plonk-z"
_COMMITMENTS = ("[a]", "[b]", "[c]", "[Z]", "[t_lo]", "[t_mid]", "[t_hi]")
_KEY_COMMITMENTS = ("[qL]", "[qR]", "[qO]", "[qM]", "[qC]", "[s1]", "[s2]", "[s3]")
_VALUES = ("a", "b", "c", "t_lo", "t_mid", "t_hi", "qL", "qR", "qO", "qM", "qC", "s1", "s2", "s3", "Z", "Z at z omega")
LOOKUP_PROOF_BYTES = 9 * 32 + 23 * 32 + 64
LOOKUP_VK_BYTES = 8 + 12 * 32
_LK_TAGS = {name: b"OZK-plookup-" + name for name in (b"beta", b"gamma", b"eta", b"theta", b"alpha", b"z")}
_LK_COMMITMENTS = ("[a]", "[b]", "[c]", "[m]", "[Z]", "[S]", "[t_lo]", "[t_mid]", "[t_hi]")
_LK_KEY_COMMITMENTS = _KEY_COMMITMENTS + ("[qK]", "[T1]", "[T2]", "[T3]")
_LK_VALUES = ("a", "b", "c", "m", "t_lo", "t_mid", "t_hi", "qL", "qR", "qO", "qM", "qC", "s1", "s2", "s3", "qK", "T1", "T2",
              "T3", "Z", "Z at z omega", "S", "S at z omega")
_UPLOAD, _WITNESS, _PRODUCT, _COSET, _QUOTIENT, _COMMIT, _OPEN, _COUNTS, _SUM = (
    "witness upload", "witness transforms", "grand product", "coset transforms", "quotient kernel", "commitments",
    "multi-opening", "lookup counts", "lookup sum")
STAGES = (_UPLOAD, _WITNESS, _PRODUCT, _COSET, _QUOTIENT, _COMMIT, _OPEN)
LOOKUP_STAGES = STAGES + (_COUNTS, _SUM)
_NO_CELL = 0xFFFFFFFF                  # the `lo` of a cell descriptor that names one element (ozk_plonk_wires_dev)
_MONT_R = 1 << 261                     # a coefficient c of the term stream is kept as c R mod r (ozk_fr_term_sums_dev)
ZK_PAD = 8                             # a row of a zero-knowledge key and proof has n + ZK_PAD coefficients
ZK_N_MIN = 8                           # the quotient of blinded rows has up to 3 n + 6 <= 4 n coefficients
ZK_BLINDERS = 13                       # a0 a1 b0 b1 c0 c1 Z0 Z1 Z2 u0 u1 v0 v1
ZK_LOOKUP_BLINDERS = 18                # a0 a1 b0 b1 c0 c1 m0 m1 Z0 Z1 Z2 S0 S1 S2 u0 u1 v0 v1


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


class LookupVerifyingKey:
    """n uint32 LE | n_public uint32 LE | [qL] [qR] [qO] [qM] [qC] [s1] [s2] [s3] [qK] [T1] [T2] [T3], compressed: 392
    bytes"""

    def __init__(self, n, n_public, commitments):
        self.n, self.n_public = int(n), int(n_public)
        if self.n < 2 or self.n & (self.n - 1) or self.n > N_MAX:
            raise ValueError("lookup verifying key: n = %d is not a power of two in [2, 2^26]" % self.n)
        if not 0 <= self.n_public <= self.n:
            raise ValueError("lookup verifying key: n_public = %d, not in [0, n = %d]" % (self.n_public, self.n))
        self.commitments = tuple(bytes(c) for c in commitments)
        if len(self.commitments) != 12 or any(len(c) != 32 for c in self.commitments):
            raise ValueError("lookup verifying key: twelve commitments of 32 bytes")

    def to_bytes(self) -> bytes:
        return self.n.to_bytes(4, "little") + self.n_public.to_bytes(4, "little") + b"".join(self.commitments)

    @staticmethod
    def from_bytes(b) -> "LookupVerifyingKey":
        """Strict and host-only, as VerifyingKey.from_bytes"""
        b = bytes(b)
        if len(b) != LOOKUP_VK_BYTES:
            raise ValueError("lookup verifying key: length %d, not %d" % (len(b), LOOKUP_VK_BYTES))
        cs = [b[8 + 32 * i:40 + 32 * i] for i in range(12)]
        vk = LookupVerifyingKey(int.from_bytes(b[:4], "little"), int.from_bytes(b[4:8], "little"), cs)
        _kzg.require_g1(zip(_LK_KEY_COMMITMENTS, cs), "lookup verifying key")
        return vk


class LookupProof:
    """[a] [b] [c] [m] [Z] [S] [t_lo] [t_mid] [t_hi] | the 23 values a, b, c, m, t_lo, t_mid, t_hi, qL, qR, qO, qM, qC,
    s1, s2, s3, qK, T1, T2, T3 at z, then Z at z, Z at z omega, S at z, S at z omega | W | W': 1088 bytes"""

    def __init__(self, commitments, values, w, w2):
        self.commitments = tuple(bytes(c) for c in commitments)
        self.values = tuple(int(v) for v in values)
        self.w, self.w2 = bytes(w), bytes(w2)
        if len(self.commitments) != 9 or any(len(c) != 32 for c in self.commitments + (self.w, self.w2)):
            raise ValueError("lookup proof: nine commitments, W and W' of 32 bytes")
        if len(self.values) != 23 or any(not 0 <= v < FR for v in self.values):
            raise ValueError("lookup proof: twenty-three values in [0, r)")

    def to_bytes(self) -> bytes:
        return b"".join(self.commitments) + le32(self.values) + self.w + self.w2

    @staticmethod
    def from_bytes(b) -> "LookupProof":
        """Strict and host-only, as Proof.from_bytes"""
        b = bytes(b)
        if len(b) != LOOKUP_PROOF_BYTES:
            raise ValueError("lookup proof: length %d, not %d" % (len(b), LOOKUP_PROOF_BYTES))
        values = ints32(b[288:1024])
        for name, v in zip(_LK_VALUES, values):
            if v >= FR:
                raise ValueError("lookup proof: the value %s is not below r" % name)
        cs = [b[32 * i:32 * i + 32] for i in range(9)]
        _kzg.require_g1(list(zip(_LK_COMMITMENTS, cs)) + [("W", b[1024:1056]), ("W'", b[1056:])], "lookup proof")
        return LookupProof(cs, values, b[1024:1056], b[1056:])


# ---------------------------------------------------------------------------- the transcript
def lookup_challenges(vk_bytes, public_inputs, abcm, zs_commitments=None, t_commitments=None) -> tuple:
    """(beta, gamma, eta, theta[, alpha[, z]]) of a proof with lookups, under tags of their own.  With D1 =
    SHA-256("OZK-plookup-beta" | the verifying key's bytes | the public inputs | [a] [b] [c] [m]) and D2 =
    SHA-256("OZK-plookup-alpha" | D1 | [Z] [S]): beta is drawn from D1, gamma, eta and theta from SHA-256 of their tag
    and D1, alpha from D2 and z from SHA-256("OZK-plookup-z" | D2 | [t_lo] [t_mid] [t_hi])."""
    parts = (bytes(vk_bytes), le32(public_inputs), b"".join(abcm))
    d1 = _transcript.digest(_LK_TAGS[b"beta"], *parts)
    out = [_transcript.challenge128(_LK_TAGS[b"beta"], *parts)]
    out += [_transcript.challenge128(_LK_TAGS[name], d1) for name in (b"gamma", b"eta", b"theta")]
    if zs_commitments is not None:
        zs = b"".join(zs_commitments)
        d2 = _transcript.digest(_LK_TAGS[b"alpha"], d1, zs)
        out.append(_transcript.challenge128(_LK_TAGS[b"alpha"], d1, zs))
        if t_commitments is not None:
            out.append(_transcript.challenge128(_LK_TAGS[b"z"], d2, b"".join(t_commitments)))
    return tuple(out)


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


def _interpolate(evals, k, n, out_len=None):
    """k rows of values on the domain of omega_n -> their coefficient rows (a new tensor), zero-extended to out_len
    elements when that is given"""
    out = torch.empty_like(evals)
    w_inv = _inv(root_of_unity(n))
    for y in range(k):
        fr_fft(evals[y], n, w_inv, out[y])
    if out_len is None:
        return fr_rows_coset(out, k, n, n, 1, _inv(n), out)
    return fr_rows_coset(out, k, n, n, 1, _inv(n), None, out_len)


def _onto_coset(coeffs, k, n, length=None):
    """k coefficient rows of n (of `length` <= 4 n when given) -> their values at g omega_4n^i, i < 4 n (a new tensor)"""
    length = n if length is None else length
    scaled = fr_rows_coset(coeffs, k, length, length, FR_MULT_GEN, 1, None, 4 * n)
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
    themselves on the coset of 4 n points (10 x 4 n x 32 bytes on the device), and the verifying key.  cells: the
    [3, n] cell descriptors (hi, lo) of ozk_plonk_wires_dev on the device, built on the first proof from an assignment
    that is already there.  zk: the key is setup(zk=True)'s; its coefficient rows, and every row its prover commits to,
    have commit_key.n = n + ZK_PAD elements."""
    zk = False

    def __init__(self, circuit, commit_key, coeffs, sigma, table, vk):
        self.circuit, self.commit_key, self.coeffs, self.sigma, self.table, self.vk = circuit, commit_key, coeffs, sigma, table, vk
        self.cells = None


class LookupProvingKey(ProvingKey):
    """The proving key of a LookupCircuit: coeffs holds twelve rows (qK, T1, T2, T3 after the eight), table fourteen
    (14 x 4 n x 32 bytes: qK, T1, T2, T3 after the ten); lookup_rows holds qK, T1, T2, T3 on the domain and index the
    table's index (ozk_plonk_lookup_index_dev), both on the device."""

    def __init__(self, circuit, commit_key, coeffs, sigma, table, vk, lookup_rows, index):
        super().__init__(circuit, commit_key, coeffs, sigma, table, vk)
        self.lookup_rows, self.index = lookup_rows, index


class R1CSProvingKey(ProvingKey):
    """The proving key of an R1CSCircuit: a vanilla key that also holds, on the device, the term stream (term_index:
    T uint32; term_coeff: T elements c R mod r, or None when every coefficient is one), the cell descriptors, in which
    an accumulator is the difference of two running sums, and the workspace of the sums."""

    def __init__(self, circuit, commit_key, coeffs, sigma, table, vk, term_index, term_coeff, cells, workspace):
        super().__init__(circuit, commit_key, coeffs, sigma, table, vk)
        self.term_index, self.term_coeff, self.cells, self.workspace = term_index, term_coeff, cells, workspace


def _plain_cells(circuit):
    """every cell names its variable alone: [3, n] descriptors (v, none)"""
    hi = circuit.wire_index().astype(np.uint32)
    return upload(np.stack([hi, np.full_like(hi, _NO_CELL)], axis=-1).view(np.uint8).reshape(-1))


def _r1cs_cells(circuit):
    """over src = [assignment | term sums]: variable v < nv is (v, none); the accumulator nv + t of a chain that starts
    at stream position t0 is (nv + t, nv + t0 - 1), and (nv + t, none) when t0 = 0"""
    nv = circuit.num_variables
    hi = circuit.wire_index()
    lo = np.full(hi.shape, _NO_CELL, dtype=np.int64)
    if circuit.term_index:
        starts = np.repeat(np.array(circuit.chain_start, dtype=np.int64), circuit.chain_length)
        below = np.where(starts == 0, _NO_CELL, nv + starts - 1)
        chained = hi >= nv
        lo[chained] = below[hi[chained] - nv]
    return upload(np.stack([hi, lo], axis=-1).astype(np.uint32).view(np.uint8).reshape(-1))


def _r1cs_key(key, device):
    circuit = key.circuit
    terms = len(circuit.term_index)
    index = coeff = workspace = None
    if terms:
        index = upload(np.array(circuit.term_index, dtype=np.uint32).view(np.uint8))
        if circuit.term_coeff is not None:
            coeff = dev_bytes(le32(c * _MONT_R % FR for c in circuit.term_coeff))
        need = int(_lib.load().ozk_fr_term_sums_workspace_bytes(terms))
        workspace = torch.empty(max(need, 256), dtype=torch.uint8, device=device)
    return R1CSProvingKey(circuit, key.commit_key, key.coeffs, key.sigma, key.table, key.vk, index, coeff,
                          _r1cs_cells(circuit), workspace)


def _key_row_len(circuit, commit_key, zk):
    """the length of the key's coefficient rows: None for n itself (interpolated in place), n + ZK_PAD for a
    zero-knowledge key; ValueError when the commit key has another number of bases"""
    n = circuit.n
    if not zk:
        if commit_key.n != n:
            raise ValueError("the circuit has n = %d gates, the commit key n = %d bases" % (n, commit_key.n))
        return None
    if n < ZK_N_MIN or commit_key.n != n + ZK_PAD:
        raise ValueError("a zero-knowledge key takes a circuit of n >= %d gates and a commit key of n + %d bases: the "
                         "circuit has n = %d, the commit key n = %d" % (ZK_N_MIN, ZK_PAD, n, commit_key.n))
    return n + ZK_PAD


def _setup_lookup(circuit, commit_key, zk):
    n = circuit.n
    row_len = _key_row_len(circuit, commit_key, zk)
    sigma = _rows(circuit.sigma_labels())
    lookup_rows = _rows([circuit.q_lookup] + circuit.table_columns())
    coeffs = _interpolate(torch.cat([_rows(circuit.selectors), sigma, lookup_rows]), 12, n, row_len)
    vk = LookupVerifyingKey(n, circuit.n_public, commit_key.commit(coeffs))
    extra = _rows([[_inv(n)] * n, [0, 1] + [0] * (n - 2)])
    table = _onto_coset(torch.cat([coeffs[:8, :32 * n], extra, coeffs[8:, :32 * n]]), 14, n)
    index = plonk_lookup_index(lookup_rows[1:], circuit.n_table, n)
    key = LookupProvingKey(circuit, commit_key, coeffs, sigma, table, vk, lookup_rows, index)
    key.zk = bool(zk)
    return key, vk


def setup(circuit, commit_key, zk=False):
    """(ProvingKey, VerifyingKey) of a circuit over a CommitKey of n bases: eight commitments, no secret; for a
    LookupCircuit (LookupProvingKey, LookupVerifyingKey), twelve commitments; for an R1CSCircuit (R1CSProvingKey,
    VerifyingKey): the circuit is a vanilla one.  zk: the proving key makes zero-knowledge proofs.
    It takes n >= 8 and a CommitKey of n + ZK_PAD bases (ValueError otherwise) and keeps its coefficient rows
    zero-extended to that length; the verifying key is the one of zk=False over n bases of the same string, byte for
    byte."""
    if isinstance(circuit, LookupCircuit):
        return _setup_lookup(circuit, commit_key, zk)
    if not isinstance(circuit, Circuit):
        raise TypeError("setup takes a plonk.Circuit")
    n = circuit.n
    row_len = _key_row_len(circuit, commit_key, zk)
    sigma = _rows(circuit.sigma_labels())
    coeffs = _interpolate(torch.cat([_rows(circuit.selectors), sigma]), 8, n, row_len)
    vk = VerifyingKey(n, circuit.n_public, commit_key.commit(coeffs))
    # L_1 = (X^n - 1) / (n (X - 1)) has every coefficient 1 / n; the points of the coset are the values of X
    extra = _rows([[_inv(n)] * n, [0, 1] + [0] * (n - 2)])
    table = _onto_coset(torch.cat([coeffs[:, :32 * n], extra]), 10, n)
    key = ProvingKey(circuit, commit_key, coeffs, sigma, table, vk)
    if isinstance(circuit, R1CSCircuit):
        key = _r1cs_key(key, table.device)
    key.zk = bool(zk)
    return key, vk


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


def _host_witness(circuit, assignment, wire_values):
    """(the three wire columns as a [3, 32 n] array of bytes, the public inputs) of an assignment or of wire values"""
    n = circuit.n
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
    return host, public


def _device_witness(pk, assignment):
    """(the three wire columns on the device, the public inputs) of an assignment that is on the device: for an
    R1CSProvingKey the running sums of the term stream are written behind a copy of it; then the cells are gathered"""
    circuit, n = pk.circuit, pk.circuit.n
    if not assignment.is_cuda or assignment.dtype != torch.uint8:
        raise TypeError("an assignment on the device is a uint8 CUDA tensor")
    r1cs = isinstance(pk, R1CSProvingKey)
    given = circuit.num_variables if r1cs else circuit.n_vars
    if assignment.numel() != 32 * given:
        raise ValueError("%d bytes for %d variables of 32 bytes" % (assignment.numel(), given))
    src = assignment.contiguous().view(-1)
    bad = torch.zeros(8, dtype=torch.uint8, device=src.device)             # two int32: of the cells, of the terms
    if r1cs and pk.term_index is not None:
        src = torch.empty(32 * circuit.n_vars, dtype=torch.uint8, device=src.device)
        src[:32 * given].copy_(assignment.reshape(-1))
        fr_term_sums(pk.term_index, pk.term_coeff, src, given, circuit.n_vars - given, src[32 * given:], bad[4:],
                     pk.workspace)
    if pk.cells is None:
        pk.cells = _plain_cells(circuit)
    wires = plonk_wires(src, circuit.n_vars, pk.cells, 3, n, n, bad)
    host = host_bytes(torch.cat([bad, wires[0, :32 * circuit.n_public]]))
    wrong = int.from_bytes(host[:4], "little") + int.from_bytes(host[4:8], "little")
    if wrong:
        raise RuntimeError("%d cell(s) or term(s) of the key point outside the assignment" % wrong)
    return wires, [v % FR for v in ints32(host[8:])]


def _r1cs_values(circuit, assignment):
    """the n_vars values of an R1CS assignment given as ints or as their 32-byte records (taken mod r)"""
    if isinstance(assignment, (bytes, bytearray)):
        if len(assignment) != 32 * circuit.num_variables:
            raise ValueError("%d bytes for %d variables of 32 bytes" % (len(assignment), circuit.num_variables))
        assignment = [v % FR for v in ints32(bytes(assignment))]
    return circuit.extend(assignment)


def _drawn_blinders(pk, blinders, count):
    """None for a key without zk (which takes no blinders: ValueError); else the `count` blinders of one proof, drawn
    here unless given (ValueError for another number of them or one outside [0, r))"""
    if not pk.zk:
        if blinders is not None:
            raise ValueError("blinders are for a key of setup(zk=True): this key makes no zero-knowledge proofs")
        return None
    if blinders is None:
        return [secrets.randbelow(FR) for _ in range(count)]
    blinders = list(blinders)
    if len(blinders) != count:
        raise ValueError("%d blinders: a proof under this key takes %d" % (len(blinders), count))
    if any(not isinstance(r, int) or not 0 <= r < FR for r in blinders):
        raise ValueError("blinders are ints in [0, r)")
    return blinders


def _witness_on_device(pk, assignment, timings, wire_values, blinders=None):
    """(the clock, the public inputs, the three wire columns on the device, their coefficient rows): how both
    provers begin.  blinders: a0 a1 b0 b1 c0 c1 of a zero-knowledge key, whose rows have commit_key.n coefficients"""
    circuit = pk.circuit
    if (assignment is None) == (wire_values is None):
        raise ValueError("prove takes an assignment or the three columns of wire values")
    clock = _Clock(timings)
    if isinstance(assignment, torch.Tensor):
        wires, public = _device_witness(pk, assignment)
    else:
        if assignment is not None and isinstance(circuit, R1CSCircuit):
            assignment = _r1cs_values(circuit, assignment)
        host, public = _host_witness(circuit, assignment, wire_values)
        wires = upload(host)
    clock.lap(_UPLOAD)
    if blinders is None:
        wire_coeffs = _interpolate(wires, 3, circuit.n)
    else:
        row_len = pk.commit_key.n
        wire_coeffs = _interpolate(wires, 3, circuit.n, row_len)
        fr_rows_blind(wire_coeffs, 3, circuit.n, row_len, [blinders[0:2], blinders[2:4], blinders[4:6]])
    clock.lap(_WITNESS)
    return clock, public, wires, wire_coeffs


def _grand_product(wires, sigma, n, beta, gamma, clock):
    """Z on the domain; RuntimeError for a zero denominator, ValueError when the product does not close"""
    z_evals, total, zero_dens = fr_perm_product(wires, sigma, n, n, root_of_unity(n), K, beta, gamma)
    if zero_dens:
        raise RuntimeError("the grand product met %d zero denominator(s) under these challenges" % zero_dens)
    if total != 1:
        raise ValueError("a copy constraint is violated: the grand product does not close")
    clock.lap(_PRODUCT)
    return z_evals


def _public_input_row(public, n, device, out_len=None):
    """the coefficients of PI: -x_i in row i of the domain"""
    pi_evals = torch.zeros((1, 32 * n), dtype=torch.uint8, device=device)
    if public:
        pi_evals[0, :32 * len(public)] = dev_bytes(le32((FR - x) % FR for x in public))
    return _interpolate(pi_evals, 1, n, out_len)


def _quotient_parts(t_evals, n, ck, clock, blinders=None):
    """(t_lo, t_mid, t_hi as three coefficient rows, their commitments) of the quotient's values on the coset;
    ValueError when its top quarter is not zero.  blinders: u0 u1 v0 v1 of a zero-knowledge key: the rows have ck.n
    coefficients and are blinded, and the quotient may reach 3 n + 6 coefficients, zero from there on"""
    t = _off_coset(t_evals, n)
    if blinders is None:
        if bool(t[32 * 3 * n:].any().item()):
            raise ValueError("a gate is violated: the quotient is no polynomial")
        t_rows = t[:32 * 3 * n].view(3, 32 * n)
    else:
        t_rows, nonzero = plonk_quotient_split(t, n, ck.n, blinders)
        if nonzero:
            raise ValueError("a gate is violated: the quotient is no polynomial")
    clock.lap(_COSET)
    t_commitments = ck.commit(t_rows)
    clock.lap(_COMMIT)
    return t_rows, t_commitments


def _outside_domain(z, n):
    if pow(z, n, FR) == 1:
        raise RuntimeError("the evaluation challenge fell into the domain")
    return z


def prove(pk, assignment=None, timings=None, wire_values=None, blinders=None) -> Proof:
    """The proof of one assignment (one Fr value per variable: a list of ints, or their 32-byte little-endian records
    back to back as bytes or as a uint8 CUDA tensor, which are taken mod r; the tensor's wire columns are gathered on
    the device, and RuntimeError is raised if the key points outside it), or of a witness produced elsewhere and given
    cell by cell (wire_values: the three columns a, b, c of n values).  With an R1CSProvingKey the assignment is the
    R1CS's, num_variables values with the leading one: the accumulators of its chains are computed here, on the device
    for a tensor.  ValueError, before any commitment to t, when the
    grand product does not close (a copy constraint is violated) or the quotient is no polynomial (a gate is violated,
    seen as a nonzero top quarter of its 4 n coefficients by one reduction on the device); RuntimeError when a
    denominator of the grand product is zero.  timings: a dict that receives the seconds of every stage of STAGES.
    With a LookupProvingKey the proof is a LookupProof (_prove_lookup).
    Under a key of setup(zk=True) the proof is zero-knowledge: every polynomial the prover
    commits to is blinded by a multiple of Z_H (the quotient's parts by terms that cancel in t), with 13 scalars, 18
    for a proof with lookups, drawn here from secrets.randbelow.  blinders: those scalars given instead, ints in
    [0, r) in the section's order, for tests and models (ValueError for another number of them, one out of range, or
    any under a key without zk); all zero, they give the proof of the key without zk.  Inputs, errors, bytes and the
    verifier are the same."""
    if isinstance(pk, LookupProvingKey):
        return _prove_lookup(pk, assignment, timings, wire_values, blinders)
    circuit, ck, n = pk.circuit, pk.commit_key, pk.circuit.n
    zk = _drawn_blinders(pk, blinders, ZK_BLINDERS)
    row_len = ck.n if zk else None
    vk_bytes = pk.vk.to_bytes()
    clock, public, wires, wire_coeffs = _witness_on_device(pk, assignment, timings, wire_values, zk)
    abc = ck.commit(wire_coeffs)
    clock.lap(_COMMIT)
    beta, gamma = challenges(vk_bytes, public, abc)
    z_evals = _grand_product(wires, pk.sigma, n, beta, gamma, clock)
    z_coeffs = _interpolate(z_evals.unsqueeze(0), 1, n, row_len)
    if zk:
        fr_rows_blind(z_coeffs, 1, n, row_len, [zk[6:9]])
    pi_coeffs = _public_input_row(public, n, wires.device, row_len)
    clock.lap(_WITNESS)
    z_commitment = ck.commit(z_coeffs)[0]
    clock.lap(_COMMIT)
    alpha = challenges(vk_bytes, public, abc, z_commitment)[2]
    wit = _onto_coset(torch.cat([wire_coeffs, z_coeffs, pi_coeffs]), 5, n, row_len)
    clock.lap(_COSET)
    t_evals = plonk_quotient(wit, 4 * n, pk.table, 4 * n, n, alpha, beta, gamma, K, zh_inverses(n))
    clock.lap(_QUOTIENT)
    t_rows, t_commitments = _quotient_parts(t_evals, n, ck, clock, zk[9:] if zk else None)
    z = _outside_domain(challenges(vk_bytes, public, abc, z_commitment, t_commitments)[3], n)
    rows = torch.cat([wire_coeffs, t_rows, pk.coeffs, z_coeffs])
    mo = ck.open_multi(rows, _point_sets(n, z), abc + t_commitments + list(pk.vk.commitments) + [z_commitment])
    clock.lap(_OPEN)
    return Proof(abc + [z_commitment] + t_commitments, [y for row in mo.values for y in row], mo.w, mo.w2)


def _point_sets(n, z):
    return [[z]] * 14 + [[z, z * root_of_unity(n) % FR]]


def _prove_lookup(pk, assignment, timings, wire_values, blinders=None) -> LookupProof:
    """The proof of a circuit with lookups.  As prove, and: ValueError naming the first offending row, before any
    commitment, when a row with qK = 1 holds a tuple that is in no table row; RuntimeError when a denominator of the
    lookup sum is zero or the sum does not close after a clean count.  timings receives LOOKUP_STAGES."""
    circuit, ck, n = pk.circuit, pk.commit_key, pk.circuit.n
    zk = _drawn_blinders(pk, blinders, ZK_LOOKUP_BLINDERS)
    row_len = ck.n if zk else None
    vk_bytes = pk.vk.to_bytes()
    clock, public, wires, wire_coeffs = _witness_on_device(pk, assignment, timings, wire_values, zk)
    m_evals, missing, first = plonk_lookup_counts(wires, pk.lookup_rows[0], n, n, pk.lookup_rows[1:], circuit.n_table, n,
                                                  pk.index, n)
    if missing:
        raise ValueError("row %d looks up a tuple that is in no row of the table (%d such row(s))" % (first, missing))
    clock.lap(_COUNTS)
    m_coeffs = _interpolate(m_evals.view(1, -1), 1, n, row_len)
    if zk:
        fr_rows_blind(m_coeffs, 1, n, row_len, [zk[6:8]])
    clock.lap(_WITNESS)
    abcm = ck.commit(torch.cat([wire_coeffs, m_coeffs]))
    clock.lap(_COMMIT)
    beta, gamma, eta, theta = lookup_challenges(vk_bytes, public, abcm)
    z_evals = _grand_product(wires, pk.sigma, n, beta, gamma, clock)
    s_evals, s_total, zero_dens = plonk_lookup_sum(wires, n, pk.lookup_rows, n, m_evals, n, eta, theta)
    if zero_dens:
        raise RuntimeError("the lookup sum met %d zero denominator(s) under these challenges" % zero_dens)
    if s_total != 0:
        raise RuntimeError("the lookup sum does not close after a clean count")
    clock.lap(_SUM)
    zs_coeffs = _interpolate(torch.stack([z_evals, s_evals]), 2, n, row_len)
    if zk:
        fr_rows_blind(zs_coeffs, 2, n, row_len, [zk[8:11], zk[11:14]])
    pi_coeffs = _public_input_row(public, n, wires.device, row_len)
    clock.lap(_WITNESS)
    zs_commitments = ck.commit(zs_coeffs)
    clock.lap(_COMMIT)
    alpha = lookup_challenges(vk_bytes, public, abcm, zs_commitments)[4]
    wit = _onto_coset(torch.cat([wire_coeffs, zs_coeffs[:1], pi_coeffs, m_coeffs, zs_coeffs[1:]]), 7, n, row_len)
    clock.lap(_COSET)
    t_evals = plonk_quotient_lookup(wit, 4 * n, pk.table, 4 * n, n, alpha, beta, gamma, K, zh_inverses(n), eta, theta)
    clock.lap(_QUOTIENT)
    t_rows, t_commitments = _quotient_parts(t_evals, n, ck, clock, zk[14:] if zk else None)
    z = _outside_domain(lookup_challenges(vk_bytes, public, abcm, zs_commitments, t_commitments)[5], n)
    rows = torch.cat([wire_coeffs, m_coeffs, t_rows, pk.coeffs, zs_coeffs])
    mo = ck.open_multi(rows, _lookup_point_sets(n, z), abcm + t_commitments + list(pk.vk.commitments) + zs_commitments)
    clock.lap(_OPEN)
    return LookupProof(abcm + zs_commitments + t_commitments, [y for row in mo.values for y in row], mo.w, mo.w2)


def _lookup_point_sets(n, z):
    return [[z]] * 19 + [[z, z * root_of_unity(n) % FR]] * 2


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


def lookup_identity_holds(vk, public_inputs, values, beta, gamma, eta, theta, alpha, z) -> bool:
    """gate + alpha P1 + alpha^2 (Z - 1) L_1 + alpha^3 L1 + alpha^4 S L_1 = t Z_H at z, on the 23 opened values, with
    L1 = (S(omega z) - S)(theta + t)(theta + f) - m (theta + f) + qK (theta + t)"""
    a, b, c, m, t_lo, t_mid, t_hi, ql, qr, qo, qm, qc, s1, s2, s3, qk, t1, t2, t3, zz, zw, ss, sw = values
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
    df, dt = theta + a + eta * b + eta * eta * c, theta + t1 + eta * t2 + eta * eta * t3
    l1 = (sw - ss) * dt * df - m * df + qk * dt
    l2 = ss * lagrange[0]
    t = t_lo + zn * (t_mid + zn * t_hi)
    return (gate + alpha * p1 + alpha ** 2 * p2 + alpha ** 3 * l1 + alpha ** 4 * l2 - t * (zn - 1)) % FR == 0


def _verify_lookup(vk, kzg_vk, public_inputs, proof) -> bool:
    try:
        proof = proof if isinstance(proof, LookupProof) else LookupProof.from_bytes(proof)
        public = [int(x) for x in public_inputs]
    except (ValueError, TypeError):
        return False
    if len(public) != vk.n_public or any(not 0 <= x < FR for x in public):
        return False
    cs = list(proof.commitments)
    beta, gamma, eta, theta, alpha, z = lookup_challenges(vk.to_bytes(), public, cs[:4], cs[4:6], cs[6:])
    if not lookup_identity_holds(vk, public, proof.values, beta, gamma, eta, theta, alpha, z):
        return False
    values = [[v] for v in proof.values[:19]] + [list(proof.values[19:21]), list(proof.values[21:])]
    try:
        mo = _kzg.MultiOpening(cs[:4] + cs[6:] + list(vk.commitments) + cs[4:6], _lookup_point_sets(vk.n, z), values,
                               proof.w, proof.w2)
    except ValueError:
        return False
    return _kzg.verify_multi(kzg_vk, mo)


def verify(vk, kzg_vk, public_inputs, proof) -> bool:
    """Whether `proof` (a Proof or its 800 bytes) proves the circuit of `vk` on these public inputs: the proof's form,
    then the identity on the opened values, then verify_multi over the MultiOpening rebuilt from the verifying key, the
    proof and z.  False, never an exception, for a malformed proof of the right size.  With a LookupVerifyingKey the
    proof is a LookupProof or its 1088 bytes."""
    if isinstance(vk, LookupVerifyingKey):
        return _verify_lookup(vk, kzg_vk, public_inputs, proof)
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


# ---------------------------------------------------------------------------- the batched verifier
BATCH_K_MAX, BATCH_ROWS_MAX = 1 << 16, 1 << 24          # PLONK_VF_K_MAX, PLONK_VF_ROWS_MAX of csrc/plonk_verify.cuh
_RHO_TAG = b"OZK-plonk-rho"
_ROW_ORDER = (0, 1, 2, 4, 5, 6, 3)                      # a proof's commitments in the row order of verify's MultiOpening
_LK_ROW_ORDER = (0, 1, 2, 3, 6, 7, 8, 4, 5)
_B_UPLOAD, _B_CHALLENGES, _B_SCALARS, _B_DECODE, _B_MSM, _B_PAIRING = (
    "upload", "challenges", "scalars", "decode", "two MSMs", "pairing product")
BATCH_STAGES = (_B_UPLOAD, _B_CHALLENGES, _B_SCALARS, _B_DECODE, _B_MSM, _B_PAIRING)
_OUT_OF_RANGE = b"\xff" * 32                            # stands for a public input that is no int in [0, 2^256): >= r


def _batch_kind(vk):
    """(kind, proof bytes, row order) of the key's kind, as the library numbers them"""
    if isinstance(vk, LookupVerifyingKey):
        return 1, LOOKUP_PROOF_BYTES, _LK_ROW_ORDER
    if isinstance(vk, VerifyingKey):
        return 0, PROOF_BYTES, _ROW_ORDER
    raise TypeError("verify_all takes a VerifyingKey or a LookupVerifyingKey")


def _is_device_bytes(t, what):
    if not isinstance(t, torch.Tensor):
        return False
    if t.dtype != torch.uint8 or not t.is_cuda:
        raise TypeError("%s on the device are a uint8 CUDA tensor" % what)
    return True


def _public_row(row, n_public):
    row = list(row)
    if len(row) != n_public:
        raise ValueError("a row of %d public inputs: the key has n_public = %d" % (len(row), n_public))
    out = []
    for x in row:
        try:
            out.append(int(x).to_bytes(32, "little"))
        except (TypeError, ValueError, OverflowError):
            out.append(_OUT_OF_RANGE)
    return b"".join(out)


def _batch_args(vk, public_inputs, proofs):
    """(kind, K, the proofs and the public inputs, each as bytes or as a uint8 CUDA tensor): every check that needs no
    device.  proofs: what _sized_objects returns.  ValueError for a buffer of the wrong size, for public inputs of
    another number of proofs, for K or K (n_public + 1) above the caps."""
    kind, proof_len, _ = _batch_kind(vk)
    if _is_device_bytes(proofs, "proofs"):
        size = proofs.numel()
    else:
        proofs = bytes(proofs) if isinstance(proofs, (bytes, bytearray)) else b"".join(proofs)
        size = len(proofs)
    if size % proof_len:
        raise ValueError("%d bytes of proofs are no whole number of %d-byte proofs" % (size, proof_len))
    k = size // proof_len
    if k > BATCH_K_MAX:
        raise ValueError("K = %d proofs: at most 2^16 in one batch" % k)
    if k * (vk.n_public + 1) > BATCH_ROWS_MAX:
        raise ValueError("K (n_public + 1) = %d: at most 2^24 in one batch" % (k * (vk.n_public + 1)))
    if _is_device_bytes(public_inputs, "public inputs"):
        have = public_inputs.numel()
    else:
        if not isinstance(public_inputs, (bytes, bytearray)):
            rows = list(public_inputs)
            if len(rows) != k:
                raise ValueError("%d rows of public inputs for %d proofs" % (len(rows), k))
            public_inputs = b"".join(_public_row(row, vk.n_public) for row in rows)
        public_inputs = bytes(public_inputs)
        have = len(public_inputs)
    if have != 32 * vk.n_public * k:
        raise ValueError("%d proofs under this key take %d bytes of public inputs, not %d" % (k, 32 * vk.n_public * k, have))
    return kind, k, proofs, public_inputs


def _sized_objects(vk, proofs):
    """a sequence of proofs whose members all have the key's size, else ValueError (before they are joined)"""
    _, proof_len, _ = _batch_kind(vk)
    if isinstance(proofs, (bytes, bytearray, torch.Tensor)):
        return proofs
    out = []
    for i, p in enumerate(proofs):
        b = p.to_bytes() if isinstance(p, (Proof, LookupProof)) else bytes(p)
        if len(b) != proof_len:
            raise ValueError("proof %d has %d bytes: a proof under this key has %d" % (i, len(b), proof_len))
        out.append(b)
    return out


class _Batch:
    """The K proofs and their public inputs on the device, and what the two kernels and the decoder make of them"""

    def __init__(self, vk, kzg_vk, kind, k, d_proofs, d_public, seed, clock):
        _, proof_len, order = _batch_kind(vk)
        nc, nkey = len(order), len(vk.commitments)
        self.k, self.nc, self.total = k, nc, k * (nc + 2) + nkey + 1
        d_vk = dev_bytes(vk.to_bytes())
        clock.lap(_B_UPLOAD)
        records = plonk_verify_challenges(kind, d_vk, vk.n, vk.n_public, d_proofs, d_public, seed)
        clock.lap(_B_CHALLENGES)
        self.scalars, self.rho, flags = plonk_verify_scalars(kind, vk.n, vk.n_public, d_proofs, d_public, records)
        clock.lap(_B_SCALARS)
        view = d_proofs.view(k, proof_len)
        own = view[:, :32 * nc].reshape(k, nc, 32)[:, list(order), :]
        encodings = torch.cat([own.reshape(-1), view[:, proof_len - 64:proof_len - 32].reshape(-1),
                               view[:, proof_len - 32:].reshape(-1), d_vk[8:]])
        points, codes = _kzg.decode_g1(encodings)
        self.points = torch.cat([points, kzg_vk.points()[0]])
        per_proof = torch.cat([codes[:k * nc].view(k, nc), codes[k * nc:k * (nc + 2)].view(2, k).t()], dim=1)
        bad = (flags != 0) | (per_proof != 0).any(dim=1)
        if bool((codes[k * (nc + 2):] != 0).any().item()):
            bad = torch.ones_like(bad)                       # the key's own commitments do not decode
        self.bad = bad.cpu().tolist()
        clock.lap(_B_DECODE)

    def holds(self, kzg_vk, clock) -> bool:
        """the pairing product over every proof that is not `bad` (their scalars and weights are zero)"""
        k, nc = self.k, self.nc
        lhs, ws1 = msm(self.points, self.scalars, self.total)
        ps, ws2 = msm(self.points[96 * k * (nc + 1):96 * k * (nc + 2)], self.rho, k)
        torch.cuda.current_stream().synchronize()
        clock.lap(_B_MSM)
        ok = _kzg._pairing_holds(lhs, wire_out_to_in(ps, 1), is_inf_out(ps), kzg_vk)
        clock.lap(_B_PAIRING)
        del ws1, ws2
        return ok


def _batch(vk, kzg_vk, kind, k, proofs, public, seed, clock):
    d_proofs = proofs if isinstance(proofs, torch.Tensor) else dev_bytes(proofs)
    d_public = None
    if vk.n_public:
        d_public = public if isinstance(public, torch.Tensor) else dev_bytes(public)
    return _Batch(vk, kzg_vk, kind, k, d_proofs.reshape(-1), None if d_public is None else d_public.reshape(-1), seed,
                  clock)


def _batch_seed(seed):
    return secrets.token_bytes(32) if seed is None else _transcript.seed_bytes(seed)


def verify_all(vk, kzg_vk, public_inputs, proofs, seed=None, timings=None) -> bool:
    """Whether every one of K proofs under ONE verifying key verifies on its public inputs, with
    one pairing product whatever K is.  proofs: a sequence of Proof / LookupProof objects or of their bytes, or one
    bytes object or uint8 CUDA tensor of K x 800 (K x 1088 under a LookupVerifyingKey) bytes; public_inputs: K
    sequences of vk.n_public ints, or K x n_public x 32 bytes as bytes or as a uint8 CUDA tensor.  The transcripts and
    the per-proof arithmetic of verify run on the device (ozk_plonk_verify_challenges_dev, ozk_plonk_verify_scalars_dev),
    with weights rho_m in [1, 2^128), the stream transcript.weights(seed, K, b"OZK-plonk-rho") drawn there; then
        e(sum_m rho_m (sum_i w_mi C_mi + s_m g1 + t_m W_m + x_m W'_m), g2) e(-sum_m rho_m W'_m, tau_g2) = 1
    as one G1 MSM over every commitment, W and W' of the batch, the key's commitments once and g1, one MSM of the K
    points W'_m, and one product of two pairings.  True exactly when verify is True for every pair, up to the 2^-128 of
    the weights; True for an empty batch; False, never an exception, for a malformed proof of the right size.
    ValueError, before any device call, for a buffer of the wrong size, public inputs for another number of proofs,
    K > 2^16 or K (n_public + 1) > 2^24.  seed: None draws 32 bytes from the system; a given seed is for tests only.
    timings: a dict that receives the seconds of every stage of BATCH_STAGES."""
    clock = _Clock(timings)                  # (the upload stage begins with the host's marshalling)
    kind, k, proofs, public = _batch_args(vk, public_inputs, _sized_objects(vk, proofs))
    if k == 0:
        return True
    batch = _batch(vk, kzg_vk, kind, k, proofs, public, _batch_seed(seed), clock)
    if any(batch.bad):
        return False
    return batch.holds(kzg_vk, clock)


def verify_each(vk, kzg_vk, public_inputs, proofs, seed=None) -> list:
    """One verdict per proof, arguments as verify_all: the batch check over the proofs that pass the per-proof checks
    (form, ranges, z outside the domain, the identity); verify one by one only when that batch fails"""
    kind, k, proofs, public = _batch_args(vk, public_inputs, _sized_objects(vk, proofs))
    if k == 0:
        return []
    seed = _batch_seed(seed)
    clock = _Clock(None)
    batch = _batch(vk, kzg_vk, kind, k, proofs, public, seed, clock)
    good = [not b for b in batch.bad]
    if not any(good):
        return good
    if batch.holds(kzg_vk, clock):       # (a proof that is `bad` has zero scalars and a zero weight: it is not in the sum)
        return good
    _, proof_len, _ = _batch_kind(vk)
    proofs = host_bytes(proofs) if isinstance(proofs, torch.Tensor) else proofs
    public = host_bytes(public) if isinstance(public, torch.Tensor) else public
    row = 32 * vk.n_public
    return [ok and verify(vk, kzg_vk, ints32(public[row * m:row * (m + 1)]), proofs[proof_len * m:proof_len * (m + 1)])
            for m, ok in enumerate(good)]
