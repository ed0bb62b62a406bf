"""Host-side mirror of the reference's SERIAL Groth16 setup and prover for BN254a — the callers of the
MSM / FFT hot path (BASELINE.json configs[4]) — with every group / transform
operation on the GPU through the C ABI of libozk_hip.so and the keys resident in HBM between them.

    serial_construct        profiler/generation/R1CSConstruction.java:28-110   (synthetic R1CS + witness)
    r1cs_to_qap_relation    reductions/r1cs_to_qap/R1CStoQAP.java:37-98        (QAP instance at t; host)
    SerialSetup.generate    zk_proof_systems/zkSNARK/SerialSetup.java:32-192   (4 x batchMSM + doubleBatchMSM)
    SerialProver.prove      zk_proof_systems/zkSNARK/SerialProver.java:26-119  (witness map, 4 x serialMSM,
                                                                                2 x doubleMSM, assembly)

What runs where.  The reference keeps field elements as BigInteger objects on the JVM heap and crosses
the JNI for each MSM / batch; here the host side is Python ints (the image has no JDK) for exactly the
parts the Java does on the CPU in the SETUP (R1CS construction, Lagrange coefficients, the sparse accumulation
of A_i(t), B_i(t), C_i(t)), and device buffers for everything else:

  * setup: the five fixed-base batches write the proving key straight into the wire-in format of the
    variable-base MSM (ozk_fixed_batch_msm_compact_dev), so the key never leaves HBM;
  * prove: the assignment goes up once (32-byte elements), the constraint matrices sit in HBM as CSR and are
    evaluated there (ozk_r1cs_evaluate_dev), ozk_qap_witness_dev leaves coefficientsH in HBM, the
    MSMs run over bases prepared once per key (ozk_var_msm_prepare_dev) — G1 through a two-stage pipeline on
    two streams, G2 on a third — and the proof is assembled on the device (ozk_points_sum_dev and one
    3-term MSM, s A + r B1 - r s delta, on a fourth stream behind the long MSMs) from the MSM results.

The prover's schedule exists once, in ShardedProver (one rank's slices of the key, one 768-byte record A | B | C per
proof); SerialProver is its rank 0 of a world of one, whose record is the proof.

Proof elements are returned in the wire-out format of the variable-base natives (affine-normalised,
64-byte little-endian coordinates).  There is no CPU fallback: without the HIP library nothing here works.
"""
import ctypes
import os
import random
import secrets
import time

import numpy as np
import torch

from . import codec as _codec
from . import device as _dev
from . import keyfile as _keyfile
from . import lib as _lib
from . import pairing as _pairing
from .device import _ptr, _stream, prepare_bases
from .distributed import shard_range
from .fft import FR, FR_MULT_GEN, SEED, fr_random, lowest_power_of_two, root_of_unity
from .fixed_base_msm import G1_WINDOW_TABLE, G2_WINDOW_TABLE, get_window_size
from .wire import dev_bytes, g1_wire, g2_wire, host_bytes, ints32, upload, vp, wire_out_to_in
from .wire import le32 as _le32

G1_ONE = (1, 2, 1)  # BN254aG1Parameters.java:23-24
G2_ONE = (  # BN254aG2Parameters.java:25-32
    (10857046999023057135944570762232829481370756359578518086990519993285655852781,
     11559732032986387107991004021392285783925812861821192530917403151452391805634),
    (8495653923123431417604973247489272438418190587263600148770280649306958101930,
     4082367875863433681332203403145435568316851327593401208105741076214120093531),
    (1, 0))


# ---------------------------------------------------------------------------- R1CS (CSR arrays)
class LinearCombinations:
    """The A (or B, or C) side of all constraints: row i = terms ptr[i] .. ptr[i+1] of (index, value).
    value is None when every coefficient is `one` (the synthetic circuits)."""

    def __init__(self, ptr, index, value=None):
        self.ptr = np.asarray(ptr, dtype=np.int64)
        self.index = np.asarray(index, dtype=np.int64)
        self.value = value  # None, or a numpy object array of Python ints

    @property
    def rows(self):
        return len(self.ptr) - 1

    def row_of_term(self):
        return np.repeat(np.arange(self.rows, dtype=np.int64), np.diff(self.ptr))

    def evaluate(self, full_obj):
        """LinearCombination.evaluate (relations/objects/LinearCombination.java:39-50) for every row: a term
        with index 0 contributes `one` whatever its coefficient."""
        vals = full_obj[self.index]
        if self.value is not None:
            vals = vals * self.value
        vals[self.index == 0] = 1
        out = np.zeros(self.rows, dtype=object)
        nz = np.diff(self.ptr) > 0
        if nz.any():
            red = np.add.reduceat(vals, self.ptr[:-1][nz])
            out[nz] = red
        return out % FR


class R1CSRelation:
    def __init__(self, A, B, C, num_inputs, num_auxiliary):
        self.A, self.B, self.C = A, B, C
        self.num_inputs, self.num_auxiliary = num_inputs, num_auxiliary
        self.num_variables = num_inputs + num_auxiliary
        self.num_constraints = A.rows


def serial_construct(num_constraints: int, num_inputs: int, seed: int = SEED):
    """R1CSConstruction.serialConstruct (R1CSConstruction.java:28-110): the alternating a + b = c / a * b = c
    chain, closed by one constraint (sum x_i)^2 = x_last.  Returns (r1cs, primary, auxiliary) with the
    assignments as lists of ints."""
    assert num_inputs <= num_constraints + 1
    nc = num_constraints
    num_auxiliary = 3 + nc - num_inputs
    nv = num_inputs + num_auxiliary
    a = fr_random(seed)
    b = fr_random(seed)
    full = [1, a, b]
    for i in range(nc - 1):
        tmp = (a * b) % FR if i % 2 else (a + b) % FR
        a, b = b, tmp
        full.append(tmp)
    res = sum(full[1:nv - 1]) % FR
    full.append(res * res % FR)
    i = np.arange(nc - 1, dtype=np.int64)
    even = (i % 2) == 0
    tail = np.arange(1, nv - 1, dtype=np.int64)
    # A: [i+1, i+2] on even rows (a + b), [i+1] on odd rows (a * b); last row: all of 1 .. nv-2
    a_cnt = np.where(even, 2, 1)
    a_ptr = np.concatenate(([0], np.cumsum(a_cnt)))
    a_idx = np.empty(int(a_ptr[-1]), dtype=np.int64)
    a_idx[a_ptr[:-1]] = i + 1
    a_idx[a_ptr[:-1][even] + 1] = i[even] + 2
    A = LinearCombinations(np.concatenate((a_ptr, [a_ptr[-1] + len(tail)])), np.concatenate((a_idx, tail)))
    # B: [0] on even rows, [i+2] on odd rows; last row as A
    b_idx = np.where(even, 0, i + 2)
    B = LinearCombinations(np.concatenate((np.arange(nc, dtype=np.int64), [nc - 1 + len(tail)])),
                           np.concatenate((b_idx, tail)))
    # C: [i+3]; last row [nv-1]
    C = LinearCombinations(np.arange(nc + 1, dtype=np.int64), np.concatenate((i + 3, [nv - 1])))
    r1cs = R1CSRelation(A, B, C, num_inputs, num_auxiliary)
    assert len(full) == nv
    return r1cs, full[:num_inputs], full[num_inputs:]


def constraint_evaluations(r1cs: R1CSRelation, full):
    """The three vectors R1CStoQAP.R1CStoQAPWitness fills before its transforms (R1CStoQAP.java:143-160,
    195-199): evaluations of A, B, C on the domain, with the extra constraints input_i * 0 = 0."""
    nc, ni = r1cs.num_constraints, r1cs.num_inputs
    m = lowest_power_of_two(nc + ni)
    z = np.array(full, dtype=object)
    ev = []
    for k, lc in enumerate((r1cs.A, r1cs.B, r1cs.C)):
        v = np.zeros(m, dtype=object)
        v[:nc] = lc.evaluate(z)
        if k == 0:
            v[nc:nc + ni] = z[:ni]
        ev.append(v)
    return ev, m


def assignment_bytes(full) -> np.ndarray:
    """The assignment as the natives take scalars: 32-byte little-endian elements (the marshalling the Java does
    per MSM with bigIntegerToByteArrayHelperCGBN, VariableBaseMSM.java:121-131,221-228)."""
    return np.frombuffer(_le32(full), dtype=np.uint8).copy()


class _CsrDevice:
    """A sparse matrix resident in HBM as CSR: u32 row offsets and column indices, optional 32-byte coefficients
    (None: every coefficient is one) and the list of the rows longer than 64 terms, which the kernels of
    ozk_r1cs_evaluate_dev / ozk_sparse_mat_vec_dev reduce in a pass of their own."""

    def __init__(self, ptr, idx, val):
        assert ptr[-1] == len(idx) < 1 << 32
        long_rows = np.nonzero(np.diff(ptr) > 64)[0].astype(np.uint32)
        self.rows, self.n_long = len(ptr) - 1, len(long_rows)
        self.ptr = upload(ptr.astype(np.uint32).view(np.uint8))
        self.idx = upload(idx.astype(np.uint32).view(np.uint8))
        self.coeff = None if val is None else dev_bytes(_le32(int(v) % FR for v in val))
        self.long = upload(long_rows.view(np.uint8)) if self.n_long else None

    @staticmethod
    def workspace(mats):
        """scratch that serves any one of `mats` at a time"""
        nbytes = int(_lib.load().ozk_r1cs_evaluate_workspace_bytes(max(mat.n_long for mat in mats)))
        return torch.empty(nbytes, dtype=torch.uint8, device="cuda")

    def apply(self, fn, d_vec, d_out, ws):
        """d_out = this matrix times d_vec through `fn` (ozk_r1cs_evaluate_dev or ozk_sparse_mat_vec_dev: one
        signature); asynchronous on the current stream"""
        opt = lambda t: None if t is None else _ptr(t)
        _lib.check(fn(_ptr(self.ptr), _ptr(self.idx), opt(self.coeff), _ptr(d_vec), self.rows, opt(self.long),
                      self.n_long, _ptr(d_out), _ptr(ws), ws.numel(), _stream()))


class R1CSDevice:
    """The three constraint matrices resident in HBM as CSR (u32 row offsets / variable indices, optional 32-byte
    coefficients), with the rows R1CStoQAPWitness adds: A gets `input_i * 0 = 0` rows behind the constraints
    (R1CStoQAP.java:149-151) and all three are padded with empty rows to the domain size, so that
    ozk_r1cs_evaluate_dev leaves exactly the vectors the transforms start from."""

    def __init__(self, r1cs: R1CSRelation):
        nc, ni = r1cs.num_constraints, r1cs.num_inputs
        self.m = m = lowest_power_of_two(nc + ni)
        self.mats = []
        for k, lc in enumerate((r1cs.A, r1cs.B, r1cs.C)):
            ptr, idx, val = lc.ptr, lc.index, lc.value
            if k == 0:   # A[nc + i] = z_i
                ptr = np.concatenate((ptr, ptr[-1] + 1 + np.arange(ni, dtype=np.int64)))
                idx = np.concatenate((idx, np.arange(ni, dtype=np.int64)))
                if val is not None:
                    val = np.concatenate((val, np.ones(ni, dtype=object)))
            ptr = np.concatenate((ptr, np.full(m + 1 - len(ptr), ptr[-1], dtype=np.int64)))
            assert len(ptr) == m + 1
            self.mats.append(_CsrDevice(ptr, idx, val))
        self.out = [torch.empty(m * 32, dtype=torch.uint8, device="cuda") for _ in range(3)]
        self.ws = _CsrDevice.workspace(self.mats)

    def evaluate(self, d_full):
        """d_full: the assignment in HBM (num_variables x 32 B).  Asynchronous on the current stream; returns the
        three evaluation vectors (m x 32 B each)."""
        fn = _lib.load().ozk_r1cs_evaluate_dev
        for mat, out in zip(self.mats, self.out):
            mat.apply(fn, d_full, out, self.ws)
        return self.out


def is_satisfied(r1cs: R1CSRelation, primary, auxiliary) -> bool:
    ev, _ = constraint_evaluations(r1cs, list(primary) + list(auxiliary))
    nc = r1cs.num_constraints
    return bool(np.all((ev[0][:nc] * ev[1][:nc] - ev[2][:nc]) % FR == 0))


# ---------------------------------------------------------------------------- QAP instance at t (host)
def _batch_inverse(xs):
    """Montgomery's trick over Python ints (the Java calls BigInteger.modInverse once per element)."""
    n = len(xs)
    pref = [1] * (n + 1)
    acc = 1
    for i, x in enumerate(xs):
        acc = acc * x % FR
        pref[i + 1] = acc
    inv = pow(acc, -1, FR)
    out = [0] * n
    for i in range(n - 1, -1, -1):
        out[i] = inv * pref[i] % FR
        inv = inv * xs[i] % FR
    return out


def lagrange_coefficients(t: int, m: int):
    """FFTAuxiliary.serialRadix2LagrangeCoefficients (FFTAuxiliary.java:250-302)."""
    if m == 1:
        return [1]
    omega = root_of_unity(m)
    if pow(t, m, FR) == 1:   # t is a domain element: one coefficient is 1
        out, w = [0] * m, 1
        for i in range(m):
            if w == t:
                out[i] = 1
                return out
            w = w * omega % FR
    Z = (pow(t, m, FR) - 1) % FR
    l = Z * pow(m, -1, FR) % FR
    ls, ds, r = [], [], 1
    for _ in range(m):
        ls.append(l)
        ds.append((t - r) % FR)
        l = l * omega % FR
        r = r * omega % FR
    inv = _batch_inverse(ds)
    return [a * b % FR for a, b in zip(ls, inv)]


class QAPRelation:
    pass


def r1cs_to_qap_relation(r1cs: R1CSRelation, t: int) -> QAPRelation:
    """R1CStoQAP.R1CStoQAPRelation (R1CStoQAP.java:37-98)."""
    nc, ni, nv = r1cs.num_constraints, r1cs.num_inputs, r1cs.num_variables
    m = lowest_power_of_two(nc + ni)
    lag = np.array(lagrange_coefficients(t, m), dtype=object)
    q = QAPRelation()
    out = []
    for k, lc in enumerate((r1cs.A, r1cs.B, r1cs.C)):
        acc = np.zeros(nv, dtype=object)
        if k == 0:
            acc[:ni] = lag[nc:nc + ni]
        contrib = lag[lc.row_of_term()]
        if lc.value is not None:
            contrib = contrib * lc.value
        np.add.at(acc, lc.index, contrib)
        out.append([int(x) for x in (acc % FR)])
    q.At, q.Bt, q.Ct = out
    ht, ti = [], 1
    for _ in range(m + 1):
        ht.append(ti)
        ti = ti * t % FR
    q.Ht = ht
    q.Zt = (pow(t, m, FR) - 1) % FR   # SerialFFT.computeZ (SerialFFT.java:140-142)
    q.t, q.num_inputs, q.num_variables, q.degree = t, ni, nv, m
    return q


# ---------------------------------------------------------------------------- QAP instance at t (device)
class R1CSTransposedDevice:
    """The constraint matrices TRANSPOSED, resident in HBM as CSR: row j = the terms (constraint i, coefficient) of
    variable j, with the `input_i * 0 = 0` rows R1CStoQAPRelation adds to A (R1CStoQAP.java:52-55: At[i] gets the
    Lagrange coefficient of constraint numConstraints + i).  Built once per R1CS on the host (a stable sort of the
    terms by variable); At / Bt / Ct at any t are then one sparse product each with the Lagrange vector."""

    def __init__(self, r1cs: R1CSRelation):
        nc, ni, nv = r1cs.num_constraints, r1cs.num_inputs, r1cs.num_variables
        self.nv = nv
        self.mats = []
        for k, lc in enumerate((r1cs.A, r1cs.B, r1cs.C)):
            rows, cols, val = lc.row_of_term(), lc.index, lc.value
            if k == 0:
                rows = np.concatenate((rows, nc + np.arange(ni, dtype=np.int64)))
                cols = np.concatenate((cols, np.arange(ni, dtype=np.int64)))
                if val is not None:
                    val = np.concatenate((val, np.ones(ni, dtype=object)))
            order = np.argsort(cols, kind="stable")
            ptr = np.concatenate(([0], np.cumsum(np.bincount(cols, minlength=nv))))
            assert len(ptr) == nv + 1
            self.mats.append(_CsrDevice(ptr, rows[order], None if val is None else val[order]))
        self.ws = _CsrDevice.workspace(self.mats)


class QAPRelationDevice:
    """R1CStoQAP.R1CStoQAPRelation (R1CStoQAP.java:37-98) with At, Bt, Ct, Ht left in HBM (n x 32-byte LE values);
    the integer lists the host version offers (At, Bt, Ct, Ht) are downloaded on first use (tests)."""

    def __init__(self):
        self._cache = {}

    def _host(self, name):
        if name not in self._cache:
            self._cache[name] = ints32(host_bytes(getattr(self, "d_" + name)))
        return self._cache[name]

    At = property(lambda self: self._host("At"))
    Bt = property(lambda self: self._host("Bt"))
    Ct = property(lambda self: self._host("Ct"))
    Ht = property(lambda self: self._host("Ht"))


def r1cs_to_qap_relation_dev(r1cs: R1CSRelation, t: int, transposed: R1CSTransposedDevice = None) -> QAPRelationDevice:
    """The QAP instance at t on the device: Lagrange coefficients (ozk_qap_lagrange_dev, FFTAuxiliary.java:250-302),
    three sparse products over the transposed matrices (ozk_sparse_mat_vec_dev), the powers of t
    (ozk_fr_powers_dev).  Falls back to the host version when t lies in the domain (t^m = 1: the reference's
    indicator branch, FFTAuxiliary.java:272-283; probability m / r for a random t)."""
    L = _lib.load()
    nc, ni, nv = r1cs.num_constraints, r1cs.num_inputs, r1cs.num_variables
    m = lowest_power_of_two(nc + ni)
    if m < 2 or pow(t, m, FR) == 1:
        return r1cs_to_qap_relation(r1cs, t)
    T = transposed if transposed is not None else R1CSTransposedDevice(r1cs)
    q = QAPRelationDevice()
    st = _stream()
    d_lag = torch.empty(m * 32, dtype=torch.uint8, device="cuda")
    d_zt = torch.empty(32, dtype=torch.uint8, device="cuda")
    wsb = int(L.ozk_qap_lagrange_workspace_bytes(m))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    tb, ob = _le32([t % FR]), _le32([root_of_unity(m)])
    _lib.check(L.ozk_qap_lagrange_dev(vp(tb), vp(ob), m, _ptr(d_lag),
                                      _ptr(d_zt), _ptr(ws), wsb, st))
    outs = []
    for mat in T.mats:
        out = torch.empty(nv * 32, dtype=torch.uint8, device="cuda")
        mat.apply(L.ozk_sparse_mat_vec_dev, d_lag, out, T.ws)
        outs.append(out)
    q.d_At, q.d_Bt, q.d_Ct = outs
    q.d_Ht = torch.empty((m + 1) * 32, dtype=torch.uint8, device="cuda")
    pwb = int(L.ozk_fr_powers_workspace_bytes(m + 1))
    pws = torch.empty(pwb, dtype=torch.uint8, device="cuda")
    one = _le32([1])
    _lib.check(L.ozk_fr_powers_dev(vp(tb), vp(one), m + 1, _ptr(q.d_Ht),
                                   _ptr(pws), pwb, st))
    torch.cuda.current_stream().synchronize()       # the host buffers and workspaces above die here
    q.Zt = int.from_bytes(bytes(d_zt.cpu().numpy()), "little")
    q.d_lagrange = d_lag
    q.t, q.num_inputs, q.num_variables, q.degree = t, ni, nv, m
    return q


# ---------------------------------------------------------------------------- fixed-base batches on the device
def batch_msm_dev(scalar_size: int, window_size: int, base_wire: bytes, scalars, type_: int) -> torch.Tensor:
    """FixedBaseMSM.batchMSM (FixedBaseMSM.java:186-315) with the result left in HBM in the variable-base
    wire-in format: uint8 tensor n x 96 (G1) / n x 192 (G2)."""
    L = _lib.load()
    on_device = isinstance(scalars, torch.Tensor)   # n x 32-byte LE values already in HBM, or a list of ints
    n = scalars.numel() // 32 if on_device else len(scalars)
    outerc = (scalar_size + window_size - 1) // window_size   # FixedBaseMSM.java:212
    if outerc * window_size < 254:
        raise _lib.OzkError("window plan covers %d bits of a 254-bit scalar" % (outerc * window_size))
    d_base = dev_bytes(base_wire)
    d_sc = scalars if on_device else dev_bytes(_le32(scalars))
    out = torch.empty(n * (96 if type_ == 1 else 192), dtype=torch.uint8, device="cuda")
    wsb = int(L.ozk_fixed_batch_msm_workspace_bytes(outerc, window_size, n, type_))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    # (per-call window table: the five batches of ONE setup differ in size, hence in the table window the library
    # chooses, so the table cache of ozk_fixed_batch_msm_base_dev would only add its allocations here — 22 -> 85 ms)
    _lib.check(L.ozk_fixed_batch_msm_compact_dev(outerc, window_size, n, _ptr(d_base), _ptr(d_sc), type_, _ptr(out),
                                                 _ptr(ws), wsb, _stream()))
    torch.cuda.current_stream().synchronize()   # ws / d_sc die here
    return out


def _bit_size(wire: bytes) -> int:
    """BNG1.bitSize / BNG2.bitSize (BNG1.java:174-176): the longest coordinate."""
    return max(int.from_bytes(wire[k:k + 32], "little").bit_length() for k in range(0, len(wire), 32))


class _LazyScalars(dict):
    """the scalars behind the key elements, as lists of ints; device-resident ones are downloaded on first use"""

    def __getitem__(self, k):
        v = dict.__getitem__(self, k)
        if isinstance(v, torch.Tensor):
            v = ints32(host_bytes(v))
            dict.__setitem__(self, k, v)
        return v


_PK_G1 = ("alpha_g1", "beta_g1", "delta_g1", "query_a", "query_b_g1", "delta_abc_g1", "query_h")
_PK_G2 = ("beta_g2", "delta_g2", "query_b_g2")


def _r1cs_from_key_file(kf) -> R1CSRelation:
    h = kf.header
    return R1CSRelation(*(LinearCombinations(*side) for side in kf.r1cs()), h.num_inputs, h.num_auxiliary)


def _key_point_failure(section, index, code):
    return ValueError("proving key: section %s, point %d does not decode: code %d (%s)"
                      % (section, index, code, _codec.CODE_NAMES.get(code, "?")))


def _first_failure(codes):
    """(index, code) of the first non-zero code of an int32 device tensor, or None"""
    bad = torch.nonzero(codes)
    if bad.numel() == 0:
        return None
    j = int(bad[0, 0].item())
    return j, int(codes[j].item())


class ProvingKey:
    """zk_proof_systems/zkSNARK/objects/ProvingKey.java, every group element resident in HBM in the
    variable-base wire-in format.  to_bytes / save and from_bytes / load move it through the key file of DESIGN.md
    section 14 (keyfile.py); a prover that only proves loads the file without this object
    (SerialProver.from_key_file)."""

    def to_bytes(self) -> bytes:
        """The key file: every point compressed on the device (32 bytes per G1 point, 64 per G2), and the R1CS."""
        r1cs = self.r1cs
        sections = {}
        for name in _PK_G1 + _PK_G2:
            enc = (_codec.compress_g1 if name in _PK_G1 else _codec.compress_g2)(getattr(self, name), "wire_in")
            sections[name] = bytes(enc.cpu().numpy())
        for name, lc in (("r1cs_a", r1cs.A), ("r1cs_b", r1cs.B), ("r1cs_c", r1cs.C)):
            sections[name] = _keyfile.r1cs_section(lc.ptr, lc.index, lc.value)
        return _keyfile.build(r1cs.num_inputs, r1cs.num_auxiliary, r1cs.num_constraints, sections)

    def save(self, path):
        with open(path, "wb") as f:
            f.write(self.to_bytes())

    @staticmethod
    def _from_key_file(kf, verify_digest) -> "ProvingKey":
        if verify_digest:
            kf.verify_digest()
        pk = ProvingKey()
        pk.r1cs = _r1cs_from_key_file(kf)
        for name in _PK_G1 + _PK_G2:
            pts, codes = (_codec.decompress_g1 if name in _PK_G1 else _codec.decompress_g2)(dev_bytes(kf.read(name)), "wire_in")
            bad = _first_failure(codes)
            if bad:
                raise _key_point_failure(name, *bad)
            setattr(pk, name, pts)
        return pk

    @staticmethod
    def from_bytes(b, verify_digest=True) -> "ProvingKey":
        """The key of a key file, its points decoded on the device into wire-in tensors, with pk.r1cs: what
        serial_setup_generate returns as crs.proving_key.  ValueError for a malformed file (keyfile.py names what is
        wrong) and for a point that does not decode (section, index and codec.CODE_NAMES[code])."""
        return ProvingKey._from_key_file(_keyfile.KeyFile(b), verify_digest)

    @staticmethod
    def load(path, verify_digest=True) -> "ProvingKey":
        kf = _keyfile.KeyFile(path)
        try:
            return ProvingKey._from_key_file(kf, verify_digest)
        finally:
            kf.close()

    def contribute(self, vk=None, d=None, *, nonce=None, previous=b""):
        """(the key after a phase-2 contribution, its verification key or None, the receipt): ceremony.contribute"""
        from . import ceremony as _ceremony
        return _ceremony.contribute(self, vk, d, nonce=nonce, previous=previous)

    def verify_contribution(self, pk_after, receipt, **kw) -> bool:
        """pk_after is this key after one honest contribution described by `receipt`: ceremony.verify_contribution"""
        from . import ceremony as _ceremony
        return _ceremony.verify_contribution(self, pk_after, receipt, **kw)


class CRS:
    pass


def serial_setup_generate(r1cs: R1CSRelation, seed: int = SEED, log=None) -> CRS:
    """SerialSetup.generate (SerialSetup.java:32-192) without the pairing of the verification key."""
    tm = {}
    t0 = time.perf_counter()
    t = alpha = beta = gamma = delta = fr_random(seed)          # :40-44
    inv_gamma, inv_delta = pow(gamma, -1, FR), pow(delta, -1, FR)
    on_device = os.environ.get("OZK_SETUP_HOST", "0") != "1"
    if on_device:
        # the transposed matrices are a property of the R1CS (built once, like the CSR arrays of R1CSDevice), not of t
        if getattr(r1cs, "_transposed_dev", None) is None:
            r1cs._transposed_dev = R1CSTransposedDevice(r1cs)
            torch.cuda.synchronize()
        tm["r1cs_transpose_once_host_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        qap = r1cs_to_qap_relation_dev(r1cs, t, r1cs._transposed_dev)                          # :50
    else:
        qap = r1cs_to_qap_relation(r1cs, t)
    on_device = isinstance(qap, QAPRelationDevice)
    if on_device:
        torch.cuda.synchronize()
    tm["qap_relation_%s_s" % ("device" if on_device else "host")] = time.perf_counter() - t0
    ni, nv = qap.num_inputs, qap.num_variables
    if on_device:
        # (beta At + alpha Bt + Ct) / gamma for the inputs, / delta for the rest (:61-74), and the non-zero counts
        # behind the window sizes (:76-88), without the values leaving HBM
        L = _lib.load()
        k3 = torch.empty(96, dtype=torch.uint8, device="cuda")
        d_gamma_abc = torch.empty(ni * 32, dtype=torch.uint8, device="cuda")
        d_delta_abc = torch.empty((nv - ni) * 32, dtype=torch.uint8, device="cuda")
        kb, ka = _le32([beta]), _le32([alpha])
        for lo, cnt, kk, out in ((0, ni, inv_gamma, d_gamma_abc), (ni, nv - ni, inv_delta, d_delta_abc)):
            if cnt > 0:
                kkb = _le32([kk])
                _lib.check(L.ozk_fr_lincomb3_dev(_ptr(qap.d_At) + 32 * lo, _ptr(qap.d_Bt) + 32 * lo, _ptr(qap.d_Ct) + 32 * lo,
                                                 cnt, vp(kb), vp(ka), vp(kkb), _ptr(out), _ptr(k3), _stream()))
                torch.cuda.current_stream().synchronize()
        gamma_abc, delta_abc = d_gamma_abc, d_delta_abc
        non_zero_at = int((qap.d_At.view(nv, 32) != 0).any(dim=1).sum().item())
        non_zero_bt = int((qap.d_Bt.view(nv, 32) != 0).any(dim=1).sum().item())
    else:
        abc = [(beta * a + alpha * b + c) % FR for a, b, c in zip(qap.At, qap.Bt, qap.Ct)]
        gamma_abc = [x * inv_gamma % FR for x in abc[:ni]]          # :61-66
        delta_abc = [x * inv_delta % FR for x in abc[ni:]]          # :69-74
        non_zero_at = sum(1 for x in qap.At if x)                   # :76-88
        non_zero_bt = sum(1 for x in qap.Bt if x)
    # :91-112 generators = one * random, window sizes from the per-curve tables
    rnd = fr_random(seed)
    gen_g1 = bytes(batch_msm_dev(254, 16, g1_wire(G1_ONE), [rnd], 1).cpu().numpy())
    gen_g2 = bytes(batch_msm_dev(254, 16, g2_wire(G2_ONE), [rnd], 2).cpu().numpy())
    scalar_size_g1, scalar_size_g2 = _bit_size(gen_g1), _bit_size(gen_g2)
    window_g1 = get_window_size(non_zero_at + non_zero_bt + nv, G1_WINDOW_TABLE)
    window_g2 = get_window_size(non_zero_bt, G2_WINDOW_TABLE)
    t1 = time.perf_counter()

    def b1(scalars):
        return batch_msm_dev(scalar_size_g1, window_g1, gen_g1, scalars, 1)

    def b2(scalars):
        return batch_msm_dev(scalar_size_g2, window_g2, gen_g2, scalars, 2)

    pk = ProvingKey()
    k1 = b1([alpha, beta, delta])                               # :117-121
    pk.alpha_g1, pk.beta_g1, pk.delta_g1 = k1[:96], k1[96:192], k1[192:288]
    k2 = b2([beta, delta, gamma])
    pk.beta_g2, pk.delta_g2, gamma_g2 = k2[:192], k2[192:384], k2[384:576]
    pk.delta_abc_g1 = b1(delta_abc)                             # :123-126
    pk.query_a = b1(qap.d_At if on_device else qap.At)          # :128-131
    pk.query_b_g1 = b1(qap.d_Bt if on_device else qap.Bt)       # :133-144 doubleBatchMSM: G1 and G2 over Bt
    pk.query_b_g2 = b2(qap.d_Bt if on_device else qap.Bt)
    inv_delta_zt = qap.Zt * inv_delta % FR                      # :146-151
    if on_device:
        L = _lib.load()
        ht_scalars = torch.empty((qap.degree + 1) * 32, dtype=torch.uint8, device="cuda")
        pwb = int(L.ozk_fr_powers_workspace_bytes(qap.degree + 1))
        pws = torch.empty(pwb, dtype=torch.uint8, device="cuda")
        tb, kb2 = _le32([t]), _le32([inv_delta_zt])
        _lib.check(L.ozk_fr_powers_dev(vp(tb), vp(kb2), qap.degree + 1,
                                       _ptr(ht_scalars), _ptr(pws), pwb, _stream()))
        torch.cuda.current_stream().synchronize()
    else:
        ht_scalars = [h * inv_delta_zt % FR for h in qap.Ht]
    pk.query_h = b1(ht_scalars)
    pk.r1cs = r1cs
    crs = CRS()
    crs.proving_key = pk
    crs.gamma_g2 = gamma_g2                                     # :160-164
    crs.gamma_abc_g1 = b1(gamma_abc)
    tm["fixed_base_gpu_s"] = time.perf_counter() - t1
    # kept for checks in the exponent (tests): the scalars behind every key element
    crs.qap = qap
    crs.secrets = dict(t=t, alpha=alpha, beta=beta, gamma=gamma, delta=delta, generator=rnd)
    crs.scalars = _LazyScalars(delta_abc=delta_abc, gamma_abc=gamma_abc, ht=ht_scalars)
    crs.gen_g1, crs.gen_g2 = gen_g1, gen_g2
    crs.window_g1, crs.window_g2 = window_g1, window_g2
    crs.scalar_size_g1, crs.scalar_size_g2 = scalar_size_g1, scalar_size_g2
    crs.timing = tm
    if log:
        log("setup: QAP instance (%s) %.3f s, fixed-base batches (GPU, incl. marshalling) %.2f s"
            % ("device" if on_device else "host", tm.get("qap_relation_device_s", tm.get("qap_relation_host_s")),
               tm["fixed_base_gpu_s"]))
    return crs


def setup_from_srs(r1cs: R1CSRelation, srs, log=None) -> CRS:
    """The key of `r1cs` from a powers-of-tau string (srs.Srs), computed on the GPU without tau, alpha or beta, with
    gamma = delta = 1: srs.setup_from_srs.  crs.secrets is None: nobody needs to know any."""
    from . import srs as _srs
    return _srs.setup_from_srs(r1cs, srs, log)


# ---------------------------------------------------------------------------- prover
def _g1_pipeline(sizes):
    """The prover's G1 pipeline (device.VarMsmPipeline3 / VarMsmPipeline over the lengths of its MSMs, throughput-shaped
    tails: the proof keeps the vector ALU busy from start to end, so the additions the serial levels save are worth more
    than the dependent additions they add) as the environment selects it: three-stage by default, one tail stream (a
    2^20-constraint proof: 15.6-15.7 ms against 15.9 with the two-stage pipeline of round 2, OZK_PROVER_PIPE3=0; two
    tail streams, OZK_PROVER_TAIL_STREAMS=2, measure the same as one); OZK_PROVER_LAST_LONE=0 sends the last MSM
    through the stages like the others.  (OZK_P3_SPLIT_ACCUM and OZK_P3_TAIL_CUS are not for the prover.)"""
    lone = os.environ.get("OZK_PROVER_LAST_LONE", "1") != "0"
    if os.environ.get("OZK_PROVER_PIPE3", "1") == "1":
        return _dev.VarMsmPipeline3(sizes, 1, depth=4, tail_streams=int(os.environ.get("OZK_PROVER_TAIL_STREAMS", "1")),
                                    tail_mode=1, last_lone=lone, split_accum=False, tail_cus=0)
    return _dev.VarMsmPipeline(sizes, 1, depth=2, tail_mode=1, last_lone=lone)


class Proof:
    """zk_proof_systems/zkSNARK/objects/Proof.java: gA (G1), gB (G2), gC (G1) — wire-out bytes."""

    def __init__(self, a, b, c):
        self.g_a, self.g_b, self.g_c = a, b, c

    def to_bytes(self) -> bytes:
        """The 128-byte compressed form A (32) | B (64) | C (32) of DESIGN.md section 13, encoded on the device."""
        a = _codec.compress_g1(dev_bytes(bytes(self.g_a)), "wire_out")
        b = _codec.compress_g2(dev_bytes(bytes(self.g_b)), "wire_out")
        c = _codec.compress_g1(dev_bytes(bytes(self.g_c)), "wire_out")
        return bytes(torch.cat([a, b, c]).cpu().numpy())

    @staticmethod
    def from_bytes(b) -> "Proof":
        """The proof of 128 compressed bytes, decoded on the device.  ValueError names the first point that does not
        decode and its code (codec.CODE_NAMES)."""
        if len(b) != 128:
            raise ValueError("a compressed proof is 128 bytes, not %d" % len(b))
        return proofs_from_bytes(b)[0]


def _decode_failure(what, index, code):
    return ValueError("%s %s does not decode: code %d (%s)" % (what, index, code, _codec.CODE_NAMES.get(code, "?")))


def proofs_from_bytes(buf) -> list:
    """The proofs of K x 128 compressed bytes, decoded in one launch.  ValueError on the first proof with a point that
    does not decode."""
    buf = bytes(buf)
    if not buf or len(buf) % 128:
        raise ValueError("%d bytes are not a whole number of 128-byte proofs" % len(buf))
    k = len(buf) // 128
    enc = dev_bytes(buf).view(k, 128)
    # the three points apart, so that a failure can name its point (the proof entry reports one code per proof)
    parts = (("A", _codec.decompress_g1(enc[:, :32], "wire_out")), ("B", _codec.decompress_g2(enc[:, 32:96], "wire_out")),
             ("C", _codec.decompress_g1(enc[:, 96:], "wire_out")))
    codes = torch.stack([c for _, (_, c) in parts], dim=1).cpu().tolist()
    for i, row in enumerate(codes):
        for (name, _), code in zip(parts, row):
            if code:
                raise _decode_failure("proof %d: point" % i, name, code)
    raws = [bytes(pts.cpu().numpy()) for _, (pts, _) in parts]
    return [Proof(raws[0][192 * i:192 * (i + 1)], raws[1][384 * i:384 * (i + 1)], raws[2][192 * i:192 * (i + 1)])
            for i in range(k)]


RECORD_BYTES = 768   # a rank's partial: A_r (G1, 192) | B_r (G2, 384) | C_r (G1, 192), wire-out


def shard_plan(nv: int, m: int, nw: int, rank: int, world: int):
    """The slices [lo, hi) rank `rank` of `world` owns of the five MSMs of a proof, as the prover lays them out:
    A, B1 and B2 over query A / query B ++ [alpha or beta, delta] (nv + 2 pairs), L over deltaABC (nw), H over
    query H (m + 1)."""
    ab = shard_range(nv + 2, rank, world)
    return {"A": ab, "B1": ab, "B2": ab, "L": shard_range(nw, rank, world), "H": shard_range(m + 1, rank, world)}


def c_share_scalars(r: int, s: int, rank: int):
    """The scalars of a rank's 3-term MSM over [A_r, B1_r, deltaG1]: s A_r + r B1_r, and the -rs delta of
    SerialProver.java:114 on rank 0 only, so that the ranks' shares sum to SerialProver's."""
    return [s, r, (FR - r * s % FR) % FR if rank == 0 else 0]


def _rows(parts, lo, hi, row_bytes):
    """rows [lo, hi) of the concatenation of `parts` (uint8 tensors of row_bytes-byte rows), without building the
    whole concatenation (a range inside one part is a view of it)"""
    out, base = [], 0
    for t in parts:
        n = t.numel() // row_bytes
        a, b = max(lo - base, 0), min(hi - base, n)
        if a < b:
            out.append(t[a * row_bytes:b * row_bytes])
        base += n
    return out[0] if len(out) == 1 else torch.cat(out)


def _prepared_bytes(n, type_):
    return int(_lib.load().ozk_var_msm_prepared_bytes(n, type_))


class ShardedProver:
    """Rank `rank` of a Groth16 prover sharded over `world` GPUs (DistributedProver.java:89-146 with its
    distributedMSM / distributedDoubleMSM): the prover's scalars are linear in the key, so each rank finishes its
    share of every proof element over its slices of the key (shard_plan) before any exchange, and sends one
    768-byte record; the proof is the sum of the records (distributed.distributed_prove, device.groth16_combine).
    Only this rank's slices are prepared (key_bytes: this rank's prepared-key bytes against SerialProver's).
    The witness map runs on every rank (a replica: DESIGN.md section 7).  This class holds the one schedule of a
    proof's device work (_enqueue); SerialProver is its rank 0 of a world of one."""

    # the five MSMs of a proof: plan key -> (the key arrays whose concatenation it runs over, group)
    # A = alpha + sum z_i A_i(t) + r delta (SerialProver.java:76-79,105): the Java sums a primary-input MSM,
    # an auxiliary-input MSM, alpha and r delta; here ONE MSM over query A ++ [alphaG1, deltaG1] with scalars
    # z ++ [1, r] — the same group element, hence the same affine bytes, without the two short MSMs (each of
    # which costs a whole latency-bound tail) and four additions.  B likewise with beta, delta and s (:82-88,108-110).
    _MSMS = (("qa", "A", ("query_a", "alpha_g1", "delta_g1"), 1), ("qb1", "B1", ("query_b_g1", "beta_g1", "delta_g1"), 1),
             ("qb2", "B2", ("query_b_g2", "beta_g2", "delta_g2"), 2), ("dabc", "L", ("delta_abc_g1",), 1),
             ("qh", "H", ("query_h",), 1))

    def __init__(self, pk: ProvingKey, rank: int, world: int):
        r1cs = pk.r1cs
        self._shape(r1cs.num_inputs, r1cs.num_variables, r1cs.num_constraints, rank, world)
        assert pk.query_h.numel() == (self.m + 1) * 96 and pk.query_a.numel() == self.nv * 96
        for attr, key, names, type_ in self._MSMS:
            lo, hi = self.plan[key]
            setattr(self, attr, prepare_bases(_rows([getattr(pk, n) for n in names], lo, hi, 96 * type_), hi - lo, type_))
            torch.cuda.current_stream().synchronize()   # a concatenated slice dies here
        self._finish(r1cs, pk.delta_g1)

    @classmethod
    def from_key_file(cls, path_or_file, rank: int = 0, world: int = 1, check_subgroup: bool = True, verify_digest=None,
                      timing=None):
        """The prover of rank `rank` straight from a key file (a path or a binary file
        object).  Read are the header, the R1CS sections and, by offset, the rows of shard_plan for this rank — joined
        compressed, uploaded compressed and decoded on the device into the prepared bases
        (codec.decompress_prepared): no wire-in copy of the key exists at any time, on the host or in HBM, and a rank
        never holds more than its 1 / world of it.  check_subgroup: the points of query B in G2, beta and delta are
        checked for order r.  ValueError for a malformed file and for a point that does not decode (section, index,
        codec.CODE_NAMES[code]).
        verify_digest: the SHA-256 of the header covers the whole file, so checking it reads the whole file.  The
        default (None) checks it when world = 1 and not when world > 1, where the point of a rank is not to read the
        other ranks' rows; pass True to check it on a rank all the same.
        `timing` (optional dict) receives read_s, upload_s and decode_s, wall times with a synchronise between."""
        kf = _keyfile.KeyFile(path_or_file)
        T = {"read_s": 0.0, "upload_s": 0.0, "decode_s": 0.0}
        try:
            if (world == 1) if verify_digest is None else verify_digest:
                kf.verify_digest()
            h = kf.header
            self = cls.__new__(cls)
            self._shape(h.num_inputs, h.nv, h.num_constraints, rank, world)
            t0 = time.perf_counter()
            r1cs = _r1cs_from_key_file(kf)
            T["read_s"] += time.perf_counter() - t0
            for attr, key, names, type_ in self._MSMS:
                lo, hi = self.plan[key]
                t0 = time.perf_counter()
                enc, parts = kf.read_joined(names, lo, hi)
                t1 = time.perf_counter()
                d_enc = dev_bytes(enc)
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                prepared, codes = _codec.decompress_prepared(d_enc, type_, check_subgroup)
                bad = _first_failure(codes)   # (synchronises)
                t3 = time.perf_counter()
                T["read_s"] += t1 - t0
                T["upload_s"] += t2 - t1
                T["decode_s"] += t3 - t2
                if bad:
                    raise _key_point_failure(*_keyfile.locate(parts, bad[0]), bad[1])
                setattr(self, attr, prepared)
            # deltaG1 once more as a wire-in point: a base of the 3-term MSM behind every rank's share of C
            delta, codes = _codec.decompress_g1(dev_bytes(kf.read("delta_g1")), "wire_in")
            bad = _first_failure(codes)
            if bad:
                raise _key_point_failure("delta_g1", *bad)
        finally:
            kf.close()
        self._finish(r1cs, delta)
        if timing is not None:
            timing.update(T)
        return self

    def _shape(self, ni, nv, nc, rank, world):
        """the sizes of the key and this rank's slices of the five MSMs"""
        self.rank, self.world = rank, world
        self.ni, self.nv = ni, nv
        self.nw = nv - ni
        self.m = lowest_power_of_two(nc + ni)
        nw, m = self.nw, self.m
        if not 0 <= rank < world:
            raise ValueError("rank %d outside a world of %d" % (rank, world))
        if world > min(nv + 2, nw, m + 1):
            raise ValueError("a world of %d leaves a rank an empty slice (slice lengths nv + 2 = %d, nw = %d, m + 1 = %d)"
                             % (world, nv + 2, nw, m + 1))
        self.plan = shard_plan(nv, m, nw, rank, world)

    def _finish(self, r1cs, delta_g1):
        """everything after "the five prepared buffers exist" (qa, qb1, qb2, dabc, qh): the same for a key in HBM and
        a key file"""
        L = _lib.load()
        nv, nw, m, plan = self.nv, self.nw, self.m, self.plan
        self.delta_g1 = delta_g1
        self.key_bytes = {
            "rank": sum(int(t.numel()) for t in (self.qa, self.qb1, self.qb2, self.dabc, self.qh)),
            "serial": (2 * _prepared_bytes(nv + 2, 1) + _prepared_bytes(nv + 2, 2) + _prepared_bytes(nw, 1)
                       + _prepared_bytes(m + 1, 1))}
        n_ab, n_l, n_h = (hi - lo for lo, hi in (plan["A"], plan["L"], plan["H"]))
        self.pipe = _g1_pipeline([n_ab, n_h, n_l])
        self.g2_ws_bytes = int(L.ozk_var_msm_head_workspace_bytes(n_ab, 2))
        self.g2_ws = torch.empty(self.g2_ws_bytes, dtype=torch.uint8, device="cuda")
        self.g2_tail_bytes = int(L.ozk_var_msm_tail_bytes(n_ab, 2))
        self.g2_tail = torch.empty(self.g2_tail_bytes, dtype=torch.uint8, device="cuda")
        self.s_g2 = torch.cuda.Stream()
        # witness map + C's share: dispatched ahead of the MSMs that do not depend on them (the H MSM waits for the map)
        self.s_fin = torch.cuda.Stream(priority=-1)
        self.fin_ws_bytes = int(L.ozk_var_msm_workspace_bytes(3, 1))
        self.fin_ws = torch.empty(self.fin_ws_bytes, dtype=torch.uint8, device="cuda")
        self.q_ws_bytes = int(L.ozk_qap_witness_workspace_bytes(m))
        self.q_ws = torch.empty(self.q_ws_bytes, dtype=torch.uint8, device="cuda")
        self.d_h = torch.empty((m + 1) * 32, dtype=torch.uint8, device="cuda")
        self.o1 = torch.zeros(4, 192, dtype=torch.uint8, device="cuda")   # B1_r, L_r, H_r, C's 3-term share
        self.r1cs_dev = R1CSDevice(r1cs)   # the constraint matrices, uploaded once per key
        self.omega = ctypes.create_string_buffer(root_of_unity(m).to_bytes(32, "little"), 32)
        self.g = ctypes.create_string_buffer(FR_MULT_GEN.to_bytes(32, "little"), 32)
        torch.cuda.synchronize()

    def close(self):
        self.pipe.close()

    def _marshal(self, primary, auxiliary, full_bytes):
        """`full_bytes` if given: the assignment primary ++ auxiliary already marshalled (assignment_bytes) — what a
        caller that keeps its witness as bytes hands over; otherwise it is marshalled here."""
        if full_bytes is None:
            full_bytes = assignment_bytes(list(primary) + list(auxiliary))
        assert full_bytes.size == self.nv * 32
        return full_bytes

    def _witness_upload(self, full_bytes, seed):
        """What _enqueue works on, in HBM: the assignment, this rank's slices of z ++ [1, r] and z ++ [1, s], the
        scalars of C's 3-term share, and the zeroed record."""
        r = fr_random(seed)                                      # SerialProver.java:58-59
        s = fr_random(seed)
        lo, hi = self.plan["A"]
        d_full = torch.from_numpy(full_bytes).cuda()
        tails = dev_bytes(_le32([1, r, 1, s] + c_share_scalars(r, s, self.rank)))
        d_sc_r = torch.cat((d_full, tails[:64]))[32 * lo:32 * hi]
        d_sc_s = torch.cat((d_full, tails[64:128]))[32 * lo:32 * hi]
        rec = torch.zeros(RECORD_BYTES, dtype=torch.uint8, device="cuda")
        return d_full, d_sc_r, d_sc_s, tails[128:], rec

    def _enqueue(self, d_full, d_sc_r, d_sc_s, d_fin_sc, rec, mark=None):
        """One proof's device work over the tensors of _witness_upload, asynchronous: on return the current stream is behind
        all of it, and `rec` will hold A_r | B_r | C_r.  mark(name, stream), if given, is called where the device
        work starts, where the witness map, the L and H MSMs and the record are done (timing events)."""
        L = _lib.load()
        ni, m, o1 = self.ni, self.m, self.o1
        (lo, hi), (llo, lhi), (hlo, hhi) = self.plan["A"], self.plan["L"], self.plan["H"]
        n_ab = hi - lo
        main = torch.cuda.current_stream()
        if mark:
            mark("start", main)
        ready = torch.cuda.Event()
        ready.record(main)
        # B_r in G2 (doubleMSM, SerialProver.java:82-88): own stream, nothing to wait for but the uploads.  Issued
        # first: its tail is the longest latency-bound chain of the proof and hides under the G1 accumulations.
        self.s_g2.wait_event(ready)
        with torch.cuda.stream(self.s_g2):
            _lib.check(L.ozk_var_msm_head_dev(_ptr(self.qb2), 1, _ptr(d_sc_s), n_ab, 2, _ptr(self.g2_ws),
                                              self.g2_ws_bytes, _ptr(self.g2_tail), self.g2_tail_bytes, _stream(), None))
            _lib.check(L.ozk_var_msm_tail_dev(n_ab, 2, _ptr(self.g2_tail), self.g2_tail_bytes, _ptr(rec[192:576]),
                                              _stream(), None, 1))
            g2_done = torch.cuda.Event()
            g2_done.record(self.s_g2)
        # witness map (SerialProver.java:36-41): constraint evaluations (R1CStoQAP.java:143-160,195-199) and the
        # seven transforms on the device; coefficientsH stay in HBM.  Own stream: only the H MSM waits for it, the
        # three MSMs over the assignment run beside it.  Whole on every rank: coefficientsH are the same on all.
        self.s_fin.wait_event(ready)
        with torch.cuda.stream(self.s_fin):
            d_ev = self.r1cs_dev.evaluate(d_full)
            _lib.check(L.ozk_qap_witness_dev(_ptr(d_ev[0]), _ptr(d_ev[1]), _ptr(d_ev[2]), m, ctypes.cast(self.omega, ctypes.c_void_p),
                                             ctypes.cast(self.g, ctypes.c_void_p), _ptr(self.d_h), _ptr(self.q_ws),
                                             self.q_ws_bytes, _stream()))
            h_ready = torch.cuda.Event()
            h_ready.record(self.s_fin)
            if mark:
                mark("map", self.s_fin)
        p = self.pipe
        submit = lambda q, d_sc, n, out, last=False: p.done(p.submit(q, d_sc, prepared=True, last=last, n=n, out=out))
        ev_a = submit(self.qa, d_sc_r, n_ab, rec[:192])           # :76-79,105  A
        ev_b = submit(self.qb1, d_sc_s, n_ab, o1[0])              # :82-88,108-110  B in G1
        # A_r and B1_r are complete once their tails are: their share of C — s A + r B1 - r s delta (:114) — is a
        # 3-term MSM that runs on its own stream while the long MSMs still occupy the pipeline.  (The waits are queued
        # NOW: the pipeline re-records these per-slot events for the next two submissions.)
        self.s_fin.wait_event(ev_a)
        self.s_fin.wait_event(ev_b)
        ev_l = submit(self.dabc, d_full[32 * (ni + llo):32 * (ni + lhi)], lhi - llo, o1[1])     # :98-101 deltaABC
        main.wait_event(h_ready)
        # query H (:91-93) is the last MSM: alone through the single-call entry point if the pipeline is last_lone,
        # otherwise through the stages exactly like the others (so not announced: no latency-shaped tail either)
        ev_h = submit(self.qh, self.d_h[32 * hlo:32 * hhi], hhi - hlo, o1[2], last=p.last_lone)
        with torch.cuda.stream(self.s_fin):
            fin_bases = torch.cat((wire_out_to_in(rec[:192], 1), wire_out_to_in(o1[0], 1), self.delta_g1))
            _lib.check(L.ozk_var_msm_dev(_ptr(fin_bases), _ptr(d_fin_sc), 3, 1, _ptr(o1[3]), _ptr(self.fin_ws),
                                         self.fin_ws_bytes, _stream()))
            fin_done = torch.cuda.Event()
            fin_done.record(self.s_fin)
        main.wait_event(ev_l)
        main.wait_event(ev_h)
        if mark:
            mark("msm", main)
        main.wait_event(fin_done)
        # C_r = L_r + H_r + (s A_r + r B1_r [- rs delta]): evaluationABC + H(t)Z(t)/delta + C's share (:102,:114)
        _lib.check(L.ozk_points_sum_dev(_ptr(o1[1:4]), 3, 1, _ptr(rec[576:]), int(main.cuda_stream)))
        main.wait_event(g2_done)
        if mark:
            mark("end", main)
        self._keep = (d_full, d_sc_r, d_sc_s, d_fin_sc, fin_bases, d_ev)

    def prove_partial(self, primary, auxiliary, seed: int = SEED, timing=None, full_bytes=None) -> torch.Tensor:
        """This rank's 768-byte record A_r | B_r | C_r (uint8 tensor in HBM, complete on return) with
        C_r = L_r + H_r + s A_r + r B1_r (- rs deltaG1 on rank 0).  `timing` (optional dict) receives the stage
        times of the device work from its start: witness map done, L and H MSMs done, record done."""
        t0 = time.perf_counter()
        up = self._witness_upload(self._marshal(primary, auxiliary, full_bytes), seed)
        at = {}

        def mark(name, stream):
            at[name] = torch.cuda.Event(enable_timing=True)
            at[name].record(stream)

        self._enqueue(*up, mark=mark if timing is not None else None)
        torch.cuda.synchronize()
        if timing is not None:
            timing.update({"witness_map_done_ms": at["start"].elapsed_time(at["map"]),
                           "lh_msm_done_ms": at["start"].elapsed_time(at["msm"]),
                           "record_done_ms": at["start"].elapsed_time(at["end"]),
                           "partial_wall_ms": (time.perf_counter() - t0) * 1e3})
        return up[-1]

    def coefficients_h(self):
        """coefficientsH of the last proof (m + 1 ints), for checks."""
        return ints32(host_bytes(self.d_h))


class SerialProver(ShardedProver):
    """SerialProver.prove (SerialProver.java:26-119) over a proving key resident in HBM: rank 0 of a world of one of
    the sharded schedule, whose record already is the proof (C_0 = L + H + s A + r B1 - rs delta), so nothing is
    exchanged or combined.  Construct once per key (prepares the bases), call prove() per witness."""

    def __init__(self, pk: ProvingKey):
        super().__init__(pk, 0, 1)

    @classmethod
    def from_key_file(cls, path_or_file, check_subgroup: bool = True, verify_digest: bool = True, timing=None):
        """The prover of a key file (ShardedProver.from_key_file for rank 0 of a world of one): the file is read once,
        its digest checked, its points decoded straight into the prepared bases."""
        return super().from_key_file(path_or_file, 0, 1, check_subgroup, verify_digest, timing)

    def prove(self, primary, auxiliary, seed: int = SEED, timing=None, full_bytes=None) -> Proof:
        """`full_bytes` (optional): the assignment already marshalled (assignment_bytes).  `timing` (optional dict)
        receives the host marshalling, the upload and the device work as wall times, a synchronise between each."""
        T = {}
        t0 = time.perf_counter()
        full_bytes = self._marshal(primary, auxiliary, full_bytes)
        T["marshal_assignment_host_ms"] = (time.perf_counter() - t0) * 1e3
        t1 = time.perf_counter()
        up = self._witness_upload(full_bytes, seed)
        torch.cuda.synchronize()
        T["upload_ms"] = (time.perf_counter() - t1) * 1e3
        t2 = time.perf_counter()
        self._enqueue(*up)
        torch.cuda.synchronize()
        T["gpu_ms"] = (time.perf_counter() - t2) * 1e3
        raw = bytes(up[-1].cpu().numpy())
        if timing is not None:
            timing.update(T)
        return Proof(raw[:192], raw[192:576], raw[576:])


# ---------------------------------------------------------------------------- verification (pairing.py)
class VerificationKey:
    """zk_proof_systems/zkSNARK/objects/VerificationKey.java: alphaG1betaG2 (GT, 384 B), gammaG2, deltaG2 (wire-in
    G2) and gammaABC (wire-in G1, one point per primary input), all in HBM; gamma and delta are also kept prepared
    (their Miller-loop line coefficients, computed once per key)."""

    def __init__(self, alpha_g1_beta_g2, gamma_g2, delta_g2, gamma_abc_g1):
        self.alpha_g1_beta_g2 = alpha_g1_beta_g2
        self.gamma_g2, self.delta_g2, self.gamma_abc_g1 = gamma_g2, delta_g2, gamma_abc_g1
        self.num_inputs = gamma_abc_g1.numel() // 96
        self.gamma_prep = _pairing.prepare_g2(gamma_g2)
        self.delta_prep = _pairing.prepare_g2(delta_g2)
        self._msm = None
        self._multi = None

    def evaluation_abc(self, primary) -> torch.Tensor:
        """sum primary_i gammaABC_i (Verifier.java:45-47, VariableBaseMSM.serialMSM) through the variable-base MSM;
        192-byte wire-out point, asynchronous on the current stream"""
        if len(primary) != self.num_inputs:
            raise ValueError("%d primary inputs for a key of %d" % (len(primary), self.num_inputs))
        if self._msm is None:
            self._msm = _dev.VarMsmWorkspace(self.num_inputs, 1)
        return self._msm.run(self.gamma_abc_g1, dev_bytes(_le32(primary))).clone()

    def evaluation_abc_batch(self, primaries) -> torch.Tensor:
        """evaluation_abc of every row of `primaries`, concatenated (K x 192 bytes, byte for byte what K calls of
        evaluation_abc return), through the shared-base batched MSM: the window table of gammaABC is built at the
        first call and kept with the key.  Asynchronous on the current stream."""
        for primary in primaries:
            if len(primary) != self.num_inputs:
                raise ValueError("%d primary inputs for a key of %d" % (len(primary), self.num_inputs))
        if self._multi is None:
            self._multi = _dev.SharedBaseMsm(self.gamma_abc_g1, self.num_inputs)
        return self._multi.run(dev_bytes(b"".join(_le32(primary) for primary in primaries)), len(primaries))


    MAGIC = b"OZKVK\x00\x00\x01"   # five letters, two zero bytes, format version 1

    def to_bytes(self) -> bytes:
        """magic and version (8) | num_inputs u32 | 4 bytes of padding | alphaG1betaG2 (384, as the device holds it) |
        gammaG2 (64) | deltaG2 (64) | gammaABC (32 each), the points compressed"""
        g2 = _codec.compress_g2(torch.cat([self.gamma_g2.reshape(-1), self.delta_g2.reshape(-1)]))
        abc = _codec.compress_g1(self.gamma_abc_g1)
        body = torch.cat([self.alpha_g1_beta_g2.reshape(-1), g2, abc])
        return self.MAGIC + self.num_inputs.to_bytes(4, "little") + bytes(4) + bytes(body.cpu().numpy())

    @staticmethod
    def from_bytes(b) -> "VerificationKey":
        """The key of to_bytes; the points are decoded on the device and the prepared lines of gamma and delta rebuilt
        by the constructor.  ValueError on a bad header or length and on any point that does not decode."""
        b = bytes(b)
        if len(b) < 16 or b[:8] != VerificationKey.MAGIC or b[12:16] != bytes(4):
            raise ValueError("not a verification key (bad magic, version or padding)")
        n = int.from_bytes(b[8:12], "little")
        if n < 1 or len(b) != 16 + 384 + 128 + 32 * n:
            raise ValueError("a verification key of %d inputs is %d bytes, not %d" % (n, 528 + 32 * n, len(b)))
        body = dev_bytes(b[16:])
        g2, c2 = _codec.decompress_g2(body[384:512])
        abc, c1 = _codec.decompress_g1(body[512:])
        for i, code in enumerate(torch.cat([c2, c1]).cpu().tolist()):
            if code:
                raise _decode_failure("verification key: point", ("gammaG2", "deltaG2")[i] if i < 2
                                      else "gammaABC[%d]" % (i - 2), code)
        return VerificationKey(body[:384].clone(), g2[:192].clone(), g2[192:].clone(), abc)


def verification_key(crs: CRS) -> VerificationKey:
    """The verification key of a CRS from serial_setup_generate (SerialSetup.java:159-164): alphaG1betaG2 =
    reducedPairing(alphaG1, betaG2) computed on the device."""
    pk = crs.proving_key
    alpha_beta = _pairing.reduced_pairing(pk.alpha_g1, pk.beta_g2)
    return VerificationKey(alpha_beta, crs.gamma_g2, pk.delta_g2, crs.gamma_abc_g1)


def proof_record(proof: Proof) -> bytes:
    """A | B | C, 768 bytes of wire-out (the layout of ozk_groth16_combine_dev)"""
    return bytes(proof.g_a) + bytes(proof.g_b) + bytes(proof.g_c)


def _pack_primaries(primaries, n):
    """one 32n-byte row (inputs mod r, little-endian) per primary input, validated as Verifier.java:31-32 asserts.
    A row object that recurs is packed once.  The cache holds the row object itself, so that its id cannot be reused
    by a later row while the cache lives (rows may be temporaries, e.g. the rows of a numpy object array)."""
    packed = {}
    rows = []
    for primary in primaries:
        hit = packed.get(id(primary))
        if hit is not None and hit[0] is primary:
            rows.append(hit[1])
            continue
        if len(primary) != n:
            raise ValueError("%d primary inputs for a key of %d" % (len(primary), n))
        if int(primary[0]) % FR != 1:
            raise ValueError("primary[0] must be 1")
        row = b"".join((int(v) % FR).to_bytes(32, "little") for v in primary)
        packed[id(primary)] = (primary, row)
        rows.append(row)
    return rows


class Verifier:
    """Verifier.verify (zkSNARK/Verifier.java:24-59) on the device.  A proof is accepted exactly when
    e(A, B) == alphaG1betaG2 e(evaluationABC, gamma) e(C, delta), the Java's boolean; no on-curve or subgroup check
    of the proof points (the Java does none)."""

    @staticmethod
    def verify(vk: VerificationKey, primary, proof: Proof) -> bool:
        return Verifier.verify_batch(vk, [primary], [proof])[0]

    # verify_batch(abc="auto") takes the batched evaluationABC from this many proofs upwards.  Per proof the
    # variable-base MSM costs ~0.7 ms; the batched path costs the table build once per key (a serial chain of 128
    # doublings, ~1 ms, plus 9 small launches per chunk of bases) and then three launches per batch, so it pays from
    # the second or third proof of the FIRST batch and from the first proof of every later one.  Below the
    # crossover a key that only ever verifies single proofs keeps the table's memory (128 KiB per input) free.
    ABC_BATCH_CROSSOVER = 4

    @staticmethod
    def verify_batch(vk: VerificationKey, primaries, proofs, abc="auto") -> list:
        """k proofs in one launch pair (the three Miller loops of every proof, then one final exponentiation per
        proof).  evaluationABC: abc="per_proof" runs one variable-base MSM per proof, abc="batched" one shared-base
        batched MSM for all of them (VerificationKey.evaluation_abc_batch), abc="auto" the batched one from
        ABC_BATCH_CROSSOVER proofs upwards (or whenever the key already has its table).  The points, and so the
        verdicts, are the same in all three."""
        if len(primaries) != len(proofs) or not proofs:
            raise ValueError("one primary input per proof, at least one proof")
        abc = Verifier._evaluation_abc(vk, primaries, abc)
        recs = dev_bytes(b"".join(proof_record(p) for p in proofs))
        return Verifier._records_verdicts(vk, recs, abc)

    @staticmethod
    def _evaluation_abc(vk: VerificationKey, primaries, abc) -> torch.Tensor:
        """the evaluationABC points of a batch (K x 192 bytes on the device) in the mode `abc` of verify_batch"""
        if abc not in ("auto", "per_proof", "batched"):
            raise ValueError("abc must be 'auto', 'per_proof' or 'batched'")
        for primary in primaries:
            assert primary[0] % FR == 1   # Verifier.java:31-32
        if abc == "auto":
            batched = len(primaries) >= Verifier.ABC_BATCH_CROSSOVER or vk._multi is not None
            abc = "batched" if batched and 1 <= vk.num_inputs <= 4096 else "per_proof"
        if abc == "batched":
            return vk.evaluation_abc_batch(primaries)
        return torch.cat([vk.evaluation_abc(primary) for primary in primaries])

    @staticmethod
    def _records_verdicts(vk: VerificationKey, recs, abc_points) -> list:
        """K records on the device (768 bytes each) and their evaluationABC points to K verdicts"""
        ok = _pairing.groth16_verify(vk.alpha_g1_beta_g2, vk.gamma_prep, vk.delta_prep, recs, abc_points)
        return [bool(v) for v in ok.cpu().tolist()]

    @staticmethod
    def _rlc(vk: VerificationKey, primaries, proofs, seed, stage_ms=None, recs=None):
        """The randomized check over the well-formed proofs: (verdict, covered flags), verdict 1 / 0 / -1 as
        ozk_groth16_verify_rlc_dev returns it.  The proofs are `proofs`, or, with proofs None, the records `recs`
        already on the device (768 bytes each)."""
        k = len(proofs) if recs is None else recs.numel() // RECORD_BYTES
        if len(primaries) != k or not k:
            raise ValueError("one primary input per proof, at least one proof")
        rows = _pack_primaries(primaries, vk.num_inputs)
        rng = random.Random(seed) if seed is not None else secrets.SystemRandom()
        weights = b"".join((rng.randrange(1, 1 << 128)).to_bytes(32, "little") for _ in range(k))
        t0 = time.perf_counter()
        if recs is None:
            recs = dev_bytes(b"".join(proof_record(p) for p in proofs))
        d_inputs = dev_bytes(b"".join(rows))
        d_r = dev_bytes(weights)
        if stage_ms is not None:
            torch.cuda.synchronize()
            stage_ms["upload"] = (time.perf_counter() - t0) * 1e3
            times = []
        else:
            times = None
        verdict, covered = _pairing.groth16_verify_rlc(vk.alpha_g1_beta_g2, vk.gamma_prep, vk.delta_prep,
                                                       vk.gamma_abc_g1, recs, d_inputs, d_r, times)
        if stage_ms is not None:
            stage_ms.update(zip(("combination", "msms", "miller", "product", "final_exp"), times))
        return int(verdict.item()), [bool(c) for c in covered.cpu().tolist()]

    @staticmethod
    def verify_all(vk: VerificationKey, primaries, proofs, *, seed=None, stage_ms=None) -> bool:
        """True exactly when every proof passes (the Java's verify on each), for a batch of any size at the cost of
        about one pairing check: a random linear combination of the equations of the well-formed proofs, with
        weights r_i uniform in [1, 2^128), is checked once (ozk_groth16_verify_rlc_dev); the other proofs, or all of
        them if the check declines, go through verify_batch.  A wrong True has probability at most 1 / (2^128 - 1)
        over the weights.

        The weights come from `secrets` unless `seed` is given.  A seeded batch is reproducible, and therefore
        UNSOUND against anyone who knows the seed: they can build invalid proofs whose errors cancel in the
        combination.  Use a seed for tests only.  stage_ms: None, or a dict that receives the stage times in ms."""
        primaries, proofs = list(primaries), list(proofs)
        verdict, covered = Verifier._rlc(vk, primaries, proofs, seed, stage_ms)
        return Verifier._all_after_rlc(verdict, covered, lambda rest: Verifier.verify_batch(
            vk, [primaries[i] for i in rest], [proofs[i] for i in rest]))

    @staticmethod
    def _all_after_rlc(verdict, covered, judge) -> bool:
        """verify_all once the randomized check has spoken; judge(indices) gives the verdicts of verify_batch"""
        if verdict == 0:
            return False
        rest = [i for i in range(len(covered)) if verdict < 0 or not covered[i]]
        return not rest or all(judge(rest))

    @staticmethod
    def _each_after_rlc(verdict, covered, judge) -> list:
        """verify_batch_rlc once the randomized check has spoken"""
        if verdict != 1:
            return judge(list(range(len(covered))))
        out = [True] * len(covered)
        rest = [i for i in range(len(covered)) if not covered[i]]
        if rest:
            for i, v in zip(rest, judge(rest)):
                out[i] = v
        return out

    @staticmethod
    def verify_batch_rlc(vk: VerificationKey, primaries, proofs, *, seed=None) -> list:
        """The verdicts of verify_batch, found with the randomized check first: when it accepts, every well-formed
        proof gets True and only the others go through verify_batch; when it rejects or declines, the whole batch
        does.  Weights and `seed` as in verify_all (a seeded batch is unsound against anyone who knows the seed)."""
        primaries, proofs = list(primaries), list(proofs)
        verdict, covered = Verifier._rlc(vk, primaries, proofs, seed)
        return Verifier._each_after_rlc(verdict, covered, lambda rest: Verifier.verify_batch(
            vk, [primaries[i] for i in rest], [proofs[i] for i in rest]))

    # ---- the same three checks on compressed proofs: K x 128 bytes as bytes, a bytearray or a
    # uint8 CUDA tensor.  The buffer is uploaded once and decoded on the device straight into the record buffer of the
    # checks above; no Proof object is built.  A proof with a point that does not decode is False and stays out of the
    # pairing work; one that decodes gets the verdict the object path gives Proof.from_bytes of the same bytes (a
    # proof containing O decodes and is then treated as that path treats it).
    @staticmethod
    def _decode_records(buf, k, stage_ms=None):
        """(K x 768 record bytes on the device as a (K, 768) tensor, the K codes as a list)"""
        t0 = time.perf_counter()
        if not isinstance(buf, torch.Tensor):
            buf = dev_bytes(bytes(buf)) if len(buf) else torch.empty(0, dtype=torch.uint8)
        if buf.numel() != 128 * k or not k:
            raise ValueError("one 128-byte proof per primary input, at least one proof (%d bytes for %d)"
                             % (buf.numel(), k))
        if stage_ms is not None:
            torch.cuda.synchronize()
            stage_ms["upload_compressed"] = (time.perf_counter() - t0) * 1e3
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
        recs, codes = _codec.decompress_proofs(buf)
        if stage_ms is not None:
            ev[1].record()
            ev[1].synchronize()
            stage_ms["decompress"] = ev[0].elapsed_time(ev[1])
        return recs.view(k, RECORD_BYTES), codes.cpu().tolist()

    @staticmethod
    def _judge_records(vk, primaries, recs, abc="auto"):
        """judge(indices) for _all_after_rlc / _each_after_rlc over the rows of `recs`"""
        def judge(rest):
            rows = recs if len(rest) == recs.shape[0] else recs[torch.tensor(rest, device=recs.device)]
            prim = [primaries[i] for i in rest]
            return Verifier._records_verdicts(vk, rows.reshape(-1), Verifier._evaluation_abc(vk, prim, abc))
        return judge

    @staticmethod
    def _decodable(primaries, recs, codes):
        """the decodable proofs of a batch: (their positions, their primary inputs, their records)"""
        good = [i for i, c in enumerate(codes) if c == 0]
        if len(good) == len(codes):
            return good, primaries, recs
        return good, [primaries[i] for i in good], recs[torch.tensor(good, dtype=torch.long, device=recs.device)]

    @staticmethod
    def verify_batch_bytes(vk: VerificationKey, primaries, buf, abc="auto") -> list:
        """verify_batch on K compressed proofs"""
        primaries = list(primaries)
        recs, codes = Verifier._decode_records(buf, len(primaries))
        good, primaries, recs = Verifier._decodable(primaries, recs, codes)
        out = [False] * len(codes)
        if good:
            for i, v in zip(good, Verifier._judge_records(vk, primaries, recs, abc)(list(range(len(good))))):
                out[i] = v
        return out

    @staticmethod
    def verify_all_bytes(vk: VerificationKey, primaries, buf, *, seed=None, stage_ms=None) -> bool:
        """verify_all on K compressed proofs: False as soon as any proof does not decode.  stage_ms also receives
        "upload_compressed" and "decompress" (the device time of the decoding launch)."""
        primaries = list(primaries)
        recs, codes = Verifier._decode_records(buf, len(primaries), stage_ms)
        if any(codes):
            return False
        verdict, covered = Verifier._rlc(vk, primaries, None, seed, stage_ms, recs=recs.reshape(-1))
        return Verifier._all_after_rlc(verdict, covered, Verifier._judge_records(vk, primaries, recs))

    @staticmethod
    def verify_batch_rlc_bytes(vk: VerificationKey, primaries, buf, *, seed=None) -> list:
        """verify_batch_rlc on K compressed proofs"""
        primaries = list(primaries)
        recs, codes = Verifier._decode_records(buf, len(primaries))
        good, primaries, recs = Verifier._decodable(primaries, recs, codes)
        out = [False] * len(codes)
        if good:
            verdict, covered = Verifier._rlc(vk, primaries, None, seed, recs=recs.reshape(-1))
            for i, v in zip(good, Verifier._each_after_rlc(verdict, covered,
                                                            Verifier._judge_records(vk, primaries, recs))):
                out[i] = v
        return out

