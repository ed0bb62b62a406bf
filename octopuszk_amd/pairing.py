"""The BN254a optimal-ate pairing on the GPU (BNPairing.java reducedPairing), batched: one pairing per lane, through
the C ABI of libozk_hip.so (include/ozk.h).  There is no CPU pairing path.

Points are device tensors of uint8 in the natives' wire-in format (G1 n x 96 B, G2 n x 192 B, any Z; infinity is
Z = 0 and is normalised to (0, 1, 0) as toAffineCoordinates does).  GT values are n x 384 B: twelve 32-byte
little-endian canonical Fq values in the order c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1.
"""
import ctypes

import torch

from . import lib as _lib
from . import wire as _wire
from .device import _ptr, _stream

G1_BYTES, G2_BYTES, GT_BYTES = 96, 192, 384


class PreparedG2:
    """The line coefficients of n G2 points (precomputeG2, BNPairing.java:284-325): computed once per fixed Q."""

    def __init__(self, q_batch):
        L = _lib.load()
        q_batch = q_batch.contiguous()
        self.n = _wire.count(q_batch, G2_BYTES, "Q")
        self.bytes = int(L.ozk_pairing_g2_prepared_bytes(self.n))
        self.data = torch.empty(self.bytes, dtype=torch.uint8, device=q_batch.device)
        _lib.check(L.ozk_pairing_g2_prepare_dev(_ptr(q_batch), self.n, _ptr(self.data), self.bytes, _stream()))
        self._q = q_batch   # alive until the stream has run the preparation


def prepare_g2(q_batch) -> PreparedG2:
    return PreparedG2(q_batch)


def reduced_pairing(p_batch, q_batch) -> torch.Tensor:
    """e(P_i, Q_i) for every i; q_batch is n wire-in G2 points or a PreparedG2 of n points.  Asynchronous on the
    current stream; returns the n x 384-byte GT tensor."""
    L = _lib.load()
    p_batch = p_batch.contiguous()
    n = _wire.count(p_batch, G1_BYTES, "P")
    if isinstance(q_batch, PreparedG2):
        prepared, q = 1, q_batch.data
        nq = q_batch.n
    else:
        prepared, q = 0, q_batch.contiguous()
        nq = _wire.count(q, G2_BYTES, "Q")
    if nq != n:
        raise ValueError("%d G1 points against %d G2 points" % (n, nq))
    out = torch.empty(n * GT_BYTES, dtype=torch.uint8, device=p_batch.device)
    _lib.check(L.ozk_reduced_pairing_dev(_ptr(p_batch), _ptr(q), prepared, n, _ptr(out), _stream()))
    return out


def groth16_verify(alpha_beta, gamma_prep: PreparedG2, delta_prep: PreparedG2, d_proofs, d_abc) -> torch.Tensor:
    """k verdicts (int32, 1 = accepted) of Verifier.verify: d_proofs k x 768-byte records A | B | C and d_abc
    k x 192-byte evaluationABC points, both in wire-out format; alpha_beta one GT value (384 B)."""
    L = _lib.load()
    d_proofs, d_abc = d_proofs.contiguous(), d_abc.contiguous()
    k = _wire.count(d_proofs, 768, "proofs")
    if _wire.count(d_abc, 192, "evaluationABC") != k:
        raise ValueError("one evaluationABC point per proof")
    if gamma_prep.n != 1 or delta_prep.n != 1 or alpha_beta.numel() != GT_BYTES:
        raise ValueError("one prepared gamma, one prepared delta and one GT value")
    ok = torch.empty(k, dtype=torch.int32, device=d_proofs.device)
    _lib.check(L.ozk_groth16_verify_dev(_ptr(alpha_beta), _ptr(gamma_prep.data), _ptr(delta_prep.data),
                                        _ptr(d_proofs), _ptr(d_abc), k, _ptr(ok), _stream()))
    return ok


def pairing_product(p_batch, q_batch) -> torch.Tensor:
    """prod_i e(P_i, Q_i) as one GT value (384 B): the n Miller values multiplied, then one final exponentiation.
    Inputs as for reduced_pairing.  Asynchronous on the current stream."""
    L = _lib.load()
    p_batch = p_batch.contiguous()
    n = _wire.count(p_batch, G1_BYTES, "P")
    if isinstance(q_batch, PreparedG2):
        prepared, q = 1, q_batch.data
        nq = q_batch.n
    else:
        prepared, q = 0, q_batch.contiguous()
        nq = _wire.count(q, G2_BYTES, "Q")
    if nq != n:
        raise ValueError("%d G1 points against %d G2 points" % (n, nq))
    out = torch.empty(GT_BYTES, dtype=torch.uint8, device=p_batch.device)
    _lib.check(L.ozk_pairing_product_dev(_ptr(p_batch), _ptr(q), prepared, n, _ptr(out), _stream()))
    return out


def gt_pow(gt_batch, exponents) -> torch.Tensor:
    """gt_i^e_i for n GT values (n x 384 B, results of reduced pairings) and n integers 0 <= e_i < 2^256, given as a
    list of ints or an n x 32-byte little-endian uint8 CUDA tensor.  Asynchronous on the current stream."""
    L = _lib.load()
    gt_batch = gt_batch.contiguous()
    n = _wire.count(gt_batch, GT_BYTES, "GT")
    if not isinstance(exponents, torch.Tensor):
        exponents = list(exponents)
        if any(not 0 <= int(e) < 1 << 256 for e in exponents):
            raise ValueError("exponents must lie in [0, 2^256)")
        raw = b"".join(int(e).to_bytes(32, "little") for e in exponents)
        exponents = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(gt_batch.device) if raw else \
            torch.empty(0, dtype=torch.uint8, device=gt_batch.device)
    exponents = exponents.contiguous()
    if _wire.count(exponents, 32, "exponents") != n:
        raise ValueError("one exponent per GT value")
    out = torch.empty_like(gt_batch)
    _lib.check(L.ozk_gt_pow_dev(_ptr(gt_batch), _ptr(exponents), n, _ptr(out), _stream()))
    return out


def wellformed(d_proofs) -> torch.Tensor:
    """k flags (int32, 1 = well-formed) of k 768-byte proof records A | B | C (wire-out): every coordinate canonical,
    A and C on the curve, B on the twist and in the order-r subgroup, no point at infinity.  Asynchronous."""
    L = _lib.load()
    d_proofs = d_proofs.contiguous()
    k = _wire.count(d_proofs, 768, "proofs")
    flags = torch.empty(k, dtype=torch.int32, device=d_proofs.device)
    _lib.check(L.ozk_groth16_wellformed_dev(_ptr(d_proofs), k, _ptr(flags), _stream()))
    return flags


def groth16_verify_rlc(alpha_beta, gamma_prep: PreparedG2, delta_prep: PreparedG2, gamma_abc, d_proofs, d_inputs,
                       d_r, stage_ms=None):
    """The randomized batch check of ozk_groth16_verify_rlc_dev over k records, k x n primary inputs and k weights
    (32-byte little-endian each).  Returns (verdict, covered): an int32 tensor of one value (1 accepted, 0 rejected,
    -1 declined) and k int32 flags (1 = the proof entered the check).  stage_ms: None, or a list that receives the
    five stage times in ms (the call then waits for the stream)."""
    L = _lib.load()
    d_proofs, d_inputs, d_r = d_proofs.contiguous(), d_inputs.contiguous(), d_r.contiguous()
    k = _wire.count(d_proofs, 768, "proofs")
    n = _wire.count(gamma_abc, G1_BYTES, "gammaABC")
    if _wire.count(d_inputs, 32 * n, "inputs") != k or _wire.count(d_r, 32, "weights") != k:
        raise ValueError("one row of %d inputs and one weight per proof" % n)
    if gamma_prep.n != 1 or delta_prep.n != 1 or alpha_beta.numel() != GT_BYTES:
        raise ValueError("one prepared gamma, one prepared delta and one GT value")
    covered = torch.empty(k, dtype=torch.int32, device=d_proofs.device)
    verdict = torch.empty(1, dtype=torch.int32, device=d_proofs.device)
    times = (ctypes.c_float * 5)() if stage_ms is not None else None
    _lib.check(L.ozk_groth16_verify_rlc_dev(_ptr(alpha_beta), _ptr(gamma_prep.data), _ptr(delta_prep.data),
                                            _ptr(gamma_abc), n, _ptr(d_proofs), _ptr(d_inputs), _ptr(d_r), k,
                                            _ptr(covered), _ptr(verdict), times, _stream()))
    if stage_ms is not None:
        stage_ms[:] = [float(t) for t in times]
    return verdict, covered
