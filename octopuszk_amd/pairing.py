"""The BN254a optimal-ate pairing on the GPU (BNPairing.java reducedPairing), batched: one pairing per lane, through
the C ABI of libozk_hip.so (include/ozk.h).  There is no CPU pairing path.

Points are device tensors of uint8 in the natives' wire-in format (G1 n x 96 B, G2 n x 192 B, any Z; infinity is
Z = 0 and is normalised to (0, 1, 0) as toAffineCoordinates does).  GT values are n x 384 B: twelve 32-byte
little-endian canonical Fq values in the order c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1.
"""
import torch

from . import lib as _lib

G1_BYTES, G2_BYTES, GT_BYTES = 96, 192, 384


def _ptr(t):
    return int(t.data_ptr())


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _count(t, rec, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8):
        raise TypeError("%s must be a uint8 CUDA tensor" % what)
    if t.numel() == 0 or t.numel() % rec:
        raise ValueError("%s: %d bytes are not a whole number of %d-byte records" % (what, t.numel(), rec))
    return t.numel() // rec


class PreparedG2:
    """The line coefficients of n G2 points (precomputeG2, BNPairing.java:284-325): computed once per fixed Q."""

    def __init__(self, q_batch):
        L = _lib.load()
        q_batch = q_batch.contiguous()
        self.n = _count(q_batch, G2_BYTES, "Q")
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
    n = _count(p_batch, G1_BYTES, "P")
    if isinstance(q_batch, PreparedG2):
        prepared, q = 1, q_batch.data
        nq = q_batch.n
    else:
        prepared, q = 0, q_batch.contiguous()
        nq = _count(q, G2_BYTES, "Q")
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
    k = _count(d_proofs, 768, "proofs")
    if _count(d_abc, 192, "evaluationABC") != k:
        raise ValueError("one evaluationABC point per proof")
    if gamma_prep.n != 1 or delta_prep.n != 1 or alpha_beta.numel() != GT_BYTES:
        raise ValueError("one prepared gamma, one prepared delta and one GT value")
    ok = torch.empty(k, dtype=torch.int32, device=d_proofs.device)
    _lib.check(L.ozk_groth16_verify_dev(_ptr(alpha_beta), _ptr(gamma_prep.data), _ptr(delta_prep.data),
                                        _ptr(d_proofs), _ptr(d_abc), k, _ptr(ok), _stream()))
    return ok
