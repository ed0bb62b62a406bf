"""Phase-2 contributions to a Groth16 key: scale delta by a secret d on the GPU, prove knowledge
of d, and verify that somebody else's contribution was honest.

    pk2, vk2, receipt = contribute(pk, vk)                     # d drawn here and forgotten on return
    verify_contribution(pk, pk2, receipt, vk_before=vk, vk_after=vk2)

A contribution replaces delta_g1, delta_g2 by d times themselves and delta_abc_g1, query_h by 1 / d times themselves
(ozk_points_scale_dev: n points times one scalar); everything else is shared with the key before.  After it, delta is
known to nobody who does not know BOTH the delta before and d.  It removes knowledge of delta only: alpha, beta, gamma
and t of serial_setup_generate stay known to whoever ran it, and there is no phase 1 here.

The receipt (296 bytes) chains to the one before through h = SHA-256(previous receipt) and carries a Schnorr proof of
knowledge of d over the base delta_g1-before.  There is no CPU path.
"""
import hashlib
import secrets
import time

import numpy as np
import torch

from . import codec as _codec
from . import transcript as _transcript
from . import vectors as _vectors
from . import wire as _wire
from .fft import FR
from .vectors import scale_points
from .zksnark import ProvingKey, VerificationKey

G1, G2 = 1, 2
MAGIC = b"OZKC2\x00\x00\x01"
RECEIPT_BYTES = 296
CHECKS = ("receipt_deltas", "unchanged", "delta_wellformed", "delta_ratio", "vectors", "pok", "vk")
_UNCHANGED_G1 = ("alpha_g1", "beta_g1", "query_a", "query_b_g1")
_UNCHANGED_G2 = ("beta_g2", "query_b_g2")
_SHARED = _UNCHANGED_G1 + _UNCHANGED_G2 + ("r1cs",)
_POK_TAG = b"OZK-phase2-pok"
_RHO_TAG = b"OZK-phase2-rho"


def _enc(points, type_) -> bytes:
    return _wire.host_bytes((_codec.compress_g1 if type_ == G1 else _codec.compress_g2)(points))


def _challenge(body: bytes, r_enc: bytes) -> int:
    """the 128-bit Schnorr challenge of a receipt, never zero (srs.py: the same under the phase-1 tag)"""
    return _transcript.challenge128(_POK_TAG, body, r_enc)


# ---------------------------------------------------------------------------- receipt
def _pok_holds(base, moved, r_enc: bytes, z: int, c: int):
    """z base - c moved - R = O as one 3-point MSM (base, moved: one wire-in G1 point each; R compressed): (a device
    flag to read after a synchronise as _pok_read, the workspace to keep until then)"""
    r_point, code = _codec.decompress_g1(_wire.dev_bytes(r_enc))
    pok, ws = _vectors.msm(torch.cat([base.reshape(-1), moved.reshape(-1), r_point]),
                           _wire.dev_bytes(_wire.le32((z, FR - c, FR - 1))), 3)
    return (pok, code), ws


def _pok_read(flag) -> bool:
    pok, code = flag
    return _wire.is_inf_out(pok) and not int(code.item())


class Receipt:
    """What a contributor publishes next to the new key: the transcript digest h, delta before and after in both
    groups, and the proof of knowledge (R, z) of the factor between them."""
    _FIELDS = (("delta_g1_before", G1), ("delta_g1_after", G1), ("delta_g2_before", G2), ("delta_g2_after", G2),
               ("r", G1))

    def __init__(self, h, delta_g1_before, delta_g1_after, delta_g2_before, delta_g2_after, r, z):
        """h: 32 bytes; the points compressed (32 / 64 bytes each); z: int"""
        self.h, self.z = bytes(h), int(z)
        self.delta_g1_before, self.delta_g1_after = bytes(delta_g1_before), bytes(delta_g1_after)
        self.delta_g2_before, self.delta_g2_after = bytes(delta_g2_before), bytes(delta_g2_after)
        self.r = bytes(r)

    def to_bytes(self) -> bytes:
        b = (MAGIC + self.h + self.delta_g1_before + self.delta_g1_after + self.delta_g2_before + self.delta_g2_after
             + self.r + self.z.to_bytes(32, "little"))
        if len(b) != RECEIPT_BYTES:
            raise ValueError("receipt: a field has the wrong length")
        return b

    @staticmethod
    def from_bytes(b) -> "Receipt":
        """Strict: ValueError naming the field for a wrong length, a wrong magic, z >= r or a point that does not
        decode (decoded on the device)."""
        b = _codec.receipt_head(b, MAGIC, RECEIPT_BYTES)
        z = int.from_bytes(b[264:], "little")
        if z >= FR:
            raise ValueError("receipt: z is not below r")
        rec = Receipt(b[8:40], b[40:72], b[72:104], b[104:168], b[168:232], b[232:264], z)
        _codec.require_points(((name, getattr(rec, name), type_) for name, type_ in Receipt._FIELDS), "receipt")
        return rec

    def body(self) -> bytes:
        """bytes 8 .. 232 of the receipt: what the challenge binds besides R"""
        return self.h + self.delta_g1_before + self.delta_g1_after + self.delta_g2_before + self.delta_g2_after


# ---------------------------------------------------------------------------- contribute
def contribute(pk, vk=None, d=None, *, nonce=None, previous=b""):
    """(pk2, vk2, receipt): the key after a contribution of the secret d in [1, r) (drawn from `secrets` when None).
    delta_g1, delta_g2 become d times themselves, delta_abc_g1 and query_h 1 / d times themselves, each with one
    scale_points call over the whole array; every other field of pk2 is the same tensor object as in pk.  vk2 is vk
    with the new delta_g2 (None for vk None).  `previous`: the bytes of the receipt before this one, empty for the
    first.  `nonce`: the u of the proof of knowledge, in [1, r); give one for reproducible receipts in tests only."""
    d = secrets.randbelow(FR - 1) + 1 if d is None else _wire.scalar_in_range(d, "d", 1)
    u = secrets.randbelow(FR - 1) + 1 if nonce is None else _wire.scalar_in_range(nonce, "nonce", 1)
    inv_d = pow(d, -1, FR)
    pk2 = ProvingKey()
    for name in _SHARED:
        setattr(pk2, name, getattr(pk, name))
    pk2.delta_g1 = scale_points(pk.delta_g1, d, G1)
    pk2.delta_g2 = scale_points(pk.delta_g2, d, G2)
    pk2.delta_abc_g1 = scale_points(pk.delta_abc_g1, inv_d, G1)
    pk2.query_h = scale_points(pk.query_h, inv_d, G1)
    r_point = scale_points(pk.delta_g1, u, G1)
    g1 = _enc(torch.cat([pk.delta_g1.reshape(-1), pk2.delta_g1, r_point]), G1)
    g2 = _enc(torch.cat([pk.delta_g2.reshape(-1), pk2.delta_g2]), G2)
    rec = Receipt(hashlib.sha256(bytes(previous)).digest(), g1[:32], g1[32:64], g2[:64], g2[64:], g1[64:], 0)
    rec.z = (u + _challenge(rec.body(), rec.r) * d) % FR
    vk2 = None
    if vk is not None:
        vk2 = VerificationKey(vk.alpha_g1_beta_g2, vk.gamma_g2, pk2.delta_g2, vk.gamma_abc_g1)
    return pk2, vk2, rec


# ---------------------------------------------------------------------------- verify
def _r1cs_equal(a, b) -> bool:
    if (a.num_inputs, a.num_auxiliary) != (b.num_inputs, b.num_auxiliary):
        return False
    for x, y in ((a.A, b.A), (a.B, b.B), (a.C, b.C)):
        if not (np.array_equal(x.ptr, y.ptr) and np.array_equal(x.index, y.index)):
            return False
        if (x.value is None) != (y.value is None):
            return False
        if x.value is not None and [int(v) for v in x.value] != [int(v) for v in y.value]:
            return False
    return True


def verify_contribution(pk_before, pk_after, receipt, *, vk_before=None, vk_after=None, seed=None, why=None,
                        stage_ms=None) -> bool:
    """True exactly when pk_after is pk_before after one honest contribution that `receipt` (a Receipt or its bytes)
    describes.  The checks run in the order of CHECKS and the first that fails ends the call with False; `why` (a list)
    then receives its name.

      receipt_deltas    the four deltas of the receipt are the compressed deltas of the two keys
      unchanged         alpha_g1, beta_g1, beta_g2, query_a, query_b_g1, query_b_g2 equal as compressed encodings, the
                        R1CS equal, delta_abc_g1 and query_h of equal lengths
      delta_wellformed  the new deltas finite, the new delta_g2 in the order-r subgroup ([r - 1] P = -P)
      delta_ratio       e(delta_g1', delta_g2) = e(delta_g1, delta_g2'): both groups moved by one factor
      vectors           with 128-bit weights rho_i over delta_abc_g1 ++ query_h, S = sum rho_i old_i and S' = sum rho_i
                        new_i: e(S', delta_g2') = e(S, delta_g2); S or S' at infinity fails
      pok               z delta_g1 - c delta_g1' - R = O, one 3-point MSM
      vk                (both given) vk_before has pk_before's delta_g2 and vk_after is vk_before with pk_after's

    The weights come from a SHA-256 counter stream over `seed` (bytes or an int); None draws 32 bytes from the
    system.  A seeded check is reproducible and so unsound against anyone who knows the seed: tests only.
    stage_ms: None, or a dict that receives the times of the stages compare, scale, msms, pairings in ms (the call
    then synchronises between them)."""
    T = {"compare": 0.0, "scale": 0.0, "msms": 0.0, "pairings": 0.0}
    t0 = [time.perf_counter()]

    def lap(stage):
        if stage_ms is not None:
            torch.cuda.synchronize()
            now = time.perf_counter()
            T[stage] += (now - t0[0]) * 1e3
            t0[0] = now

    def no(name, stage="compare"):
        lap(stage)
        if why is not None:
            why.append(name)
        if stage_ms is not None:
            stage_ms.update(T)
        return False

    rec = receipt if isinstance(receipt, Receipt) else Receipt.from_bytes(receipt)
    # 1 receipt_deltas
    d1 = _enc(torch.cat([pk_before.delta_g1.reshape(-1), pk_after.delta_g1.reshape(-1)]), G1)
    d2 = _enc(torch.cat([pk_before.delta_g2.reshape(-1), pk_after.delta_g2.reshape(-1)]), G2)
    if (rec.delta_g1_before, rec.delta_g1_after, rec.delta_g2_before, rec.delta_g2_after) != \
            (d1[:32], d1[32:], d2[:64], d2[64:]):
        return no("receipt_deltas")
    # 2 unchanged
    for name in _UNCHANGED_G1 + _UNCHANGED_G2:
        a, b = getattr(pk_before, name), getattr(pk_after, name)
        if a is b:
            continue
        compress = _codec.compress_g1 if name in _UNCHANGED_G1 else _codec.compress_g2
        if a.numel() != b.numel() or not torch.equal(compress(a), compress(b)):
            return no("unchanged")
    if pk_before.r1cs is not pk_after.r1cs and not _r1cs_equal(pk_before.r1cs, pk_after.r1cs):
        return no("unchanged")
    n_abc, n_h = pk_before.delta_abc_g1.numel() // 96, pk_before.query_h.numel() // 96
    if pk_after.delta_abc_g1.numel() != 96 * n_abc or pk_after.query_h.numel() != 96 * n_h:
        return no("unchanged")
    lap("compare")
    # 3 delta_wellformed
    if d1[63] & 0x40 or d2[127] & 0x40:
        return no("delta_wellformed")
    minus = _enc(scale_points(pk_after.delta_g2, FR - 1, G2), G2)
    if minus != d2[64:127] + bytes([d2[127] ^ 0x80]):      # the same x, the other y (no twist point has y = 0)
        return no("delta_wellformed", "scale")
    neg_d1 = scale_points(pk_before.delta_g1, FR - 1, G1)
    lap("scale")
    # 4 delta_ratio
    if not _vectors.pairs_are_one(torch.cat([pk_after.delta_g1.reshape(-1), neg_d1]),
                                  torch.cat([pk_before.delta_g2.reshape(-1), pk_after.delta_g2.reshape(-1)])):
        return no("delta_ratio", "pairings")
    lap("pairings")
    # 5 vectors
    n = n_abc + n_h
    rho = _transcript.weights(_transcript.seed_bytes(seed), n, _RHO_TAG)
    lap("compare")
    s_old, ws1 = _vectors.msm(torch.cat([pk_before.delta_abc_g1.reshape(-1), pk_before.query_h.reshape(-1)]),
                              _wire.dev_bytes(rho), n)
    s_new, ws2 = _vectors.msm(torch.cat([pk_after.delta_abc_g1.reshape(-1), pk_after.query_h.reshape(-1)]),
                              _wire.dev_bytes(rho), n)
    # 6 pok (its MSM with the two above)
    pok, ws3 = _pok_holds(pk_before.delta_g1, pk_after.delta_g1, rec.r, rec.z, _challenge(rec.body(), rec.r))
    inf_old, inf_new, pok_ok = _wire.is_inf_out(s_old), _wire.is_inf_out(s_new), _pok_read(pok)
    lap("msms")
    if inf_old or inf_new:
        return no("vectors")
    neg_s = scale_points(_wire.wire_out_to_in(s_old, G1), FR - 1, G1)
    lap("scale")
    if not _vectors.pairs_are_one(torch.cat([_wire.wire_out_to_in(s_new, G1), neg_s]),
                                  torch.cat([pk_after.delta_g2.reshape(-1), pk_before.delta_g2.reshape(-1)])):
        return no("vectors", "pairings")
    lap("pairings")
    if not pok_ok:
        return no("pok")
    # 7 vk
    if vk_before is not None and vk_after is not None:
        want = VerificationKey(vk_before.alpha_g1_beta_g2, vk_before.gamma_g2, pk_after.delta_g2, vk_before.gamma_abc_g1)
        vb = vk_before.to_bytes()
        if vb[528 - 64:528] != d2[:64] or vk_after.to_bytes() != want.to_bytes():
            return no("vk")
    lap("compare")
    if stage_ms is not None:
        stage_ms.update(T)
    del ws1, ws2, ws3
    return True


def verify_chain(keys, receipts, *, vks=None, seed=None, why=None) -> bool:
    """keys[0] .. keys[k] and the k receipts between them: every step passes verify_contribution, the first receipt's
    h is the SHA-256 of the empty string and every later one's that of the receipt before it (`why` receives
    "chain" for a broken link, else the failed check of the step).  vks: None, or the k + 1 verification keys."""
    keys = list(keys)
    raw = [r.to_bytes() if isinstance(r, Receipt) else bytes(r) for r in receipts]
    if len(keys) != len(raw) + 1 or not raw or (vks is not None and len(vks) != len(keys)):
        raise ValueError("k receipts go with k + 1 keys, k >= 1")
    previous = b""
    for i, b in enumerate(raw):
        rec = Receipt.from_bytes(b)
        if rec.h != hashlib.sha256(previous).digest():
            if why is not None:
                why.append("chain")
            return False
        if not verify_contribution(keys[i], keys[i + 1], rec, seed=seed, why=why,
                                   vk_before=None if vks is None else vks[i],
                                   vk_after=None if vks is None else vks[i + 1]):
            return False
        previous = b
    return True
