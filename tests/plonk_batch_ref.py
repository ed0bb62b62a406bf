"""Exact-integer model of the batched PLONK verifier, on top of tests/plonk_ref.py,
tests/plonk_lookup_ref.py and tests/kzg_multi_ref.py: the challenge record of one proof, the four per-proof flags, the
folded list of scalars in the order of the MSM's points, and the combined equation in the exponent, where every point
is known by its logarithm (known tau).  Written from the statement of the check, not from csrc/plonk_verify.cuh or
octopuszk_amd/plonk, which the tests compare with it."""
import hashlib

import kzg_multi_ref as km
import kzg_ref as kr
import plonk_lookup_ref as lm
import plonk_ref as pm

R = pm.R
RHO_TAG = b"OZK-plonk-rho"
VALUE, PUBLIC, DOMAIN, IDENTITY = 1, 2, 4, 8          # the bits of a proof's flags
# kind 0: a vanilla proof, kind 1: a proof with lookups.  order: the proof's commitments in the row order of the
# MultiOpening that the verifier builds (a b c t_lo t_mid t_hi Z; a b c m t_lo t_mid t_hi Z S)
SHAPES = {0: {"proof": 800, "vk": 264, "nc": 7, "nv": 16, "nkey": 8, "rec": 8, "order": (0, 1, 2, 4, 5, 6, 3), "model": pm},
          1: {"proof": 1088, "vk": 392, "nc": 9, "nv": 23, "nkey": 12, "rec": 12, "order": (0, 1, 2, 3, 6, 7, 8, 4, 5),
              "model": lm}}


def weights(seed: bytes, k: int):
    """rho_0 .. rho_{k-1}: half m % 2 of SHA-256(tag | seed | m // 2 as 8 bytes LE), 1 if its 16 bytes are zero"""
    out = []
    for m in range(k):
        block = hashlib.sha256(RHO_TAG + seed + (m // 2).to_bytes(8, "little")).digest()
        out.append(int.from_bytes(block[16 * (m % 2):16 * (m % 2) + 16], "little") or 1)
    return out


def parse(kind, proof: bytes):
    """(commitments, values, W, W') of a proof of the right size, whatever its values"""
    nc, nv = SHAPES[kind]["nc"], SHAPES[kind]["nv"]
    assert len(proof) == SHAPES[kind]["proof"]
    return ([proof[32 * i:32 * i + 32] for i in range(nc)], kr.ints(proof[32 * nc:32 * (nc + nv)]),
            proof[32 * (nc + nv):32 * (nc + nv + 1)], proof[32 * (nc + nv + 1):])


def statement(kind, vk: bytes, public, proof: bytes):
    """(n, the transcript's challenges, the multi-opening's commitments, sets and rows) of one proof"""
    return SHAPES[kind]["model"]._statement(vk, list(public), parse(kind, proof))


def flags_of(kind, vk: bytes, public, proof: bytes, z=None):
    """the four bits; z: the evaluation challenge when it is not the transcript's (a planted one).  The identity is
    evaluated only when the other three bits are clear."""
    _, values, _, _ = parse(kind, proof)
    n, ch, _, _, _ = statement(kind, vk, public, proof)
    z = ch[-1] if z is None else z
    flags = (VALUE if any(v >= R for v in values) else 0) | (PUBLIC if any(x >= R for x in public) else 0)
    flags |= DOMAIN if pow(z, n, R) == 1 else 0
    if not flags and not SHAPES[kind]["model"].identity_holds(n, public, values, *ch[:-1], z):
        flags |= IDENTITY
    return flags


def record(kind, vk: bytes, public, proof: bytes, rho: int):
    """the challenge record of one proof: the transcript's challenges, the multi-opening's two, rho, zero padding"""
    _, ch, commitments, sets, rows = statement(kind, vk, public, proof)
    g, u = km.challenges(commitments, sets, rows, parse(kind, proof)[2])
    out = list(ch) + [g, u, rho]
    return out + [0] * (SHAPES[kind]["rec"] - len(out))


def terms(kind, vk: bytes, public, proof: bytes):
    """(the weights of the proof's own commitments in row order, those of the key's, the scalars of g1, W and W') of
    an unflagged proof"""
    nc, nkey = SHAPES[kind]["nc"], SHAPES[kind]["nkey"]
    _, _, commitments, sets, rows = statement(kind, vk, public, proof)
    g, u = km.challenges(commitments, sets, rows, parse(kind, proof)[2])
    w, total, z_t = km.at_z(sets, rows, g, u)
    own_single = nc - len([s for s in sets if len(s) == 2])       # the proof's rows at {z} come first, then the key's
    own = w[:own_single] + w[own_single + nkey:]
    return own, w[own_single:own_single + nkey], (-total) % R, (-z_t) % R, u


def folded(kind, vk: bytes, publics, proofs, rho, planted=None):
    """(the scalars in the order of the points: per proof its commitments in row order, then K of W, K of W', the key's
    sums, g1's sum; the K weights, zero for a flagged proof; the K flags).  planted: {m: z} for proofs whose evaluation
    challenge is given."""
    nc, nkey = SHAPES[kind]["nc"], SHAPES[kind]["nkey"]
    own, s_w, s_w2, key, g1, rho_out, flags = [], [], [], [0] * nkey, 0, [], []
    for m, (public, proof, r) in enumerate(zip(publics, proofs, rho)):
        f = flags_of(kind, vk, public, proof, (planted or {}).get(m))
        flags.append(f)
        if f:
            own += [0] * nc
            s_w.append(0)
            s_w2.append(0)
            rho_out.append(0)
            continue
        mine, keys, t_g1, t_w, u = terms(kind, vk, public, proof)
        own += [r * x % R for x in mine]
        s_w.append(r * t_w % R)
        s_w2.append(r * u % R)
        key = [(a + r * x) % R for a, x in zip(key, keys)]
        g1 = (g1 + r * t_g1) % R
        rho_out.append(r)
    return own + s_w + s_w2 + key + [g1], rho_out, flags


def point_logs(kind, proof_logs, key_logs):
    """the logarithms of the MSM's points from those of K proofs (each in the order of its bytes: its commitments, W,
    W') and of the key's commitments; g1 is 1"""
    nc, order = SHAPES[kind]["nc"], SHAPES[kind]["order"]
    own = [logs[i] for logs in proof_logs for i in order]
    return own + [logs[nc] for logs in proof_logs] + [logs[nc + 1] for logs in proof_logs] + list(key_logs) + [1]


def equation_holds(kind, scalars, rho_out, proof_logs, key_logs, tau) -> bool:
    """e(sum s_i P_i, g2) e(-sum rho_m W'_m, tau g2) = 1 in the exponent"""
    nc = SHAPES[kind]["nc"]
    lhs = sum(s * p for s, p in zip(scalars, point_logs(kind, proof_logs, key_logs))) % R
    return (lhs - tau * sum(r * logs[nc + 1] for r, logs in zip(rho_out, proof_logs))) % R == 0


def verify_all(kind, vk: bytes, publics, proofs, seed: bytes, proof_logs, key_logs, tau) -> bool:
    scalars, rho_out, flags = folded(kind, vk, publics, proofs, weights(seed, len(proofs)))
    return not any(flags) and equation_holds(kind, scalars, rho_out, proof_logs, key_logs, tau)
