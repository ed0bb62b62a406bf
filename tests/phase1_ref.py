"""Exact-integer model of a phase-1 contribution to a powers-of-tau string over oracle.bn254:
the contribution in the exponent, the receipt and its bytes, the challenge, every check of srs.verify_contribution with
the group elements replaced by their discrete logarithms, and the OZKSRS file layout.  Written from the protocol's
description, not from octopuszk_amd/srs.py, which the tests compare with it.

A string in the exponent: {m, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1: lists of logarithms to the generator of
their group; beta_g2: one logarithm; gen_g1, gen_g2: the generators as points, for the bytes}."""
import hashlib

import ceremony_ref as cref
import codec_ref as ref
from oracle import bn254 as o

Q, R = o.Q, o.R
MAGIC = b"OZKC1\x00\x00\x01"
RECEIPT_BYTES = 432
FILE_MAGIC = b"OZKSRS\x00\x01"
CHECKS = ("receipt_points", "generators", "pok", "wellformed")
SECRETS = ("tau", "alpha", "beta")
ARRAYS = ("tau_g1", "alpha_tau_g1", "beta_tau_g1", "tau_g2")          # file order, beta_g2 last
LAMBDA = cref.LAMBDA


def scalars():
    """the scalars of DESIGN.md section 15's list and ten seeded random ones"""
    import random
    rng = random.Random(21)
    fixed = [0, 1, 2, 3, LAMBDA, LAMBDA + 1, LAMBDA - 1, R - LAMBDA, (1 << 127) + 1, (1 << 127) - 1, 1 << 128, R - 1, R - 2]
    return fixed + [rng.randrange(R) for _ in range(10)]


# ---------------------------------------------------------------------------- strings in the exponent
def counts(m):
    return {"tau_g1": 2 * m + 1, "alpha_tau_g1": m, "beta_tau_g1": m, "tau_g2": m}


def from_secrets_exp(m, tau, alpha, beta, gen_g1=o.G1.one, gen_g2=o.G2.one):
    return {"m": m, "tau_g1": [pow(tau, i, R) for i in range(2 * m + 1)], "tau_g2": [pow(tau, i, R) for i in range(m)],
            "alpha_tau_g1": [alpha * pow(tau, i, R) % R for i in range(m)],
            "beta_tau_g1": [beta * pow(tau, i, R) % R for i in range(m)], "beta_g2": beta % R,
            "gen_g1": gen_g1, "gen_g2": gen_g2}


def initial_exp(m, **gens):
    return from_secrets_exp(m, 1, 1, 1, **gens)


def pok_bases(s):
    return [s["tau_g1"][1], s["alpha_tau_g1"][0], s["beta_tau_g1"][0]]


def wellformed(s) -> bool:
    """some tau, alpha, beta stand behind all of the string (what Srs.check decides with pairings)"""
    m = s["m"]
    if m < 2 or m & (m - 1) or any(len(s[name]) != n for name, n in counts(m).items()):
        return False
    g1, g2 = s["tau_g1"][0], s["tau_g2"][0]
    if not all(v % R for v in (g1, s["tau_g1"][1], g2, s["tau_g2"][1], s["alpha_tau_g1"][0], s["beta_tau_g1"][0], s["beta_g2"])):
        return False
    tau = s["tau_g1"][1] * pow(g1, -1, R) % R
    for name in ARRAYS:
        if any(x != s[name][0] * pow(tau, i, R) % R for i, x in enumerate(s[name])):
            return False
    return (s["beta_g2"] * g1 - s["beta_tau_g1"][0] * g2) % R == 0


# ---------------------------------------------------------------------------- receipt
def challenge(j, head40: bytes, six: bytes, r_enc: bytes) -> int:
    """head40: bytes 8 .. 48 of the receipt (m and h); six: before | after of tau, alpha, beta; 128 bits, never zero"""
    assert len(head40) == 40 and len(six) == 192 and len(r_enc) == 32
    return int.from_bytes(hashlib.sha256(b"OZK-phase1-pok" + bytes([j]) + head40 + six + r_enc).digest()[:16], "little") or 1


def receipt_bytes(m, h, blocks) -> bytes:
    """blocks: three (before, after, R: affine G1 points; z)"""
    b = MAGIC + m.to_bytes(8, "little") + h + b"".join(
        ref.encode_g1(x) + ref.encode_g1(y) + ref.encode_g1(r) + int(z).to_bytes(32, "little") for x, y, r, z in blocks)
    assert len(b) == RECEIPT_BYTES
    return b


def parse_receipt(b: bytes):
    """{m, h, blocks: [(before, after, R: points, z)]}; ValueError naming the field"""
    if len(b) != RECEIPT_BYTES:
        raise ValueError("length")
    if b[:8] != MAGIC:
        raise ValueError("magic")
    m = int.from_bytes(b[8:16], "little")
    if m < 2 or m & (m - 1):
        raise ValueError("m")
    blocks = []
    for j, name in enumerate(SECRETS):
        off = 48 + 128 * j
        pts = []
        for i, part in enumerate(("before", "after", "r")):
            code, P = ref.decode_g1(b[off + 32 * i:off + 32 * i + 32])
            if code:
                raise ValueError("%s_%s" % (name, part))
            pts.append(P)
        z = int.from_bytes(b[off + 96:off + 128], "little")
        if z >= R:
            raise ValueError("%s_z" % name)
        blocks.append((pts[0], pts[1], pts[2], z))
    return {"m": m, "h": b[16:48], "blocks": blocks}


def receipt_exp(before, after, factors, nonces, previous=b"", m=None, pok_over=(0, 1, 2)):
    """the receipt a contributor who used `factors` and `nonces` writes for these two strings (whatever they hold).
    pok_over: the base each proof's R is taken over, (0, 1, 2) for the honest one"""
    g1 = before["gen_g1"]
    m = before["m"] if m is None else m
    h = hashlib.sha256(previous).digest()
    bl, al = pok_bases(before), pok_bases(after)
    bp, ap = [cref.scale(1, g1, x) for x in bl], [cref.scale(1, g1, x) for x in al]
    six = b"".join(ref.encode_g1(x) + ref.encode_g1(y) for x, y in zip(bp, ap))
    head = m.to_bytes(8, "little") + h
    blocks = []
    for j in range(3):
        r_point = cref.scale(1, g1, nonces[j] * bl[pok_over[j]] % R)
        z = (nonces[j] + challenge(j, head, six, ref.encode_g1(r_point)) * factors[j]) % R
        blocks.append((bp[j], ap[j], r_point, z))
    return receipt_bytes(m, h, blocks)


def contribute_exp(s, factors, nonces, previous=b""):
    """(the string after, the receipt bytes) for the secrets (s, a, b)"""
    t, a, b = factors
    assert all(1 <= v < R for v in tuple(factors) + tuple(nonces))
    new = dict(s)
    new["tau_g1"] = [x * pow(t, i, R) % R for i, x in enumerate(s["tau_g1"])]
    new["tau_g2"] = [x * pow(t, i, R) % R for i, x in enumerate(s["tau_g2"])]
    new["alpha_tau_g1"] = [x * a * pow(t, i, R) % R for i, x in enumerate(s["alpha_tau_g1"])]
    new["beta_tau_g1"] = [x * b * pow(t, i, R) % R for i, x in enumerate(s["beta_tau_g1"])]
    new["beta_g2"] = s["beta_g2"] * b % R
    return new, receipt_exp(s, new, factors, nonces, previous)


def verify_contribution_exp(before, after, receipt: bytes):
    """(accepted, the name of the first failed check or None)"""
    try:
        rec = parse_receipt(receipt)
    except ValueError:
        return False, "receipt"
    g1 = before["gen_g1"]
    # 1
    if not (before["m"] == after["m"] == rec["m"]):
        return False, "receipt_points"
    for s in (before, after):
        if any(len(s[name]) != n for name, n in counts(rec["m"]).items()):
            return False, "receipt_points"
    bl, al = pok_bases(before), pok_bases(after)
    for j in range(3):
        if (rec["blocks"][j][0], rec["blocks"][j][1]) != (cref.scale(1, g1, bl[j]), cref.scale(1, g1, al[j])):
            return False, "receipt_points"
    # 2: logarithms to one generator each, and the generator's own is 1
    if before["tau_g1"][0] != after["tau_g1"][0] or before["tau_g2"][0] != after["tau_g2"][0] \
            or before["gen_g1"] != after["gen_g1"] or before["gen_g2"] != after["gen_g2"]:
        return False, "generators"
    # 3: z before - c after - R = O
    six = receipt[48:112] + receipt[176:240] + receipt[304:368]
    for j in range(3):
        c = challenge(j, receipt[8:48], six, receipt[48 + 128 * j + 64:48 + 128 * j + 96])
        if cref.scale(1, g1, (rec["blocks"][j][3] * bl[j] - c * al[j]) % R) != rec["blocks"][j][2]:
            return False, "pok"
    # 4
    if not wellformed(after):
        return False, "wellformed"
    return True, None


def verify_chain_exp(strings, receipts):
    previous = b""
    for i, b in enumerate(receipts):
        if b[16:48] != hashlib.sha256(previous).digest():
            return False, "chain"
        ok, why = verify_contribution_exp(strings[i], strings[i + 1], b)
        if not ok:
            return False, why
        previous = b
    return True, None


# ---------------------------------------------------------------------------- the file
def file_size(m) -> int:
    return 48 + 32 * (4 * m + 1) + 64 * (m + 1)


def sections_exp(s):
    """{section: compressed points} of a string in the exponent"""
    out = {}
    for name in ARRAYS:
        type_ = 2 if name == "tau_g2" else 1
        gen = s["gen_g2"] if type_ == 2 else s["gen_g1"]
        out[name] = b"".join(cref.encode(type_, cref.scale(type_, gen, x)) for x in s[name])
    out["beta_g2"] = cref.encode(2, cref.scale(2, s["gen_g2"], s["beta_g2"]))
    return out


def file_bytes(m, sections) -> bytes:
    payload = b"".join(sections[name] for name in ARRAYS + ("beta_g2",))
    return FILE_MAGIC + m.to_bytes(8, "little") + hashlib.sha256(payload).digest() + payload


def parse_file(b: bytes):
    """(m, {section: bytes}); ValueError naming the problem"""
    if len(b) < 48 or b[:8] != FILE_MAGIC:
        raise ValueError("magic")
    m = int.from_bytes(b[8:16], "little")
    if m < 2 or m & (m - 1):
        raise ValueError("m")
    if len(b) != file_size(m):
        raise ValueError("length")
    if hashlib.sha256(b[48:]).digest() != b[16:48]:
        raise ValueError("digest")
    out, off = {}, 48
    for name, n in list(counts(m).items()) + [("beta_g2", 1)]:
        size = n * (64 if name in ("tau_g2", "beta_g2") else 32)
        out[name] = b[off:off + size]
        off += size
    return m, out
