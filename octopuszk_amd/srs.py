"""A structured reference string (powers of tau in the exponent) and the Groth16 setup from it.

    srs = Srs.from_secrets(m, tau, alpha, beta)      # tests, tools and measurements: the caller knows the trapdoor
    assert srs.check()                               # a string somebody else supplies
    crs = setup_from_srs(r1cs, srs)                  # nobody needs tau, alpha or beta for this step

For a domain of size m (a power of two, m >= 2), every array a uint8 CUDA tensor of wire-in points:

    tau_g1[i]       = [tau^i] g1         0 <= i <= 2 m   (query_h has m + 1 entries and entry m needs tau^(2 m))
    tau_g2[i]       = [tau^i] g2         0 <= i < m
    alpha_tau_g1[i] = [alpha tau^i] g1   0 <= i < m
    beta_tau_g1[i]  = [beta tau^i] g1    0 <= i < m
    beta_g2         = [beta] g2

A string starts public and is re-randomised by several parties in turn:

    srs0 = Srs.initial(m)                            # tau = alpha = beta = 1: no secret at all
    srs1, receipt = srs0.contribute()                # the three factors drawn here and forgotten on return
    assert verify_contribution(srs0, srs1, receipt)  # anybody
    srs1.save(path); srs1 = Srs.load(path)           # the OZKSRS v1 file; load decodes, it does not check()

Out of scope: interoperability with other tools' .ptau files and receipts, hash-to-curve, a random beacon and a
device-side weight stream.  There is no CPU path.
"""
import ctypes
import hashlib
import secrets
import struct
import time

import torch

from . import ceremony as _ceremony
from . import codec as _codec
from . import keyfile as _keyfile
from . import lib as _lib
from . import transcript as _transcript
from . import vectors as _vectors
from . import wire as _wire
from . import zksnark as _zksnark
from .device import _ptr, _stream
from .fft import FR, SEED, fr_random, lowest_power_of_two, root_of_unity
from .fixed_base_msm import G1_WINDOW_TABLE, G2_WINDOW_TABLE, get_window_size
from .vectors import ec_fft, mul_points, points_add, scale_points, sparse_mat_points

G1, G2 = 1, 2
# phase-1 contributions
MAGIC = b"OZKC1\x00\x00\x01"
RECEIPT_BYTES = 432
CONTRIBUTION_CHECKS = ("receipt_points", "generators", "pok", "wellformed")
_POK_TAG = b"OZK-phase1-pok"
_SECRETS = ("tau", "alpha", "beta")
# the string file: (section, point type, count as a function of m), in file order
FILE_MAGIC = b"OZKSRS\x00\x01"
FILE_HEADER_BYTES = 48
FILE_SECTIONS = (("tau_g1", G1, lambda m: 2 * m + 1), ("alpha_tau_g1", G1, lambda m: m), ("beta_tau_g1", G1, lambda m: m),
                 ("tau_g2", G2, lambda m: m), ("beta_g2", G2, lambda m: 1))
CHECKS = ("shape", "powers_g1", "powers_g2", "alpha_powers", "beta_powers", "beta_g2")
_RHO_TAG = b"OZK-srs-rho"


def _point(t, i, type_):
    n = 96 * type_
    return t.reshape(-1)[n * i:n * (i + 1)]


class Srs:
    def __init__(self, m, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2):
        self.m = int(m)
        self.tau_g1, self.tau_g2 = tau_g1, tau_g2
        self.alpha_tau_g1, self.beta_tau_g1, self.beta_g2 = alpha_tau_g1, beta_tau_g1, beta_g2

    @staticmethod
    def from_secrets(m, tau, alpha, beta, generator=None) -> "Srs":
        """The string of KNOWN secrets tau, alpha, beta in [1, r), over generator * G1_ONE / G2_ONE (the generators of
        serial_setup_generate; default fr_random(SEED)).  For tests, tools and measurements only: whoever calls this
        knows the trapdoor of every key built from the result and can forge proofs for it."""
        m = int(m)
        if m < 2 or m & (m - 1):
            raise ValueError("the domain size must be a power of two >= 2, not %d" % m)
        tau, alpha, beta = (_wire.scalar_in_range(v, what, 1)
                            for v, what in ((tau, "tau"), (alpha, "alpha"), (beta, "beta")))
        rnd = fr_random(SEED) if generator is None else _wire.scalar_in_range(generator, "generator", 1)
        L = _lib.load()
        gens = {G1: bytes(_zksnark.batch_msm_dev(254, 16, _wire.g1_wire(_zksnark.G1_ONE), [rnd], G1).cpu().numpy()),
                G2: bytes(_zksnark.batch_msm_dev(254, 16, _wire.g2_wire(_zksnark.G2_ONE), [rnd], G2).cpu().numpy())}

        def powers(k, n, type_):
            d_sc = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            wsb = int(L.ozk_fr_powers_workspace_bytes(n))
            ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
            tb, kb = _wire.le32([tau]), _wire.le32([k])
            _lib.check(L.ozk_fr_powers_dev(_wire.vp(tb), _wire.vp(kb), n, _ptr(d_sc), _ptr(ws), wsb, _stream()))
            torch.cuda.current_stream().synchronize()
            window = get_window_size(n, G1_WINDOW_TABLE if type_ == G1 else G2_WINDOW_TABLE)
            bits = _zksnark._bit_size(gens[type_])
            if -(-bits // window) * window < 254:     # a few points take window 1: the plan must still cover a scalar
                bits = 254
            return _zksnark.batch_msm_dev(bits, window, gens[type_], d_sc, type_)

        beta_g2 = _zksnark.batch_msm_dev(_zksnark._bit_size(gens[G2]), 16, gens[G2], [beta], G2)
        return Srs(m, powers(1, 2 * m + 1, G1), powers(1, m, G2), powers(alpha, m, G1), powers(beta, m, G1), beta_g2)

    @staticmethod
    def initial(m, generator=None) -> "Srs":
        """The string of tau = alpha = beta = 1: every entry the generator of its group.  It holds no secret and is
        the public start of a chain of contributions."""
        return Srs.from_secrets(m, 1, 1, 1, generator)

    # ------------------------------------------------------------------------ phase 1
    def contribute(self, tau=None, alpha=None, beta=None, *, nonces=None, previous=b""):
        """(the string after, the receipt bytes): tau, alpha, beta of this string multiplied by the secrets s, a, b
        in [1, r) given as `tau`, `alpha`, `beta` (each drawn from `secrets` when None):

            tau_g1[i] times s^i, tau_g2[i] times s^i, alpha_tau_g1[i] times a s^i, beta_tau_g1[i] times b s^i
            (four mul_points calls over scalars ozk_fr_powers_dev writes on the device), beta_g2 times b

        The scalar buffers are zeroed on the device before they are released.  `previous`: the bytes of the receipt
        before this one, empty for the first.  `nonces`: the three u of the proofs of knowledge, in [1, r); give them
        for reproducible receipts in tests only."""
        s, a, b = (secrets.randbelow(FR - 1) + 1 if v is None else _wire.scalar_in_range(v, what, 1)
                   for v, what in zip((tau, alpha, beta), _SECRETS))
        if nonces is None:
            nonces = [secrets.randbelow(FR - 1) + 1 for _ in _SECRETS]
        nonces = [_wire.scalar_in_range(u, "nonce", 1) for u in nonces]
        if len(nonces) != 3:
            raise ValueError("three nonces: one per secret")
        m = self.m
        L = _lib.load()
        spent = []

        def powers(k, n):
            """k s^i, i < n, on the device"""
            d_sc = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            wsb = int(L.ozk_fr_powers_workspace_bytes(n))
            ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device="cuda")
            tb = (ctypes.c_uint8 * 32).from_buffer_copy(s.to_bytes(32, "little"))
            kb = (ctypes.c_uint8 * 32).from_buffer_copy(k.to_bytes(32, "little"))
            _lib.check(L.ozk_fr_powers_dev(ctypes.cast(tb, ctypes.c_void_p), ctypes.cast(kb, ctypes.c_void_p), n,
                                           _ptr(d_sc), _ptr(ws), wsb, _stream()))
            spent.extend((d_sc, ws))
            return d_sc

        try:
            pw = powers(1, 2 * m + 1)
            new = Srs(m, mul_points(self.tau_g1, pw, G1), mul_points(self.tau_g2, pw[:32 * m], G2),
                      mul_points(self.alpha_tau_g1, powers(a, m), G1), mul_points(self.beta_tau_g1, powers(b, m), G1),
                      scale_points(self.beta_g2, b, G2))
        finally:
            for t in spent:
                t.zero_()
            torch.cuda.current_stream().synchronize()
            del spent
        bases = _pok_bases(self)
        rs = _ceremony._enc(torch.cat([scale_points(p, u, G1) for p, u in zip(bases, nonces)]), G1)
        pts = _ceremony._enc(torch.cat(bases + _pok_bases(new)), G1)
        rec = Receipt(m, hashlib.sha256(bytes(previous)).digest(),
                      [(pts[32 * j:32 * j + 32], pts[96 + 32 * j:128 + 32 * j], rs[32 * j:32 * j + 32], 0) for j in range(3)])
        for j, (k, u) in enumerate(zip((s, a, b), nonces)):
            before, after, r, _ = rec.blocks[j]
            rec.blocks[j] = (before, after, r, (u + rec.challenge(j) * k) % FR)
        return new, rec.to_bytes()

    # ------------------------------------------------------------------------ file
    def save(self, path) -> None:
        """Write the string as an OZKSRS version 1 file: the points compressed on the device,
        magic | m | SHA-256 of the payload | tau_g1 | alpha_tau_g1 | beta_tau_g1 | tau_g2 | beta_g2."""
        sections = {name: _ceremony._enc(getattr(self, name).reshape(-1), type_) for name, type_, _ in FILE_SECTIONS}
        with open(path, "wb") as f:
            f.write(string_file_bytes(self.m, sections))

    @staticmethod
    def load(src) -> "Srs":
        """The string of an OZKSRS file (`src`: a path, bytes, or a binary file object), parsed strictly
        (parse_string_file) and decoded on the device with ozk_points_decompress_dev; ValueError naming the first
        section and index whose point does not decode.  load does NOT run check(): the points are on their curves and
        nothing more is known.  In particular a decoded G2 point is on the twist and not yet in the order-r
        subgroup.  Run check() on a string somebody else supplies."""
        m, sections = parse_string_file(src)
        arrays = {}
        for name, type_, _ in FILE_SECTIONS:
            arrays[name], codes = _codec._decompress(_wire.dev_bytes(sections[name]), type_, "wire_in")
            bad = torch.nonzero(codes)
            if bad.numel():
                i = int(bad[0].item())
                code = int(codes[i].item())
                raise ValueError("section %s: point %d does not decode: code %d (%s)"
                                 % (name, i, code, _codec.CODE_NAMES.get(code, "?")))
        return Srs(m, *(arrays[name] for name in ("tau_g1", "tau_g2", "alpha_tau_g1", "beta_tau_g1", "beta_g2")))

    # ------------------------------------------------------------------------ check
    def check(self, seed=None, why=None) -> bool:
        """True exactly when the string is well formed: some tau, alpha, beta stand behind all of it.  The checks run
        in the order of CHECKS; the name of the first that fails is appended to `why` (a list).

          shape         the lengths of the module docstring; tau_g1[0], tau_g1[1], tau_g2[0], tau_g2[1],
                        alpha_tau_g1[0], beta_tau_g1[0] and beta_g2 finite; tau_g2[1] and beta_g2 in the order-r
                        subgroup ([r - 1] P = -P)
          powers_g1     with 128-bit weights rho_i, S = sum rho_i tau_g1[i] and S' = sum rho_i tau_g1[i + 1] over
                        i < 2 m: S != O and e(S', g2) e(-S, tau_g2[1]) = 1
          powers_g2     every tau_g2[i] in the order-r subgroup, and the same shift test over tau_g2 against
                        (tau_g1[0], tau_g1[1])
          alpha_powers  the shift test over alpha_tau_g1 against (g2, tau_g2[1]), the combination not O
          beta_powers   the same over beta_tau_g1
          beta_g2       e(beta_tau_g1[0], g2) = e(g1, beta_g2)

        The weights come from a SHA-256 counter stream over `seed` (bytes or an int) under this module's own tag; None
        draws 32 bytes from the system.  A seeded check is reproducible and so unsound against anyone who knows the
        seed: tests only."""
        def no(name):
            if why is not None:
                why.append(name)
            return False

        m = self.m
        enc, scale, ones = _ceremony._enc, scale_points, _vectors.pairs_are_one
        # 1 shape
        if m < 2 or m & (m - 1):
            return no("shape")
        for t, type_, n in ((self.tau_g1, G1, 2 * m + 1), (self.tau_g2, G2, m), (self.alpha_tau_g1, G1, m),
                            (self.beta_tau_g1, G1, m), (self.beta_g2, G2, 1)):
            if t.numel() != 96 * type_ * n:
                return no("shape")
        g1, tg1 = _point(self.tau_g1, 0, G1), _point(self.tau_g1, 1, G1)
        g2, tg2 = _point(self.tau_g2, 0, G2), _point(self.tau_g2, 1, G2)
        e1 = enc(torch.cat([g1, tg1, _point(self.alpha_tau_g1, 0, G1), _point(self.beta_tau_g1, 0, G1)]), G1)
        sub = torch.cat([tg2, self.beta_g2.reshape(-1)])
        e2 = enc(torch.cat([g2, sub]), G2)
        if any(e1[32 * i + 31] & 0x40 for i in range(4)) or any(e2[64 * i + 63] & 0x40 for i in range(3)):
            return no("shape")
        if not _vectors.in_subgroup_g2(sub, e2[64:]):
            return no("shape")
        rho = _wire.dev_bytes(_transcript.weights(_transcript.seed_bytes(seed), 2 * m, _RHO_TAG))
        keep = []

        def shift_g1(points, n, q_lo, q_hi):
            """sum rho_i points[i] =: S, sum rho_i points[i + 1] =: S', i < n: S != O and e(S', q_lo) e(-S, q_hi) = 1"""
            flat = points.reshape(-1)
            s_lo, w1 = _vectors.msm(flat[:96 * n], rho[:32 * n], n, G1)
            s_hi, w2 = _vectors.msm(flat[96:96 * (n + 1)], rho[:32 * n], n, G1)
            keep.extend((w1, w2))
            if _wire.is_inf_out(s_lo):
                return False
            neg = scale(_wire.wire_out_to_in(s_lo, G1), FR - 1, G1)
            return ones(torch.cat([_wire.wire_out_to_in(s_hi, G1), neg]), torch.cat([q_lo, q_hi]))

        # 2 powers_g1
        if not shift_g1(self.tau_g1, 2 * m, g2, tg2):
            return no("powers_g1")
        # 3 powers_g2
        if not _vectors.in_subgroup_g2(self.tau_g2, enc(self.tau_g2, G2)):
            return no("powers_g2")
        flat = self.tau_g2.reshape(-1)
        t_lo, w1 = _vectors.msm(flat[:192 * (m - 1)], rho[:32 * (m - 1)], m - 1, G2)
        t_hi, w2 = _vectors.msm(flat[192:], rho[:32 * (m - 1)], m - 1, G2)
        if _wire.is_inf_out(t_lo, G2):
            return no("powers_g2")
        if not ones(torch.cat([g1, scale(tg1, FR - 1, G1)]),
                    torch.cat([_wire.wire_out_to_in(t_hi, G2), _wire.wire_out_to_in(t_lo, G2)])):
            return no("powers_g2")
        # 4 alpha_powers, beta_powers
        for name, points in (("alpha_powers", self.alpha_tau_g1), ("beta_powers", self.beta_tau_g1)):
            if not shift_g1(points, m - 1, g2, tg2):
                return no(name)
        # 5 beta_g2
        if not ones(torch.cat([_point(self.beta_tau_g1, 0, G1), scale(g1, FR - 1, G1)]),
                    torch.cat([g2, self.beta_g2.reshape(-1)])):
            return no("beta_g2")
        torch.cuda.current_stream().synchronize()
        del keep, w1, w2
        return True


# ---------------------------------------------------------------------------- phase 1: receipt and verification
def _pok_bases(srs):
    """the three points whose factors a contribution proves knowledge of: tau_g1[1], alpha_tau_g1[0], beta_tau_g1[0]"""
    return [_point(srs.tau_g1, 1, G1), _point(srs.alpha_tau_g1, 0, G1), _point(srs.beta_tau_g1, 0, G1)]


class Receipt:
    """What a phase-1 contributor publishes next to the new string (432 bytes): m, the transcript digest h, and for
    each of tau, alpha, beta a block (before, after, R, z): the base before and after and the Schnorr proof of
    knowledge of the factor between them, exactly as ceremony.Receipt proves its d."""

    def __init__(self, m, h, blocks):
        """h: 32 bytes; blocks: three (before, after, r: compressed G1, 32 bytes each; z: int)"""
        self.m, self.h, self.blocks = int(m), bytes(h), [(bytes(x), bytes(y), bytes(r), int(z)) for x, y, r, z in blocks]

    def to_bytes(self) -> bytes:
        b = MAGIC + struct.pack("<Q", self.m) + self.h + b"".join(
            x + y + r + z.to_bytes(32, "little") for x, y, r, z in self.blocks)
        if len(b) != RECEIPT_BYTES:
            raise ValueError("receipt: a field has the wrong length")
        return b

    @staticmethod
    def from_bytes(b) -> "Receipt":
        """Strict and host-only: ValueError naming the field for a wrong length, a wrong magic, an m that is no power
        of two >= 2, a z >= r or a point that does not decode."""
        b = _codec.receipt_head(b, MAGIC, RECEIPT_BYTES)
        m = struct.unpack_from("<Q", b, 8)[0]
        if m < 2 or m & (m - 1):
            raise ValueError("receipt: m = %d is not a power of two >= 2" % m)
        blocks, fields = [], []
        for j, name in enumerate(_SECRETS):
            o = 48 + 128 * j
            z = int.from_bytes(b[o + 96:o + 128], "little")
            if z >= FR:
                raise ValueError("receipt: %s_z is not below r" % name)
            blocks.append((b[o:o + 32], b[o + 32:o + 64], b[o + 64:o + 96], z))
            fields += [("%s_%s" % (name, part), b[o + 32 * i:o + 32 * i + 32], G1)
                       for i, part in enumerate(("before", "after", "r"))]
        _codec.require_points(fields, "receipt")
        return Receipt(m, b[16:48], blocks)

    def challenge(self, j) -> int:
        """c_j: what block j's response answers; it binds m, h, all six points and R_j"""
        body = bytes([j]) + struct.pack("<Q", self.m) + self.h + b"".join(x + y for x, y, _, _ in self.blocks)
        return _transcript.challenge128(_POK_TAG, body, self.blocks[j][2])


def _shaped(srs) -> bool:
    m = srs.m
    return m >= 2 and not m & (m - 1) and all(
        getattr(srs, name).numel() == 96 * type_ * count(m) for name, type_, count in FILE_SECTIONS)


def verify_contribution(before, after, receipt, *, seed=None, why=None) -> bool:
    """True exactly when `after` is `before` after one contribution that `receipt` (a Receipt or its bytes)
    describes.  The checks run in the order of CONTRIBUTION_CHECKS and the first that fails ends the call with False;
    `why` (a list) then receives its name.

      receipt_points  both strings have the receipt's m and the lengths that go with it, and the receipt's six points
                      are the compressed tau_g1[1], alpha_tau_g1[0], beta_tau_g1[0] of the two strings
      generators      tau_g1[0] and tau_g2[0] equal as compressed encodings
      pok             z_j before_j - c_j after_j - R_j = O for tau, alpha and beta: three 3-point MSMs
      wellformed      after.check(seed=seed)

    `before` is taken on trust, or from the step before it (verify_chain)."""
    def no(name):
        if why is not None:
            why.append(name)
        return False

    rec = receipt if isinstance(receipt, Receipt) else Receipt.from_bytes(receipt)
    if not (before.m == after.m == rec.m and _shaped(before) and _shaped(after)):
        return no("receipt_points")
    b_pts, a_pts = _pok_bases(before), _pok_bases(after)
    pts = _ceremony._enc(torch.cat(b_pts + a_pts), G1)
    if any((pts[32 * j:32 * j + 32], pts[96 + 32 * j:128 + 32 * j]) != rec.blocks[j][:2] for j in range(3)):
        return no("receipt_points")
    g1 = _ceremony._enc(torch.cat([_point(before.tau_g1, 0, G1), _point(after.tau_g1, 0, G1)]), G1)
    g2 = _ceremony._enc(torch.cat([_point(before.tau_g2, 0, G2), _point(after.tau_g2, 0, G2)]), G2)
    if g1[:32] != g1[32:] or g2[:64] != g2[64:]:
        return no("generators")
    flags = [_ceremony._pok_holds(b_pts[j], a_pts[j], rec.blocks[j][2], rec.blocks[j][3], rec.challenge(j))
             for j in range(3)]
    ok = [_ceremony._pok_read(flag) for flag, _ in flags]
    del flags
    if not all(ok):
        return no("pok")
    if not after.check(seed=seed):
        return no("wellformed")
    return True


def verify_chain(strings, receipts, *, seed=None, why=None) -> bool:
    """strings[0] .. strings[k] and the k receipts between them: every step passes verify_contribution, the first
    receipt's h is the SHA-256 of the empty string and every later one's that of the receipt before it (`why`
    receives "chain" for a broken link, else the failed check of the step)."""
    strings = list(strings)
    raw = [r.to_bytes() if isinstance(r, Receipt) else bytes(r) for r in receipts]
    if len(strings) != len(raw) + 1 or not raw:
        raise ValueError("k receipts go with k + 1 strings, k >= 1")
    previous = b""
    for i, b in enumerate(raw):
        rec = Receipt.from_bytes(b)
        if rec.h != hashlib.sha256(previous).digest():
            if why is not None:
                why.append("chain")
            return False
        if not verify_contribution(strings[i], strings[i + 1], rec, seed=seed, why=why):
            return False
        previous = b
    return True


# ---------------------------------------------------------------------------- the string file (host only)
def string_file_size(m) -> int:
    return FILE_HEADER_BYTES + sum(32 * type_ * count(m) for _, type_, count in FILE_SECTIONS)


def string_file_bytes(m, sections) -> bytes:
    """The OZKSRS version 1 file of a string: `sections` maps every name of FILE_SECTIONS to its compressed points."""
    m = int(m)
    if m < 2 or m & (m - 1):
        raise ValueError("the domain size must be a power of two >= 2, not %d" % m)
    for name, type_, count in FILE_SECTIONS:
        if len(sections[name]) != 32 * type_ * count(m):
            raise ValueError("section %s: %d bytes, m says %d" % (name, len(sections[name]), 32 * type_ * count(m)))
    payload = b"".join(bytes(sections[name]) for name, _, _ in FILE_SECTIONS)
    return FILE_MAGIC + struct.pack("<Q", m) + hashlib.sha256(payload).digest() + payload


def parse_string_file(src):
    """(m, {section: compressed points}) of an OZKSRS file, strictly: ValueError for a wrong magic or version, an m
    that is no power of two >= 2, a length that does not follow from m, a digest mismatch.  `src`: a path, bytes, or
    a binary file object (seek, read).  Host only; the points are not decoded here."""
    own = None
    if isinstance(src, (bytes, bytearray, memoryview)):
        f = _keyfile._Bytes(bytes(src))
    elif hasattr(src, "read"):
        f = src
    else:
        f = own = open(src, "rb")
    try:
        size = f.seek(0, 2)

        def read_at(off, n):
            f.seek(off)
            out = f.read(n)
            if len(out) != n:
                raise ValueError("truncated file: %d bytes at offset %d, %d read" % (n, off, len(out)))
            return out

        head = read_at(0, min(FILE_HEADER_BYTES, size))
        if len(head) < 8 or head[:7] != FILE_MAGIC[:7]:
            raise ValueError("header: not a string file (wrong magic)")
        if head[7] != FILE_MAGIC[7]:
            raise ValueError("header: string file version %d, this library reads version 1 (wrong magic)" % head[7])
        if len(head) < FILE_HEADER_BYTES:
            raise ValueError("header: truncated file (length %d, the header alone is %d)" % (len(head), FILE_HEADER_BYTES))
        m = struct.unpack_from("<Q", head, 8)[0]
        if m < 2 or m & (m - 1):
            raise ValueError("header: m = %d is not a power of two >= 2" % m)
        if size != string_file_size(m):
            raise ValueError("length %d, m = %d says %d" % (size, m, string_file_size(m)))
        if _keyfile.digest_from(read_at, FILE_HEADER_BYTES, size) != head[16:48]:
            raise ValueError("digest mismatch: the bytes after the header are not the ones the string was saved with")
        sections, off = {}, FILE_HEADER_BYTES
        for name, type_, count in FILE_SECTIONS:
            n = 32 * type_ * count(m)
            sections[name] = read_at(off, n)
            off += n
        return m, sections
    finally:
        if own is not None:
            own.close()


# ---------------------------------------------------------------------------- the setup
def setup_from_srs(r1cs, srs: Srs, log=None):
    """The Groth16 key of `r1cs` instantiated at the tau of `srs`, with gamma = delta = 1 (the shape of Bowe, Gabizon
    and Miers; contribute / verify_chain then randomise delta), computed without tau, alpha or beta: four inverse
    transforms of the string into the Lagrange basis, sparse products with the transposed constraint matrices, and
    pointwise sums.  Returns a CRS with proving_key (and its .r1cs), gamma_g2, gamma_abc_g1, timing and secrets = None.
    ValueError when the string's m is not lowest_power_of_two(num_constraints + num_inputs), and when tau lies in the
    domain (tau^m = 1: tau_g1[m] equals tau_g1[0])."""
    nc, ni, nv = r1cs.num_constraints, r1cs.num_inputs, r1cs.num_variables
    m = lowest_power_of_two(nc + ni)
    if m != srs.m:
        raise ValueError("the circuit needs a string of m = %d, this one has m = %d" % (m, srs.m))
    tm = {}

    def lap(name, t0):
        torch.cuda.synchronize()
        tm[name] = time.perf_counter() - t0
        return time.perf_counter()

    t0 = time.perf_counter()
    tau_g1 = srs.tau_g1.reshape(-1)
    ends = _ceremony._enc(torch.cat([tau_g1[:96], tau_g1[96 * m:96 * (m + 1)]]), G1)
    if ends[:32] == ends[32:]:
        raise ValueError("tau lies in the domain of size %d (tau_g1[m] = tau_g1[0]): no key can be built at it" % m)
    if getattr(r1cs, "_transposed_dev", None) is None:
        r1cs._transposed_dev = _zksnark.R1CSTransposedDevice(r1cs)
    At, Bt, Ct = r1cs._transposed_dev.mats
    t0 = lap("r1cs_transpose_once_host_s", t0)
    omega = root_of_unity(m)
    pk = _zksnark.ProvingKey()
    # G2 first: its Lagrange array is the largest and has one product
    L2 = ec_fft(srs.tau_g2, G2, omega, inverse=True)
    t0 = lap("fft_g2_s", t0)
    pk.query_b_g2 = sparse_mat_points(Bt, L2, G2)
    del L2
    t0 = lap("product_b_g2_s", t0)
    La = ec_fft(srs.alpha_tau_g1, G1, omega, inverse=True)
    t0 = lap("fft_alpha_s", t0)
    abc = sparse_mat_points(Bt, La, G1)
    del La
    t0 = lap("product_b_alpha_s", t0)
    Lb = ec_fft(srs.beta_tau_g1, G1, omega, inverse=True)
    t0 = lap("fft_beta_s", t0)
    abc = points_add(abc, sparse_mat_points(At, Lb, G1), G1)
    del Lb
    t0 = lap("product_a_beta_s", t0)
    L1 = ec_fft(tau_g1[:96 * m], G1, omega, inverse=True)
    t0 = lap("fft_tau_s", t0)
    pk.query_a = sparse_mat_points(At, L1, G1)
    t0 = lap("product_a_s", t0)
    pk.query_b_g1 = sparse_mat_points(Bt, L1, G1)
    t0 = lap("product_b_g1_s", t0)
    abc = points_add(abc, sparse_mat_points(Ct, L1, G1), G1)
    del L1
    t0 = lap("product_c_s", t0)
    pk.query_h = points_add(tau_g1[96 * m:], tau_g1[:96 * (m + 1)], G1, negate_b=True)
    t0 = lap("query_h_s", t0)
    pk.delta_abc_g1 = abc[96 * ni:].clone()
    pk.alpha_g1 = srs.alpha_tau_g1.reshape(-1)[:96].clone()
    pk.beta_g1 = srs.beta_tau_g1.reshape(-1)[:96].clone()
    pk.beta_g2 = srs.beta_g2.reshape(-1).clone()
    pk.delta_g1 = tau_g1[:96].clone()
    pk.delta_g2 = srs.tau_g2.reshape(-1)[:192].clone()
    pk.r1cs = r1cs
    crs = _zksnark.CRS()
    crs.proving_key = pk
    crs.gamma_g2 = pk.delta_g2.clone()
    crs.gamma_abc_g1 = abc[:96 * ni].clone()
    crs.secrets = None
    crs.timing = tm
    if log:
        log("setup from a string: " + ", ".join("%s %.3f s" % (k[:-2], v) for k, v in tm.items()))
    return crs
