"""KZG polynomial commitments over a powers-of-tau string.

    ck = CommitKey.from_srs(srs)                     # tau_g1[:n] as prepared MSM bases
    vk = VerifyKey.from_srs(srs)                     # tau_g1[0], tau_g2[0], tau_g2[1]; 160 bytes
    c = ck.commit(coeffs)                            # K rows of n coefficients -> K compressed commitments
    openings = ck.open(coeffs, [z_0, ..., z_K-1])    # Opening: C | z | y | pi, 128 bytes
    assert verify(vk, openings[0]) and verify_all(vk, openings)

Polynomials are rows of a uint8 CUDA tensor, 32 bytes little-endian per element, 16-byte aligned: a 1-D tensor is one
row, a 2-D tensor [K, 32 len] is K rows (the row stride may exceed the row: the caller pads).  A coefficient row has
exactly the key's n elements (shorter polynomials are zero-padded); an evaluation row has a power of two n <= 2 m of
them, p(omega_n^i) in natural order, and is committed over the Lagrange form of the string (CommitKey.lagrange).

The commitment is C = [p(tau)] g1; an opening at z is pi = [q(tau)] g1 for q = (p - p(z)) / (X - z), and it verifies when
e(C - [y] g1 + [z] pi, g2) e(-pi, [tau] g2) = 1.  The quotient comes from ozk_fr_poly_open_dev / ozk_fr_evals_open_dev
(csrc/kzg.cuh); every group operation is an existing entry point: the variable-base MSM over prepared bases, the group
FFT, the pairing product and the point codec.

Several points of one polynomial under ONE proof: for S = (z_1 .. z_t), I the interpolant of
p on S and Z_S = prod (X - z_i), the proof is pi = [q(tau)] g1 for q = (p - I) / Z_S (ozk_fr_poly_open_set_dev /
ozk_fr_evals_open_set_dev, csrc/kzg_set.cuh), accepted when e(C - [I(tau)] g1, g2) e(-pi, [Z_S(tau)] g2) = 1.

    svk = SetVerifyKey.from_srs(srs, t_max)          # tau_g1[:t_max], tau_g2[:t_max + 1]
    ops = ck.open_set(coeffs, [z_1, ..., z_t])       # SetOpening: C | t | z | y | pi, 68 + 64 t bytes; one per row
    assert verify_set(svk, ops[0]) and verify_set_all(svk, ops)

Every point of the evaluation domain, or every coset of it, at once (the FK20 construction): for
n a power of two, l a power of two dividing n and r = n / l, the r proofs of the cosets S_k = (omega^(k + r j), j < l),
each the pi of open_set(coeffs, S_k) (of open(coeffs, omega^k) for l = 1), from l transforms over Fr, one
multiply-accumulate kernel over points (ozk_points_mac_dev) and two group FFTs, instead of r quotients and r MSMs.

    ak = OpenAllKey.from_srs(srs, n, coset=l)        # the l prepared tables of one (n, l)
    all_ = ak.open_all(coeffs)[0]                    # AllOpenings: c, values (n x 32 B on the device), proofs (r x 32 B)
    assert verify_set(svk, all_.opening(k))          # an Opening for l = 1, a SetOpening for l > 1

Many polynomials, each at its own set of points, under ONE proof of two G1 points (the
two-element scheme of Boneh, Drake, Fisch and Gabizon): the verifier holds the plain VerifyKey and runs two pairings
whatever the sets.  The rows of every distinct set are summed by ozk_fr_rows_combine_groups_dev and the values come
from ozk_fr_poly_eval_set_dev (csrc/kzg_multi.cuh); the divisions are those of the sections above.

    mo = ck.open_multi(coeffs, [[z], [z, z w], [z]]) # MultiOpening: K | per row C, t, z, y | W | W'
    assert verify_multi(vk, mo) and verify_multi_all(vk, [mo])

A proof system over these openings, with no per-circuit secrets: the `plonk` package.

Out of scope: hiding commitments, degree-bound proofs, multi-openings of evaluation rows, G2 commitments,
interoperability with other tools' byte formats.  There is no CPU path.
"""
import secrets

import torch

from . import ceremony as _ceremony
from . import codec as _codec
from . import lib as _lib
from . import transcript as _transcript
from . import vectors as _vectors
from . import wire as _wire
from .device import VarMsmWorkspace, _ptr, _stream, prepare_bases
from .fft import FR, root_of_unity
from .vectors import ec_fft, fr_fft, fr_poly_eval, points_mac, points_mac_prepare, scale_points
from .wire import ints32, le32, vp, wire_out_to_in

G1, G2 = 1, 2
OPENING_BYTES, VK_BYTES = 128, 160
_RHO_TAG = b"OZK-kzg-rho"
_GAMMA_TAG = b"OZK-kzg-gamma"
_G1_INF = bytes(31) + b"\x40"
SET_T_MAX, SET_EVALS_T_MAX = 32, 8        # KZG_SET_T, KZG_SET_EV_T of csrc/kzg_set.cuh
_SET_RHO_TAG = b"OZK-kzg-set-rho"
_SET_GAMMA_TAG = b"OZK-kzg-set-gamma"


# ---------------------------------------------------------------------------- argument checks (no library call)
def _rows(t, what, n=None):
    """(K, elements per row, row stride in elements) of a tensor of rows; n: the row length the caller requires"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise TypeError("%s must be a uint8 CUDA tensor" % what)
    if not t.is_cuda:
        raise TypeError("%s must be a uint8 CUDA tensor, not one on %s" % (what, t.device))
    if t.dim() not in (1, 2) or t.numel() == 0:
        raise ValueError("%s must be one row (1-D) or K rows (2-D), not %d-D" % (what, t.dim()))
    if t.dim() == 1:
        t = t.unsqueeze(0)
    if t.stride(1) != 1 or t.shape[1] % 32 or (t.shape[0] > 1 and (t.stride(0) % 32 or t.stride(0) < t.shape[1])):
        raise ValueError("%s: rows of whole 32-byte elements, contiguous, at a stride that is a multiple of 32" % what)
    if t.data_ptr() % 16:
        raise ValueError("%s is not 16-byte aligned" % what)
    k, length = t.shape[0], t.shape[1] // 32
    if n is not None and length != n:
        raise ValueError("%s: rows of %d elements, the key has n = %d (zero-pad shorter polynomials)" % (what, length, n))
    return k, length, (t.stride(0) // 32 if k > 1 else length)


def _eval_size(length, m):
    """the size of an evaluation row: a power of two in [2, 2 m]"""
    if length < 2 or length & (length - 1):
        raise ValueError("an evaluation row has a power of two >= 2 of elements, not %d" % length)
    if length > 2 * m:
        raise ValueError("evaluation rows of %d elements: the string has m = %d and carries at most 2 m" % (length, m))
    return length


def _scalars(values, k, what):
    """k ints in [0, r) (one int serves k = 1)"""
    values = [values] if isinstance(values, int) else list(values)
    if len(values) != k:
        raise ValueError("%d %s for %d rows" % (len(values), what, k))
    return [_wire.scalar_in_range(v, what) for v in values]


def _enc_of(b, what, size=32) -> bytes:
    b = bytes(b)
    if len(b) != size:
        raise ValueError("%s: %d bytes, not %d" % (what, len(b), size))
    return b


def require_g1(fields, owner):
    """fields: (name, compressed G1 encoding) of the points of a byte format built on this module (`owner`); ValueError
    naming the first that does not decode.  Strict and host-only, as the from_bytes here."""
    _codec.require_points([(name, enc, G1) for name, enc in fields], owner)


# ---------------------------------------------------------------------------- bytes
class Opening:
    """C | z | y | pi (128 bytes): the compressed commitment, the point, the value, the compressed proof"""

    def __init__(self, c, z, y, pi):
        self.c, self.pi = _enc_of(c, "opening: C"), _enc_of(pi, "opening: pi")
        self.z, self.y = _wire.scalar_in_range(z, "opening: z"), _wire.scalar_in_range(y, "opening: y")

    def to_bytes(self) -> bytes:
        return self.c + le32([self.z, self.y]) + self.pi

    @staticmethod
    def from_bytes(b) -> "Opening":
        """Strict and host-only: ValueError naming the field for a wrong length, z or y >= r, a point that does not
        decode."""
        b = bytes(b)
        if len(b) != OPENING_BYTES:
            raise ValueError("opening: length %d, not %d" % (len(b), OPENING_BYTES))
        z, y = ints32(b[32:96])
        for name, v in (("z", z), ("y", y)):
            if v >= FR:
                raise ValueError("opening: %s is not below r" % name)
        _codec.require_points((("C", b[:32], G1), ("pi", b[96:], G1)), "opening")
        return Opening(b[:32], z, y, b[96:])


def _g2_in_subgroup(points, encodings: bytes) -> bool:
    return _vectors.in_subgroup_g2(points, encodings)


class VerifyKey:
    """g1 = tau_g1[0], g2 = tau_g2[0], tau_g2 = tau_g2[1]: 32 | 64 | 64 bytes, compressed as DESIGN.md section 13"""

    def __init__(self, g1, g2, tau_g2):
        self.g1 = _enc_of(g1, "verification key: g1")
        self.g2, self.tau_g2 = _enc_of(g2, "verification key: g2", 64), _enc_of(tau_g2, "verification key: tau_g2", 64)
        self._points = None

    @staticmethod
    def from_srs(srs) -> "VerifyKey":
        e1 = _ceremony._enc(srs.tau_g1.reshape(-1)[:96], G1)
        e2 = _ceremony._enc(srs.tau_g2.reshape(-1)[:384], G2)
        return VerifyKey(e1, e2[:64], e2[64:])

    def to_bytes(self) -> bytes:
        return self.g1 + self.g2 + self.tau_g2

    @staticmethod
    def from_bytes(b) -> "VerifyKey":
        """Strict: ValueError naming the field for a wrong length, a point that does not decode or is infinity (host
        checks), then for a G2 point outside the order-r subgroup ([r - 1] P = -P on the device, as Srs.check)."""
        b = bytes(b)
        if len(b) != VK_BYTES:
            raise ValueError("verification key: length %d, not %d" % (len(b), VK_BYTES))
        fields = (("g1", b[:32], G1), ("g2", b[32:96], G2), ("tau_g2", b[96:], G2))
        _codec.require_points(fields, "verification key")
        for name, enc, _ in fields:
            if enc[-1] & 0x40:
                raise ValueError("verification key: %s is the point at infinity" % name)
        vk = VerifyKey(b[:32], b[32:96], b[96:])
        for i, name in enumerate(("g2", "tau_g2")):
            if not _g2_in_subgroup(vk.points()[1][192 * i:192 * (i + 1)], fields[1 + i][1]):
                raise ValueError("verification key: %s is not in the order-r subgroup" % name)
        return vk

    def points(self):
        """(g1: one wire-in point, g2 | tau_g2: two wire-in points) on the device, decoded once"""
        if self._points is None:
            p1, c1 = _codec.decompress_g1(_wire.dev_bytes(self.g1))
            p2, c2 = _codec.decompress_g2(_wire.dev_bytes(self.g2 + self.tau_g2))
            if int(c1.any().item()) or int(c2.any().item()):
                raise ValueError("verification key: a point does not decode")
            self._points = (p1, p2)
        return self._points


# ---------------------------------------------------------------------------- the committer
class CommitKey:
    """The first n powers of a string as prepared bases of the variable-base MSM, and (built on first use) the
    Lagrange form of its first n_e powers for every evaluation-row size n_e used."""

    def __init__(self, tau_g1, n, m):
        self.n, self.m = int(n), int(m)
        self._tau_g1 = tau_g1          # wire-in, at least min(2 m, all) points: the source of the Lagrange forms
        self._bases = None
        self._lagrange = {}
        self._msm = {}

    @staticmethod
    def from_srs(srs, n=None) -> "CommitKey":
        have = 2 * int(srs.m) + 1
        n = have if n is None else int(n)
        if not 1 <= n <= have:
            raise ValueError("n = %d: a string of m = %d carries %d powers in G1" % (n, srs.m, have))
        return CommitKey(srs.tau_g1.reshape(-1), n, srs.m)

    # ---- bases
    def bases(self):
        if self._bases is None:
            self._bases = prepare_bases(self._tau_g1[:96 * self.n].contiguous(), self.n, G1)
        return self._bases

    def lagrange(self, n):
        """prepared bases of L_i(tau) g1, i < n, for the domain of omega_n: the inverse group transform of tau_g1[:n]"""
        n = _eval_size(int(n), self.m)
        if n not in self._lagrange:
            pts = ec_fft(self._tau_g1[:96 * n].contiguous(), G1, root_of_unity(n), inverse=True)
            self._lagrange[n] = prepare_bases(pts, n, G1)
        return self._lagrange[n]

    def _row_msms(self, bases, n, scalars, k, stride):
        """k MSMs of n scalars each (row y at element y stride of `scalars`) over prepared bases -> k x 32 bytes"""
        if n not in self._msm:
            self._msm[n] = VarMsmWorkspace(n, G1)
        ws = self._msm[n]
        flat = scalars.reshape(-1) if scalars.is_contiguous() else None
        outs = []
        for y in range(k):
            row = flat[32 * y * stride:32 * (y * stride + n)] if flat is not None else scalars[y].contiguous()
            outs.append(ws.run(bases, row, prepared=True).clone())
        return _wire.host_bytes(_codec.compress_g1(torch.cat(outs), "wire_out"))

    # ---- commit
    def commit(self, coeffs) -> list:
        """K rows of n coefficients -> K compressed commitments (one MSM per row)"""
        k, _, stride = _rows(coeffs, "coeffs", self.n)
        enc = self._row_msms(self.bases(), self.n, _as2d(coeffs), k, stride)
        return [enc[32 * i:32 * i + 32] for i in range(k)]

    def commit_evals(self, evals) -> list:
        """K rows of evaluations on the domain of omega_n -> the commitments of their interpolants"""
        k, n, stride = _rows(evals, "evals")
        _eval_size(n, self.m)
        enc = self._row_msms(self.lagrange(n), n, _as2d(evals), k, stride)
        return [enc[32 * i:32 * i + 32] for i in range(k)]

    # ---- open
    def _openings(self, commitments, zs, quot, n, bases, values):
        k = len(zs)
        pis = self._row_msms(bases, n, quot, k, n)
        ys = ints32(_wire.host_bytes(values))
        return [Opening(commitments[i], zs[i], ys[i], pis[32 * i:32 * i + 32]) for i in range(k)]

    def open(self, coeffs, z) -> list:
        """K rows and K points -> K openings (row i at z_i)"""
        k, _, stride = _rows(coeffs, "coeffs", self.n)
        zs = _scalars(z, k, "points")
        quot, values = poly_open(_as2d(coeffs), k, self.n, stride, zs)
        return self._openings(self.commit(coeffs), zs, quot, self.n, self.bases(), values)

    def open_many_points(self, coeffs, points) -> list:
        """ONE polynomial opened at K points (poly_stride = 0): K openings with the same C"""
        k, _, _ = _rows(coeffs, "coeffs", self.n)
        if k != 1:
            raise ValueError("open_many_points takes one row")
        points = [points] if isinstance(points, int) else list(points)
        zs = _scalars(points, len(points), "points")
        quot, values = poly_open(_as2d(coeffs), len(zs), self.n, 0, zs)
        return self._openings(self.commit(coeffs) * len(zs), zs, quot, self.n, self.bases(), values)

    def open_evals(self, evals, z) -> list:
        """K evaluation rows and K points -> K openings; pi is committed over the Lagrange form"""
        k, n, stride = _rows(evals, "evals")
        _eval_size(n, self.m)
        zs = _scalars(z, k, "points")
        quot, values = evals_open(_as2d(evals), k, n, stride, zs)
        return self._openings(self.commit_evals(evals), zs, quot, n, self.lagrange(n), values)

    def open_combined(self, coeffs, z):
        """K polynomials at ONE point with one proof: (the K commitments, the K values, pi).  The rows are combined
        with the weights gamma^i (combine_challenge) by ozk_fr_rows_combine_dev and the combination is opened at z."""
        k, _, stride = _rows(coeffs, "coeffs", self.n)
        z = _wire.scalar_in_range(z, "the point")
        rows = _as2d(coeffs)
        if k > 1 and stride != self.n:
            rows = rows.contiguous()
        commitments = self.commit(coeffs)
        values = ints32(_wire.host_bytes(fr_poly_eval(rows.reshape(-1), z, k)))
        gamma = combine_challenge(z, commitments, values)
        combined = rows_combine(rows, k, self.n, self.n, [pow(gamma, i, FR) for i in range(k)])
        quot, _ = poly_open(combined.unsqueeze(0), 1, self.n, self.n, [z])
        return commitments, values, self._row_msms(self.bases(), self.n, quot, 1, self.n)

    # ---- open at a set of points with one proof
    def _set_openings(self, commitments, sets, quot, n, bases, values):
        k, t = len(sets), len(sets[0])
        pis = self._row_msms(bases, n, quot, k, n)
        ys = ints32(_wire.host_bytes(values))
        return [SetOpening(commitments[i], sets[i], ys[t * i:t * (i + 1)], pis[32 * i:32 * i + 32]) for i in range(k)]

    def open_set(self, coeffs, points) -> list:
        """K rows, and one list of t points shared by all rows or K lists of t -> K SetOpenings: one kernel call for all
        rows, one MSM per quotient row"""
        k, _, stride = _rows(coeffs, "coeffs", self.n)
        sets = _point_sets(points, k, min(SET_T_MAX, self.m - 1), "the string has m = %d" % self.m)
        quot, values = poly_open_set(_as2d(coeffs), k, self.n, stride, sets)
        return self._set_openings(self.commit(coeffs), sets, quot, self.n, self.bases(), values)

    def open_set_evals(self, evals, points) -> list:
        """The same over K evaluation rows; every point must lie outside the domain (open an in-domain set in
        coefficient form); pi is committed over the Lagrange form"""
        k, n, stride = _rows(evals, "evals")
        _eval_size(n, self.m)
        sets = _point_sets(points, k, min(SET_EVALS_T_MAX, self.m - 1), "the string has m = %d" % self.m)
        for row in sets:
            for z in row:
                if pow(z, n, FR) == 1:
                    raise ValueError("the point %d lies in the domain of %d elements: open such a set in coefficient form"
                                     % (z, n))
        quot, values = evals_open_set(_as2d(evals), k, n, stride, sets)
        return self._set_openings(self.commit_evals(evals), sets, quot, n, self.lagrange(n), values)

    def open_set_combined(self, coeffs, points):
        """K polynomials at ONE shared set with one proof: (the K commitments, the K rows of t values, pi).  The rows
        are combined with the weights gamma^i (set_combine_challenge) and the combination is opened at the set."""
        k, _, stride = _rows(coeffs, "coeffs", self.n)
        points = _point_sets(points, 1, min(SET_T_MAX, self.m - 1), "the string has m = %d" % self.m, shared=True)[0]
        rows = _as2d(coeffs)
        if k > 1 and stride != self.n:
            rows = rows.contiguous()
        commitments = self.commit(coeffs)
        at = [ints32(_wire.host_bytes(fr_poly_eval(rows.reshape(-1), z, k))) for z in points]
        values = [[col[i] for col in at] for i in range(k)]
        gamma = set_combine_challenge(points, commitments, values)
        combined = rows_combine(rows, k, self.n, self.n, [pow(gamma, i, FR) for i in range(k)])
        quot, _ = poly_open_set(combined.unsqueeze(0), 1, self.n, self.n, [points])
        return commitments, values, self._row_msms(self.bases(), self.n, quot, 1, self.n)

    # ---- open many rows, each at its own set, with one proof
    def open_multi(self, coeffs, point_sets, commitments=None) -> "MultiOpening":
        """K rows, row i at its own set point_sets[i] of t_i points, under ONE proof of two G1 points (DESIGN.md section
        28): the values from one ozk_fr_poly_eval_set_dev call (from one ozk_fr_poly_eval_dev call per point where every
        set lies inside one of at most 8 points), the sums F_g = sum_{i in g} gamma^i f_i of the rows of
        every distinct set from one ozk_fr_rows_combine_groups_dev call, one ozk_fr_poly_open_set_dev call per distinct
        set size for h = sum_g (F_g - I_g) / Z_{S_g} and W = [h(tau)] g1, then L = sum_g c_g F_g - Z_T(z) h opened at z for
        W'.  1 <= K <= 256, 1 <= t_i <= 32 (whatever the string's m), at most 32 distinct sets.  `commitments`: the K
        compressed commitments, for a caller who holds them already (else K MSMs)."""
        k, _, stride = _rows(coeffs, "coeffs", self.n)
        sets = _multi_sets(point_sets, "point_sets", k)
        groups, group_of = _multi_groups(sets, MULTI_SETS_MAX)
        if commitments is not None:
            commitments = [_enc_of(c, "commitment") for c in commitments]
            if len(commitments) != k:
                raise ValueError("%d commitments for %d rows" % (len(commitments), k))
        rows, n, ng = _as2d(coeffs), self.n, len(groups)
        if commitments is None:
            commitments = self.commit(coeffs)
        t_top = max(len(row) for row in sets)
        union = groups[-1] if all(set(g) <= set(groups[-1]) for g in groups) else None
        if union is not None and t_top <= MULTI_EVAL_CALLS_T:
            # every set lies inside the largest one (z and z omega): one pass of ozk_fr_poly_eval_dev per point over
            # all rows measured faster than the set kernel for up to 8 points
            at = dict(zip(union, poly_eval_points(rows, k, n, stride, union)))
            values = [tuple(at[z][i] for z in row) for i, row in enumerate(sets)]
        else:
            # short sets are padded with their first point; the values of the padding are dropped
            padded = [row + (row[0],) * (t_top - len(row)) for row in sets]
            ys = ints32(_wire.host_bytes(poly_eval_set(rows, k, n, stride, padded)))
            values = [tuple(ys[t_top * i:t_top * i + len(row)]) for i, row in enumerate(sets)]
        gamma, digest = _multi_gamma(commitments, sets, values)
        # rows 0 .. G - 1: the F_g; row G: h
        buf = torch.empty((ng + 1, 32 * n), dtype=torch.uint8, device=rows.device)
        rows_combine_groups(rows, k, n, stride, [pow(gamma, i, FR) for i in range(k)], group_of, ng, buf, n)
        quot = torch.empty((ng, 32 * n), dtype=torch.uint8, device=rows.device)
        a = 0
        while a < ng:                                                   # the groups of one size are neighbours
            b = a + 1
            while b < ng and len(groups[b]) == len(groups[a]):
                b += 1
            poly_open_set(buf[a:b], b - a, n, n, groups[a:b], quot[a:b])
            a = b
        rows_combine(quot, ng, n, n, [1] * ng, buf[ng])
        w = self._row_msms(self.bases(), n, buf[ng:], 1, n)
        z = _multi_z(digest, w)
        c, _, _, z_t = _multi_at(sets, values, groups, group_of, gamma, z)
        combined = rows_combine(buf, ng + 1, n, n, c + [(FR - z_t) % FR])
        quot2, _ = poly_open(combined.unsqueeze(0), 1, n, n, [z])
        return MultiOpening(commitments, sets, values, w, self._row_msms(self.bases(), n, quot2, 1, n))


def _as2d(t):
    return t.unsqueeze(0) if t.dim() == 1 else t


# ---------------------------------------------------------------------------- the Fr kernels
def poly_open(coeffs, k, n, stride, zs):
    """ozk_fr_poly_open_dev on k rows (stride 0: one row at k points): (quotient rows [k, 32 n], values [32 k]) on the
    device.  Synchronises (the workspace dies here)."""
    L = _lib.load()
    quot = torch.empty((k, 32 * n), dtype=torch.uint8, device=coeffs.device)
    values = torch.empty(32 * k, dtype=torch.uint8, device=coeffs.device)
    wsb = int(L.ozk_fr_poly_open_workspace_bytes(k, n))
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=coeffs.device)
    pts = _wire.dev_bytes(le32(zs))
    _lib.check(L.ozk_fr_poly_open_dev(_ptr(coeffs), k, n, stride, _ptr(pts), _ptr(quot), n, _ptr(values), _ptr(ws),
                                      ws.numel(), _stream()))
    torch.cuda.current_stream().synchronize()
    return quot, values


def evals_open(evals, k, n, stride, zs):
    """ozk_fr_evals_open_dev on k evaluation rows over the domain of omega_n: (quotient rows, values) on the device"""
    L = _lib.load()
    quot = torch.empty((k, 32 * n), dtype=torch.uint8, device=evals.device)
    values = torch.empty(32 * k, dtype=torch.uint8, device=evals.device)
    wsb = int(L.ozk_fr_evals_open_workspace_bytes(k, n))
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=evals.device)
    pts = _wire.dev_bytes(le32(zs))
    _lib.check(L.ozk_fr_evals_open_dev(_ptr(evals), k, n, stride, vp(le32([root_of_unity(n)])), _ptr(pts), _ptr(quot), n,
                                       _ptr(values), _ptr(ws), ws.numel(), _stream()))
    torch.cuda.current_stream().synchronize()
    return quot, values


def rows_combine(rows, k, n, stride, weights, out=None):
    """sum_i w_i rows[i] as a row of n elements, a new one unless `out` is given (ozk_fr_rows_combine_dev)"""
    L = _lib.load()
    if out is None:
        out = torch.empty(32 * n, dtype=torch.uint8, device=rows.device)
    w = _wire.dev_bytes(le32(weights))
    _lib.check(L.ozk_fr_rows_combine_dev(_ptr(rows), k, n, stride, _ptr(w), _ptr(out), _stream()))
    torch.cuda.current_stream().synchronize()
    return out


# ---------------------------------------------------------------------------- verification
def combine_challenge(z, commitments, values) -> int:
    """gamma: the first 16 bytes, little-endian, of SHA-256("OZK-kzg-gamma" | K as 8 bytes LE | z | the K compressed
    commitments | the K values); 1 if they are zero"""
    return _transcript.challenge128(_GAMMA_TAG, len(commitments).to_bytes(8, "little"), le32([z]),
                                    b"".join(commitments), le32(values))


def _pairing_holds(lhs_out, neg_weight_pi, pi_is_inf, vk) -> bool:
    """e(lhs, g2) e(-P, tau_g2) = 1 for lhs (wire-out) and P (wire-in, to be negated).  The pairing kernels take O as
    the affine (0, 1), which is no neutral element, so a pair whose G1 point is O is left out here: its factor is 1."""
    lhs_inf = _wire.is_inf_out(lhs_out)
    if lhs_inf or pi_is_inf:
        return lhs_inf and pi_is_inf      # one factor alone is e(X, Q) with X != O: not 1
    neg = scale_points(neg_weight_pi, FR - 1, G1)
    return _vectors.pairs_are_one(torch.cat([wire_out_to_in(lhs_out, G1), neg]), vk.points()[1])


def decode_g1(encodings):
    """n x 32 bytes of compressed G1 encodings on the device (a uint8 CUDA tensor) -> (n wire-in points with Z = 1,
    n int32 codes, 0 where the point decoded): the strict decoder for the byte formats built on this module.  A point
    with a nonzero code, like infinity, is written as (0, 1, 0).  Asynchronous on the current stream."""
    return _codec.decompress_g1(encodings.reshape(-1))


def _decoded(encs):
    """the wire-in points of compressed G1 encodings, or None when one does not decode"""
    pts, codes = decode_g1(_wire.dev_bytes(b"".join(encs)))
    return None if int(codes.any().item()) else pts


def verify(vk, opening) -> bool:
    """e(C - [y] g1 + [z] pi, g2) e(-pi, tau_g2) = 1: one 3-point MSM and one product of two pairings"""
    o = opening if isinstance(opening, Opening) else Opening.from_bytes(opening)
    pts = _decoded([o.c, o.pi])
    if pts is None:
        return False
    lhs, ws = _vectors.msm(torch.cat([pts[:96], vk.points()[0], pts[96:]]),
                           _wire.dev_bytes(le32([1, (FR - o.y) % FR, o.z])), 3)
    ok = _pairing_holds(lhs, pts[96:], o.pi == _G1_INF, vk)
    del ws
    return ok


def verify_all(vk, openings, seed=None) -> bool:
    """All K openings at once with weights rho_i in [1, 2^128) (the SHA-256 counter stream of transcript.py under this
    module's tag; `seed` None draws 32 bytes from the system, a given seed is for tests only):
        e(sum rho_i (C_i - [y_i] g1 + [z_i] pi_i), g2) e(-sum rho_i pi_i, tau_g2) = 1
    as one MSM of 2 K + 1 points, one of K points and one pairing product."""
    os_ = [o if isinstance(o, Opening) else Opening.from_bytes(o) for o in openings]
    k = len(os_)
    if k == 0:
        return True
    seed = secrets.token_bytes(32) if seed is None else _transcript.seed_bytes(seed)
    rho = ints32(_transcript.weights(seed, k, _RHO_TAG))
    pts = _decoded([o.c for o in os_] + [o.pi for o in os_])
    if pts is None:
        return False
    sc = rho + [r * o.z % FR for r, o in zip(rho, os_)] + [-sum(r * o.y for r, o in zip(rho, os_)) % FR]
    lhs, ws1 = _vectors.msm(torch.cat([pts, vk.points()[0]]), _wire.dev_bytes(le32(sc)), 2 * k + 1)
    ps, ws2 = _vectors.msm(pts[96 * k:], _wire.dev_bytes(le32(rho)), k)
    ok = _pairing_holds(lhs, wire_out_to_in(ps, G1), _wire.is_inf_out(ps), vk)
    del ws1, ws2
    return ok


def verify_each(vk, openings, seed=None) -> list:
    """One verdict per opening: the batch check first, single checks only when it fails"""
    openings = list(openings)
    if verify_all(vk, openings, seed):
        return [True] * len(openings)
    return [verify(vk, o) for o in openings]


def verify_combined(vk, commitments, z, values, pi) -> bool:
    """The proof of open_combined: sum gamma^i C_i opens to sum gamma^i y_i at z"""
    commitments = [_enc_of(c, "commitment") for c in commitments]
    z = _wire.scalar_in_range(z, "the point")
    values = _scalars(values, len(commitments), "values")
    pi = _enc_of(pi, "pi")
    if not commitments:
        raise ValueError("no commitment")
    gamma = combine_challenge(z, commitments, values)
    pw = [pow(gamma, i, FR) for i in range(len(commitments))]
    pts = _decoded(commitments)
    if pts is None:
        return False
    c, ws = _vectors.msm(pts, _wire.dev_bytes(le32(pw)), len(commitments))
    c_enc = _wire.host_bytes(_codec.compress_g1(c, "wire_out"))
    del ws
    return verify(vk, Opening(c_enc, z, sum(w * y for w, y in zip(pw, values)) % FR, pi))


# ============================================================================ several points under one proof (section 23)
def _point_sets(points, k, t_max, why, shared=False):
    """k tuples of t pairwise distinct ints in [0, r), 1 <= t <= t_max, from one list of t points (shared by the k
    rows) or, unless `shared`, k lists of t"""
    if isinstance(points, (int, str, bytes)) or not hasattr(points, "__iter__"):
        raise TypeError("points must be a list of points, or one list per row")
    points = list(points)
    if not points:
        raise ValueError("an empty set of points (1 <= t)")
    nested = [hasattr(p, "__iter__") and not isinstance(p, (str, bytes)) for p in points]
    if any(nested) and (shared or not all(nested)):
        raise ValueError("points: one list of points%s" % ("" if shared else ", or one list per row, not a mix"))
    sets = [list(p) for p in points] if nested[0] else [points] * k
    if len(sets) != k:
        raise ValueError("%d lists of points for %d rows" % (len(sets), k))
    t = len(sets[0])
    if any(len(row) != t for row in sets):
        raise ValueError("ragged lists of points: every row takes the same number t")
    if not 1 <= t <= t_max:
        raise ValueError("t = %d points: 1 <= t <= %d here (%s)" % (t, t_max, why))
    sets = [tuple(_wire.scalar_in_range(z, "a point") for z in row) for row in sets]
    for row in sets:
        if len(set(row)) != t:
            raise ValueError("repeated points in a set: %s" % (row,))
    return sets


def _vanishing(points):
    """the t + 1 coefficients of Z_S = prod (X - z_i), lowest first"""
    z = [1]
    for p in points:
        z = [((z[j - 1] if j else 0) - p * (z[j] if j < len(z) else 0)) % FR for j in range(len(z) + 1)]
    return z


def _interpolant(points, values):
    """the t coefficients of the polynomial of degree < t through (z_i, y_i), in host integers (t is small): the
    Lagrange numerators are Z_S / (X - z_i) by synthetic division, their denominators the numerators at z_i"""
    t = len(points)
    zs = _vanishing(points)
    out = [0] * t
    for zi, yi in zip(points, values):
        num, acc = [0] * t, 0
        for j in range(t, 0, -1):
            acc = (zs[j] + zi * acc) % FR
            num[j - 1] = acc
        den = 0
        for c in reversed(num):
            den = (den * zi + c) % FR
        s = yi * pow(den, -1, FR) % FR
        for j in range(t):
            out[j] = (out[j] + s * num[j]) % FR
    return out


class SetOpening:
    """C 32 | t uint32 LE | z 32 t | y 32 t | pi 32 (68 + 64 t bytes): the compressed commitment, the points, the
    values at them, the compressed proof"""

    def __init__(self, c, points, values, pi):
        self.c, self.pi = _enc_of(c, "set opening: C"), _enc_of(pi, "set opening: pi")
        self.points = tuple(_wire.scalar_in_range(z, "set opening: z") for z in points)
        self.values = tuple(_wire.scalar_in_range(y, "set opening: y") for y in values)
        if not 1 <= len(self.points) <= SET_T_MAX:
            raise ValueError("set opening: t = %d, not in [1, %d]" % (len(self.points), SET_T_MAX))
        if len(self.values) != len(self.points):
            raise ValueError("set opening: %d values for %d points" % (len(self.values), len(self.points)))
        if len(set(self.points)) != len(self.points):
            raise ValueError("set opening: z has repeated points")

    @property
    def t(self):
        return len(self.points)

    def to_bytes(self) -> bytes:
        return self.c + self.t.to_bytes(4, "little") + le32(self.points) + le32(self.values) + self.pi

    @staticmethod
    def from_bytes(b) -> "SetOpening":
        """Strict and host-only: ValueError naming the field for a wrong length, t outside [1, 32], z or y >= r,
        repeated points, a point that does not decode."""
        b = bytes(b)
        if len(b) < 36:
            raise ValueError("set opening: length %d, too short for C and t" % len(b))
        t = int.from_bytes(b[32:36], "little")
        if not 1 <= t <= SET_T_MAX:
            raise ValueError("set opening: t = %d, not in [1, %d]" % (t, SET_T_MAX))
        if len(b) != 68 + 64 * t:
            raise ValueError("set opening: length %d, not %d for t = %d" % (len(b), 68 + 64 * t, t))
        zs, ys = ints32(b[36:36 + 32 * t]), ints32(b[36 + 32 * t:36 + 64 * t])
        for name, vs in (("z", zs), ("y", ys)):
            if any(v >= FR for v in vs):
                raise ValueError("set opening: %s is not below r" % name)
        if len(set(zs)) != t:
            raise ValueError("set opening: z has repeated points")
        _codec.require_points((("C", b[:32], G1), ("pi", b[-32:], G1)), "set opening")
        return SetOpening(b[:32], zs, ys, b[-32:])


class SetVerifyKey:
    """tau_g1[:t_max] and tau_g2[:t_max + 1]: what the verifier of openings at up to t_max points commits I and Z_S
    with.  Bytes: t_max uint32 LE | 32 t_max | 64 (t_max + 1), compressed as DESIGN.md section 13."""

    def __init__(self, t_max, g1s, g2s):
        self.t_max = int(t_max)
        if not 1 <= self.t_max <= SET_T_MAX:
            raise ValueError("set verification key: t_max = %d, not in [1, %d]" % (self.t_max, SET_T_MAX))
        self.g1s = _enc_of(g1s, "set verification key: tau_g1", 32 * self.t_max)
        self.g2s = _enc_of(g2s, "set verification key: tau_g2", 64 * (self.t_max + 1))
        self._points = None

    @staticmethod
    def from_srs(srs, t_max) -> "SetVerifyKey":
        t_max = int(t_max)
        if not 1 <= t_max <= min(SET_T_MAX, int(srs.m) - 1):
            raise ValueError("t_max = %d: a string of m = %d carries m powers in G2, so 1 <= t_max <= %d"
                             % (t_max, srs.m, min(SET_T_MAX, int(srs.m) - 1)))
        e1 = _ceremony._enc(srs.tau_g1.reshape(-1)[:96 * t_max].contiguous(), G1)
        e2 = _ceremony._enc(srs.tau_g2.reshape(-1)[:192 * (t_max + 1)].contiguous(), G2)
        return SetVerifyKey(t_max, e1, e2)

    def to_bytes(self) -> bytes:
        return self.t_max.to_bytes(4, "little") + self.g1s + self.g2s

    @staticmethod
    def from_bytes(b) -> "SetVerifyKey":
        """Strict, as VerifyKey.from_bytes: ValueError naming the field for a wrong length, t_max outside [1, 32], a
        point that does not decode or is infinity (host checks), then for a G2 point outside the order-r subgroup (on
        the device)."""
        b = bytes(b)
        if len(b) < 4:
            raise ValueError("set verification key: length %d, too short for t_max" % len(b))
        t_max = int.from_bytes(b[:4], "little")
        if not 1 <= t_max <= SET_T_MAX:
            raise ValueError("set verification key: t_max = %d, not in [1, %d]" % (t_max, SET_T_MAX))
        if len(b) != 4 + 32 * t_max + 64 * (t_max + 1):
            raise ValueError("set verification key: length %d, not %d for t_max = %d"
                             % (len(b), 4 + 32 * t_max + 64 * (t_max + 1), t_max))
        g1s, g2s = b[4:4 + 32 * t_max], b[4 + 32 * t_max:]
        fields = [("tau_g1[%d]" % i, g1s[32 * i:32 * i + 32], G1) for i in range(t_max)]
        fields += [("tau_g2[%d]" % i, g2s[64 * i:64 * i + 64], G2) for i in range(t_max + 1)]
        _codec.require_points(fields, "set verification key")
        for name, enc, _ in fields:
            if enc[-1] & 0x40:
                raise ValueError("set verification key: %s is the point at infinity" % name)
        vk = SetVerifyKey(t_max, g1s, g2s)
        for i in range(t_max + 1):
            if not _g2_in_subgroup(vk.points()[1][192 * i:192 * (i + 1)], g2s[64 * i:64 * i + 64]):
                raise ValueError("set verification key: tau_g2[%d] is not in the order-r subgroup" % i)
        return vk

    def points(self):
        """(tau_g1[:t_max], tau_g2[:t_max + 1]) as wire-in points on the device, decoded once"""
        if self._points is None:
            p1, c1 = _codec.decompress_g1(_wire.dev_bytes(self.g1s))
            p2, c2 = _codec.decompress_g2(_wire.dev_bytes(self.g2s))
            if int(c1.any().item()) or int(c2.any().item()):
                raise ValueError("set verification key: a point does not decode")
            self._points = (p1, p2)
        return self._points


def poly_open_set(coeffs, k, n, stride, sets, quot=None):
    """ozk_fr_poly_open_set_dev on k rows, row y at the t points sets[y]: (quotient rows [k, 32 n], new ones unless
    `quot` is given, values [32 k t]) on the device.  Synchronises (the workspace dies here)."""
    L = _lib.load()
    t = len(sets[0])
    if quot is None:
        quot = torch.empty((k, 32 * n), dtype=torch.uint8, device=coeffs.device)
    values = torch.empty(32 * k * t, dtype=torch.uint8, device=coeffs.device)
    wsb = int(L.ozk_fr_poly_open_set_workspace_bytes(k, n, t))
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=coeffs.device)
    pts = le32([z for row in sets for z in row])
    _lib.check(L.ozk_fr_poly_open_set_dev(_ptr(coeffs), k, n, stride, t, vp(pts), _ptr(quot), n, _ptr(values), _ptr(ws),
                                          ws.numel(), _stream()))
    torch.cuda.current_stream().synchronize()
    return quot, values


def evals_open_set(evals, k, n, stride, sets):
    """ozk_fr_evals_open_set_dev on k evaluation rows over the domain of omega_n: (quotient rows, values)"""
    L = _lib.load()
    t = len(sets[0])
    quot = torch.empty((k, 32 * n), dtype=torch.uint8, device=evals.device)
    values = torch.empty(32 * k * t, dtype=torch.uint8, device=evals.device)
    wsb = int(L.ozk_fr_evals_open_set_workspace_bytes(k, n, t))
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=evals.device)
    pts = le32([z for row in sets for z in row])
    _lib.check(L.ozk_fr_evals_open_set_dev(_ptr(evals), k, n, stride, vp(le32([root_of_unity(n)])), t, vp(pts),
                                           _ptr(quot), n, _ptr(values), _ptr(ws), ws.numel(), _stream()))
    torch.cuda.current_stream().synchronize()
    return quot, values


def set_combine_challenge(points, commitments, values) -> int:
    """gamma: the first 16 bytes, little-endian, of SHA-256("OZK-kzg-set-gamma" | K as 8 bytes LE | t as 8 bytes LE | the
    t points | the K compressed commitments | the K rows of t values); 1 if they are zero"""
    return _transcript.challenge128(_SET_GAMMA_TAG, len(commitments).to_bytes(8, "little"),
                                    len(points).to_bytes(8, "little"), le32(points), b"".join(commitments),
                                    le32([v for row in values for v in row]))


def _set_opening(vk, o):
    o = o if isinstance(o, SetOpening) else SetOpening.from_bytes(o)
    if o.t > vk.t_max:
        raise ValueError("an opening at t = %d points: the key covers t_max = %d" % (o.t, vk.t_max))
    return o


def _pairs_hold(pairs) -> bool:
    """prod e(P_i, Q_i) = 1 over (P wire-in G1, whether P is O, Q wire-in G2); a pair whose G1 point is O is left out
    (_pairing_holds: the kernels take O as an affine point, which is no neutral element), and one pair alone is
    e(P, Q) with P != O and Q != O of order r: not 1"""
    live = [(p, q) for p, inf, q in pairs if not inf]
    if len(live) < 2:
        return not live
    return _vectors.pairs_are_one(torch.cat([p for p, _ in live]), torch.cat([q for _, q in live]))


def verify_set(vk, opening) -> bool:
    """e(C - [I(tau)] g1, g2) e(-pi, [Z_S(tau)] g2) = 1: one G1 MSM of t + 1 points (C with scalar 1, tau_g1[:t] with the
    coefficients of -I), one G2 MSM of t + 1 points and one product of two pairings.  I and Z_S come from (z_i, y_i) in
    host integers.  lhs = pi = O is accepted (a polynomial of degree < t), one of them O alone is not, and neither is
    [Z_S(tau)] g2 = O."""
    return _verify_sets(vk, [_set_opening(vk, opening)], [1])


def verify_set_all(vk, openings, seed=None) -> bool:
    """All K openings at once with weights rho_i in [1, 2^128) (the stream of transcript.py under this module's set tag;
    `seed` as verify_all).  Openings are grouped by identical point tuple D:
        e(sum rho_i (C_i - [I_i(tau)] g1), g2) prod_D e(-sum_{i in D} rho_i pi_i, [Z_D(tau)] g2) = 1
    as one G1 MSM of K + t points, one of |D| points and one G2 MSM of t + 1 points per distinct set, and one pairing
    product."""
    os_ = [_set_opening(vk, o) for o in openings]
    if not os_:
        return True
    seed = secrets.token_bytes(32) if seed is None else _transcript.seed_bytes(seed)
    return _verify_sets(vk, os_, ints32(_transcript.weights(seed, len(os_), _SET_RHO_TAG)))


def _verify_sets(vk, os_, rho) -> bool:
    """the equation of verify_set_all over parsed openings with the weights rho"""
    k = len(os_)
    pts = _decoded([o.c for o in os_] + [o.pi for o in os_])
    if pts is None:
        return False
    g1s, g2s = vk.points()
    t_top = max(o.t for o in os_)
    minus_i = [0] * t_top
    groups = {}
    for i, o in enumerate(os_):
        groups.setdefault(o.points, []).append(i)
    for points, members in groups.items():
        # interpolation is linear in the values: one interpolant per distinct set, of the weighted sums
        ys = [sum(rho[i] * os_[i].values[j] for i in members) % FR for j in range(len(points))]
        for j, c in enumerate(_interpolant(points, ys)):
            minus_i[j] = (minus_i[j] - c) % FR
    keep = []
    lhs, ws = _vectors.msm(torch.cat([pts[:96 * k], g1s[:96 * t_top]]), _wire.dev_bytes(le32(rho + minus_i)),
                           k + t_top)
    keep.append(ws)
    pairs = [(wire_out_to_in(lhs, G1), _wire.is_inf_out(lhs), g2s[:192])]
    for points, members in groups.items():
        zq, ws = _vectors.msm(g2s[:192 * (len(points) + 1)], _wire.dev_bytes(le32(_vanishing(points))),
                              len(points) + 1, G2)
        keep.append(ws)
        if _wire.is_inf_out(zq, G2):
            return False
        ps, ws = _vectors.msm(torch.cat([pts[96 * (k + i):96 * (k + i + 1)] for i in members]),
                              _wire.dev_bytes(le32([rho[i] for i in members])), len(members))
        keep.append(ws)
        inf = _wire.is_inf_out(ps)
        neg = None if inf else scale_points(wire_out_to_in(ps, G1), FR - 1, G1)
        pairs.append((neg, inf, wire_out_to_in(zq, G2)))
    ok = _pairs_hold(pairs)
    torch.cuda.current_stream().synchronize()
    del keep
    return ok


def verify_set_each(vk, openings, seed=None) -> list:
    """One verdict per opening: the batch check first, single checks only when it fails"""
    openings = list(openings)
    if verify_set_all(vk, openings, seed):
        return [True] * len(openings)
    return [verify_set(vk, o) for o in openings]


def verify_set_combined(vk, commitments, points, values, pi) -> bool:
    """The proof of open_set_combined: sum gamma^i C_i opens to (sum gamma^i y_ij)_j at the set"""
    commitments = [_enc_of(c, "commitment") for c in commitments]
    if not commitments:
        raise ValueError("no commitment")
    points = _point_sets(points, 1, vk.t_max, "the key covers t_max = %d" % vk.t_max, shared=True)[0]
    values = [list(row) for row in values]
    if len(values) != len(commitments) or any(len(row) != len(points) for row in values):
        raise ValueError("values: %d rows of %d for %d commitments" % (len(values), len(points), len(commitments)))
    values = [_scalars(row, len(points), "values") for row in values]
    pi = _enc_of(pi, "pi")
    gamma = set_combine_challenge(points, commitments, values)
    pw = [pow(gamma, i, FR) for i in range(len(commitments))]
    pts = _decoded(commitments)
    if pts is None:
        return False
    c, ws = _vectors.msm(pts, _wire.dev_bytes(le32(pw)), len(commitments))
    c_enc = _wire.host_bytes(_codec.compress_g1(c, "wire_out"))
    del ws
    ys = [sum(w * row[j] for w, row in zip(pw, values)) % FR for j in range(len(points))]
    return verify_set(vk, SetOpening(c_enc, points, ys, pi))


# ============================================================================ every coset at once (section 25)
ALL_COSETS = (1, 2, 4, 8, 16, 32)     # coset sizes l: up to the t of a set opening (SET_T_MAX)
ALL_MAX_TRANSFORM = 1 << 22           # the largest group FFT (ozk_ec_fft_dev); the construction runs one of 2 n / l
_G1_INF_WIRE = bytes(32) + (1).to_bytes(32, "little") + bytes(32)


class AllOpenings:
    """What open_all returns per polynomial: c (the compressed commitment), values (n x 32 bytes on the device, p(omega^i)
    in natural order) and proofs (r x 32 bytes on the device, compressed as DESIGN.md section 13; proof k is that of the
    coset S_k = (omega^(k + r j), j < l))."""

    def __init__(self, c, values, proofs, n, coset):
        self.c, self.values, self.proofs = _enc_of(c, "commitment"), values, proofs
        self.n, self.coset, self.cosets = int(n), int(coset), int(n) // int(coset)
        self._host = None

    def opening(self, k):
        """the Opening at omega^k (coset size 1) or the SetOpening at S_k, points in the order j = 0 .. l - 1"""
        k = int(k)
        if not 0 <= k < self.cosets:
            raise ValueError("coset %d: there are %d" % (k, self.cosets))
        if self._host is None:
            self._host = (ints32(_wire.host_bytes(self.values)), _wire.host_bytes(self.proofs))
        ys, pis = self._host
        omega, pi = root_of_unity(self.n), pis[32 * k:32 * k + 32]
        if self.coset == 1:
            return Opening(self.c, pow(omega, k, FR), ys[k], pi)
        at = [k + self.cosets * j for j in range(self.coset)]
        return SetOpening(self.c, [pow(omega, i, FR) for i in at], [ys[i] for i in at], pi)


class OpenAllKey:
    """One (n, l): the l tables X_v = ECFFT_2r(tau_g1[l (r - 1 - j) + v], j < r, then r points at infinity) in the
    prepared form of ozk_points_mac_dev, built on first use, and a CommitKey for the commitments."""

    def __init__(self, tau_g1, n, coset, commit_key):
        self.n, self.coset, self.cosets = int(n), int(coset), int(n) // int(coset)
        self._tau_g1, self._ck, self._tables = tau_g1, commit_key, None

    @staticmethod
    def from_srs(srs, n, coset=1, commit_key=None) -> "OpenAllKey":
        n, coset = int(n), int(coset)
        have = 2 * int(srs.m) + 1
        if n < 2 or n & (n - 1):
            raise ValueError("n = %d: a power of two >= 2" % n)
        if n > have:
            raise ValueError("n = %d: a string of m = %d carries %d powers in G1" % (n, srs.m, have))
        if coset not in ALL_COSETS or coset > n:
            raise ValueError("coset = %d: one of %s, at most n = %d" % (coset, ALL_COSETS, n))
        if 2 * (n // coset) > ALL_MAX_TRANSFORM:
            raise ValueError("n / coset = %d: the group FFT of twice that exceeds 2^22 points" % (n // coset))
        if commit_key is not None and commit_key.n != n:
            raise ValueError("the commit key has n = %d, not %d" % (commit_key.n, n))
        flat = srs.tau_g1.reshape(-1)
        return OpenAllKey(flat, n, coset, commit_key if commit_key is not None else CommitKey(flat, n, srs.m))

    def tables(self):
        """the prepared tables, l x 2r points (None for r = 1: the one proof is O)"""
        if self._tables is None and self.cosets > 1:
            l, r = self.coset, self.cosets
            powers = self._tau_g1[:96 * self.n].view(r, l, 96)              # power l i + v at [i, v]
            inf = torch.frombuffer(bytearray(_G1_INF_WIRE), dtype=torch.uint8).to(powers.device)
            x = torch.cat([powers.flip(0).transpose(0, 1), inf.expand(l, r, 96)], dim=1).contiguous()
            w2 = root_of_unity(2 * r)
            big = torch.cat([ec_fft(x[v].reshape(-1), G1, w2) for v in range(l)])
            self._tables = points_mac_prepare(big, l, 2 * r)
            torch.cuda.current_stream().synchronize()
        return self._tables

    # ---- the stages of one row (tools/kzg_all_bench.py times each)
    def values(self, row):
        """p(omega^i), i < n: one transform over Fr"""
        return fr_fft(row, self.n, root_of_unity(self.n))

    def coefficient_ffts(self, row):
        """c_v = FFT_2r(p[l i + v], i < r, then r zeros), v < l: l x 2r elements, term-major"""
        l, r = self.coset, self.cosets
        padded = torch.zeros((l, 2 * r, 32), dtype=torch.uint8, device=row.device)
        padded[:, :r] = row.view(r, l, 32).transpose(0, 1)
        out = torch.empty((l, 64 * r), dtype=torch.uint8, device=row.device)
        w2 = root_of_unity(2 * r)
        for v in range(l):
            fr_fft(padded[v].reshape(-1), 2 * r, w2, out[v])
        return out

    def mac(self, c):
        """U[i] = sum_v [c_v[i]] X_v[i], i < 2r"""
        return points_mac(self.tables(), c.reshape(-1), self.coset, 2 * self.cosets)

    def upper_half(self, u):
        """H = the upper half of the inverse group FFT of U (its last element is O by construction)"""
        return ec_fft(u, G1, root_of_unity(2 * self.cosets), inverse=True)[96 * self.cosets:].contiguous()

    def proofs_of(self, h):
        """(pi_0 .. pi_{r-1}) = ECFFT_r(H) with the root omega^l, as wire-in points"""
        return ec_fft(h, G1, root_of_unity(self.cosets))

    def open_all(self, coeffs) -> list:
        """K rows of n coefficients -> K AllOpenings.  No point leaves the device between the stages."""
        k, _, _ = _rows(coeffs, "coeffs", self.n)
        rows = _as2d(coeffs)
        commitments = self._ck.commit(coeffs)
        out = []
        for y in range(k):
            row = rows[y]
            if self.cosets == 1:
                proofs = torch.frombuffer(bytearray(_G1_INF), dtype=torch.uint8).to(row.device)
            else:
                h = self.upper_half(self.mac(self.coefficient_ffts(row)))
                proofs = _codec.compress_g1(self.proofs_of(h))
            out.append(AllOpenings(commitments[y], self.values(row), proofs, self.n, self.coset))
        return out


# ============================================================================ many polynomials, each at its own set (section 28)
MULTI_K_MAX, MULTI_SETS_MAX = 256, 32     # KZG_MULTI_ROWS, KZG_MULTI_GROUPS of csrc/kzg_multi.cuh
MULTI_EVAL_CALLS_T = 8                    # up to here t passes of ozk_fr_poly_eval_dev beat the set kernel (measured)
_MULTI_GAMMA_TAG = b"OZK-kzg-multi-gamma"
_MULTI_Z_TAG = b"OZK-kzg-multi-z"
_MULTI_RHO_TAG = b"OZK-kzg-multi-rho"


def _multi_sets(point_sets, what, k=None):
    """K tuples of t_i pairwise distinct ints in [0, r), 1 <= K <= 256 (k when the caller has K rows), 1 <= t_i <= 32"""
    if isinstance(point_sets, (int, str, bytes)) or not hasattr(point_sets, "__iter__"):
        raise TypeError("%s must be one list of points per row" % what)
    sets = list(point_sets)
    if k is not None and len(sets) != k:
        raise ValueError("%d lists of points for %d rows" % (len(sets), k))
    if not 1 <= len(sets) <= MULTI_K_MAX:
        raise ValueError("K = %d rows: 1 <= K <= %d" % (len(sets), MULTI_K_MAX))
    out = []
    for row in sets:
        if isinstance(row, (int, str, bytes)) or not hasattr(row, "__iter__"):
            raise ValueError("%s: one list of points per row, not a mix of lists and points" % what)
        row = tuple(row)
        if not 1 <= len(row) <= SET_T_MAX:
            raise ValueError("t = %d points: 1 <= t <= %d" % (len(row), SET_T_MAX))
        row = tuple(_wire.scalar_in_range(z, "%s: z" % what) for z in row)
        if len(set(row)) != len(row):
            raise ValueError("%s: z has repeated points in a set: %s" % (what, row))
        out.append(row)
    return out


def _multi_values(values, sets, what):
    """K tuples of t_i ints in [0, r), one value per point"""
    values = [tuple(row) for row in values]
    if len(values) != len(sets) or any(len(ys) != len(row) for ys, row in zip(values, sets)):
        raise ValueError("%s: the values are not one per point" % what)
    return [tuple(_wire.scalar_in_range(y, "%s: y" % what) for y in ys) for ys in values]


def _multi_groups(sets, limit=None):
    """(the distinct sets, smallest first and each as its first row wrote it; the group of every row): two rows are of
    one group when their sets hold the same points in any order"""
    first = {}
    for row in sets:
        first.setdefault(frozenset(row), row)
    if limit is not None and len(first) > limit:
        raise ValueError("%d distinct sets of points: at most %d" % (len(first), limit))
    keys = sorted(first, key=len)                                   # (stable: sets of one size stay in row order)
    index = {key: g for g, key in enumerate(keys)}
    return [first[key] for key in keys], [index[frozenset(row)] for row in sets]


def _multi_at(sets, values, groups, group_of, gamma, z):
    """What prover and verifier derive at z, in host integers: c_g = Z_{T \\ S_g}(z) per group (T the union of the
    sets; the empty product is 1), the weight gamma^i c_{g(i)} of every row, sum_i gamma^i c_{g(i)} r_i(z) for r_i the
    interpolant of row i's values on its set, and Z_T(z)"""
    union = list(dict.fromkeys(p for s in groups for p in s))

    def z_over(points):
        acc = 1
        for p in points:
            acc = acc * (z - p) % FR
        return acc

    c = [z_over([p for p in union if p not in s]) for s in map(frozenset, groups)]
    weights, at_z, g = [], 0, 1
    for row, ys, grp in zip(sets, values, group_of):
        weights.append(g * c[grp] % FR)
        r_at = 0
        for coeff in reversed(_interpolant(row, ys)):
            r_at = (r_at * z + coeff) % FR
        at_z = (at_z + weights[-1] * r_at) % FR
        g = g * gamma % FR
    return c, weights, at_z, z_over(union)


def _multi_gamma(commitments, sets, values) -> tuple:
    """(gamma, the digest D that z is drawn over) of checked arguments"""
    parts = [len(sets).to_bytes(8, "little")]
    for c, row, ys in zip(commitments, sets, values):
        parts += [len(row).to_bytes(8, "little"), le32(row), c, le32(ys)]
    return _transcript.challenge128(_MULTI_GAMMA_TAG, *parts), _transcript.digest(_MULTI_GAMMA_TAG, *parts)


def _multi_z(digest, w) -> int:
    return _transcript.challenge128(_MULTI_Z_TAG, digest, w)


def multi_challenges(commitments, point_sets, values, w) -> tuple:
    """(gamma, z).  gamma: the first 16 bytes, little-endian, of D = SHA-256("OZK-kzg-multi-gamma" | K as 8 bytes LE |
    per row: t_i as 8 bytes LE, its t_i points, its compressed commitment, its t_i values); z: the first 16 bytes of
    SHA-256("OZK-kzg-multi-z" | D | the compressed W); either is 1 if those bytes are zero"""
    commitments = [_enc_of(c, "commitment") for c in commitments]
    sets = _multi_sets(point_sets, "point_sets", len(commitments))
    gamma, digest = _multi_gamma(commitments, sets, _multi_values(values, sets, "values"))
    return gamma, _multi_z(digest, _enc_of(w, "W"))


class MultiOpening:
    """K uint32 LE | per row: C 32 | t uint32 LE | z 32 t | y 32 t | then W 32 | W' 32: the compressed commitments, every
    row's points and the values at them, and the two compressed proof points"""

    def __init__(self, commitments, point_sets, values, w, w2):
        self.commitments = tuple(_enc_of(c, "multi opening: C") for c in commitments)
        self.point_sets = tuple(_multi_sets(point_sets, "multi opening", len(self.commitments)))
        self.values = tuple(_multi_values(values, self.point_sets, "multi opening"))
        self.w, self.w2 = _enc_of(w, "multi opening: W"), _enc_of(w2, "multi opening: W'")

    @property
    def k(self):
        return len(self.commitments)

    def to_bytes(self) -> bytes:
        rows = [c + len(zs).to_bytes(4, "little") + le32(zs) + le32(ys)
                for c, zs, ys in zip(self.commitments, self.point_sets, self.values)]
        return self.k.to_bytes(4, "little") + b"".join(rows) + self.w + self.w2

    @staticmethod
    def from_bytes(b) -> "MultiOpening":
        """Strict and host-only: ValueError naming the field for a wrong length, K outside [1, 256], a t outside
        [1, 32], z or y >= r, a repeated point within a row, a point that does not decode."""
        b = bytes(b)
        if len(b) < 4:
            raise ValueError("multi opening: length %d, too short for K" % len(b))
        k = int.from_bytes(b[:4], "little")
        if not 1 <= k <= MULTI_K_MAX:
            raise ValueError("multi opening: K = %d, not in [1, %d]" % (k, MULTI_K_MAX))
        at, cs, sets, values = 4, [], [], []
        for i in range(k):
            if len(b) < at + 36:
                raise ValueError("multi opening: length %d, too short for C and t of row %d" % (len(b), i))
            t = int.from_bytes(b[at + 32:at + 36], "little")
            if not 1 <= t <= SET_T_MAX:
                raise ValueError("multi opening: t = %d in row %d, not in [1, %d]" % (t, i, SET_T_MAX))
            if len(b) < at + 36 + 64 * t:
                raise ValueError("multi opening: length %d, too short for the %d points of row %d" % (len(b), t, i))
            cs.append(b[at:at + 32])
            sets.append(ints32(b[at + 36:at + 36 + 32 * t]))
            values.append(ints32(b[at + 36 + 32 * t:at + 36 + 64 * t]))
            at += 36 + 64 * t
        if len(b) != at + 64:
            raise ValueError("multi opening: length %d, not %d for these K and t" % (len(b), at + 64))
        for name, rows in (("z", sets), ("y", values)):
            if any(v >= FR for row in rows for v in row):
                raise ValueError("multi opening: %s is not below r" % name)
        if any(len(set(row)) != len(row) for row in sets):
            raise ValueError("multi opening: z has repeated points")
        fields = [("C[%d]" % i, c, G1) for i, c in enumerate(cs)] + [("W", b[at:at + 32], G1), ("W'", b[at + 32:], G1)]
        _codec.require_points(fields, "multi opening")
        return MultiOpening(cs, sets, values, b[at:at + 32], b[at + 32:])


def poly_eval_set(coeffs, k, n, stride, sets):
    """ozk_fr_poly_eval_set_dev on k rows, row y at the t points sets[y] (which may repeat): values [32 k t] on the
    device.  Synchronises (the workspace dies here)."""
    L = _lib.load()
    t = len(sets[0])
    values = torch.empty(32 * k * t, dtype=torch.uint8, device=coeffs.device)
    wsb = int(L.ozk_fr_poly_eval_set_workspace_bytes(k, n, t))
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=coeffs.device)
    pts = le32([z for row in sets for z in row])
    _lib.check(L.ozk_fr_poly_eval_set_dev(_ptr(coeffs), k, n, stride, t, vp(pts), _ptr(values), _ptr(ws), ws.numel(),
                                          _stream()))
    torch.cuda.current_stream().synchronize()
    return values


def poly_eval_points(coeffs, k, n, stride, points):
    """every one of k rows at every point: one ozk_fr_poly_eval_dev call per point -> per point, the k values as ints"""
    L = _lib.load()
    out = torch.empty(32 * k * len(points), dtype=torch.uint8, device=coeffs.device)
    ws = torch.empty(max(int(L.ozk_fr_poly_eval_workspace_bytes(k)), 256), dtype=torch.uint8, device=coeffs.device)
    for i, z in enumerate(points):
        _lib.check(L.ozk_fr_poly_eval_dev(_ptr(coeffs), k, n, stride, vp(le32([z])), _ptr(out[32 * k * i:]), _ptr(ws),
                                          ws.numel(), _stream()))
    ys = ints32(_wire.host_bytes(out))
    return [ys[k * i:k * (i + 1)] for i in range(len(points))]


def rows_combine_groups(rows, k, n, stride, weights, group_of, groups, out, out_stride):
    """out[g] = sum_{i : group_of[i] = g} w_i rows[i] for g < groups (ozk_fr_rows_combine_groups_dev)"""
    L = _lib.load()
    w = _wire.dev_bytes(le32(weights))
    ids = b"".join(int(g).to_bytes(4, "little", signed=True) for g in group_of)
    _lib.check(L.ozk_fr_rows_combine_groups_dev(_ptr(rows), k, n, stride, _ptr(w), vp(ids), groups, _ptr(out), out_stride,
                                                _stream()))
    torch.cuda.current_stream().synchronize()
    return out


def _multi_terms(o):
    """the scalars of one opening's check: (of every C_i, of g1, of W, of W')"""
    gamma, z = multi_challenges(o.commitments, o.point_sets, o.values, o.w)
    groups, group_of = _multi_groups(o.point_sets)
    _, weights, at_z, z_t = _multi_at(o.point_sets, o.values, groups, group_of, gamma, z)
    return weights, (FR - at_z) % FR, (FR - z_t) % FR, z


def _multi_opening(o):
    return o if isinstance(o, MultiOpening) else MultiOpening.from_bytes(o)


def verify_multi(vk, opening) -> bool:
    """With F = sum_i gamma^i c_{g(i)} C_i - [sum_i gamma^i c_{g(i)} r_i(z)] g1 - [Z_T(z)] W:
        e(F + [z] W', g2) e(-W', tau_g2) = 1
    as one G1 MSM of K + 3 points (the C_i, g1, W, W') and one product of two pairings, over the plain VerifyKey;
    everything else is host integers.  Both G1 points O is accepted, one of them alone is not."""
    o = _multi_opening(opening)
    k = o.k
    pts = _decoded(list(o.commitments) + [o.w, o.w2])
    if pts is None:
        return False
    weights, s_g1, s_w, z = _multi_terms(o)
    lhs, ws = _vectors.msm(torch.cat([pts[:96 * k], vk.points()[0], pts[96 * k:]]),
                           _wire.dev_bytes(le32(weights + [s_g1, s_w, z])), k + 3)
    ok = _pairing_holds(lhs, pts[96 * (k + 1):], o.w2 == _G1_INF, vk)
    del ws
    return ok


def verify_multi_all(vk, openings, seed=None) -> bool:
    """All M openings at once with weights rho_m in [1, 2^128) (the stream of transcript.py under this module's multi
    tag; `seed` as verify_all):
        e(sum_m rho_m (F_m + [z_m] W'_m), g2) e(-sum_m rho_m W'_m, tau_g2) = 1
    as one G1 MSM over every commitment, W and W' of the batch and g1, one of the M points W'_m, and one product of
    two pairings."""
    os_ = [_multi_opening(o) for o in openings]
    if not os_:
        return True
    seed = secrets.token_bytes(32) if seed is None else _transcript.seed_bytes(seed)
    rho = ints32(_transcript.weights(seed, len(os_), _MULTI_RHO_TAG))
    pts = _decoded([c for o in os_ for c in o.commitments] + [o.w for o in os_] + [o.w2 for o in os_])
    if pts is None:
        return False
    sc_c, sc_w, sc_w2, sc_g1 = [], [], [], 0
    for r, o in zip(rho, os_):
        weights, s_g1, s_w, z = _multi_terms(o)
        sc_c += [r * x % FR for x in weights]
        sc_w.append(r * s_w % FR)
        sc_w2.append(r * z % FR)
        sc_g1 = (sc_g1 + r * s_g1) % FR
    total = len(sc_c) + 2 * len(os_)
    lhs, ws1 = _vectors.msm(torch.cat([pts, vk.points()[0]]), _wire.dev_bytes(le32(sc_c + sc_w + sc_w2 + [sc_g1])),
                            total + 1)
    ps, ws2 = _vectors.msm(pts[96 * (total - len(os_)):], _wire.dev_bytes(le32(rho)), len(os_))
    ok = _pairing_holds(lhs, wire_out_to_in(ps, G1), _wire.is_inf_out(ps), vk)
    del ws1, ws2
    return ok


def verify_multi_each(vk, openings, seed=None) -> list:
    """One verdict per opening: the batch check first, single checks only when it fails"""
    openings = list(openings)
    if verify_multi_all(vk, openings, seed):
        return [True] * len(openings)
    return [verify_multi(vk, o) for o in openings]
