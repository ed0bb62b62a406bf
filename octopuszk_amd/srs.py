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

Out of scope: a file format for the string, phase-1 contributions (re-randomising tau, alpha, beta of an existing
string) and interoperability with other tools' .ptau files.  There is no CPU path.
"""
import ctypes
import hashlib
import time

import torch

from . import ceremony as _ceremony
from . import codec as _codec
from . import lib as _lib
from .device import VarMsmWorkspace, _ptr, _stream
from .fft import FR, root_of_unity

G1, G2 = 1, 2
CHECKS = ("shape", "powers_g1", "powers_g2", "alpha_powers", "beta_powers", "beta_g2")
_RHO_TAG = b"OZK-srs-rho"


def _count(t, type_):
    return t.numel() // (96 * type_)


def _point(t, i, type_):
    n = 96 * type_
    return t.reshape(-1)[n * i:n * (i + 1)]


def _weights(seed: bytes, n: int) -> bytes:
    """n weights in [1, 2^128) as n x 32 bytes little-endian: the SHA-256 counter stream of ceremony.py under this
    module's own tag"""
    out = bytearray(32 * n)
    pad = bytes(16)
    one = (1).to_bytes(16, "little")
    for j in range((n + 1) // 2):
        block = hashlib.sha256(_RHO_TAG + seed + j.to_bytes(8, "little")).digest()
        for half in (0, 1):
            i = 2 * j + half
            if i < n:
                w = block[16 * half:16 * half + 16]
                out[32 * i:32 * i + 32] = (w if w != pad else one) + pad
    return bytes(out)


def _msm(bases, d_scalars, n, type_):
    ws = VarMsmWorkspace(n, type_)
    return ws.run(bases.contiguous(), d_scalars), ws


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
        from . import zksnark as z
        from .fixed_base_msm import G1_WINDOW_TABLE, G2_WINDOW_TABLE, get_window_size
        m = int(m)
        if m < 2 or m & (m - 1):
            raise ValueError("the domain size must be a power of two >= 2, not %d" % m)
        tau, alpha, beta = (_ceremony._scalar(v, what, 1) for v, what in ((tau, "tau"), (alpha, "alpha"), (beta, "beta")))
        rnd = z.fr_random(z.SEED) if generator is None else _ceremony._scalar(generator, "generator", 1)
        L = _lib.load()
        gens = {G1: bytes(z.batch_msm_dev(254, 16, z.g1_wire(z.G1_ONE), [rnd], G1).cpu().numpy()),
                G2: bytes(z.batch_msm_dev(254, 16, z.g2_wire(z.G2_ONE), [rnd], G2).cpu().numpy())}

        def powers(k, n, type_):
            d_sc = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
            wsb = int(L.ozk_fr_powers_workspace_bytes(n))
            ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
            tb, kb = z._le32_one(tau), z._le32_one(k)
            _lib.check(L.ozk_fr_powers_dev(ctypes.cast(tb, ctypes.c_void_p), ctypes.cast(kb, ctypes.c_void_p), n,
                                           _ptr(d_sc), _ptr(ws), wsb, _stream()))
            torch.cuda.current_stream().synchronize()
            window = get_window_size(n, G1_WINDOW_TABLE if type_ == G1 else G2_WINDOW_TABLE)
            return z.batch_msm_dev(z._bit_size(gens[type_]), window, gens[type_], d_sc, type_)

        beta_g2 = z.batch_msm_dev(z._bit_size(gens[G2]), 16, gens[G2], [beta], G2)
        return Srs(m, powers(1, 2 * m + 1, G1), powers(1, m, G2), powers(alpha, m, G1), powers(beta, m, G1), beta_g2)

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
        from .zksnark import _dev_bytes, wire_out_to_in

        def no(name):
            if why is not None:
                why.append(name)
            return False

        m = self.m
        enc, scale, ones = _ceremony._enc, _ceremony.scale_points, _ceremony._pairs_are_one
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
        if not _in_subgroup(sub, e2[64:]):
            return no("shape")
        rho = _dev_bytes(_weights(_ceremony._seed_bytes(seed), 2 * m))
        keep = []

        def shift_g1(points, n, q_lo, q_hi):
            """sum rho_i points[i] =: S, sum rho_i points[i + 1] =: S', i < n: S != O and e(S', q_lo) e(-S, q_hi) = 1"""
            flat = points.reshape(-1)
            s_lo, w1 = _msm(flat[:96 * n], rho[:32 * n], n, G1)
            s_hi, w2 = _msm(flat[96:96 * (n + 1)], rho[:32 * n], n, G1)
            keep.extend((w1, w2))
            if _ceremony._is_inf_out(s_lo):
                return False
            neg = scale(wire_out_to_in(s_lo, G1), FR - 1, G1)
            return ones(torch.cat([wire_out_to_in(s_hi, G1), neg]), torch.cat([q_lo, q_hi]))

        # 2 powers_g1
        if not shift_g1(self.tau_g1, 2 * m, g2, tg2):
            return no("powers_g1")
        # 3 powers_g2
        if not _in_subgroup(self.tau_g2, enc(self.tau_g2, G2)):
            return no("powers_g2")
        flat = self.tau_g2.reshape(-1)
        t_lo, w1 = _msm(flat[:192 * (m - 1)], rho[:32 * (m - 1)], m - 1, G2)
        t_hi, w2 = _msm(flat[192:], rho[:32 * (m - 1)], m - 1, G2)
        if not bool(t_lo.view(6, 64)[4:].any().item()):
            return no("powers_g2")
        if not ones(torch.cat([g1, scale(tg1, FR - 1, G1)]), torch.cat([wire_out_to_in(t_hi, G2), wire_out_to_in(t_lo, G2)])):
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


def _in_subgroup(points, encodings: bytes) -> bool:
    """every G2 point of `points` (finite or not) satisfies [r - 1] P = -P: the same x, the other y (no twist point
    has y = 0), O for O"""
    minus = _ceremony._enc(_ceremony.scale_points(points, FR - 1, G2), G2)
    want = bytearray(encodings)
    for i in range(63, len(want), 64):
        if not want[i] & 0x40:
            want[i] ^= 0x80
    return minus == bytes(want)


# ---------------------------------------------------------------------------- point kernels
def ec_fft(points, type_, omega, inverse=False) -> torch.Tensor:
    """The radix-2 transform of n = 2^k wire-in points in the exponent (ozk_ec_fft_dev): out[j] = sum_i
    [omega^(i j)] in[i]; inverse=True uses omega^-1 and multiplies by 1 / n.  A new tensor, Z = 1."""
    L = _lib.load()
    points = points.contiguous()
    n = _codec._count(points, 96 * type_, "points")
    out = torch.empty_like(points)
    wsb = int(L.ozk_ec_fft_workspace_bytes(n, type_))
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=points.device)
    ob = (ctypes.c_uint8 * 32).from_buffer_copy(int(omega).to_bytes(32, "little"))
    _lib.check(L.ozk_ec_fft_dev(_ptr(points), n, type_, ctypes.cast(ob, ctypes.c_void_p), int(bool(inverse)), _ptr(out),
                                _ptr(ws), ws.numel(), _stream()))
    torch.cuda.current_stream().synchronize()    # the workspace dies here
    return out


def points_add(a, b, type_, negate_b=False) -> torch.Tensor:
    """a[i] + b[i], or a[i] - b[i]: n wire-in points, Z = 1 (ozk_points_add_dev).  Asynchronous on the current stream."""
    L = _lib.load()
    a, b = a.contiguous(), b.contiguous()
    n = _codec._count(a, 96 * type_, "points")
    if b.numel() != a.numel():
        raise ValueError("two vectors of one length")
    out = torch.empty_like(a)
    _lib.check(L.ozk_points_add_dev(_ptr(a), _ptr(b), n, type_, int(bool(negate_b)), _ptr(out), _stream()))
    return out


def sparse_mat_points(mat, points, type_) -> torch.Tensor:
    """mat (a zksnark._CsrDevice) times a vector of wire-in points: one point per row (ozk_sparse_mat_points_dev)"""
    L = _lib.load()
    points = points.contiguous()
    out = torch.empty(mat.rows * 96 * type_, dtype=torch.uint8, device=points.device)
    wsb = int(L.ozk_sparse_mat_points_workspace_bytes(mat.n_long, type_))
    ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=points.device)
    opt = lambda t: None if t is None else _ptr(t)
    _lib.check(L.ozk_sparse_mat_points_dev(_ptr(mat.ptr), _ptr(mat.idx), opt(mat.coeff), _ptr(points), mat.rows, type_,
                                           opt(mat.long), mat.n_long, _ptr(out), _ptr(ws), ws.numel(), _stream()))
    torch.cuda.current_stream().synchronize()    # the workspace dies here
    return out


# ---------------------------------------------------------------------------- the setup
def setup_from_srs(r1cs, srs: Srs, log=None):
    """The Groth16 key of `r1cs` instantiated at the tau of `srs`, with gamma = delta = 1 (the shape of Bowe, Gabizon
    and Miers; contribute / verify_chain then randomise delta), computed without tau, alpha or beta: four inverse
    transforms of the string into the Lagrange basis, sparse products with the transposed constraint matrices, and
    pointwise sums.  Returns a CRS with proving_key (and its .r1cs), gamma_g2, gamma_abc_g1, timing and secrets = None.
    ValueError when the string's m is not lowest_power_of_two(num_constraints + num_inputs), and when tau lies in the
    domain (tau^m = 1: tau_g1[m] equals tau_g1[0])."""
    from . import zksnark as z
    nc, ni, nv = r1cs.num_constraints, r1cs.num_inputs, r1cs.num_variables
    m = z.lowest_power_of_two(nc + ni)
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
        r1cs._transposed_dev = z.R1CSTransposedDevice(r1cs)
    At, Bt, Ct = r1cs._transposed_dev.mats
    t0 = lap("r1cs_transpose_once_host_s", t0)
    omega = root_of_unity(m)
    pk = z.ProvingKey()
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
    crs = z.CRS()
    crs.proving_key = pk
    crs.gamma_g2 = pk.delta_g2.clone()
    crs.gamma_abc_g1 = abc[:96 * ni].clone()
    crs.secrets = None
    crs.timing = tm
    if log:
        log("setup from a string: " + ", ".join("%s %.3f s" % (k[:-2], v) for k, v in tm.items()))
    return crs
