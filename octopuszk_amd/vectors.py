"""One-call wrappers of the library's vector entry points over points and over Fr (include/ozk.h): uint8 CUDA tensors
in, uint8 CUDA tensors out, on the current stream.  There is no CPU path."""
import ctypes

import torch

from . import codec as _codec
from . import lib as _lib
from . import pairing as _pairing
from . import wire as _wire
from .device import VarMsmWorkspace, _ptr, _stream
from .fft import FR

G1, G2 = 1, 2
_GT_ONE = (1).to_bytes(32, "little") + bytes(352)


# ---------------------------------------------------------------------------- points
def scale_points(points, k, type_) -> torch.Tensor:
    """[k] P for every wire-in point P of `points` (a uint8 CUDA tensor, n x 96 bytes for type_ 1 = G1, n x 192 for
    2 = G2, any Z) and one int k in [0, r): n wire-in points with Z = 1, infinity as (0, 1, 0) / ((0, 0), (1, 0),
    (0, 0)).  Exact for every point of the curve (of the twist, inside the order-r subgroup or not).  Asynchronous on
    the current stream."""
    k = _wire.scalar_in_range(k, "the scalar")
    if type_ not in (G1, G2):
        raise ValueError("type_ must be 1 (G1) or 2 (G2)")
    L = _lib.load()
    n = _wire.count(points, 96 * type_, "points")
    points = points.contiguous()
    out = torch.empty_like(points)
    kb = (ctypes.c_uint8 * 32).from_buffer_copy(k.to_bytes(32, "little"))   # read before the call returns
    _lib.check(L.ozk_points_scale_dev(_ptr(points), n, type_, ctypes.cast(kb, ctypes.c_void_p), _ptr(out), _stream()))
    return out


def mul_points(points, scalars, type_, codes=False):
    """[k_i] P_i for the n wire-in points of `points` and the n scalars of `scalars` (n x 32 bytes little-endian on
    the device, as ozk_fr_powers_dev writes them): n wire-in points with Z = 1 (ozk_points_mul_dev).  A scalar >= r
    gives infinity for that point alone; codes=True returns (points, n int32 codes), 1 for such a point.  Exact for
    every point of the curve or twist.  Asynchronous on the current stream."""
    if type_ not in (G1, G2):
        raise ValueError("type_ must be 1 (G1) or 2 (G2)")
    for t, what in ((points, "points"), (scalars, "scalars")):
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.uint8):
            raise ValueError("%s must be a uint8 tensor" % what)
    rec = 96 * type_
    if points.numel() == 0 or points.numel() % rec:
        raise ValueError("points: %d bytes are not a whole number of %d-byte records" % (points.numel(), rec))
    n = points.numel() // rec
    if scalars.numel() != 32 * n:
        raise ValueError("%d points need %d bytes of scalars, not %d" % (n, 32 * n, scalars.numel()))
    L = _lib.load()
    _wire.count(points, rec, "points")
    _wire.count(scalars, 32, "scalars")
    points, scalars = points.contiguous(), scalars.contiguous()
    out = torch.empty_like(points)
    d_codes = torch.empty(n, dtype=torch.int32, device=points.device) if codes else None
    _lib.check(L.ozk_points_mul_dev(_ptr(points), _ptr(scalars), n, type_, _ptr(out),
                                    None if d_codes is None else _ptr(d_codes), _stream()))
    return (out, d_codes) if codes else out


def ec_fft(points, type_, omega, inverse=False) -> torch.Tensor:
    """The radix-2 transform of n = 2^k wire-in points in the exponent (ozk_ec_fft_dev): out[j] = sum_i
    [omega^(i j)] in[i]; inverse=True uses omega^-1 and multiplies by 1 / n.  A new tensor, Z = 1."""
    L = _lib.load()
    points = points.contiguous()
    n = _wire.count(points, 96 * type_, "points")
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
    n = _wire.count(a, 96 * type_, "points")
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


def points_mac_prepare(points, terms, n):
    """terms x n wire-in G1 points, term-major -> the prepared table of ozk_points_mac_dev (ozk_points_mac_prepare_dev).
    Asynchronous on the current stream."""
    L = _lib.load()
    points = points.contiguous()
    if _wire.count(points, 96, "points") != terms * n:
        raise ValueError("%d x %d points need %d bytes, not %d" % (terms, n, 96 * terms * n, points.numel()))
    nbytes = int(L.ozk_points_mac_prepared_bytes(terms, n, G1))
    table = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=points.device)
    _lib.check(L.ozk_points_mac_prepare_dev(_ptr(points), terms, n, G1, _ptr(table), table.numel(), _stream()))
    return table


def points_mac(table, scalars, terms, n, codes=False, workspace=None):
    """out[i] = sum_v [k_v[i]] P_v[i] over a prepared table and terms x n scalars (32 bytes little-endian, term-major,
    on the device): n wire-in points, Z = 1 (ozk_points_mac_dev); codes=True returns (points, n int32 codes), 1 for a
    lane with a scalar >= r.  Asynchronous on the current stream when the caller passes (and keeps) the workspace,
    else it synchronises: the workspace dies here."""
    L = _lib.load()
    scalars = scalars.contiguous()
    if scalars.numel() != 32 * terms * n:
        raise ValueError("%d x %d scalars need %d bytes, not %d" % (terms, n, 32 * terms * n, scalars.numel()))
    out = torch.empty(96 * n, dtype=torch.uint8, device=scalars.device)
    d_codes = torch.empty(n, dtype=torch.int32, device=scalars.device) if codes else None
    ws = workspace
    if ws is None:
        ws = torch.empty(max(int(L.ozk_points_mac_workspace_bytes(terms, n, G1)), 256), dtype=torch.uint8,
                         device=scalars.device)
    _lib.check(L.ozk_points_mac_dev(_ptr(table), _ptr(scalars), terms, n, G1, _ptr(out),
                                    None if d_codes is None else _ptr(d_codes), _ptr(ws), ws.numel(), _stream()))
    if workspace is None:
        torch.cuda.current_stream().synchronize()
    return (out, d_codes) if codes else out


def msm(bases, d_scalars, n, type_=1):
    """sum s_i P_i over n wire-in points through ozk_var_msm_dev: one wire-out point (192 bytes for G1, 384 for G2);
    the workspace is returned too, to be kept until the stream has run"""
    ws = VarMsmWorkspace(n, type_)
    return ws.run(bases.contiguous(), d_scalars), ws


def in_subgroup_g2(points, encodings: bytes) -> bool:
    """every G2 point of `points` (finite or not) satisfies [r - 1] P = -P: the same x, the other y (no twist point
    has y = 0), O for O"""
    minus = _wire.host_bytes(_codec.compress_g2(scale_points(points, FR - 1, G2)))
    want = bytearray(encodings)
    for i in range(63, len(want), 64):
        if not want[i] & 0x40:
            want[i] ^= 0x80
    return minus == bytes(want)


def pairs_are_one(p_batch, q_batch) -> bool:
    return _wire.host_bytes(_pairing.pairing_product(p_batch, q_batch)) == _GT_ONE


# ---------------------------------------------------------------------------- Fr
def fr_fft(values, n, omega, out=None):
    """The transform of n = 2^k elements of Fr (32 bytes little-endian each) on the device: out[j] = sum_i
    omega^(i j) in[i], canonical (ozk_fft_compact_dev).  Synchronises (the workspace dies here)."""
    L = _lib.load()
    if out is None:
        out = torch.empty(32 * n, dtype=torch.uint8, device=values.device)
    ws = torch.empty(max(int(L.ozk_fft_workspace_bytes(n)), 256), dtype=torch.uint8, device=values.device)
    _lib.check(L.ozk_fft_compact_dev(_ptr(values), n, _wire.vp(_wire.le32([omega])), _ptr(out), _ptr(ws), ws.numel(),
                                     _stream()))
    torch.cuda.current_stream().synchronize()
    return out


def fr_poly_eval(coeffs, r, npolys=1):
    """sum_i c_yi r^i for npolys polynomials of equal length stored back to back in a uint8 CUDA tensor (32-byte LE
    coefficients, any 256-bit word: reduced mod r on load): a CUDA tensor of npolys x 32 canonical bytes."""
    L = _lib.load()
    total = coeffs.numel() // 32
    if coeffs.numel() % 32 or total % npolys or total == 0:
        raise ValueError("coefficients do not split into %d polynomials" % npolys)
    length = total // npolys
    out = torch.empty(npolys * 32, dtype=torch.uint8, device=coeffs.device)
    ws = torch.empty(int(L.ozk_fr_poly_eval_workspace_bytes(npolys)), dtype=torch.uint8, device=coeffs.device)
    rb = (int(r) % FR).to_bytes(32, "little")
    _lib.check(L.ozk_fr_poly_eval_dev(_ptr(coeffs), npolys, length, length, _wire.vp(rb), _ptr(out), _ptr(ws),
                                      ws.numel(), _stream()))
    return out


def fr_rows_coset(rows, k, length, stride, s, c=1, out=None, out_len=None, out_stride=None):
    """out[y][i] = c s^i rows[y][i] for i < length, zero up to out_len (ozk_fr_rows_coset_dev): k rows at `stride`
    elements -> k rows of out_len (default length) at out_stride (default out_len), new ones unless `out` is given;
    out may be `rows` itself when the lengths and strides agree.  Synchronises (the workspace dies here)."""
    L = _lib.load()
    out_len = length if out_len is None else int(out_len)
    out_stride = out_len if out_stride is None else int(out_stride)
    if out is None:
        out = torch.empty((k, 32 * out_stride), dtype=torch.uint8, device=rows.device)
    ws = torch.empty(max(int(L.ozk_fr_rows_coset_workspace_bytes(k, length, out_len)), 256), dtype=torch.uint8,
                     device=rows.device)
    _lib.check(L.ozk_fr_rows_coset_dev(_ptr(rows), k, length, stride, _wire.vp(_wire.le32([int(s) % FR])),
                                       _wire.vp(_wire.le32([int(c) % FR])), _ptr(out), out_len, out_stride, _ptr(ws),
                                       ws.numel(), _stream()))
    torch.cuda.current_stream().synchronize()
    return out


def fr_perm_product(wires, sigma, length, stride, omega, ks, beta, gamma):
    """The permutation grand product of three wire rows and three sigma rows of `length` elements at `stride`
    (ozk_fr_perm_product_dev; cell (j, i) has the identity label ks[j] omega^i): (z, `length` x 32 bytes on the device
    with z[0] = 1; the product over all rows as an int; the number of rows with a zero denominator).  Synchronises."""
    L = _lib.load()
    z = torch.empty(32 * length, dtype=torch.uint8, device=wires.device)
    tail = torch.empty(48, dtype=torch.uint8, device=wires.device)         # the total, then the count
    ws = torch.empty(max(int(L.ozk_fr_perm_product_workspace_bytes(length)), 256), dtype=torch.uint8, device=wires.device)
    le = lambda vs: _wire.vp(_wire.le32([int(v) % FR for v in vs]))
    _lib.check(L.ozk_fr_perm_product_dev(_ptr(wires), _ptr(sigma), length, stride, le([omega]), le(ks), le([beta]),
                                         le([gamma]), _ptr(z), _ptr(tail), _ptr(tail[32:]), _ptr(ws), ws.numel(),
                                         _stream()))
    host = _wire.host_bytes(tail)
    return z, int.from_bytes(host[:32], "little"), int.from_bytes(host[32:36], "little", signed=True)


def plonk_quotient(wit, wit_stride, key, key_stride, n, alpha, beta, gamma, ks, zh_inv, out=None):
    """t on the coset of 4 n points from the five witness rows and the ten key rows (ozk_plonk_quotient_dev): 4 n x 32
    bytes on the device, a new tensor unless `out` is given.  Asynchronous on the current stream."""
    L = _lib.load()
    if out is None:
        out = torch.empty(32 * 4 * n, dtype=torch.uint8, device=wit.device)
    le = lambda vs: _wire.vp(_wire.le32([int(v) % FR for v in vs]))
    _lib.check(L.ozk_plonk_quotient_dev(_ptr(wit), wit_stride, _ptr(key), key_stride, n, le([alpha]), le([beta]),
                                        le([gamma]), le(ks), le(zh_inv), _ptr(out), _stream()))
    return out


def plonk_lookup_index(table, n_rows, table_stride):
    """The index of a lookup table's first n_rows tuples (ozk_plonk_lookup_index_dev; table: the rows T1, T2, T3 at
    table_stride): uint32 row numbers on the device, built once per key.  Asynchronous on the current stream."""
    L = _lib.load()
    index = torch.empty(max(int(L.ozk_plonk_lookup_index_bytes(n_rows)), 16), dtype=torch.uint8, device=table.device)
    _lib.check(L.ozk_plonk_lookup_index_dev(_ptr(table), n_rows, table_stride, _ptr(index), index.numel(), _stream()))
    return index


def plonk_lookup_counts(wires, qk, length, stride, table, n_rows, table_stride, index, m_len):
    """How often the rows with qK != 0 name each table row (ozk_plonk_lookup_counts_dev): (m, m_len x 32 bytes on the
    device; the number of rows whose tuple is in no table row; the first of them, or None).  Synchronises."""
    L = _lib.load()
    m = torch.empty(32 * m_len, dtype=torch.uint8, device=wires.device)
    tail = torch.empty(16, dtype=torch.uint8, device=wires.device)         # missing, then first_missing
    _lib.check(L.ozk_plonk_lookup_counts_dev(_ptr(wires), _ptr(qk), length, stride, _ptr(table), n_rows, table_stride,
                                             _ptr(index), index.numel(), _ptr(m), m_len, _ptr(tail), _ptr(tail[4:]),
                                             _stream()))
    host = _wire.host_bytes(tail)
    missing = int.from_bytes(host[:4], "little", signed=True)
    return m, missing, int.from_bytes(host[4:8], "little", signed=True) if missing else None


def plonk_lookup_sum(wires, stride, key4, key_stride, m, length, eta, theta):
    """The running sum of the lookup argument over three wire rows, the key rows qK, T1, T2, T3 and the counts m
    (ozk_plonk_lookup_sum_dev): (S, `length` x 32 bytes on the device with S[0] = 0; the sum over all rows as an int;
    the number of zero denominators).  Synchronises."""
    L = _lib.load()
    s = torch.empty(32 * length, dtype=torch.uint8, device=wires.device)
    tail = torch.empty(48, dtype=torch.uint8, device=wires.device)         # the total, then the count
    ws = torch.empty(max(int(L.ozk_plonk_lookup_sum_workspace_bytes(length)), 256), dtype=torch.uint8, device=wires.device)
    le = lambda vs: _wire.vp(_wire.le32([int(v) % FR for v in vs]))
    _lib.check(L.ozk_plonk_lookup_sum_dev(_ptr(wires), stride, _ptr(key4), key_stride, _ptr(m), length, le([eta]),
                                          le([theta]), _ptr(s), _ptr(tail), _ptr(tail[32:]), _ptr(ws), ws.numel(),
                                          _stream()))
    host = _wire.host_bytes(tail)
    return s, int.from_bytes(host[:32], "little"), int.from_bytes(host[32:36], "little", signed=True)


def plonk_quotient_lookup(wit, wit_stride, key, key_stride, n, alpha, beta, gamma, ks, zh_inv, eta, theta, out=None):
    """t on the coset of 4 n points from the seven witness rows and the fourteen key rows of a circuit with lookups
    (ozk_plonk_quotient_lookup_dev): 4 n x 32 bytes on the device.  Asynchronous on the current stream."""
    L = _lib.load()
    if out is None:
        out = torch.empty(32 * 4 * n, dtype=torch.uint8, device=wit.device)
    le = lambda vs: _wire.vp(_wire.le32([int(v) % FR for v in vs]))
    _lib.check(L.ozk_plonk_quotient_lookup_dev(_ptr(wit), wit_stride, _ptr(key), key_stride, n, le([alpha]), le([beta]),
                                               le([gamma]), le(ks), le(zh_inv), le([eta]), le([theta]), _ptr(out),
                                               _stream()))
    return out


def fr_term_sums(index, coeff, vec, n_vec, terms, out, bad, workspace=None):
    """out[t] = sum_{u <= t} coeff[u] vec[index[u]], t < terms (ozk_fr_term_sums_dev): index `terms` uint32 on the
    device, coeff their coefficients in the form c 2^261 mod r or None (every one is 1), vec n_vec elements, out
    `terms` x 32 bytes, bad an int32 on the device that receives the number of indices >= n_vec.  Asynchronous on the
    current stream over a `workspace` of the caller's; without one, synchronises (the workspace dies here)."""
    L = _lib.load()
    ws = workspace
    if ws is None:
        ws = torch.empty(max(int(L.ozk_fr_term_sums_workspace_bytes(terms)), 256), dtype=torch.uint8, device=vec.device)
    _lib.check(L.ozk_fr_term_sums_dev(_ptr(index), None if coeff is None else _ptr(coeff), _ptr(vec), n_vec, terms,
                                      _ptr(out), _ptr(bad), _ptr(ws), ws.numel(), _stream()))
    if workspace is None:
        torch.cuda.current_stream().synchronize()
    return out


def plonk_wires(src, n_src, cells, k, length, cell_stride, bad, out=None, out_stride=None):
    """out[y][i] = src[hi] - src[lo], or src[hi] where lo = 0xFFFFFFFF, for k rows of `length` descriptors (hi, lo) of
    two uint32 at cell_stride (ozk_plonk_wires_dev): k rows at out_stride (default length), a new tensor unless `out`
    is given; bad an int32 on the device that receives the number of descriptors pointing outside src.  Asynchronous
    on the current stream."""
    L = _lib.load()
    out_stride = length if out_stride is None else int(out_stride)
    if out is None:
        out = torch.empty((k, 32 * out_stride), dtype=torch.uint8, device=src.device)
    _lib.check(L.ozk_plonk_wires_dev(_ptr(src), n_src, _ptr(cells), k, length, cell_stride, _ptr(out), out_stride,
                                     _ptr(bad), _stream()))
    return out


def fr_rows_blind(rows, k, n, stride, blinders):
    """In place on k coefficient rows at `stride` >= n + 4 elements (ozk_fr_rows_blind_dev): row y takes the blinders
    blinders[y] (a sequence of up to four ints), row[j] -= r_j and row[n + j] = r_j, which leaves its values on the
    domain of n points as they are.  Returns `rows`.  Asynchronous on the current stream."""
    L = _lib.load()
    if len(blinders) != k:
        raise ValueError("%d sequences of blinders for %d rows" % (len(blinders), k))
    counts = (ctypes.c_int32 * k)(*[len(row) for row in blinders])
    flat = _wire.le32([int(r) % FR for row in blinders for r in row]) or bytes(32)
    _lib.check(L.ozk_fr_rows_blind_dev(_ptr(rows), k, n, stride, _wire.vp(flat), ctypes.cast(counts, ctypes.c_void_p),
                                       _stream()))
    return rows


def plonk_quotient_split(t, n, out_stride, blinders, out=None):
    """The 4 n coefficients of a quotient -> (its three parts t_lo', t_mid', t_hi' as rows at out_stride >= n + 8
    elements, zero up to the stride and blinded by blinders = (u0, u1, v0, v1), a new [3, 32 out_stride] tensor unless
    `out` is given; how many of the coefficients from 3 n + 6 are not zero) (ozk_plonk_quotient_split_dev).
    Synchronises."""
    L = _lib.load()
    if len(blinders) != 4:
        raise ValueError("%d blinders of the quotient's parts, not 4" % len(blinders))
    if out is None:
        out = torch.empty((3, 32 * out_stride), dtype=torch.uint8, device=t.device)
    count = torch.empty(16, dtype=torch.uint8, device=t.device)
    _lib.check(L.ozk_plonk_quotient_split_dev(_ptr(t), n, _ptr(out), out_stride,
                                              _wire.vp(_wire.le32([int(r) % FR for r in blinders])), _ptr(count), _stream()))
    return out, int.from_bytes(_wire.host_bytes(count[:4]), "little", signed=True)


PLONK_VERIFY_K_MAX, PLONK_VERIFY_ROWS_MAX = 1 << 16, 1 << 24    # PLONK_VF_K_MAX, PLONK_VF_ROWS_MAX of csrc/plonk_verify.cuh
_PLONK_VERIFY_SHAPES = ((800, 264, 8, 7, 8), (1088, 392, 12, 9, 12))   # proof, key, record, NC, NKEY of kind 0 and 1


def _plonk_verify_buffers(kind, vk_bytes, n_public, proofs, public):
    proof_len, vk_len = _PLONK_VERIFY_SHAPES[kind][:2]
    if vk_bytes.numel() != vk_len:
        raise ValueError("a verifying key of %d bytes, not %d" % (vk_len, vk_bytes.numel()))
    k = _wire.count(proofs, proof_len, "proofs")
    have = 0 if public is None else public.numel()
    if have != 32 * n_public * k:
        raise ValueError("%d proofs need %d bytes of public inputs, not %d" % (k, 32 * n_public * k, have))
    return k, proofs.contiguous(), (public.contiguous() if have else None)


def plonk_verify_challenges(kind, vk_bytes, n, n_public, proofs, public, seed):
    """The transcripts of K proofs under one key (ozk_plonk_verify_challenges_dev): kind 0 vanilla, 1 with lookups;
    vk_bytes the key's bytes, proofs K x 800 (1088) bytes and public K x n_public x 32 bytes on the device (None when
    n_public = 0); seed: 32 bytes.  Returns [K, 8 (12), 32] bytes on the device: beta, gamma, [eta, theta,] alpha, z,
    the multi-opening's gamma and point, rho_m, zero padding.  Asynchronous on the current stream."""
    L = _lib.load()
    k, proofs, public = _plonk_verify_buffers(kind, vk_bytes, n_public, proofs, public)
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("the seed is 32 bytes, not %d" % len(seed))
    rec = _PLONK_VERIFY_SHAPES[kind][2]
    out = torch.empty((k, rec, 32), dtype=torch.uint8, device=proofs.device)
    _lib.check(L.ozk_plonk_verify_challenges_dev(kind, _ptr(vk_bytes.contiguous()), n, n_public, _ptr(proofs),
                                                 None if public is None else _ptr(public), k, _wire.vp(seed), _ptr(out),
                                                 _stream()))
    return out


def plonk_verify_scalars(kind, n, n_public, proofs, public, challenges, workspace=None):
    """The scalars of the batch check of K proofs from their challenge records (ozk_plonk_verify_scalars_dev):
    (scalars, K x NC + 2 K + NKEY + 1 elements in the order of the MSM's points; rho, K x 32 bytes; flags, K int32)
    on the device.  Asynchronous on the current stream over a `workspace` of the caller's; without one, synchronises
    (the workspace dies here)."""
    L = _lib.load()
    proof_len, _, rec, nc, nkey = _PLONK_VERIFY_SHAPES[kind]
    k = _wire.count(proofs, proof_len, "proofs")
    have = 0 if public is None else public.numel()
    if have != 32 * n_public * k or challenges.numel() != 32 * rec * k:
        raise ValueError("%d proofs need %d bytes of public inputs and %d of challenges" % (k, 32 * n_public * k, 32 * rec * k))
    proofs, challenges = proofs.contiguous(), challenges.contiguous()
    public = public.contiguous() if have else None
    dev = proofs.device
    scalars = torch.empty(32 * (k * (nc + 2) + nkey + 1), dtype=torch.uint8, device=dev)
    rho = torch.empty(32 * k, dtype=torch.uint8, device=dev)
    flags = torch.empty(k, dtype=torch.int32, device=dev)
    ws = workspace
    if ws is None:
        ws = torch.empty(max(int(L.ozk_plonk_verify_scalars_workspace_bytes(kind, k)), 256), dtype=torch.uint8, device=dev)
    _lib.check(L.ozk_plonk_verify_scalars_dev(kind, n, n_public, _ptr(proofs), None if public is None else _ptr(public),
                                              _ptr(challenges), k, _ptr(scalars), _ptr(rho), _ptr(flags), _ptr(ws),
                                              ws.numel(), _stream()))
    if workspace is None:
        torch.cuda.current_stream().synchronize()
    return scalars, rho, flags
