"""Driver, cases and exact-integer expectations for the pairing-tower conformance harness: tests/native/tower_ops.h,
compiled by hipcc into towercheck.hip (the device build: __noinline__ tower functions, arguments through the private
stack, 64 lanes per workgroup) and by g++ into towercheck_host.cpp (the host branch).  Shared by
test_tower_ops_cpu.py (host build; cross-compiles the device harness) and test_tower_ops_gpu.py (device build).

Operands and results are raw 9-limb Montgomery records per Fq component (devarith.py), in the GT wire order.  Every
expected value is pairing_ref.py's, on the operands taken out of the Montgomery domain: the tower is linear and
multiplicative, so op(a R, b R) = op(a, b) R, its constants included.  The one convention pairing_ref.py lacks is
zero -> zero for the inversions and the two final-exponentiation entries that invert.

Cases, for an element of m components (each below its bound B p / 16, B = 32 except for f2n):
  1. every component at the same edge record of devarith.element_records, for each edge record;
  2. one component at 1, p - 1, the largest value or the maximal limb vector, the others zero written alternately
     as 0 and as p, for every position;
  3. zero in every spelling (all 0, all p, alternating), then with one component at 1 or p + 1;
  4. one, as the Montgomery one and as that plus p;
  5. independent random components (a quarter of them in the top percent of the range).
The exponentiations take 128 cases, which 1. to 4. alone would fill at m = 12: they keep 1., 4., the zeros and the
true cyclotomic elements whole and spread the rest of half their cases evenly over 2. and 3."""
import ctypes
import functools
import os
import random
import subprocess

import numpy as np

import devarith as da
import pairing_ref as pr
from oracle import bn254 as o

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NATIVE = os.path.join(HERE, "native")
CSRC = os.path.join(ROOT, "octopuszk_amd", "csrc")
DEV_SRC = os.path.join(NATIVE, "towercheck.hip")
DEV_LIB = os.path.join(NATIVE, "_towercheck.so")
HOST_SRC = os.path.join(NATIVE, "towercheck_host.cpp")
HOST_LIB = os.path.join(NATIVE, "_towercheck_host.so")
SHARED = [os.path.join(NATIVE, f) for f in ("tower_ops.h", "devcheck_common.h")] + \
         [os.path.join(CSRC, f) for f in ("batch_verify.cuh", "fq12.cuh", "fq2.cuh", "fp29.cuh", "ec.cuh", "curve.cuh",
                                          "pairing_consts_gen.h", "consts_gen.h", "mad_chain_gen.h")]

Q = o.Q
F2 = o.Fq2Ops
N_CHEAP, N_SLOW, N_STORE = 1024, 128, 193
LANES_CHEAP, LANES_SLOW = 4096, 1024
SLOW = ("exp_by_neg_z", "final_exp_first_chunk", "final_exp_last_chunk", "final_exponentiation", "gt_pow")


def build_device(force=False):
    """cross-compile the device harness for gfx950 with the library's flags; rebuilt only when missing or stale"""
    from octopuszk_amd import build as b
    if force or b._newer(DEV_LIB, [DEV_SRC] + SHARED):
        subprocess.check_call([b.hipcc()] + b.HIPCC_FLAGS + ["-shared", "-o", DEV_LIB, DEV_SRC])
    return DEV_LIB


def build_host(force=False):
    from octopuszk_amd import build as b
    if force or b._newer(HOST_LIB, [HOST_SRC] + SHARED):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-maybe-uninitialized", "-Wno-unknown-pragmas",
                               "-shared", "-fPIC", "-o", HOST_LIB, HOST_SRC])
    return HOST_LIB


def _proto(lib):
    lib.tc_info.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
    lib.tc_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                           ctypes.c_void_p]
    return lib


_libs = {}


def load_host():
    if "host" not in _libs:
        _libs["host"] = _proto(ctypes.CDLL(build_host()))
    return _libs["host"]


def load_device():
    if "device" not in _libs:
        # torch first: device pointers from torch are valid only in the HIP runtime torch loaded (devarith.load())
        import torch  # noqa: F401
        _libs["device"] = _proto(ctypes.CDLL(build_device()))
    return _libs["device"]


class OpInfo:
    def __init__(self, idx, name, v, scratch):
        self.idx, self.name, self.scratch = idx, name, scratch
        nin, nout, self.kp = v[1], v[2], v[3]
        self.ins = list(zip(v[4:4 + nin], v[4 + nin:4 + 2 * nin]))             # (B, LU) per operand component
        self.outs = list(zip(v[4 + 2 * nin:4 + 2 * nin + nout], v[4 + 2 * nin + nout:4 + 2 * nin + 2 * nout]))
        self.id = name if not self.kp else "%s<%d>" % (name, self.kp)


def ops(lib):
    out = []
    for i in range(lib.tc_count()):
        name = ctypes.create_string_buffer(64)
        v = (ctypes.c_int * 128)()
        assert lib.tc_info(i, name, v) == 0
        out.append(OpInfo(i, name.value.decode(), list(v), lib.tc_scratch(i)))
    return out


# ---------------------------------------------------------------- values: flat component lists <-> pairing_ref's nesting
SIZE = {"fq": 1, "f2": 2, "f6": 6, "f12": 12, "ell": 6, "g2p": 6}


def nest(kind, v):
    """flat list of Fq integers -> pairing_ref's tuples (ell and g2p: three Fq2, like an Fq6)"""
    if kind == "fq":
        return v[0]
    if kind == "f2":
        return (v[0], v[1])
    if kind == "f12":
        return (nest("f6", v[:6]), nest("f6", v[6:]))
    return tuple((v[2 * j], v[2 * j + 1]) for j in range(3))


def flat(x):
    if isinstance(x, int):
        return [x]
    return [c for y in x for c in flat(y)]


def demont(rec):
    return da.from_limbs(rec) * da.RQI % Q


F12_ZERO = pr.F12_ZERO


def f2_inv0(a):
    return a if a == F2.zero else F2.inv(a)


def f6_inv0(a):
    return a if a == pr.F6_ZERO else pr.f6_inv(a)


def f12_inv0(a):
    return a if a == F12_ZERO else pr.f12_inv(a)


def _step(new, ell):
    return flat(ell) + flat(new)


# name -> (operand kinds, function of the operands (out of the Montgomery domain) and the op's parameter giving the flat
# list of expected output components).  Kinds "expo" (a plain integer) and "wire12" are handled in cases_for().
OPS = {
    "mul_xi": (["f2"], lambda k, a: pr.mul_xi(a)),
    "f2_conj": (["f2"], lambda k, a: pr.f2_frob(a, 1)),
    "f2_neg": (["f2"], lambda k, a: F2.neg(a)),
    "f2_add": (["f2", "f2"], lambda k, a, b: F2.add(a, b)),
    "f2_sub": (["f2", "f2"], lambda k, a, b: F2.sub(a, b)),
    "f2n": (["f2"], lambda k, a: a),
    "f6_add": (["f6", "f6"], lambda k, a, b: pr.f6_add(a, b)),
    "f6_sub": (["f6", "f6"], lambda k, a, b: pr.f6_sub(a, b)),
    "f6_neg": (["f6"], lambda k, a: pr.f6_neg(a)),
    "f6_mul": (["f6", "f6"], lambda k, a, b: pr.f6_mul(a, b)),
    "f6_mul_f2": (["f6", "f2"], lambda k, a, b: pr.f6_mul_f2(a, b)),
    "f6_sqr": (["f6"], lambda k, a: pr.f6_sqr(a)),
    "f6_inv": (["f6"], lambda k, a: f6_inv0(a)),
    "f6_frobenius": (["f6"], lambda k, a: pr.f6_frob(a, k)),
    "f6_mul_by_v": (["f6"], lambda k, a: pr.f6_mul_by_v(a)),
    "f6_is_zero": (["f6"], lambda k, a: [int(a == pr.F6_ZERO)]),
    "f12_mul": (["f12", "f12"], lambda k, a, b: pr.f12_mul(a, b)),
    "f12_sqr": (["f12"], lambda k, a: pr.f12_sqr(a)),
    "f12_inv": (["f12"], lambda k, a: f12_inv0(a)),
    "f12_conj": (["f12"], lambda k, a: pr.f12_conj(a)),
    "f12_frobenius": (["f12"], lambda k, a: pr.f12_frob(a, k)),
    "f12_cyclotomic_sqr": (["f12"], lambda k, a: pr.f12_cyclotomic_sqr(a)),
    "f12_mul_by_024": (["f12", "f2", "f2", "f2"], lambda k, a, e0, evw, evv: pr.f12_mul_by_024(a, e0, evw, evv)),
    "f12_is_zero": (["f12"], lambda k, a: [int(a == F12_ZERO)]),
    "f12_eq": (["f12", "f12"], lambda k, a, b: [int(a == b)]),
    "exp_by_neg_z": (["f12"], lambda k, a: pr.exp_by_neg_z(a)),
    "final_exp_first_chunk": (["f12"], lambda k, a: a if a == F12_ZERO else pr.final_exp_first_chunk(a)),
    "final_exp_last_chunk": (["f12"], lambda k, a: pr.final_exp_last_chunk(a)),
    "final_exponentiation": (["f12"], lambda k, a: a if a == F12_ZERO else pr.final_exponentiation(a)),
    "gt_pow": (["f12", "expo"], lambda k, a, e: pr.f12_cyclotomic_exp(a, e)),
    "doubling_step": (["g2p"], lambda k, cur: _step(*pr.doubling_step(cur))),
    "mixed_addition_step": (["f2", "f2", "g2p"], lambda k, x2, y2, cur: _step(*pr.mixed_addition_step((x2, y2), cur))),
    "mul_by_q": (["f2", "f2"], lambda k, x, y: pr.mul_by_q((x, y, F2.one))[:2]),
    "apply_line": (["f12", "ell", "fq", "fq"], lambda k, f, c, px, py: pr.f12_mul_by_024(
        f, c[0], pr.f2_scale(c[1], py), pr.f2_scale(c[2], px))),
    "store_load_f12": (["f12"], None),     # the raw limbs, unchanged
    "f12_to_wire": (["f12"], None),        # the canonical value out of the Montgomery domain, exactly
    "f12_from_wire": (["wire12"], None),
}
INVERSE = {"f2": f2_inv0, "f6": f6_inv0, "f12": f12_inv0}


# ---------------------------------------------------------------- cases
def edge_records(B, rng):
    n = len(da.edge_values(B, Q)) + (da.maximal(B, 2, Q) is not None)
    return da.element_records(B, 2, Q, n, rng)


def random_records(B, n, rng):
    skip = len(edge_records(B, rng))
    return da.element_records(B, 2, Q, skip + n, rng)[skip:]


def structured(m, B, rng):
    """the case lists 1. to 4. of the module docstring, as (mandatory, the rest)"""
    Z0 = da.to_limbs(0)
    ZP = da.to_limbs(Q) if B > 16 else Z0
    alt = [Z0 if j % 2 == 0 else ZP for j in range(m)]
    zeros = [[Z0] * m, [ZP] * m, alt, alt[1:] + alt[:1]]
    must = [[e] * m for e in edge_records(B, rng)] + zeros
    one = da.RQ
    must += [[da.to_limbs(one)] + [Z0] * (m - 1)]
    if 16 * (one + Q) < B * Q:
        must += [[da.to_limbs(one + Q)] + [ZP] * (m - 1), [da.to_limbs(one + Q)] + alt[1:]]
    rest = []
    singles = [da.to_limbs(1), da.to_limbs(Q - 1), da.to_limbs(da.vmax(B, Q))]
    if da.maximal(B, 2, Q) is not None:
        singles.append(da.maximal(B, 2, Q))
    for pos in range(m):
        for k, s in enumerate(singles):
            el = list(alt if k % 2 == 0 else alt[1:] + alt[:1])
            el[pos] = s
            rest.append(el)
    for z in zeros[:3]:
        for pos in range(m):
            for v in (1, Q + 1):
                if 16 * v < B * Q:
                    el = list(z)
                    el[pos] = da.to_limbs(v)
                    rest.append(el)
    return must, rest


def elements(m, n, seed, B=32, extra=()):
    """n elements of m component records each"""
    rng = random.Random(seed)
    must, rest = structured(m, B, rng)
    must = must + [list(e) for e in extra]
    room = n - len(must)
    assert room >= 0
    if len(rest) > room // 2:                       # the 128-case sets: spread evenly over the single-slot cases
        keep = room // 2
        rest = [rest[(2 * i + 1) * len(rest) // (2 * keep)] for i in range(keep)]
    out = must + rest
    pool = random_records(B, m * (n - len(out)), rng)
    rng.shuffle(pool)
    out += [pool[i * m:(i + 1) * m] for i in range(n - len(out))]
    assert len(out) == n
    return out


def other_rep(el):
    """the same field element with every component in its other representative below 2p"""
    out = []
    for rec in el:
        v = da.from_limbs(rec)
        out.append(da.to_limbs(v + Q if v < Q else v - Q))
    return out


def mont_records(kind, val, rng):
    """pairing_ref value -> Montgomery records, each component canonical or plus p"""
    return [da.to_limbs(c * da.RQ % Q + rng.randrange(2) * Q) for c in flat(val)]


@functools.lru_cache(maxsize=None)
def cyclotomic_elements():
    """true elements of the cyclotomic subgroup: the first chunk of random values, canonical and with every component
    plus p"""
    rng = random.Random(41)
    out = []
    for _ in range(12):
        x = pr.final_exp_first_chunk(pr.fq12_from_flat(rng.randrange(Q) for _ in range(12)))
        assert pr.f12_cyclotomic_sqr(x) == pr.f12_sqr(x)
        lo = [da.to_limbs(c * da.RQ % Q) for c in flat(x)]
        out += [lo, other_rep(lo)]
    return out


def shuffled(lst, seed):
    lst = list(lst)
    random.Random(seed).shuffle(lst)
    return lst


def pairs(kind, n, seed):
    """two operands of one kind: each a with a permutation of the list, then with itself, with the same element in its
    other representation, with its inverse and with zero in some spelling"""
    m = SIZE[kind]
    rng = random.Random(seed + 1)
    n2 = n // 6
    n1 = n - 4 * n2
    A = elements(m, n1, seed)
    Bs = shuffled(A, seed + 2)
    S = A[:n2] if n2 <= n1 else (A * 2)[:n2]
    Z0, ZP = da.to_limbs(0), da.to_limbs(Q)
    a_out, b_out = list(A), list(Bs)
    for i, a in enumerate(S):
        inv = INVERSE[kind](nest(kind, [demont(r) for r in a]))
        zero = [(Z0, ZP)[(i >> (j % 3)) & 1] for j in range(m)]
        for b in (a, other_rep(a), mont_records(kind, inv, rng), zero):
            a_out.append(a)
            b_out.append(b)
    return a_out, b_out


R_ORDER = o.R


def exponents(words, n, seed):
    rng = random.Random(seed)
    top = 1 << (32 * words)
    vals = [0, 1, 2, R_ORDER - 1, R_ORDER, (1 << 128) - 1, (1 << 256) - 1, 1 << 127, 1 << 255, 3, (1 << 64) - 1]
    vals = [v for v in vals if v < top]
    while len(vals) < n:
        vals.append(rng.randrange(top) >> rng.choice((0, 0, 0, 7, 64)))
    return vals[:n]


def _cols(*operands):
    """operands: lists (over the cases) of elements (lists of records) -> per component a list of records"""
    cols = []
    for op_cases in operands:
        cols += [list(c) for c in zip(*op_cases)]
    return cols


def _operands(op, n):
    """the operand lists of an operation, one list of n elements per operand"""
    name = op.name
    kinds = OPS[name][0]
    s = 1000 + 17 * op.idx
    if name == "f2n":
        return [elements(2, n, s, B=op.ins[0][0])]
    if name == "store_load_f12":
        return [elements(12, N_STORE, 5)]
    if name == "f12_from_wire":
        rng = random.Random(s)
        comp = [da.wire_records(Q, n, rng) for _ in range(12)]
        comp = [comp[0]] + [shuffled(c, s + k) for k, c in enumerate(comp[1:])]
        return [[[c[i] for c in comp] for i in range(n)]]
    if name == "gt_pow":
        words = op.kp
        es = exponents(words, n, s)
        recs = [[[(e >> (32 * i)) & 0xffffffff for i in range(8)] + [0]] for e in es]
        return [shuffled(elements(12, n, 5, extra=cyclotomic_elements()), s), recs]
    if len(kinds) == 2 and kinds[0] == kinds[1]:
        return list(pairs(kinds[0], n, 5))
    if name == "doubling_step":
        rng = random.Random(s)
        Z0, ZP = da.to_limbs(0), da.to_limbs(Q)
        zs = ([Z0, Z0], [ZP, ZP], [Z0, ZP], [ZP, Z0])
        extra = [random_records(32, 4, rng) + z for z in zs]                                  # Z = 0
        extra += [random_records(32, 2, rng) + zs[(k + 1) % 4] + z for k, z in enumerate(zs)]   # Y = Z = 0
        return [elements(6, n, 5, extra=extra)]
    if name == "mixed_addition_step":
        rng = random.Random(s)
        x2, y2 = shuffled(elements(2, n, 5), s + 1), shuffled(elements(2, n, 6), s + 2)
        cur = shuffled(elements(6, n, 5), s + 3)
        one = [[da.to_limbs(da.RQ), da.to_limbs(0)], [da.to_limbs(da.RQ + Q), da.to_limbs(Q)]]
        for i in range(0, n, 16):                   # the current point equal to the base: D = E = 0
            cur[i] = (other_rep(x2[i]) if i & 16 else list(x2[i])) + list(y2[i]) + one[(i >> 5) & 1]
        return [x2, y2, cur]
    if name == "apply_line":
        rng = random.Random(s)
        px = shuffled([[r] for r in da.element_records(32, 2, Q, n, rng)], s + 1)
        py = shuffled([[r] for r in da.element_records(32, 2, Q, n, rng)], s + 2)
        for i, (x, y) in enumerate(((0, da.RQ), (Q, da.RQ), (0, da.RQ + Q), (Q, da.RQ + Q))):   # (px, py) = (0, 1)
            px[i], py[i] = [da.to_limbs(x)], [da.to_limbs(y)]
        return [elements(12, n, 5), shuffled(elements(6, n, 5), s + 3), px, py]
    if name in ("f12_cyclotomic_sqr",) + SLOW:
        return [elements(12, n, 5, extra=cyclotomic_elements())]
    out = [elements(SIZE[kinds[0]], n, 5)]
    for k, kind in enumerate(kinds[1:]):
        out.append(shuffled(elements(SIZE[kind], n, 6 + k), s + k))
    return out


_CASES = {}
SIZE_IN = dict(SIZE, expo=1, wire12=12)


def _make_distinct(op, cols, seed):
    """replace every repeated case (structured cases coincide here and there: all components at the edge 0 is also
    zero spelled as 0) by one of random operands, so that the case count is a count of distinct cases"""
    rng = random.Random(seed)
    seen = set()
    for i in range(len(cols[0])):
        key = tuple(tuple(c[i]) for c in cols)
        while key in seen:
            for c, (B, LU) in zip(cols, op.ins):
                if B > 0:
                    c[i] = da.to_limbs(rng.randrange(da.vmax(B, Q) + 1))
                elif B == -2:
                    c[i] = [rng.randrange(1 << 32) for _ in range(8)] + [0]
                else:                                   # an exponent of LU words
                    c[i] = [rng.randrange(1 << 32) if j < LU else 0 for j in range(8)] + [0]
            key = tuple(tuple(c[i]) for c in cols)
        seen.add(key)
    return cols


def cases_for(op):
    """(cols, wants) of an operation: per operand component a list of C records (C distinct cases), and per case the
    flat list of expected outputs (a field component as its canonical Montgomery value, a bool or packed words as
    they are).  Computed once per session: the CPU and the GPU test share them."""
    if op.id in _CASES:
        return _CASES[op.id]
    name = op.name
    n = N_SLOW if name in SLOW else N_CHEAP
    kinds, fn = OPS[name]
    cols = _cols(*_operands(op, n))
    assert len(cols) == len(op.ins) == sum(SIZE_IN[k] for k in kinds), op.id
    cols = _make_distinct(op, cols, 77 + op.idx)
    wants = []
    for i in range(len(cols[0])):
        recs = [c[i] for c in cols]
        if name == "store_load_f12":
            wants.append([list(r) for r in recs])
            continue
        if name == "f12_to_wire":
            wants.append([demont(r) for r in recs])
            continue
        if name == "f12_from_wire":
            wants.append([sum(int(w) << (32 * j) for j, w in enumerate(r[:8])) % Q * da.RQ % Q for r in recs])
            continue
        args, at = [], 0
        for kind in kinds:
            el = recs[at:at + SIZE_IN[kind]]
            at += SIZE_IN[kind]
            if kind == "expo":
                args.append(sum(int(w) << (32 * j) for j, w in enumerate(el[0][:8])))
            else:
                args.append(nest(kind, [demont(r) for r in el]))
        got = flat_out(fn(op.kp, *args))
        wants.append(got if op.outs[0][0] == 0 else [c * da.RQ % Q for c in got])
    _CASES[op.id] = (cols, wants)
    return _CASES[op.id]


def flat_out(x):
    return list(x) if isinstance(x, list) else flat(x)


def distinct(cols):
    return len({tuple(tuple(c[i]) for c in cols) for i in range(len(cols[0]))})


# ---------------------------------------------------------------- running
def run_host(lib, op, cols):
    """-> outputs (C, NOUT, 9)"""
    C = len(cols[0])
    a = np.ascontiguousarray(np.asarray(cols, dtype=np.uint32).reshape(len(op.ins), C, 9))
    out = np.zeros((C, len(op.outs), 9), dtype=np.uint32)
    scratch = np.zeros(max(1, C * op.scratch), dtype=np.uint32)
    rc = lib.tc_run(op.idx, a.ctypes.data, out.ctypes.data, scratch.ctypes.data, C, None)
    assert rc == 0, rc
    return out


def run_device(lib, op, cols, lanes):
    """the case set tiled over `lanes` lanes (neighbouring lanes hold different cases); returns the outputs of the
    first copy, shape (C, NOUT, 9), after checking that every copy agrees bit for bit"""
    import torch
    C = len(cols[0])
    nin, nout = len(op.ins), len(op.outs)
    a = np.asarray(cols, dtype=np.uint32).reshape(nin, C, 9)
    rep = max(1, lanes // C)
    a = np.tile(a, (1, rep, 1))
    n = a.shape[1]
    d_in = torch.from_numpy(a.view(np.int32).copy()).cuda()
    d_out = torch.zeros((n, nout, 9), dtype=torch.int32, device="cuda")
    d_scr = torch.zeros(max(1, n * op.scratch), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream()
    rc = lib.tc_run(op.idx, d_in.data_ptr(), d_out.data_ptr(), d_scr.data_ptr(), n, s.cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint32).reshape(rep, C, nout, 9)
    bad = np.nonzero((out != out[0:1]).any(axis=(2, 3)))
    assert bad[0].size == 0, "%s: copies disagree (copy, case): %s" % (
        op.id, list(zip(*[b[:5].tolist() for b in bad])))
    return out[0], n


def lanes_for(op):
    return N_STORE if op.name == "store_load_f12" else LANES_SLOW if op.name in SLOW else LANES_CHEAP


# ---------------------------------------------------------------- checking
def describe(cols, i):
    return "case %d, operand components %s" % (i, [hex(da.from_limbs(c[i])) for c in cols])


def check(op, cols, wants, out):
    """every output of every case: limbs 0..7 below the type's limit, the value below the type's bound (both as
    tc_info reports them), the value congruent to the reference mod p; bools, wire words and stored limbs exactly"""
    assert out.shape == (len(wants), len(op.outs), 9)
    for i, want in enumerate(wants):
        for j, (B, LU) in enumerate(op.outs):
            rec = out[i, j]
            what = "%s output %d of %s" % (op.id, j, describe(cols, i))
            if B == 0:
                assert int(rec[0]) == want[j] and not rec[1:].any(), "%s: got %s, want %d" % (what, list(rec), want[j])
                continue
            if B == -1:
                got = sum(int(w) << (32 * k) for k, w in enumerate(rec[:8]))
                assert got < Q, "%s: wire value %#x is not canonical" % (what, got)
                assert got == want[j] and int(rec[8]) == 0, "%s: got %#x, want %#x" % (what, got, want[j])
                continue
            assert all(int(x) < LU << 28 for x in rec[:8]), "%s: limbs %s above LU %d" % (what, list(rec), LU)
            v = da.from_limbs(rec)
            assert 16 * v < B * Q, "%s: value %d/16 p above its bound %d/16 p" % (what, 16 * v // Q, B)
            if op.name == "store_load_f12":
                assert [int(x) for x in rec] == [int(x) for x in want[j]], "%s: limbs changed" % what
            else:
                assert (v - want[j]) % Q == 0, "%s: got %#x, want %#x (mod p)" % (what, v, want[j])


def canonical(out):
    """outputs (C, NOUT, 9) -> per case the list of values mod p"""
    return [[da.from_limbs(r) % Q for r in case] for case in out]
