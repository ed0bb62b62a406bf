"""Driver, cases and exact-integer expectations for the group-law conformance harness: tests/native/group_ops.h,
compiled by hipcc into groupcheck.hip (the device build, one kernel per operation) and by g++ into groupcheck_host.cpp
(the host branch).  Shared by test_group_ops_cpu.py (host build; cross-compiles the device harness) and
test_group_ops_gpu.py (device build).

Operands and results are raw 9-limb Montgomery records per Fq component (devarith.py): an affine point is x | y, a
Jacobian point X | Y | Z, an XYZZ point X | Y | ZZ | ZZZ, two records per coordinate over Fq2.  Every operand respects
its type's invariant (value < B p / 16, limbs normalised) and nothing else: a coordinate is its canonical Montgomery
value plus any multiple of p below the bound, infinity is Z (or ZZ and ZZZ) at any multiple of p, per component.
Expected points are oracle.bn254's group law applied to the operands READ BACK from the records, so a mistake of the
builder cannot hide one of the code.

Binary operations cycle through eight kinds (case index mod 8):
  0 (a) random P, Q, random + k p on every component        4 (e) infinity on the right
  1 (b) P == Q under another Z, random + k p                5 (f) infinity on both sides
  2 (c) P == -Q, likewise                                   6 (g) every component at its largest + k p, or at a
  3 (d) infinity on the left                                      record at the top of its bound (below)
                                                            7 (b) P == Q with every component at its largest + k p
so the doubling result, the infinity result and each operand at infinity take a quarter of the cases each.  The
signed forms take negate = (case index / 8) mod 2, and the kinds speak of the point that is effectively added: with
negate set, (b) hands in -P and reaches the doubling, (c) hands in P and reaches infinity.  Infinite Jacobian and XYZZ
operands run through every tuple of multiples of p their Z / ZZ bound admits; an infinite affine operand is (0, 0).
The largest + k p has k >= 1 on every component: where a bound is below 2 p (the affine bound; G1's ZZ and ZZZ) the
values are searched for, an affine point whose Montgomery coordinates lie below p / 16 (over Fq2 the x components or
the y components, in turn: all four at once are too rare to search for) and a z whose z^2 and z^3 do.  Only the
accumulator of the affine + affine form keeps ZZ = ZZZ = one: its contract admits nothing else.

Kind 6 rotates over its forms (top_forms): all components at their largest + k p; then every coordinate of either
operand, one at a time, at the top of its bound, once as the largest value below the bound and once as the "all limbs
maximal" record (limbs 0..7 at their limit, limb 8 the largest the bound admits).  A coordinate is driven there
through z: Z = z itself, ZZ = z^2 and X = x z^2 by a square root, ZZZ = z^3 and Y = y z^3 by a cube root (p = 1 mod 3:
Field.cbrt); an affine operand's x or y by solving the curve equation for the other coordinate.  Where the root does
not exist the target steps down (by one, the maximal record by one in limb 8) until it does; over Fq2 every component
of the coordinate sits at the top and the first one steps.

Unary operations run the same sweep: random offsets, the largest offsets, infinity in every multiple, the top records.
G2 takes every third base point from the twist outside the r-subgroup (the group law holds on the whole curve, and
scalar_mul's subgroup check runs exactly there)."""
import ctypes
import functools
import itertools
import os
import random
import subprocess

import numpy as np

import codec_ref as ref
import devarith as da
from oracle import bn254 as o

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NATIVE = os.path.join(HERE, "native")
CSRC = os.path.join(ROOT, "octopuszk_amd", "csrc")
DEV_SRC = os.path.join(NATIVE, "groupcheck.hip")
DEV_LIB = os.path.join(NATIVE, "_groupcheck.so")
HOST_SRC = os.path.join(NATIVE, "groupcheck_host.cpp")
HOST_LIB = os.path.join(NATIVE, "_groupcheck_host.so")
SHARED = [os.path.join(NATIVE, f) for f in ("group_ops.h", "devcheck_common.h")] + \
         [os.path.join(CSRC, f) for f in ("ec.cuh", "fq2.cuh", "fp29.cuh", "curve.cuh", "glv.cuh", "quad.cuh",
                                          "consts_gen.h", "mad_chain_gen.h")]

Q = o.Q
LISTS = ("g1", "g2", "misc", "lane")
CURVE = {0: o.G1, 1: o.G2}
N_CHEAP = {0: 1024, 1: 256}
N_SMUL = {0: 256, 1: 128}
N_GLV = 4096
N_LANE = {"g1": 256, "g2": 128}
LANES = 1 << 16
POOL, HIGH, TWIST = {0: 2400, 1: 1500}, {0: 1100, 1: 280}, 520      # base points: subgroup, room for + p, twist
YHIGH = 48                                                           # G2 points with room for + p on y
LAM = 4407920970296243842393367215006156084916469457145843978461      # the GLV eigenvalue (tests/test_glv.py)


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
    lib.gc_info.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
    lib.gc_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
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
    def __init__(self, lst, idx, name, v):
        self.list, self.idx, self.name = lst, idx, name
        self.group, nin, nout, self.kp = v[0], v[1], v[2], v[3]
        self.ins = list(zip(v[4:4 + nin], v[4 + nin:4 + 2 * nin]))             # (B, LU) per operand component
        self.outs = list(zip(v[4 + 2 * nin:4 + 2 * nin + nout], v[4 + 2 * nin + nout:4 + 2 * nin + 2 * nout]))
        self.id = "%s:%s" % (LISTS[lst], name if not self.kp else "%s<%d>" % (name, self.kp))


def ops(lib, lists=(0, 1, 2, 3)):
    out = []
    for lst in lists:
        for i in range(lib.gc_count(lst)):
            name = ctypes.create_string_buffer(64)
            v = (ctypes.c_int * 128)()
            assert lib.gc_info(lst, i, name, v) == 0
            out.append(OpInfo(lst, i, name.value.decode(), list(v)))
    return out


# ---------------------------------------------------------------- the table: operand kinds and what the oracle says
# kinds: a affine, j Jacobian, x XYZZ, s the accumulator xyzz_from_affine_signed returns, f the negate flag,
# e a scalar; outputs: jac, xyzz, aff, bool
def _signed(C, Qp, neg):
    return C.negate(Qp) if neg and not C.is_zero(Qp) else Qp


SPEC = {
    "from_affine": ("a", "jac", lambda C, P: P),
    "xyzz_from_affine": ("a", "xyzz", lambda C, P: P),
    "is_inf_aff": ("a", "bool", lambda C, P: C.is_zero(P)),
    "is_inf_jac": ("j", "bool", lambda C, P: C.is_zero(P)),
    "is_inf_xyzz": ("x", "bool", lambda C, P: C.is_zero(P)),
    "jac_dbl": ("j", "jac", lambda C, P: C.twice(P)),
    "jac_add": ("jj", "jac", lambda C, P, Qp: C.add(P, Qp)),
    "jac_madd": ("ja", "jac", lambda C, P, Qp: C.add(P, Qp)),
    "aff_dbl": ("a", "jac", lambda C, P: C.twice(P)),
    "jac_neg": ("j", "jac", lambda C, P: P if C.is_zero(P) else C.negate(P)),
    "xyzz_dbl_affine": ("a", "xyzz", lambda C, P: C.twice(P)),
    "xyzz_madd": ("xa", "xyzz", lambda C, P, Qp: C.add(P, Qp)),
    "xyzz_dbl": ("x", "xyzz", lambda C, P: C.twice(P)),
    "xyzz_add": ("xx", "xyzz", lambda C, P, Qp: C.add(P, Qp)),
    "xyzz_to_jac": ("x", "jac", lambda C, P: P),
    "glv_image": ("a", "aff", None),
    "scalar_mul": ("ae", "jac", lambda C, P, e: C.mul(P, e) if e else C.zero),
    "xyzz_madd_lazy": ("xaf", "xyzz", lambda C, P, Qp, neg: C.add(P, _signed(C, Qp, neg))),
    "xyzz_from_affine_signed": ("af", "xyzz", lambda C, P, neg: _signed(C, P, neg)),
    "xyzz_add_affine2_lazy": ("saf", "xyzz", lambda C, P, Qp, neg: C.add(P, _signed(C, Qp, neg))),
    "jac_to_xyzz": ("j", "xyzz", lambda C, P: P),
}
BINARY = [n for n, s in SPEC.items() if sum(k in "ajxs" for k in s[0]) == 2]
SIGNED = ("xyzz_madd_lazy", "xyzz_add_affine2_lazy", "xyzz_from_affine_signed")
# the G1-only forms and why (group_ops.h lists an operation for a configuration only if production instantiates it
# there): the lazily carried additions exist where CV::LAZY_MADD is set, jac_to_xyzz in the row / column window sums
G1_ONLY = ("xyzz_madd_lazy", "xyzz_from_affine_signed", "xyzz_add_affine2_lazy", "jac_to_xyzz")
SCALAR_WORDS = {0: (8, 4), 1: (8,)}        # scalar_mul: 8 words everywhere, 4 in batch_verify.cuh's bv_g1_mul_affine
NCOORD = {"a": 2, "j": 3, "x": 4, "s": 4}


# ---------------------------------------------------------------- field helpers over either coordinate field
class Field:
    """the coordinate field of a curve, on tuples of base-field components"""

    def __init__(self, C):
        self.C, self.F = C, C.F
        self.nc = 1 if C.F is o.FqOps else 2

    def comps(self, x):
        return [x] if self.nc == 1 else list(x)

    def el(self, c):
        return c[0] if self.nc == 1 else (c[0], c[1])

    def mont(self, x):
        return [c * da.RQ % Q for c in self.comps(x)]

    def demont(self, vals):
        return self.el([v * da.RQI % Q for v in vals])

    def sqrt(self, a):
        return ref.fq_sqrt(a) if self.nc == 1 else ref.fq2_sqrt(a)

    def rand(self, rng):
        while True:
            c = [rng.randrange(Q) for _ in range(self.nc)]
            if any(c):
                return self.el(c)

    def pow(self, a, e):
        return pow(a, e, Q) if self.nc == 1 else ref.fq2_pow(a, e)

    def cbrt(self, a):
        """a cube root of a, or None when there is none.  The group order is N = 9 t with 3 not dividing t, and with
        3 k = 1 mod t the power a^k cubes to a b, b = a^(3 k - 1) of order dividing 9; if a is a cube so is b, one of
        the three cubes c^(3 m) of the subgroup of order 9 that c generates, and a^k / c^m is the root"""
        if self.F.is_zero(a):
            return a
        t, k, c, cubes = _cbrt_setup(self.nc)
        m = cubes.get(self.pow(a, 3 * k - 1))
        if m is None:
            return None
        r = self.F.mul(self.pow(a, k), self.pow(c, 9 - m))
        assert self.F.mul(self.F.sqr(r), r) == a
        return r


@functools.lru_cache(maxsize=None)
def _cbrt_setup(nc):
    fld = Field(CURVE[nc - 1])
    F = fld.F
    N = Q - 1 if nc == 1 else Q * Q - 1
    assert N % 9 == 0 and N % 27 != 0
    t = N // 9
    rng = random.Random(94)
    while True:
        g = fld.rand(rng)
        if fld.pow(g, N // 3) != F.one:                  # no cube: g^t has order 9
            break
    c = fld.pow(g, t)
    return t, pow(3, -1, t), c, {fld.pow(c, 3 * m): m for m in range(3)}


def kcount(B):
    """how many multiples of p lie below B p / 16"""
    return (B + 15) // 16


def kmax(v, B):
    """the largest k with v + k p below B p / 16 (v canonical)"""
    return (da.vmax(B, Q) - v) // Q


def lift(vals, bounds, mode, rng):
    """canonical component values -> records with + k p: k random, the largest, or none"""
    out = []
    for v, B in zip(vals, bounds):
        k = kmax(v, B)
        assert k >= 0
        out.append(da.to_limbs(v + Q * (k if mode in ("max", "top") else rng.randint(0, k) if mode == "rand" else 0)))
    return out


# ---------------------------------------------------------------- point pools (oracle values, affine, Z = 1)
@functools.lru_cache(maxsize=None)
def pool(lst, n):
    """n distinct points of the r-subgroup"""
    return [(a[0], a[1]) for a in da.random_points(CURVE[lst], n, 90 + lst)]


@functools.lru_cache(maxsize=None)
def twist_pool(n):
    """n distinct points of the twist outside the r-subgroup: T + i S for two points found by solving the curve
    equation at random x (as the codec's decoder does; codec_ref.fq2_sqrt)"""
    C, F = o.G2, o.Fq2Ops
    rng = random.Random(91)
    found = []
    while len(found) < 2:
        x = (rng.randrange(Q), rng.randrange(Q))
        y = ref.fq2_sqrt(F.add(F.mul(F.sqr(x), x), C.b))
        if y is not None:
            found.append((x, y, F.one))
    T, S = found
    assert not C.is_zero(C.mul(T, o.R)) and not C.is_zero(C.mul(S, o.R))
    out = []
    for _ in range(n):
        a = C.to_affine(T)
        out.append((a[0], a[1]))
        T = C.add(T, S)
    return out


def _b(lst):
    return CURVE[lst].b if lst else 3


@functools.lru_cache(maxsize=None)
def high_pool(lst, n):
    """n distinct curve points with room for + p within the affine bound, that is with Montgomery components below
    p / 16: over Fq on x and on y, over Fq2 on both components of x (y_high_pool has those with room on y)"""
    C, fld = CURVE[lst], Field(CURVE[lst])
    F = C.F
    rng = random.Random(92 + lst)
    out, seen = [], set()
    while len(out) < n:
        xm = [rng.randrange(Q // 16 - 1) for _ in range(fld.nc)]
        x = fld.demont(xm)
        y = fld.sqrt(F.add(F.mul(F.sqr(x), x), _b(lst)))
        if y is None or tuple(xm) in seen:
            continue
        if lst == 0:
            y = next((v for v in (y, F.neg(y)) if 16 * (v * da.RQ % Q) < Q - 16), None)
            if y is None:
                continue
        elif rng.randrange(2):
            y = F.neg(y)
        seen.add(tuple(xm))
        out.append((x, y))
    return out


@functools.lru_cache(maxsize=None)
def y_high_pool(n):
    """n distinct points of the twist whose Montgomery y components are both below p / 16 (x by a cube root)"""
    C, fld = o.G2, Field(o.G2)
    F = C.F
    rng = random.Random(95)
    out = []
    while len(out) < n:
        y = fld.demont([rng.randrange(Q // 16 - 1) for _ in range(2)])
        x = fld.cbrt(F.sub(F.sqr(y), C.b))
        if x is not None and (x, y) not in out:
            out.append((x, y))
    return out


def base_point(lst, i, high=False, ysel=None):
    """the i-th base point of a case list: G2 takes every third from the twist outside the subgroup; high: a point
    with room for + p (over Fq2 on x, or with ysel on y)"""
    if high and lst == 1 and ysel is not None:
        return y_high_pool(YHIGH)[ysel % YHIGH]
    if high:
        return high_pool(lst, HIGH[lst])[i % HIGH[lst]]
    if lst == 1 and i % 3 == 2:
        return twist_pool(TWIST)[(i // 3) % TWIST]
    return pool(lst, POOL[lst])[i % POOL[lst]]


# ---------------------------------------------------------------- operands as records
class Shape:
    """component bounds of the operand types of one list, read from an operation's info"""

    def __init__(self, lst, all_ops):
        self.lst, self.C = lst, CURVE[lst]
        self.fld = Field(self.C)
        nc = self.fld.nc
        by = {op.name: op for op in all_ops if op.list == lst}
        cut = lambda ins, k: [[b for b, _ in ins[i * nc:(i + 1) * nc]] for i in range(k)]   # noqa: E731
        self.a = cut(by["is_inf_aff"].ins, 2)
        self.j = cut(by["is_inf_jac"].ins, 3)
        self.x = cut(by["is_inf_xyzz"].ins, 4)
        self.s = self.x

    def bounds(self, kind):
        return getattr(self, kind)


def inf_multiples(bounds):
    """every tuple of multiples of p (as k per component) the marker coordinate admits"""
    return list(itertools.product(*[range(kcount(B)) for B in bounds]))


def aff_recs(sh, A, mode, rng, fixed=None):
    """A: an oracle affine (x, y), or None for infinity = (0, 0); fixed: (coordinate, its records as they are to be)"""
    fld = sh.fld
    if A is None:
        return [da.to_limbs(0)] * (2 * fld.nc)
    out = lift(fld.mont(A[0]), sh.a[0], mode, rng) + lift(fld.mont(A[1]), sh.a[1], mode, rng)
    if fixed is not None:
        out[fixed[0] * fld.nc:(fixed[0] + 1) * fld.nc] = fixed[1]
    return out


def proj_recs(sh, kind, A, z, mode, rng, inf_k=None):
    """the affine point A under Z = z as a Jacobian (x z^2, y z^3, z) or an XYZZ (x z^2, y z^3, z^2, z^3) operand;
    A None: infinity, the marker coordinate at the multiples inf_k of p (XYZZ: ZZZ at multiples drawn from rng),
    X and Y any field elements"""
    fld, F = sh.fld, sh.C.F
    bnd = sh.bounds(kind)
    if A is None:
        out = lift(fld.mont(fld.rand(rng)), bnd[0], "rand", rng) + lift(fld.mont(fld.rand(rng)), bnd[1], "rand", rng)
        out += [da.to_limbs(k * Q) for k in inf_k]
        if kind != "j":
            out += [da.to_limbs(rng.randrange(kcount(B)) * Q) for B in bnd[3]]
        return out
    while True:
        z2 = F.sqr(z)
        z3 = F.mul(z2, z)
        # the largest + k p is to have k >= 1: where ZZ and ZZZ are bounded below 2 p (G1), a z that leaves room
        if mode != "max" or kind == "j" or all(v <= da.vmax(B, Q) - Q for c, b in zip((z2, z3), bnd[2:])
                                               for v, B in zip(fld.mont(c), b)):
            break
        z = fld.rand(rng)
    coords = [F.mul(A[0], z2), F.mul(A[1], z3)] + ([z] if kind == "j" else [z2, z3])
    out = []
    for c, b in zip(coords, bnd):
        out += lift(fld.mont(c), b, mode, rng)
    return out


def acc_recs(sh, A, mode, rng, inf_k=None, inf_xy=None, fixed=None):
    """the accumulator xyzz_add_affine2_lazy takes, which is what xyzz_from_affine_signed returns: a point with ZZ =
    ZZZ = the Montgomery one and X, Y within the AFFINE bound; or infinity (ZZ, ZZZ multiples of p; X, Y an affine
    pair or zeros)"""
    if A is None:
        return aff_recs(sh, inf_xy, "rand", rng) + [da.to_limbs(inf_k[0] * Q),
                                                    da.to_limbs(rng.randrange(kcount(sh.x[3][0])) * Q)]
    return aff_recs(sh, A, mode, rng, fixed) + [da.to_limbs(da.RQ)] * 2


def top_values(bounds, which, t):
    """the component values of a coordinate at the top of its bound, t steps down: the largest values below the bound
    (a step is one), or the all-limbs-maximal records (a step is one in limb 8); the first component steps"""
    if which == "maximal":
        vals = [da.from_limbs(da.maximal(B, 2, Q)) for B in bounds]
        vals[0] -= t << (8 * da.W)
    else:
        vals = [da.vmax(B, Q) for B in bounds]
        vals[0] -= t
    assert vals[0] > 0
    return vals


def top_forms(kinds):
    """kind 6's forms for operands of these kinds: None (every component at its largest + k p), then (operand,
    coordinate, which) for every coordinate of every operand at the top of its bound (the accumulator of the affine +
    affine form has X and Y only: its ZZ and ZZZ are one)"""
    return [None] + [(pos, co, which) for pos, k in enumerate(kinds) for co in range(2 if k in "as" else NCOORD[k])
                     for which in ("vmax", "maximal")]


def z_for_target(sh, A, kind, coord, which):
    """the z under which the given coordinate of A's Jacobian / XYZZ form sits at the top of its bound, and that
    coordinate's records: X = x z^2 and ZZ = z^2 by a square root, Y = y z^3 and ZZZ = z^3 by a cube root, the Jacobian
    Z = z as it is; the target steps down until the root exists"""
    fld, F = sh.fld, sh.C.F
    bounds = sh.bounds(kind)[coord]
    t = 0
    while True:
        vals = top_values(bounds, which, t)
        t += 1
        T = fld.demont(vals)
        if coord == 0:
            z = fld.sqrt(F.mul(T, F.inv(A[0])))
        elif coord == 1:
            z = fld.cbrt(F.mul(T, F.inv(A[1])))
        elif kind == "j":
            z = T
        else:
            z = fld.sqrt(T) if coord == 2 else fld.cbrt(T)
        if z is not None and not F.is_zero(z):
            return z, [da.to_limbs(v) for v in vals]


def proj_top(sh, kind, A, top, rng):
    """a Jacobian / XYZZ operand with the coordinate top = (coordinate, which) at the top of its bound, the others at
    their largest + k p"""
    nc = sh.fld.nc
    z, recs = z_for_target(sh, A, kind, *top)
    out = proj_recs(sh, kind, A, z, "top", rng)
    out[top[0] * nc:(top[0] + 1) * nc] = recs
    return out


_AFF_TOPS = {}


def aff_top(sh, coord, which, use):
    """the use-th curve point, counting down from the top of the affine bound, whose x (coord 0) or y (coord 1) sits
    there (the other coordinate solves the curve equation: a square root for y, a cube root for x): (the point, the
    records of that coordinate)"""
    fld, F = sh.fld, sh.C.F
    found = _AFF_TOPS.setdefault((sh.lst, coord, which), [[], 0])
    while len(found[0]) <= use:
        vals = top_values(sh.a[coord], which, found[1])
        found[1] += 1
        T = fld.demont(vals)
        if coord == 0:
            other = fld.sqrt(F.add(F.mul(F.sqr(T), T), _b(sh.lst)))
            if other is not None and found[1] % 2:
                other = F.neg(other)
        else:
            other = fld.cbrt(F.sub(F.sqr(T), _b(sh.lst)))
        if other is not None:
            found[0].append(((T, other) if coord == 0 else (other, T), [da.to_limbs(v) for v in vals]))
    return found[0][use]


def operand(sh, kind, A, mode, rng, inf_k=None, top=None, inf_xy=None, use=0):
    """top = (coordinate, which): that coordinate at the top of its bound; an affine operand (and the affine +
    affine accumulator) then IS the use-th point that has it there, whatever A says"""
    fixed = None
    if top is not None and kind in "as":
        A, recs = aff_top(sh, top[0], top[1], use)
        fixed = (top[0], recs)
    if kind == "a":
        return aff_recs(sh, A, mode, rng, fixed)
    if kind == "s":
        return acc_recs(sh, A, mode, rng, inf_k, inf_xy, fixed)
    if A is not None and top is not None:
        return proj_top(sh, kind, A, top, rng)
    return proj_recs(sh, kind, A, sh.fld.rand(rng), mode, rng, inf_k)


class Cycle:
    """hands out the elements of a list in turn, for ever"""

    def __init__(self, items):
        self.items, self.i = items, 0

    def __call__(self):
        self.i += 1
        return self.items[(self.i - 1) % len(self.items)]


def marker_bounds(sh, kind):
    return sh.bounds(kind)[2] if kind in "jxs" else None


def binary_cases(sh, op, n, seed):
    """the eight kinds of the module docstring for a two-point operation"""
    kinds = SPEC[op.name][0]
    k1, k2 = kinds[0], kinds[1]
    signed = "f" in kinds
    rng = random.Random(seed)
    F = sh.C.F
    inf1 = Cycle(inf_multiples(marker_bounds(sh, k1)))
    inf2 = Cycle(inf_multiples(marker_bounds(sh, k2))) if k2 != "a" else (lambda: None)
    forms = top_forms((k1, k2))
    rows = []
    for i in range(n):
        kind = i % 8
        neg = (i // 8) % 2 if signed else 0
        form = forms[(i // 8) % len(forms)] if kind == 6 else None
        use = i // 8 // len(forms)                    # how often this form came before
        top = kind in (6, 7)
        high = top and "a" in (k1, k2) or top and k1 == "s"
        # over Fq2 the points with room on x and those with room on y take turns, in kind 6's first form and in kind 7
        turn = use if kind == 6 else i // 8
        ysel = turn // 2 if turn % 2 else None
        A = base_point(sh.lst, i, high, ysel)
        Bq = base_point(sh.lst, 1200 + i, high, None if ysel is None else ysel + YHIGH // 2)
        if k1 == "s" and (i // 4) % 2:                # the accumulator holds +-A as xyzz_from_affine_signed made it
            A = (A[0], F.neg(A[1]))
        if kind in (1, 7):
            Bq = A
        elif kind == 2:
            Bq = (A[0], F.neg(A[1]))
        if neg:                                       # the operand handed in is the negative of the point added
            Bq = (Bq[0], F.neg(Bq[1]))
        P_ = None if kind in (3, 5) else A
        Q_ = None if kind in (4, 5) else Bq
        mode = "max" if top else "rand"
        # an infinite accumulator of the affine + affine form: X = Y = 0 as xyzz_from_affine_signed leaves them (the
        # cases stay distinct through the other operand), or the coordinates of some point
        inf_xy = None if kind == 3 and i % 16 < 8 else A
        tops = [form[1:] if form is not None and form[0] == pos else None for pos in (0, 1)]
        r1 = operand(sh, k1, P_, mode, rng, inf1() if P_ is None else None, top=tops[0], inf_xy=inf_xy, use=use)
        r2 = operand(sh, k2, Q_, mode, rng, inf2() if Q_ is None else None, top=tops[1], use=use)
        rows.append(r1 + r2 + ([[neg] + [0] * 8] if signed else []))
    return rows


def unary_cases(sh, op, n, seed):
    """the sweep of a one-point operation, by case index mod 8: 0, 4 random + k p; 1, 7 the largest + k p; 2, 5
    infinity (every multiple in turn; doubling it is included); 3 canonical; 6 every coordinate in turn at the top of
    its bound, as in kind 6 above"""
    kinds = SPEC[op.name][0]
    k = kinds[0]
    signed = "f" in kinds
    rng = random.Random(seed)
    rows = []
    forms = top_forms((k,))[1:]
    if k == "a":
        # one infinity per sign ((0, 0) is its only spelling here), a third of the points with room for + p (over Fq2
        # on x and on y in turn), an eighth with x or y at the top of the bound
        for i in range(n):
            neg = (i // 2) % 2 if signed else 0
            flag = [[neg] + [0] * 8] if signed else []
            if i % 8 == 6:
                form = forms[(i // 8) % len(forms)]
                rows.append(operand(sh, k, None, "max", rng, top=form[1:], use=i // 8 // len(forms)) + flag)
                continue
            A = None if i in ((2, 4) if signed else (2,)) else \
                base_point(sh.lst, i, high=i % 3 == 1, ysel=i // 6 if i % 6 == 4 else None)
            rows.append(aff_recs(sh, A, "max" if i % 3 == 1 else "rand", rng) + flag)
        if op.name == "is_inf_aff":
            # every spelling of zero the affine bound admits, and one component off zero around each
            nc = sh.fld.nc
            spell = list(itertools.product((0, Q), repeat=2 * nc))
            extra = [list(s) for s in spell]
            for s in spell:
                for pos in range(2 * nc):
                    for v in (s[pos] + 1,) + ((Q - 1,) if s[pos] == 0 else ()):
                        extra.append(list(s[:pos]) + [v] + list(s[pos + 1:]))
            seen, at = {tuple(tuple(r) for r in rows[2])}, 8
            for e in extra:
                recs = [da.to_limbs(v) for v in e]
                if tuple(tuple(r) for r in recs) not in seen:
                    seen.add(tuple(tuple(r) for r in recs))
                    rows[at] = recs
                    at += 1
        return rows
    inf = Cycle(inf_multiples(marker_bounds(sh, k)))
    for i in range(n):
        kind = i % 8
        A = None if kind in (2, 5) else base_point(sh.lst, i)
        form = forms[(i // 8) % len(forms)] if kind == 6 else None
        mode = "max" if kind in (1, 7) else "none" if kind == 3 else "rand"
        rows.append(operand(sh, k, A, mode, rng, inf() if A is None else None, top=form and form[1:]))
    return rows


R_ORDER = o.R


def special_scalars(words):
    vals = [0, 1, 2, R_ORDER - 1, R_ORDER, R_ORDER + 1, (1 << 256) - 1, 1 << 255, (1 << 128) - 1, 1 << 127, 3, LAM]
    return [v for v in vals if v < 1 << (32 * words)]


def scalars(words, n, rng):
    top = 1 << (32 * words)
    vals = special_scalars(words) * 2                   # each on a subgroup point and on the next kind of point
    while len(vals) < n:
        vals.append(rng.randrange(top) >> rng.choice((0, 0, 0, 0, 7, 64)))
    return vals[:n]


def scalar_cases(sh, op, n, seed):
    """[e] q for an affine q: the special scalars on subgroup points and again off the subgroup (G2) or on points
    with x in [p, 17 p / 16) (G1), the affine infinity, the group order on further points of both kinds (on the twist
    the result must not be infinity: the codec's and the verifier's subgroup check), then random scalars"""
    rng = random.Random(seed)
    words = op.kp
    es = scalars(words, n, rng)
    rows = []
    base = len(special_scalars(words))
    for i, e in enumerate(es):
        if i < base:
            A = pool(sh.lst, POOL[sh.lst])[i]           # the special scalars on subgroup points ...
        elif i < 2 * base:                              # ... and on twist points (G2) / high points (G1)
            A = twist_pool(TWIST)[i] if sh.lst == 1 else high_pool(0, HIGH[0])[i]
        elif i < 2 * base + 2:
            A = None                                    # the affine infinity, as jac_madd takes it
        elif i < 2 * base + 10:                         # the order on further twist and subgroup points
            e = R_ORDER if words == 8 else e
            A = base_point(sh.lst, 3 * i + (2 if i % 2 else 0))
        else:
            A = base_point(sh.lst, i, high=i % 4 == 1)
        rows.append(aff_recs(sh, A, "max" if i % 4 == 1 else "rand", rng) +
                    [[(e >> (32 * j)) & 0xffffffff for j in range(8)] + [0]])
    return rows


def glv_values():
    from test_glv_split import EDGE, UNREDUCED
    rng = random.Random(93)
    vals = list(dict.fromkeys(EDGE + UNREDUCED))
    seen = set(vals)
    while len(vals) < N_GLV:
        v = rng.randrange(1 << 256)
        if v not in seen:
            seen.add(v)
            vals.append(v)
    return vals


def glv_want(k):
    from test_glv import model
    k1, k2 = model(k)
    assert abs(k1) < 1 << 127 and abs(k2) < 1 << 127
    return [abs(k1) | (abs(k2) << 128), int(k1 < 0), int(k2 < 0)]


# ---------------------------------------------------------------- reading operands back, expectations
def read_point(sh, kind, recs):
    """operand records -> oracle point (affine with Z = 1, or the curve's zero)"""
    C, fld = sh.C, sh.fld
    nc = fld.nc
    vals = [da.from_limbs(r) % Q for r in recs]
    co = [fld.el(vals[i * nc:(i + 1) * nc]) for i in range(len(vals) // nc)]
    if kind == "a":
        a = tuple(da.demont(c, C.F) for c in co)
        return C.zero if C.F.is_zero(a[0]) and C.F.is_zero(a[1]) else (a[0], a[1], C.F.one)
    a = da.affine_of_jac(C, *co) if kind == "j" else da.affine_of_xyzz(C, *co)
    return C.zero if a is None else (a[0], a[1], C.F.one)


def split_operands(sh, kinds, row):
    """one case's records -> [(kind, records)] per operand"""
    out, at = [], 0
    for k in kinds:
        w = NCOORD[k] * sh.fld.nc if k in NCOORD else 1
        out.append((k, row[at:at + w]))
        at += w
    assert at == len(row)
    return out


def read_args(sh, kinds, row):
    args = []
    for k, recs in split_operands(sh, kinds, row):
        if k == "f":
            args.append(int(recs[0][0]))
        elif k == "e":
            args.append(sum(int(w) << (32 * j) for j, w in enumerate(recs[0][:8])))
        else:
            args.append(read_point(sh, k, recs))
    return args


@functools.lru_cache(maxsize=None)
def beta(lst):
    """the x multiplier of the endomorphism, from the oracle alone: x(lambda G) / x(G), a cube root of one in Fq"""
    C = CURVE[lst]
    F = C.F
    G = C.to_affine(C.one)
    b = F.mul(C.to_affine(C.mul(C.one, LAM))[0], F.inv(G[0]))
    assert F.mul(b, F.sqr(b)) == F.one and b != F.one and (lst == 0 or b[1] == 0)
    return b


_SHAPES, _CASES = {}, {}


def shape(op, all_ops):
    if op.list not in _SHAPES:
        _SHAPES[op.list] = Shape(op.list, all_ops)
    return _SHAPES[op.list]


def size_of(op):
    if op.list == 2:
        return N_GLV
    if op.list == 3:
        return N_LANE[op.name[:2]]
    return N_SMUL[op.list] if op.name == "scalar_mul" else N_CHEAP[op.list]


def cases_for(op, all_ops):
    """(cols, wants): per operand component a list of C records, and per case the expectation: an affine oracle point
    or None (point outputs), a list of integers (bool, words).  Computed once per session; the CPU and the GPU test
    use the same builder and seeds."""
    if op.id in _CASES:
        return _CASES[op.id]
    n = size_of(op)
    if op.list == 2:
        vals = glv_values()
        rows = [[[(v >> (32 * j)) & 0xffffffff for j in range(8)] + [0]] for v in vals]
        wants = [glv_want(v) for v in vals]
    elif op.list == 3:
        # the lane-group conversions: a Jacobian operand per group, swept as a unary operation's
        lst = 0 if op.name.startswith("g1") else 1
        ref_op = next(x for x in all_ops if x.list == lst and x.name == "jac_dbl")
        sh = shape(ref_op, all_ops)
        rows = unary_cases(sh, ref_op, n, 500 + op.idx)
        wants = []
        for row in rows:
            P = read_point(sh, "j", row)
            wants.append(da.oracle_affine(sh.C, sh.C.twice(P) if op.name.endswith("dbl") else P))
    else:
        sh = shape(op, all_ops)
        kinds, outk, fn = SPEC[op.name]
        seed = 300 + 40 * op.list + op.idx
        if op.name == "scalar_mul":
            rows = scalar_cases(sh, op, n, seed)
        elif op.name in BINARY:
            rows = binary_cases(sh, op, n, seed)
        else:
            rows = unary_cases(sh, op, n, seed)
        wants = []
        for row in rows:
            args = read_args(sh, kinds, row)
            if outk == "bool":
                wants.append([int(fn(sh.C, *args))])
            elif outk == "aff":                         # glv_image: beta x canonical, y as it came; O stays (0, 0)
                P = args[0]
                F, nc = sh.C.F, sh.fld.nc
                wants.append(([0] * nc if sh.C.is_zero(P) else sh.fld.mont(F.mul(beta(op.list), P[0]))) +
                             [da.from_limbs(r) for r in row[nc:]])
            else:
                wants.append(da.oracle_affine(sh.C, fn(sh.C, *args)))
    cols = [list(c) for c in zip(*rows)]
    assert len(cols) == len(op.ins), (op.id, len(cols), len(op.ins))
    _CASES[op.id] = (cols, wants)
    return _CASES[op.id]


def distinct(cols):
    return len({tuple(tuple(c[i]) for c in cols) for i in range(len(cols[0]))})


def out_kind(op):
    if op.list == 2:
        return "split"
    if op.list == 3:
        return "jac"
    return SPEC[op.name][1]


# ---------------------------------------------------------------- running
def run_host(lib, op, cols):
    """-> outputs (C, NOUT, 9)"""
    C = len(cols[0])
    a = np.ascontiguousarray(np.asarray(cols, dtype=np.uint32).reshape(len(op.ins), C, 9))
    out = np.zeros((C, len(op.outs), 9), dtype=np.uint32)
    rc = lib.gc_run(op.list, op.idx, a.ctypes.data, out.ctypes.data, C, None)
    assert rc == 0, rc
    return out


def run_device(lib, op, cols, lanes=LANES):
    """each case on op.group adjacent lanes, the whole case set repeated up to `lanes` lanes (neighbouring lanes or
    groups hold different cases).  Returns the outputs of the first copy, shape (C, NOUT, 9), after checking that
    every copy and every lane of a group agree bit for bit, and the number of lanes run."""
    import torch
    C = len(cols[0])
    nin, nout, group = len(op.ins), len(op.outs), op.group
    a = np.asarray(cols, dtype=np.uint32).reshape(nin, C, 9)
    a = np.repeat(a, group, axis=1)
    rep = max(1, lanes // (C * group))
    a = np.tile(a, (1, rep, 1))
    n = a.shape[1]
    d_in = torch.from_numpy(a.view(np.int32).copy()).cuda()
    d_out = torch.zeros((n, nout, 9), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream()
    rc = lib.gc_run(op.list, op.idx, d_in.data_ptr(), d_out.data_ptr(), n, s.cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint32).reshape(rep, C, group, nout, 9)
    bad = np.nonzero((out != out[0:1, :, 0:1]).any(axis=(3, 4)))
    assert bad[0].size == 0, "%s: copies disagree (copy, case, lane): %s" % (
        op.id, list(zip(*[b[:5].tolist() for b in bad])))
    return out[0, :, 0], n


# ---------------------------------------------------------------- checking
def describe(cols, i):
    return "case %d (kind %d), operand components %s" % (i, i % 8, [hex(da.from_limbs(c[i])) for c in cols])


def _element(what, rec, B, LU):
    """one output element within what its C++ type claims (test_device_arith_gpu._check_element): limbs 0..7 below
    LU 2^28, the value below B p / 16"""
    assert all(int(x) < LU << 28 for x in rec[:8]), "%s: limbs %s above LU %d" % (what, list(rec), LU)
    v = da.from_limbs(rec)
    assert 16 * v < B * Q, "%s: value %d/16 p above its bound %d/16 p" % (what, 16 * v // Q, B)
    return v % Q


def check(op, cols, wants, out):
    """every output of every case: the type's limb and value bounds, then the point (as an affine point of the oracle,
    an infinite XYZZ with ZZ and ZZZ both zero, a finite one with ZZ^3 = ZZZ^2), the canonical affine pair, the bool or
    the words exactly"""
    assert out.shape == (len(wants), len(op.outs), 9)
    kind = out_kind(op)
    if kind in ("jac", "xyzz", "aff"):
        C = CURVE[0 if op.id.startswith(("g1", "lane:g1")) else 1]
        fld = Field(C)
        F, nc = C.F, fld.nc
    for i, want in enumerate(wants):
        what = "%s, %s" % (op.id, describe(cols, i))
        if kind in ("bool", "split"):
            for j, (B, LU) in enumerate(op.outs):
                rec = out[i, j]
                if B == 0:
                    assert int(rec[0]) == want[j] and not rec[1:].any(), "%s: output %d is %s, want %d" % (
                        what, j, list(rec), want[j])
                else:
                    got = sum(int(w) << (32 * k) for k, w in enumerate(rec[:8]))
                    assert got == want[j] and int(rec[8]) == 0, "%s: got %#x, want %#x" % (what, got, want[j])
            continue
        vals = [_element("%s output %d" % (what, j), out[i, j], B, LU) for j, (B, LU) in enumerate(op.outs)]
        co = [fld.el(vals[k * nc:(k + 1) * nc]) for k in range(len(vals) // nc)]
        if kind == "aff":
            raw = [da.from_limbs(out[i, j]) for j in range(len(op.outs))]
            assert raw == want, "%s: got %s, want %s (x canonical, y unchanged)" % (what, [hex(v) for v in raw], [hex(v) for v in want])
            continue
        if kind == "jac":
            got = da.affine_of_jac(C, *co)
        else:
            got = da.affine_of_xyzz(C, *co)
            zz, zzz = co[2], co[3]
            if got is None:
                assert F.is_zero(zzz), "%s: infinity with ZZ = 0 and ZZZ = %s" % (what, zzz)
            else:
                zz, zzz = da.demont(zz, F), da.demont(zzz, F)
                assert F.mul(F.sqr(zz), zz) == F.sqr(zzz), "%s: ZZ^3 != ZZZ^2" % what
        assert got == want, "%s: got %s, want %s" % (what, got, want)
