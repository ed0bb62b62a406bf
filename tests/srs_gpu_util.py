"""Shared by the GPU tests of DESIGN.md section 16: points of known logarithm to the standard generators, made and
encoded with entry points that have their own oracle tests (batch_msm_dev, the codec) and are not under test here."""
import numpy as np
import torch

import ceremony_ref as cref
import codec_cases as cases
from oracle import bn254 as o

R, Q = o.R, o.Q
ORACLE_UP_TO = 64          # expected values come from the oracle up to this many points, from batch_msm_dev above


def dev(b: bytes):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def host(t):
    torch.cuda.synchronize()
    return bytes(t.cpu().numpy())


def one(type_):
    return o.G1.one if type_ == 1 else o.G2.one


def inf_wire(type_):
    return cases.wire(type_, cases.curve(type_).zero, 0)


def points(type_, scalars, gen=1):
    """[s gen] ONE for every s, wire-in on the device; s = 0 is written as O"""
    from octopuszk_amd import zksnark as z
    base = z.g1_wire(z.G1_ONE) if type_ == 1 else z.g2_wire(z.G2_ONE)
    live = [s * gen % R or 1 for s in scalars]
    raw = bytearray(host(z.batch_msm_dev(254, 16, base, live, type_)))
    n = 96 * type_
    for i, s in enumerate(scalars):
        if s % R == 0:
            raw[n * i:n * (i + 1)] = inf_wire(type_)
    return dev(bytes(raw))


def compress(t, type_):
    from octopuszk_amd import codec
    return host((codec.compress_g1 if type_ == 1 else codec.compress_g2)(t))


def expected(type_, scalars, gen=1):
    """the compressed encodings of [s gen] ONE"""
    scalars = [s * gen % R for s in scalars]
    live = [s for s in scalars if s]
    if len(live) <= ORACLE_UP_TO:
        enc = iter([cref.encode(type_, cref.scale(type_, one(type_), s)) for s in live])
    else:
        raw = compress(points(type_, live), type_)
        enc = iter([raw[32 * type_ * i:32 * type_ * (i + 1)] for i in range(len(live))])
    zero = cref.encode(type_, cases.curve(type_).to_affine(cases.curve(type_).zero))
    return b"".join(next(enc) if s else zero for s in scalars)


def rescale_g1(wire: bytes, zz: int) -> bytes:
    """the same G1 point written with Z = zz"""
    x, y = int.from_bytes(wire[:32], "little"), int.from_bytes(wire[32:64], "little")
    return b"".join(v.to_bytes(32, "little") for v in (x * zz * zz % Q, y * pow(zz, 3, Q) % Q, zz))


def relation(r1cs):
    """an oracle.groth16.R1CS as the zksnark.R1CSRelation the device code takes, with explicit coefficients"""
    from octopuszk_amd import zksnark as z
    sides = []
    for k in range(3):
        ptr, idx, val = [0], [], []
        for c in r1cs.constraints:
            for index, value in c[k]:
                idx.append(index)
                val.append(value)
            ptr.append(len(idx))
        sides.append(z.LinearCombinations(ptr, idx, np.array(val, dtype=object)))
    return z.R1CSRelation(sides[0], sides[1], sides[2], r1cs.num_inputs, r1cs.num_auxiliary)
