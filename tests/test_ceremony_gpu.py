"""Phase-2 key contributions on hardware: the scaling kernel against oracle integers at the
wave boundaries, in place, with the exceptional lanes and the scalars at which a GLV ladder meets P == +-Q; a
contribution to a 100-constraint key against the model, point for point and receipt byte for receipt byte, proved with
and saved; verification of it, of every tamper class, and of a chain of two."""
import ctypes
import functools
import hashlib
import random

import pytest
import torch

import ceremony_ref as cref
import codec_cases as cases
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

Q, R = o.Q, o.R
INVALID = -1   # OZK_E_INVALID (include/ozk.h)
D, U, SEED = 0x1234567890ABCDEF1234567890ABCDEF % R, 0xFEDCBA0987654321 % R, b"seed of the gpu tests"
D2, U2 = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0 % R, 0x1122334455667788 % R
NC, NI = 100, 3            # delta_abc_g1 ++ query_h: 100 + 129 = 229 points, three waves and a part of a fourth


def _dev(b: bytes):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    torch.cuda.synchronize()
    return bytes(t.cpu().numpy())


# ---------------------------------------------------------------------------- kernel inputs and expected outputs
# Lane i holds sign * (S + i T), or O: [k] of it is sign * ([k] S + i [k] T), one oracle addition per lane after two
# oracle multiplications per scalar.  Lanes given outright (the twist point outside the subgroup) are multiplied directly.
@functools.lru_cache(maxsize=None)
def _lanes(type_, n):
    """(descriptors, the input bytes): a descriptor is None for O, (i, sign, z) for sign * (S + i T) written with Z = z
    (1: affine), or ("direct", P)"""
    rng = random.Random(100 * type_ + n)
    lanes = [(i, 1, 1) for i in range(n)]
    for i in range(n):
        if i % 7 == 5:
            lanes[i] = (i, 1, rng.randrange(2, Q))                 # Z != 1
    if type_ == 1 and n >= 63:
        lanes[2] = lanes[1]                                        # a repeated point
        lanes[4] = (3, -1, 1)                                      # P and -P
        for i in (0, 31, n - 1):
            lanes[i] = None                                        # infinity
    if type_ == 2:
        if n >= 5:
            lanes[0], lanes[3] = None, (2, -1, 1)
        lanes[1 if n >= 5 else 0] = ("direct", cref.twist_point_outside_the_subgroup())
    S, T = _base(type_)
    C = cases.curve(type_)
    raw = []
    for lane in lanes:
        if lane is None:
            P = C.zero
        elif lane[0] == "direct":
            P = lane[1]
        else:
            i, sign, zz = lane
            P = C.to_affine(C.add(S, C.mul(T, i)) if i else S)
            if sign < 0:
                P = C.negate(P)
            if zz != 1:
                P = cases.rescale(type_, P, zz)
        raw.append(cases.wire(type_, P, 0))
    return tuple(lanes), b"".join(raw)


@functools.lru_cache(maxsize=None)
def _base(type_):
    C, rng = cases.curve(type_), random.Random(77 + type_)
    return (C.to_affine(C.mul(C.one, rng.randrange(1, R))), C.to_affine(C.mul(C.one, rng.randrange(1, R))))


@functools.lru_cache(maxsize=None)
def _multiples(type_, k, count):
    """[k] (S + i T) for i < count, affine"""
    C = cases.curve(type_)
    S, T = _base(type_)
    kS, kT = C.mul(S, k) if k else C.zero, C.mul(T, k) if k else C.zero
    out, P = [], kS
    for _ in range(count):
        out.append(C.to_affine(P))
        P = C.add(P, kT)
    return out


def _expected(type_, n, k):
    C = cases.curve(type_)
    lanes, _ = _lanes(type_, n)
    mult = _multiples(type_, k, max(n, 65))
    out = []
    for lane in lanes:
        if lane is None:
            P = C.to_affine(C.zero)
        elif lane[0] == "direct":
            P = cref.scale(type_, lane[1], k)
        else:
            P = mult[lane[0]]
            if lane[1] < 0 and not C.is_zero(P):
                P = C.to_affine(C.negate(P))
        out.append(cref.wire(type_, P))
    return b"".join(out)


def _raw_scale(d_in, n, type_, k, d_out):
    from octopuszk_amd import lib
    from octopuszk_amd.device import _ptr
    kb = (ctypes.c_uint8 * 32).from_buffer_copy(int(k).to_bytes(32, "little"))
    return lib.load().ozk_points_scale_dev(_ptr(d_in), n, type_, ctypes.cast(kb, ctypes.c_void_p), _ptr(d_out), None)


def _g1_scalars(n):
    all_ = cref.scalars()
    return all_ if n == 65 else [all_[6], all_[4], all_[-1]]       # lambda, r - 1, a random one


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_g1_scaling_matches_the_oracle(n):
    from octopuszk_amd import ceremony
    lanes, raw = _lanes(1, n)
    if n >= 63:
        assert lanes[0] is None and lanes[31] is None and lanes[n - 1] is None and lanes[1] == lanes[2]
        assert any(lane and lane[2] != 1 for lane in lanes)
    d_in = _dev(raw)
    for k in _g1_scalars(n):
        got = _host(ceremony.scale_points(d_in, k, 1))
        want = _expected(1, n, k)
        for i in range(n):
            assert got[96 * i:96 * i + 96] == want[96 * i:96 * i + 96], (k, i, lanes[i])
    assert _host(d_in) == raw                                      # the input is left alone


@pytest.mark.parametrize("n", [1, 5, 65])
def test_g2_scaling_matches_the_oracle_inside_the_subgroup_and_outside(n):
    from octopuszk_amd import ceremony
    rng = random.Random(21)
    lanes, raw = _lanes(2, n)
    outside = next(i for i, lane in enumerate(lanes) if lane and lane[0] == "direct")
    d_in = _dev(raw)
    for k in (0, 1, R - 1, rng.randrange(R), rng.randrange(R)):
        got = _host(ceremony.scale_points(d_in, k, 2))
        want = _expected(2, n, k)
        for i in range(n):
            assert got[192 * i:192 * i + 192] == want[192 * i:192 * i + 192], (k, i)
        if k == R - 1:     # the subgroup test: [r - 1] P = -P inside, and not outside
            affine = _expected(2, n, 1)
            for i, lane in enumerate(lanes):
                if lane is None:
                    continue
                v = [int.from_bytes(affine[192 * i + 32 * j:192 * i + 32 * j + 32], "little") for j in range(6)]
                minus = cref.wire(2, o.G2.negate(((v[0], v[1]), (v[2], v[3]), (v[4], v[5]))))
                assert (got[192 * i:192 * i + 192] == minus) == (i != outside), i


@pytest.mark.parametrize("type_,n", [(1, 65), (1, 257), (2, 5)])
def test_in_place_poisoned_outputs_and_repeatability(type_, n):
    _, raw = _lanes(type_, n)
    k = cref.scalars()[-2]
    want = _expected(type_, n, k)
    runs = []
    for _ in range(2):
        out = torch.full((len(raw),), 0xA5, dtype=torch.uint8, device="cuda")
        assert _raw_scale(_dev(raw), n, type_, k, out) == 0
        runs.append(_host(out))
    assert runs[0] == runs[1] == want
    buf = _dev(raw)
    assert _raw_scale(buf, n, type_, k, buf) == 0                   # d_out == d_in
    assert _host(buf) == want


def test_argument_checks_leave_the_output_untouched():
    from octopuszk_amd import ceremony, lib
    L = lib.load()
    n = 65
    _, raw = _lanes(1, n)
    d_in = _dev(raw)
    out = torch.full((len(raw),), 0xA5, dtype=torch.uint8, device="cuda")
    for k in (R, (1 << 256) - 1):
        assert _raw_scale(d_in, n, 1, k, out) == INVALID
        assert b"below r" in L.ozk_last_error()
    assert _raw_scale(d_in, 0, 1, 5, out) == INVALID and _raw_scale(d_in, -1, 1, 5, out) == INVALID
    assert _raw_scale(d_in, n, 3, 5, out) == INVALID and _raw_scale(d_in, n, 0, 5, out) == INVALID
    assert _raw_scale(d_in[1:], n - 1, 1, 5, out) == INVALID       # misaligned
    from octopuszk_amd.device import _ptr
    kb = (ctypes.c_uint8 * 32)()
    assert L.ozk_points_scale_dev(None, n, 1, ctypes.cast(kb, ctypes.c_void_p), _ptr(out), None) == INVALID
    assert L.ozk_points_scale_dev(_ptr(d_in), n, 1, ctypes.cast(kb, ctypes.c_void_p), None, None) == INVALID
    assert L.ozk_points_scale_dev(_ptr(d_in), n, 1, None, _ptr(out), None) == INVALID
    assert _host(out) == b"\xa5" * len(raw)
    with pytest.raises(TypeError):
        ceremony.scale_points(raw, 5, 1)
    with pytest.raises(ValueError):
        ceremony.scale_points(d_in[:100], 5, 1)
    assert _raw_scale(d_in, n, 1, 0, out) == 0                      # k = 0 is legal: n points at infinity
    assert _host(out) == cref.wire(1, o.G1.to_affine(o.G1.zero)) * n


# ---------------------------------------------------------------------------- a contribution, end to end
def _points_of(t, type_):
    """the affine points of a wire-in tensor with Z = 1 or 0"""
    raw = _host(t)
    size, out = 96 * type_, []
    for i in range(len(raw) // size):
        v = [int.from_bytes(raw[size * i + 32 * j:size * i + 32 * j + 32], "little") for j in range(3 * type_)]
        P = tuple(v) if type_ == 1 else ((v[0], v[1]), (v[2], v[3]), (v[4], v[5]))
        assert P[2] in (0, 1, (0, 0), (1, 0))
        out.append(P)
    return out


@pytest.fixture(scope="module")
def made():
    from octopuszk_amd import ceremony
    from octopuszk_amd import zksnark as z
    r1cs, primary, auxiliary = z.serial_construct(NC, NI)
    crs = z.serial_setup_generate(r1cs)
    pk, vk = crs.proving_key, z.verification_key(crs)
    pk2, vk2, rec = ceremony.contribute(pk, vk, D, nonce=U)
    torch.cuda.synchronize()
    return {"pk": pk, "vk": vk, "pk2": pk2, "vk2": vk2, "rec": rec, "primary": primary, "auxiliary": auxiliary}


def test_contribution_matches_the_model_point_for_point(made):
    pk, pk2 = made["pk"], made["pk2"]
    key = {"delta_g1": _points_of(pk.delta_g1, 1)[0], "delta_g2": _points_of(pk.delta_g2, 2)[0],
           "delta_abc_g1": _points_of(pk.delta_abc_g1, 1), "query_h": _points_of(pk.query_h, 1)}
    n = len(key["delta_abc_g1"]) + len(key["query_h"])
    assert n > 64 and n % 64 and len(key["query_h"]) == 129
    new, receipt = cref.contribute_points(key, D, U)
    assert _host(pk2.delta_g1) == cref.wire(1, new["delta_g1"]) and _host(pk2.delta_g2) == cref.wire(2, new["delta_g2"])
    for name in ("delta_abc_g1", "query_h"):
        got, want = _host(getattr(pk2, name)), b"".join(cref.wire(1, P) for P in new[name])
        assert len(got) == len(want)
        for i in range(len(want) // 96):
            assert got[96 * i:96 * i + 96] == want[96 * i:96 * i + 96], (name, i)
    assert made["rec"].to_bytes() == receipt                        # fixed d, nonce: the receipt is the model's
    assert cref.parse_receipt(receipt)["h"] == hashlib.sha256(b"").digest()


def test_contribution_shares_what_it_does_not_change(made):
    pk, pk2, vk, vk2 = made["pk"], made["pk2"], made["vk"], made["vk2"]
    for name in ("alpha_g1", "beta_g1", "beta_g2", "query_a", "query_b_g1", "query_b_g2", "r1cs"):
        assert getattr(pk2, name) is getattr(pk, name), name
    for name in ("delta_g1", "delta_g2", "delta_abc_g1", "query_h"):
        assert getattr(pk2, name) is not getattr(pk, name)
        assert getattr(pk2, name).numel() == getattr(pk, name).numel()
    assert vk2.alpha_g1_beta_g2 is vk.alpha_g1_beta_g2 and vk2.gamma_g2 is vk.gamma_g2
    assert vk2.gamma_abc_g1 is vk.gamma_abc_g1 and vk2.delta_g2 is pk2.delta_g2


def _proof_bytes(p):
    return bytes(p.g_a) + bytes(p.g_b) + bytes(p.g_c)


def test_proofs_follow_the_key(made, tmp_path):
    from octopuszk_amd import zksnark as z
    primary, auxiliary = made["primary"], made["auxiliary"]
    p2 = z.SerialProver(made["pk2"])
    proof2 = p2.prove(primary, auxiliary, seed=5)
    p2.close()
    assert z.Verifier.verify(made["vk2"], primary, proof2)
    assert not z.Verifier.verify(made["vk"], primary, proof2)
    p1 = z.SerialProver(made["pk"])
    proof1 = p1.prove(primary, auxiliary, seed=5)
    p1.close()
    assert z.Verifier.verify(made["vk"], primary, proof1)
    assert not z.Verifier.verify(made["vk2"], primary, proof1)
    path = str(tmp_path / "after.ozkpk")
    made["pk2"].save(path)
    pf = z.SerialProver.from_key_file(path)
    assert _proof_bytes(pf.prove(primary, auxiliary, seed=5)) == _proof_bytes(proof2)
    pf.close()


# ---------------------------------------------------------------------------- verification
def _with(pk, **changes):
    from octopuszk_amd import zksnark as z
    p = z.ProvingKey()
    for name in z._PK_G1 + z._PK_G2 + ("r1cs",):
        setattr(p, name, changes.get(name, getattr(pk, name)))
    return p


def _row(t, i, wire):
    t = t.clone()
    t[96 * i:96 * i + 96] = _dev(wire)
    return t


def _receipt(rec, **changes):
    from octopuszk_amd import ceremony
    f = dict(h=rec.h, delta_g1_before=rec.delta_g1_before, delta_g1_after=rec.delta_g1_after,
             delta_g2_before=rec.delta_g2_before, delta_g2_after=rec.delta_g2_after, r=rec.r, z=rec.z)
    f.update(changes)
    return ceremony.Receipt(**f)


def test_honest_contribution_verifies(made):
    from octopuszk_amd import ceremony
    from octopuszk_amd import zksnark as z
    pk, pk2, rec = made["pk"], made["pk2"], made["rec"]
    for seed in (SEED, 7, None):
        why = []
        assert ceremony.verify_contribution(pk, pk2, rec, vk_before=made["vk"], vk_after=made["vk2"], seed=seed, why=why)
        assert why == []
    assert ceremony.verify_contribution(pk, pk2, rec.to_bytes(), seed=SEED)
    reloaded = z.ProvingKey.from_bytes(pk2.to_bytes())              # through the file: other tensors, decoded anew
    assert reloaded.query_a is not pk.query_a
    stage_ms = {}
    assert ceremony.verify_contribution(pk, reloaded, rec, seed=SEED, stage_ms=stage_ms)
    assert set(stage_ms) == {"compare", "scale", "msms", "pairings"} and all(v >= 0 for v in stage_ms.values())
    jac = _with(pk, query_a=_dev(b"".join(                          # another Z representative is no difference
        cases.wire(1, cases.rescale(1, P, 5 + i) if P[2] else P, 0) for i, P in enumerate(_points_of(pk.query_a, 1)))))
    assert ceremony.verify_contribution(jac, pk2, rec, seed=SEED)


TAMPERS = ("query_h[first]", "query_h[middle]", "query_h[last]", "delta_abc_g1 doubled", "query_h by another d",
           "delta_g2 by another factor", "query_a changed", "r1cs changed", "delta_g1 at infinity", "z + 1",
           "the deltas of another key", "vk_after with the old delta")


def _tamper(made, label):
    """(pk_after, receipt, vk_after, the check that must fail)"""
    from octopuszk_amd import ceremony, codec
    from octopuszk_amd import zksnark as z
    pk, pk2, rec, vk2 = made["pk"], made["pk2"], made["rec"], made["vk2"]
    gen = cref.wire(1, o.G1.one)
    nh = pk2.query_h.numel() // 96
    if label.startswith("query_h["):
        i = {"first": 0, "middle": nh // 2, "last": nh - 1}[label[8:-1]]
        return _with(pk2, query_h=_row(pk2.query_h, i, gen)), rec, vk2, "vectors"
    if label == "delta_abc_g1 doubled":
        t = pk2.delta_abc_g1.clone()
        t[96 * 70:96 * 71] = ceremony.scale_points(t[96 * 70:96 * 71], 2, 1)
        assert not torch.equal(t, pk2.delta_abc_g1)
        return _with(pk2, delta_abc_g1=t), rec, vk2, "vectors"
    if label == "query_h by another d":
        return _with(pk2, query_h=ceremony.scale_points(pk.query_h, pow(D + 1, -1, R), 1)), rec, vk2, "vectors"
    if label == "delta_g2 by another factor":
        d2 = ceremony.scale_points(pk.delta_g2, D + 1, 2)
        return (_with(pk2, delta_g2=d2), _receipt(rec, delta_g2_after=_host(codec.compress_g2(d2))),
                z.VerificationKey(vk2.alpha_g1_beta_g2, vk2.gamma_g2, d2, vk2.gamma_abc_g1), "delta_ratio")
    if label == "query_a changed":
        return _with(pk2, query_a=_row(pk2.query_a, 1, gen)), rec, vk2, "unchanged"
    if label == "r1cs changed":
        r = pk.r1cs
        index = r.A.index.copy()
        index[3] += 1
        other = z.R1CSRelation(z.LinearCombinations(r.A.ptr, index, r.A.value), r.B, r.C, r.num_inputs, r.num_auxiliary)
        return _with(pk2, r1cs=other), rec, vk2, "unchanged"
    if label == "delta_g1 at infinity":
        inf = _dev(cref.wire(1, o.G1.to_affine(o.G1.zero)))
        return _with(pk2, delta_g1=inf), _receipt(rec, delta_g1_after=bytes(31) + b"\x40"), vk2, "delta_wellformed"
    if label == "z + 1":
        return pk2, _receipt(rec, z=(rec.z + 1) % R), vk2, "pok"
    if label == "the deltas of another key":
        return pk2, _receipt(rec, delta_g1_before=cases.encode(1, o.G1.one)), vk2, "receipt_deltas"
    if label == "vk_after with the old delta":
        return pk2, rec, made["vk"], "vk"
    raise KeyError(label)


@pytest.mark.parametrize("label", TAMPERS)
def test_every_tamper_class_is_rejected_by_its_check(made, label):
    from octopuszk_amd import ceremony
    pk_after, rec, vk_after, want = _tamper(made, label)
    for seed in (SEED, None):
        why = []
        ok = ceremony.verify_contribution(made["pk"], pk_after, rec, vk_before=made["vk"], vk_after=vk_after, seed=seed,
                                          why=why)
        assert not ok and why == [want], (label, seed, why)
    assert ceremony.Receipt.from_bytes(rec.to_bytes()).to_bytes() == rec.to_bytes()


def test_chain_of_two_contributions(made):
    from octopuszk_amd import ceremony
    pk, pk2, rec = made["pk"], made["pk2"], made["rec"]
    pk3, vk3, rec3 = ceremony.contribute(pk2, made["vk2"], D2, nonce=U2, previous=rec.to_bytes())
    assert rec3.h == hashlib.sha256(rec.to_bytes()).digest()
    keys, vks = [pk, pk2, pk3], [made["vk"], made["vk2"], vk3]
    assert ceremony.verify_chain(keys, [rec, rec3], vks=vks, seed=SEED)
    assert ceremony.verify_chain(keys, [rec.to_bytes(), rec3.to_bytes()])
    why = []
    assert not ceremony.verify_chain(keys, [rec3, rec], seed=SEED, why=why) and why == ["chain"]
    _, _, stray = ceremony.contribute(pk2, None, D2, nonce=U2, previous=b"not the receipt before")
    why = []
    assert not ceremony.verify_chain(keys, [rec, stray], seed=SEED, why=why) and why == ["chain"]
    # a key that is not the one the receipt was written for breaks the step, not the chain
    why = []
    assert not ceremony.verify_chain([pk, pk3, pk3], [rec, rec3], seed=SEED, why=why) and why == ["receipt_deltas"]
    with pytest.raises(ValueError):
        ceremony.verify_chain(keys, [rec])
