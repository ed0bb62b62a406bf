"""Proving keys through the key file on hardware: compressed points decoded straight into the
prepared bases against decompress + prepare, byte for byte and code for code; the subgroup check against r-multiples in
oracle integers; a 2^10-constraint key saved, loaded both ways and proved with, serially and as two ranks that read
only their rows; and a corrupted file."""
import functools
import io
import random

import pytest
import torch

import codec_cases as cases
import codec_ref as ref
import keyfile_ref as kref
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 4096]
NC, NI = 1 << 10, 15


def _dev(b: bytes):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    torch.cuda.synchronize()
    return bytes(t.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _case(type_, n):
    """(the encodings as one bytes object; the records and codes of decompress + prepare): the codec cases with
    infinity encodings added, once per (group, size)"""
    from octopuszk_amd import codec
    from octopuszk_amd.device import prepare_bases
    encs, bad = cases.encodings(type_, n, seed=7 * type_)
    inf = cases.encode(type_, cases.curve(type_).zero)
    if n > 1:
        for pos in {n // 3, n - 1} - set(bad):
            encs[pos] = inf
    if n >= 63:
        assert {cls for cls, _ in bad.values()} == set(cases.G1_CLASSES if type_ == 1 else cases.G2_CLASSES)
        assert inf in encs
    enc = b"".join(encs)
    wire, codes = (codec.decompress_g1 if type_ == 1 else codec.decompress_g2)(_dev(enc), "wire_in")
    want = _host(prepare_bases(wire, n, type_))[:2 * n * 64 * type_]
    return enc, want, codes.cpu().tolist()


@pytest.mark.parametrize("side_stream", [False, True])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("type_", [1, 2])
def test_fused_decode_equals_decompress_then_prepare(type_, n, side_stream):
    from octopuszk_amd import codec
    enc, want, want_codes = _case(type_, n)
    d_enc = _dev(enc)
    torch.cuda.synchronize()
    if side_stream:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            got, codes = codec.decompress_prepared(d_enc, type_)
        s.synchronize()
    else:
        got, codes = codec.decompress_prepared(d_enc, type_)
    assert codes.cpu().tolist() == want_codes
    if n >= 63:
        assert set(want_codes) == {0, 1, 2, 3}
    raw = _host(got)
    assert len(raw) >= len(want) and raw[:len(want)] == want
    rec = 64 * type_
    for i, code in enumerate(want_codes):
        if code:   # a point that does not decode is the (0, 0) marker in both records
            assert raw[rec * i:rec * (i + 1)] == bytes(rec) == raw[rec * (n + i):rec * (n + i + 1)]


@pytest.mark.parametrize("type_", [1, 2])
def test_fused_decode_matches_the_integer_model(type_):
    from octopuszk_amd import codec
    n = 65
    enc, _, _ = _case(type_, n)
    size = 32 * type_
    want, want_codes = kref.prepared(type_, [enc[size * i:size * (i + 1)] for i in range(n)])
    got, codes = codec.decompress_prepared(_dev(enc), type_)
    assert codes.cpu().tolist() == want_codes
    assert _host(got)[:len(want)] == want


def test_argument_checks():
    from octopuszk_amd import codec, lib
    from octopuszk_amd.device import _ptr
    L = lib.load()
    n = 64
    enc = _dev(_case(1, n)[0])
    nbytes = int(L.ozk_var_msm_prepared_bytes(n, 1))
    out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    codes = torch.empty(n, dtype=torch.int32, device="cuda")
    INVALID = -1   # OZK_E_INVALID (include/ozk.h)
    assert L.ozk_points_decompress_prepared_dev(_ptr(enc), n, 1, _ptr(out), nbytes - 1, _ptr(codes), 0, None) == INVALID
    assert L.ozk_points_decompress_prepared_dev(_ptr(enc), (1 << 23) + 1, 1, _ptr(out), 1 << 40, _ptr(codes), 0,
                                                None) == INVALID
    assert L.ozk_points_decompress_prepared_dev(_ptr(enc), n, 3, _ptr(out), nbytes, _ptr(codes), 0, None) == INVALID
    assert L.ozk_points_decompress_prepared_dev(_ptr(enc), n, 1, _ptr(out), nbytes, _ptr(codes), 0, None) == 0
    torch.cuda.synchronize()
    with pytest.raises(TypeError):
        codec.decompress_prepared(bytes(64), 1)
    with pytest.raises(ValueError):
        codec.decompress_prepared(enc[:33], 1)


def test_subgroup_check():
    from octopuszk_amd import codec
    rng = random.Random(99)
    inside = [o.G2.to_affine(o.G2.mul(o.G2.one, rng.randrange(1, o.R))) for _ in range(32)]
    outside = []
    while len(outside) < 32:   # twist points from random x: the cofactor is about 2^254
        enc = cases._le(rng.randrange(o.Q)) + cases._le(rng.randrange(o.Q))
        code, P = ref.decode_g2(enc)
        if code == 0:
            outside.append(P)
    pts = [P for pair in zip(inside, outside) for P in pair]   # interleaved: both kinds in every half wave
    member = [kref.in_subgroup(P) for P in pts]
    assert member == [True, False] * 32                        # on the CPU: all 32 of the second kind are outside
    encs = [cases.encode(2, P) for P in pts]
    want, _ = kref.prepared(2, encs)
    d_enc = _dev(b"".join(encs))
    got, codes = codec.decompress_prepared(d_enc, 2, check_subgroup=False)
    assert codes.cpu().tolist() == [0] * 64 and _host(got)[:len(want)] == want
    got, codes = codec.decompress_prepared(d_enc, 2, check_subgroup=True)
    assert codes.cpu().tolist() == [0, codec.E_SUBGROUP] * 32
    assert codec.E_SUBGROUP == 4 and codec.CODE_NAMES[4]
    raw = _host(got)
    for i in range(64):
        for base in (i, 64 + i):
            rec = raw[128 * base:128 * (base + 1)]
            assert rec == (want[128 * base:128 * (base + 1)] if member[i] else bytes(128)), (i, base)
    # G1 ignores the flag
    enc1, want1, codes1 = _case(1, 65)
    got1, c1 = codec.decompress_prepared(_dev(enc1), 1, check_subgroup=True)
    assert c1.cpu().tolist() == codes1 and _host(got1)[:len(want1)] == want1


# ---------------------------------------------------------------------------- a key, saved and loaded
@pytest.fixture(scope="module")
def key(tmp_path_factory):
    from octopuszk_amd import zksnark as z
    r1cs, primary, auxiliary = z.serial_construct(NC, NI)
    crs = z.serial_setup_generate(r1cs)
    pk = crs.proving_key
    path = str(tmp_path_factory.mktemp("key") / "proving.ozkpk")
    pk.save(path)
    prover = z.SerialProver(pk)
    proof = prover.prove(primary, auxiliary)
    prover.close()
    with open(path, "rb") as f:
        raw = f.read()
    return {"crs": crs, "pk": pk, "path": path, "raw": raw, "primary": primary, "auxiliary": auxiliary, "proof": proof}


def _proof_bytes(p):
    return bytes(p.g_a) + bytes(p.g_b) + bytes(p.g_c)


def test_key_round_trip(key):
    from octopuszk_amd import keyfile
    from octopuszk_amd import zksnark as z
    from octopuszk_amd.device import prepare_bases
    pk = key["pk"]
    assert pk.to_bytes() == key["raw"]
    kref.parse(key["raw"])                                     # the model reads what the library wrote
    pk2 = z.ProvingKey.load(key["path"])
    assert z.ProvingKey.from_bytes(key["raw"]).query_h.numel() == pk.query_h.numel()
    for name in keyfile.NAMES[:10]:
        type_ = 2 if name in kref.G2_NAMES else 1
        a, b = getattr(pk, name), getattr(pk2, name)
        n = a.numel() // (96 * type_)
        assert b.numel() == a.numel()
        assert _host(prepare_bases(a, n, type_))[:n * 128 * type_] == _host(prepare_bases(b, n, type_))[:n * 128 * type_], name
    for s1, s2 in zip((pk.r1cs.A, pk.r1cs.B, pk.r1cs.C), (pk2.r1cs.A, pk2.r1cs.B, pk2.r1cs.C)):
        assert list(s1.ptr) == list(s2.ptr) and list(s1.index) == list(s2.index) and s2.value is None
    assert (pk2.r1cs.num_inputs, pk2.r1cs.num_auxiliary, pk2.r1cs.num_constraints) == (NI, 3 + NC - NI, NC)
    # every current consumer works on the loaded key
    p2 = z.SerialProver(pk2)
    assert _proof_bytes(p2.prove(key["primary"], key["auxiliary"])) == _proof_bytes(key["proof"])
    p2.close()


def test_prover_from_key_file(key):
    from octopuszk_amd import zksnark as z
    want = z.SerialProver(key["pk"])
    prover = z.SerialProver.from_key_file(key["path"])
    for a in ("qa", "qb1", "qb2", "dabc", "qh"):
        n = getattr(want, a).numel()
        assert getattr(prover, a).numel() == n
    assert prover.key_bytes == want.key_bytes
    want.close()
    proof = prover.prove(key["primary"], key["auxiliary"])
    prover.close()
    assert _proof_bytes(proof) == _proof_bytes(key["proof"])
    assert proof.to_bytes() == key["proof"].to_bytes()
    assert z.Verifier.verify(z.verification_key(key["crs"]), key["primary"], proof)


class _Recording(io.BytesIO):
    """a file that records every (offset, length) read"""

    def __init__(self, b):
        super().__init__(b)
        self.reads = []

    def read(self, n=-1):
        at = self.tell()
        out = super().read(n)
        self.reads.append((at, len(out)))
        return out


def test_sharded_load_reads_only_its_rows(key):
    from octopuszk_amd import device, keyfile
    from octopuszk_amd import zksnark as z
    table = keyfile.KeyFile(key["raw"]).header.table
    nv, m = NI + 3 + NC - NI, z.lowest_power_of_two(NC + NI)
    arrays = ("query_a", "query_b_g1", "query_b_g2", "delta_abc_g1", "query_h")
    records, touched = [], []
    for rank in range(2):
        f = _Recording(key["raw"])
        prover = z.ShardedProver.from_key_file(f, rank, 2)
        records.append(prover.prove_partial(key["primary"], key["auxiliary"]))
        prover.close()
        plan = z.shard_plan(nv, m, nv - NI, rank, 2)
        mine = {}
        for attr, pkey, names, type_ in z.ShardedProver._MSMS:
            lo, hi = plan[pkey]
            rows = keyfile.KeyFile(key["raw"]).rows(names[0])
            mine[names[0]] = (lo, min(hi, rows))
        seen = {}
        for name in arrays:
            off, length = table[name]
            stride = keyfile.STRIDE[name]
            got = set()
            for at, n in f.reads:
                a, b = max(at, off), min(at + n, off + length)
                if a < b:
                    assert (a - off) % stride == 0 and (b - off) % stride == 0
                    got |= set(range((a - off) // stride, (b - off) // stride))
            assert got == set(range(*mine[name])), (rank, name)     # its rows and no others
            seen[name] = got
        touched.append(seen)
    for name in arrays:
        assert not touched[0][name] & touched[1][name]
        assert len(touched[0][name] | touched[1][name]) == table[name][1] // keyfile.STRIDE[name]
    proof = device.groth16_combine(torch.cat(records), 2)
    assert _proof_bytes(proof) == _proof_bytes(key["proof"])


def test_corrupted_point_is_named(key):
    from octopuszk_amd import codec, keyfile
    from octopuszk_amd import zksnark as z
    off, _ = keyfile.KeyFile(key["raw"]).header.table["query_b_g2"]
    entry = key["raw"][off + 64 * 17:off + 64 * 18]
    # one flipped bit of x after which, by the model, no curve point has this x
    for bit in range(200):
        flipped = bytearray(entry)
        flipped[bit >> 3] ^= 1 << (bit & 7)
        code, _ = ref.decode_g2(bytes(flipped))
        if code == ref.E_NO_POINT:
            break
    assert code == ref.E_NO_POINT
    bad = bytearray(key["raw"])
    bad[off + 64 * 17 + (bit >> 3)] ^= 1 << (bit & 7)
    bad = bytes(bad)
    for load in (lambda **kw: z.SerialProver.from_key_file(io.BytesIO(bad), **kw),
                 lambda **kw: z.ProvingKey.from_bytes(bad, **kw),
                 lambda **kw: z.ShardedProver.from_key_file(io.BytesIO(bad), 0, 2, **kw)):
        with pytest.raises(ValueError) as e:
            load(verify_digest=False)
        msg = str(e.value)
        assert "query_b_g2" in msg and "17" in msg and codec.CODE_NAMES[codec.E_NO_POINT] in msg, msg
        with pytest.raises(ValueError) as e:
            load(verify_digest=True)
        assert "digest" in str(e.value)
    with pytest.raises(ValueError) as e:
        z.SerialProver.from_key_file(io.BytesIO(bad))          # the digest check is on by default for a world of one
    assert "digest" in str(e.value)
