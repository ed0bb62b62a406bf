"""Compressed Groth16 proofs and verification keys on hardware: Proof.to_bytes / from_bytes, the three *_bytes
checks of the Verifier against the object path on the same proofs, and VerificationKey.to_bytes / from_bytes.  Key
and proofs are built as in tests/test_batch_verify_gpu.py (the 2^10 circuit, one proof per prover seed)."""
import random

import pytest
import torch

import codec_cases as cases
import codec_ref as ref
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

NC, NI = 1 << 10, 15
VALID = 12


@pytest.fixture(scope="module")
def setup():
    from octopuszk_amd import zksnark as z
    r1cs, primary, auxiliary = z.serial_construct(NC, NI)
    crs = z.serial_setup_generate(r1cs)
    vk = z.verification_key(crs)
    prover = z.SerialProver(crs.proving_key)
    try:
        proofs = [prover.prove(primary, auxiliary, seed=2000 + i) for i in range(VALID)]
    finally:
        prover.close()
    assert len({bytes(p.g_a) for p in proofs}) == VALID
    return z, vk, primary, proofs


@pytest.fixture(scope="module")
def batch(setup):
    """16 compressed proofs: 12 valid ones, then -A, -B, a C with no curve point (code 3) and an A with x = q
    (code 1), shuffled at seeded positions.  Returns (buffers, codes, what each one is)."""
    z, vk, primary, proofs = setup
    good = [p.to_bytes() for p in proofs]
    rng = random.Random(16)

    def flipped(b, byte):
        b = bytearray(b)
        b[byte] ^= ref.Y_LARGER
        return bytes(b)

    neg_a = flipped(good[0], 31)
    neg_b = flipped(good[1], 95)
    no_point = good[2][:96] + cases.non_residue_x(1, rng)
    range_a = o.Q.to_bytes(32, "little") + good[3][32:]
    items = [(b, 0, "valid") for b in good]
    items += [(neg_a, 0, "neg_a"), (neg_b, 0, "neg_b"), (no_point, ref.E_NO_POINT, "no_point"),
              (range_a, ref.E_RANGE, "range")]
    rng.shuffle(items)
    assert len(items) == 16
    for b, code, _ in items:
        assert len(b) == 128 and ref.proof_from_bytes(b)[0] == code
    return [b for b, _, _ in items], [c for _, c, _ in items], [w for _, _, w in items]


def _object_verdicts(z, vk, primary, bufs, codes):
    """verify_batch on the objects of the decodable proofs, False for the others"""
    idx = [i for i, c in enumerate(codes) if c == 0]
    objs = [z.Proof.from_bytes(bufs[i]) for i in idx]
    got = z.Verifier.verify_batch(vk, [primary] * len(idx), objs)
    out = [False] * len(bufs)
    for i, v in zip(idx, got):
        out[i] = v
    return out


def test_proof_bytes_round_trip(setup):
    z, vk, primary, proofs = setup
    for p in proofs[:4]:
        b = p.to_bytes()
        assert isinstance(b, bytes) and len(b) == 128
        A, B, C = (o.g1_from_out_le(bytes(p.g_a)), o.g2_from_out_le(bytes(p.g_b)), o.g1_from_out_le(bytes(p.g_c)))
        assert b == ref.proof_to_bytes(A, B, C)
        back = z.Proof.from_bytes(b)
        assert (bytes(back.g_a), bytes(back.g_b), bytes(back.g_c)) == (bytes(p.g_a), bytes(p.g_b), bytes(p.g_c))
        assert z.proof_record(back) == z.proof_record(p)
    many = z.proofs_from_bytes(b"".join(p.to_bytes() for p in proofs))
    assert [z.proof_record(p) for p in many] == [z.proof_record(p) for p in proofs]


def test_from_bytes_names_the_point_and_the_code(setup, batch):
    z = setup[0]
    bufs, codes, what = batch
    with pytest.raises(ValueError, match=r"point C .*code 3"):
        z.Proof.from_bytes(bufs[what.index("no_point")])
    with pytest.raises(ValueError, match=r"point A .*code 1"):
        z.Proof.from_bytes(bufs[what.index("range")])
    with pytest.raises(ValueError):
        z.Proof.from_bytes(bufs[0][:127])
    with pytest.raises(ValueError, match=r"proof 1: point C"):
        z.proofs_from_bytes(bufs[what.index("valid")] + bufs[what.index("no_point")])


def test_a_proof_with_infinity_decodes_to_the_librarys_o(setup):
    z, vk, primary, proofs = setup
    inf_a = bytes(31) + bytes([ref.INFINITY]) + proofs[0].to_bytes()[32:]
    p = z.Proof.from_bytes(inf_a)
    assert bytes(p.g_a) == o.g1_out_le(o.G1.zero_affine)
    inf_b = proofs[0].to_bytes()[:32] + bytes(63) + bytes([ref.INFINITY]) + proofs[0].to_bytes()[96:]
    assert bytes(z.Proof.from_bytes(inf_b).g_b) == o.g2_out_le(o.G2_ZERO_AFFINE)
    # it decodes, and is then judged as the object path judges it
    for b in (inf_a, inf_b):
        want = z.Verifier.verify_batch(vk, [primary], [z.Proof.from_bytes(b)])
        assert z.Verifier.verify_batch_bytes(vk, [primary], b) == want
        assert z.Verifier.verify_all_bytes(vk, [primary], b, seed=1) == want[0]


def test_batch_of_16_equals_the_object_path(setup, batch):
    z, vk, primary, proofs = setup
    bufs, codes, what = batch
    want = _object_verdicts(z, vk, primary, bufs, codes)
    assert [w == "valid" for w in what] == want   # -A and -B are well-formed wrong proofs, the others do not decode
    prims, buf = [primary] * 16, b"".join(bufs)
    for abc in ("auto", "per_proof", "batched"):
        assert z.Verifier.verify_batch_bytes(vk, prims, buf, abc=abc) == want, abc
    assert z.Verifier.verify_batch_rlc_bytes(vk, prims, buf, seed=5) == want
    assert z.Verifier.verify_batch_rlc_bytes(vk, prims, buf) == want
    assert z.Verifier.verify_batch_bytes(vk, prims, bytearray(buf)) == want


def test_verify_all_bytes(setup, batch):
    z, vk, primary, proofs = setup
    bufs, codes, what = batch
    valid = [b for b, w in zip(bufs, what) if w == "valid"]
    assert z.Verifier.verify_all_bytes(vk, [primary] * len(valid), b"".join(valid), seed=3) is True
    assert z.Verifier.verify_all_bytes(vk, [primary] * len(valid), b"".join(valid)) is True
    for w in ("neg_a", "neg_b", "no_point", "range"):
        for pos in (0, 5, len(valid)):
            mixed = valid[:pos] + [bufs[what.index(w)]] + valid[pos:]
            assert z.Verifier.verify_all_bytes(vk, [primary] * len(mixed), b"".join(mixed), seed=3) is False, (w, pos)
    stages = {}
    assert z.Verifier.verify_all_bytes(vk, [primary] * len(valid), b"".join(valid), stage_ms=stages)
    assert stages["decompress"] > 0 and "miller" in stages


def test_device_tensor_buffer_gives_the_same_verdicts(setup, batch):
    z, vk, primary, proofs = setup
    bufs, codes, what = batch
    prims, buf = [primary] * 16, b"".join(bufs)
    d_buf = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    want = z.Verifier.verify_batch_bytes(vk, prims, buf)
    assert z.Verifier.verify_batch_bytes(vk, prims, d_buf) == want
    assert z.Verifier.verify_batch_bytes(vk, prims, d_buf.view(16, 128)) == want
    assert z.Verifier.verify_batch_rlc_bytes(vk, prims, d_buf, seed=9) == want
    assert z.Verifier.verify_all_bytes(vk, prims, d_buf, seed=9) is False
    valid = [b for b, w in zip(bufs, what) if w == "valid"]
    d_valid = torch.frombuffer(bytearray(b"".join(valid)), dtype=torch.uint8).cuda()
    assert z.Verifier.verify_all_bytes(vk, [primary] * len(valid), d_valid, seed=9) is True
    with pytest.raises(ValueError):
        z.Verifier.verify_batch_bytes(vk, prims, buf[:-1])
    with pytest.raises(ValueError):
        z.Verifier.verify_all_bytes(vk, prims[:15], buf)


def test_verification_key_round_trip(setup, batch):
    z, vk, primary, proofs = setup
    bufs, codes, what = batch
    raw = vk.to_bytes()
    assert len(raw) == 16 + 384 + 128 + 32 * NI and raw[:8] == ref.VK_MAGIC
    assert int.from_bytes(raw[8:12], "little") == NI and raw[12:16] == bytes(4)
    # the model reads the same key
    gt, gamma, delta, abc = ref.vk_from_bytes(raw)
    host = lambda t: bytes(t.cpu().numpy())
    assert gt == host(vk.alpha_g1_beta_g2)
    assert o.g2_to_wire(gamma) == host(vk.gamma_g2) and o.g2_to_wire(delta) == host(vk.delta_g2)
    assert b"".join(o.g1_to_wire(P) for P in abc) == host(vk.gamma_abc_g1)
    vk2 = z.VerificationKey.from_bytes(raw)
    assert vk2.num_inputs == vk.num_inputs and vk2.to_bytes() == raw
    for name in ("alpha_g1_beta_g2", "gamma_g2", "delta_g2", "gamma_abc_g1"):
        assert host(getattr(vk2, name)) == host(getattr(vk, name)), name
    assert host(vk2.gamma_prep.data) == host(vk.gamma_prep.data)
    prims, buf = [primary] * 16, b"".join(bufs)
    want = z.Verifier.verify_batch_bytes(vk, prims, buf)
    assert z.Verifier.verify_batch_bytes(vk2, prims, buf) == want
    assert z.Verifier.verify_batch_rlc_bytes(vk2, prims, buf, seed=2) == want
    objs = [z.Proof.from_bytes(b) for b, w in zip(bufs, what) if w == "valid"]
    assert z.Verifier.verify_all(vk2, [primary] * len(objs), objs, seed=2) is True


def test_broken_key_bytes_raise(setup):
    z, vk, primary, proofs = setup
    raw = vk.to_bytes()
    bad_abc = raw[:528 + 32 * 4] + cases.non_residue_x(1, random.Random(8)) + raw[528 + 32 * 5:]
    with pytest.raises(ValueError, match=r"gammaABC\[4\].*code 3"):
        z.VerificationKey.from_bytes(bad_abc)
    for broken in (raw[:-1], raw[:100], b"", b"X" + raw[1:], raw[:7] + b"\x02" + raw[8:], raw[:12] + b"\x01" + raw[13:],
                   raw + bytes(32)):
        with pytest.raises(ValueError):
            z.VerificationKey.from_bytes(broken)
