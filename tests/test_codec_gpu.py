"""Point compression and decompression on hardware (octopuszk_amd/codec.py) against the integer model
(tests/codec_ref.py): every output byte and every code, G1 and G2, both uncompressed formats, batch sizes around the
wave size, malformed encodings of every class mixed in, and two streams at once."""
import functools

import pytest
import torch

import codec_cases as cases
import codec_ref as ref

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 4096]
FORMATS = ["wire_in", "wire_out"]


def _dev(b: bytes):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _host(t):
    torch.cuda.synchronize()
    return bytes(t.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _decode_case(type_, n):
    """(encodings, codes, decoded points) of the model, once per (group, size)"""
    encs, bad = cases.encodings(type_, n, seed=7 * type_)
    decoded = [cases.decode(type_, e) for e in encs]
    for pos, (cls, code) in bad.items():
        assert decoded[pos][0] == code != 0, cls
    if n >= 63:
        assert {cls for cls, _ in bad.values()} == set(cases.G1_CLASSES if type_ == 1 else cases.G2_CLASSES)
        assert 0.04 * n <= len(bad) <= max(0.06 * n, 7)
    return encs, [c for c, _ in decoded], [P for _, P in decoded]


@functools.lru_cache(maxsize=None)
def _encode_case(type_, n):
    pts = cases.points(type_, n, seed=100 + type_)
    return pts, [cases.encode(type_, P) for P in pts]


def _decompress(type_, enc, fmt):
    from octopuszk_amd import codec
    return (codec.decompress_g1 if type_ == 1 else codec.decompress_g2)(enc, fmt)


def _compress(type_, pts, fmt):
    from octopuszk_amd import codec
    return (codec.compress_g1 if type_ == 1 else codec.compress_g2)(pts, fmt)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("type_", [1, 2])
def test_decompress_matches_model(type_, n, fmt):
    encs, codes, pts = _decode_case(type_, n)
    f = FORMATS.index(fmt)
    out, got_codes = _decompress(type_, _dev(b"".join(encs)), fmt)
    got_codes = got_codes.cpu().tolist()
    raw = _host(out)
    size = 96 * type_ * (1 + f)
    assert len(raw) == n * size
    assert got_codes == codes
    zero = cases.wire(type_, cases.curve(type_).zero_affine, f)
    for i in range(n):
        assert raw[size * i:size * (i + 1)] == cases.wire(type_, pts[i], f), (i, encs[i].hex())
        if codes[i]:
            assert raw[size * i:size * (i + 1)] == zero   # a point that does not decode is written as O


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("type_", [1, 2])
def test_compress_matches_model(type_, n, fmt):
    pts, want = _encode_case(type_, n)
    f = FORMATS.index(fmt)
    got = _host(_compress(type_, _dev(b"".join(cases.wire(type_, P, f) for P in pts)), fmt))
    size = 32 * type_
    for i in range(n):
        assert got[size * i:size * (i + 1)] == want[i], (i, pts[i])


@pytest.mark.parametrize("type_", [1, 2])
def test_round_trip_on_the_device(type_):
    """compress(decompress(e)) == e for every valid encoding, and O for the others"""
    encs, codes, _ = _decode_case(type_, 4096)
    out, got_codes = _decompress(type_, _dev(b"".join(encs)), "wire_in")
    back = _host(_compress(type_, out, "wire_in"))
    size = 32 * type_
    inf = bytes(size - 1) + bytes([ref.INFINITY])
    for i, e in enumerate(encs):
        assert back[size * i:size * (i + 1)] == (e if codes[i] == 0 else inf), i


def test_side_stream_does_not_disturb_the_current_stream():
    from octopuszk_amd import codec
    e1, c1, p1 = _decode_case(1, 4096)
    e2, c2, p2 = _decode_case(2, 4096)
    d1, d2 = _dev(b"".join(e1)), _dev(b"".join(e2))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out2, codes2 = codec.decompress_g2(d2, "wire_out")
    out1, codes1 = codec.decompress_g1(d1, "wire_out")
    side.synchronize()
    torch.cuda.synchronize()
    assert codes1.cpu().tolist() == c1 and codes2.cpu().tolist() == c2
    assert _host(out1) == b"".join(cases.wire(1, P, 1) for P in p1)
    assert _host(out2) == b"".join(cases.wire(2, P, 1) for P in p2)


def test_proofs_entry_matches_model_and_reports_the_first_code():
    from octopuszk_amd import codec
    g1, _, _ = _decode_case(1, 4096)
    g2, _, _ = _decode_case(2, 4096)
    k = 300
    bufs = [g1[i] + g2[i] + g1[4095 - i] for i in range(k)]
    want = [ref.proof_record(b) for b in bufs]
    assert {c for c, _ in want} == {0, 1, 2, 3}
    recs, codes = codec.decompress_proofs(_dev(b"".join(bufs)))
    assert codes.cpu().tolist() == [c for c, _ in want]
    raw = _host(recs)
    for i in range(k):
        assert raw[768 * i:768 * (i + 1)] == want[i][1], i


def test_bad_arguments_are_errors():
    from octopuszk_amd import codec
    from octopuszk_amd import lib
    good = _dev(bytes(64))
    with pytest.raises(ValueError):
        codec.decompress_g1(_dev(bytes(33)))
    with pytest.raises(ValueError):
        codec.decompress_g2(good, "affine")
    with pytest.raises(TypeError):
        codec.compress_g1(bytes(96))
    L = lib.load()
    out = torch.empty(192, dtype=torch.uint8, device="cuda")
    codes = torch.empty(2, dtype=torch.int32, device="cuda")
    args = (good.data_ptr(), out.data_ptr(), codes.data_ptr())
    assert L.ozk_points_decompress_dev(args[0], -1, 1, 0, args[1], args[2], None) < 0
    assert L.ozk_points_decompress_dev(args[0], 2, 3, 0, args[1], args[2], None) < 0
    assert L.ozk_points_decompress_dev(args[0], 2, 1, 2, args[1], args[2], None) < 0
    assert L.ozk_points_decompress_dev(None, 2, 1, 0, args[1], args[2], None) < 0
    assert L.ozk_points_compress_dev(args[1], 2, 1, 5, args[0], None) < 0
    assert L.ozk_groth16_proofs_decompress_dev(args[0], 0, args[1], args[2], None) < 0
    assert b"format" in L.ozk_last_error() or b"argument" in L.ozk_last_error()
