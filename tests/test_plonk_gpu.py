"""GPU tests of the PLONK prover: the three entry points of csrc/plonk.cuh against the integer
model (tests/plonk_ref.py), byte for byte, with sentinel-filled outputs and gaps, and the protocol of octopuszk_amd/plonk
over a string of known tau, where every commitment and proof point is [p(tau)] g1."""
import ctypes
import random

import pytest
import torch

import kzg_ref as kr
import plonk_ref as pm
import srs_gpu_util as u
from fr_gpu_util import perm_product as _perm_product
from fr_gpu_util import plonk_quotient as _quotient
from fr_gpu_util import rows_coset as _rows_coset
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

R = o.R
T = 1024                       # PLONK_TILE = PLONK_CO_TILE: the elements one workgroup handles
BATCH = 8                      # KZG_INV_BATCH: the rows of one lane of the grand product, inverted together
SCAN = 256                     # PLONK_SCAN_WG: the tile products one round of the scan takes
E_INVALID = -1
TAU = 0x5eed0123456789abcdef0123456789abcdef0123456789abcdef % R
M = 512                        # 2 M + 1 >= 1024 powers in G1
SENTINEL = 0xA5
SENTINEL_INT = int.from_bytes(bytes([SENTINEL]) * 32, "little")


def _lib():
    from octopuszk_amd import lib
    return lib.load()


def _ptr(t):
    return ctypes.c_void_p(int(t.data_ptr()))


def _stream():
    return ctypes.c_void_p(int(torch.cuda.current_stream().cuda_stream))


def _host_ints(values):
    buf = ctypes.create_string_buffer(b"".join(kr.le(v) for v in values), 32 * len(values))
    return buf, ctypes.cast(buf, ctypes.c_void_p)


def _ws(nbytes):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="cuda")


def _flat(rows, stride, fill=7):
    out = []
    for row in rows:
        out += list(row) + [fill] * (stride - len(row))
    return out


# ---------------------------------------------------------------------------- rows by powers
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("length", [1, 255, T, T + 1, 2 * T + 1])
def test_rows_coset_matches_the_model(k, length):
    rng = random.Random(2900 + 10 * length + k)
    rows = [[rng.randrange(R) for _ in range(length)] for _ in range(k)]
    written = [list(row) for row in rows]
    written[k - 1][length // 2] += R                                      # one element written as x + r
    c = rng.randrange(R)
    for s in (1, pm.G):
        for out_len in (length, 4 * length):
            stride, out_stride = length + 3, out_len + 2
            got, gaps = _rows_coset(_flat(written, stride), k, length, stride, s, c, out_len, out_stride)
            assert got == pm.rows_coset(rows, s, c, out_len), (s, out_len)
            assert all(v == SENTINEL_INT for v in gaps)
        # in place: the input's gaps stay as they are
        stride = length + 3
        got, gaps = _rows_coset(_flat(written, stride), k, length, stride, s, c + R if c + R < 1 << 256 else c, length,
                                stride, in_place=True)
        assert got == pm.rows_coset(rows, s, c) and all(v == 7 for v in gaps)


# ---------------------------------------------------------------------------- the grand product
def _random_rows(rng, length):
    return [[rng.getrandbits(253) for _ in range(length)] for _ in range(3)]


def _omega_for(length):
    """an element whose first `length` powers differ"""
    n = 2
    while n < length:
        n *= 2
    return kr.root(n)


LENGTHS = [1, BATCH - 1, BATCH, BATCH + 1, T - 1, T, T + 1, 2 * T + 1]


@pytest.mark.parametrize("length", LENGTHS)
def test_perm_product_matches_the_model(length):
    rng = random.Random(2910 + length)
    wires, sigma = _random_rows(rng, length), _random_rows(rng, length)
    written = [list(row) for row in wires]
    written[1][length // 2] += R                                          # one element written as w + r
    omega, beta, gamma = _omega_for(length), rng.randrange(R), rng.randrange(R)
    z, behind, total, zeros = _perm_product(written, sigma, length, length + 3, omega, beta, gamma)
    want = pm.perm_product(wires, sigma, omega, pm.KS, beta, gamma)
    assert (z, total, zeros) == want and zeros == 0 and z[0] == 1
    assert behind == [SENTINEL_INT] * 2


@pytest.mark.parametrize("length", LENGTHS)
def test_perm_product_of_a_valid_permutation_closes(length):
    rng = random.Random(2920 + length)
    values = [rng.randrange(R) for _ in range(max(1, length // 2))]
    cells = pm.Circuit(length, [], [[rng.randrange(len(values)) for _ in range(length)] for _ in range(3)], 0)
    omega, beta, gamma = _omega_for(length), rng.randrange(R), rng.randrange(R)
    wires, sigma = cells.wire_values(values), pm.sigma_labels(cells, omega)
    z, _, total, zeros = _perm_product(wires, sigma, length, length, omega, beta, gamma)
    assert (z, total, zeros) == pm.perm_product(wires, sigma, omega, pm.KS, beta, gamma)
    assert total == 1 and zeros == 0


@pytest.mark.parametrize("length,at", [(BATCH - 1, 0), (BATCH + 1, 3), (T + 1, T - 1), (2 * T + 1, T + BATCH + 3),
                                       (2 * T + 1, 2 * T)])
def test_perm_product_with_one_zero_denominator(length, at):
    """first of all, in the middle of a batch, last of a tile, in a later tile, last of all: the row's factor is 1, the
    count is 1 and every other factor is exact"""
    rng = random.Random(2930 + length + at)
    wires, sigma = _random_rows(rng, length), _random_rows(rng, length)
    omega, beta = _omega_for(length), rng.randrange(R)
    j = at % 3
    gamma = -(wires[j][at] + beta * sigma[j][at]) % R
    z, _, total, zeros = _perm_product(wires, sigma, length, length, omega, beta, gamma)
    want = pm.perm_product(wires, sigma, omega, pm.KS, beta, gamma)
    assert want[2] == 1 and (z, total, zeros) == want
    if at + 1 < length:
        assert z[at + 1] == z[at]


def test_perm_product_past_one_round_of_the_scan():
    """SCAN tiles + 1: the scan of the tile products, one level for any length, takes a second round of SCAN tiles"""
    length = SCAN * T + T + 1
    rng = random.Random(2940)
    wires, sigma = _random_rows(rng, length), _random_rows(rng, length)
    omega, beta, gamma = _omega_for(length), rng.randrange(R), rng.randrange(R)
    z, _, total, zeros = _perm_product(wires, sigma, length, length, omega, beta, gamma)
    assert (z, total, zeros) == pm.perm_product(wires, sigma, omega, pm.KS, beta, gamma)


# ---------------------------------------------------------------------------- the quotient
def _coset_rows(rows, n):
    w4 = kr.root(4 * n)
    return [kr.ntt(row, w4) for row in pm.rows_coset(rows, pm.G, 1, 4 * n)]


def _quotient_inputs(n, break_gate=False):
    """(the five witness rows and the ten key rows on the coset, the challenges) of a valid or a broken witness"""
    rng = random.Random(2950 + n)
    circuit, assignment = pm.chain(n, 1, rng, constant=n >= 8)
    if break_gate:
        assignment = assignment[:-1] + [(assignment[-1] + 1) % R] if n > 2 else [(assignment[0] + 1) % R]
    omega = kr.root(n)
    alpha, beta, gamma = (rng.randrange(R) for _ in range(3))
    wires = circuit.wire_values(assignment)
    public = circuit.public_inputs(assignment) if n > 2 or not break_gate else [(assignment[0] - 1) % R]
    zs, total, _ = pm.perm_product(wires, pm.sigma_labels(circuit), omega, pm.KS, beta, gamma)
    assert total == 1
    wit = [kr.intt(col, omega) for col in wires] + [kr.intt(zs, omega), kr.intt(pm.pi_evals(n, public), omega)]
    key = pm.key_polys(circuit) + [[pm.inv(n)] * n, [0, 1] + [0] * (n - 2)]
    return _coset_rows(wit, n), _coset_rows(key, n), (alpha, beta, gamma)


@pytest.mark.parametrize("n", [2, 4, 256, 1024])
def test_quotient_of_a_valid_witness_is_a_polynomial(n):
    wit, key, ch = _quotient_inputs(n)
    written = [list(row) for row in wit]
    written[3][4 * n - 1] += R                                            # Z's last value, read again by point 4 n - 5
    got = _quotient(written, key, n, ch, 4 * n + 3, 4 * n + 1)
    assert got == pm.quotient_on_coset(wit, key, n, *ch, pm.KS, pm.zh_inverses(n))
    t = pm.rows_coset([kr.intt(got, kr.root(4 * n))], pm.inv(pm.G), 1)[0]
    assert t[3 * n:] == [0] * n


@pytest.mark.parametrize("n", [2, 4, 256, 1024])
def test_quotient_of_a_broken_gate_is_no_polynomial(n):
    wit, key, ch = _quotient_inputs(n, break_gate=True)
    got = _quotient(wit, key, n, ch, 4 * n, 4 * n)
    assert got == pm.quotient_on_coset(wit, key, n, *ch, pm.KS, pm.zh_inverses(n))
    t = pm.rows_coset([kr.intt(got, kr.root(4 * n))], pm.inv(pm.G), 1)[0]
    assert any(t[3 * n:])


# ---------------------------------------------------------------------------- rejections
def test_rejected_shapes_launch_nothing():
    L = _lib()
    n = 8
    buf = torch.full((40 * 4 * n * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    ws = _ws(1 << 20)
    null = ctypes.c_void_p(0)
    stream = _stream()
    keep_one, one = _host_ints([1])
    keep_ks, ks = _host_ints(list(pm.KS))
    keep_zh, zh = _host_ints(pm.zh_inverses(n))
    rows, out = buf[:3 * n * 32], buf[3 * n * 32:]

    def coset(r, k, length, stride, s, c, o_, out_len, ostride, w=_ptr(ws), wbytes=1 << 20):
        return L.ozk_fr_rows_coset_dev(r, k, length, stride, s, c, o_, out_len, ostride, w, wbytes, stream)

    for bad in ((0, n, n), (3, 0, n), (3, n, n - 1), (3, n, (1 << 28) // 3 + 1)):
        assert L.ozk_fr_rows_coset_workspace_bytes(*bad) == 0
        assert coset(null, bad[0], bad[1], n, null, null, null, bad[2], bad[2], w=null, wbytes=0) == E_INVALID
    assert coset(_ptr(rows), 3, n, n - 1, one, one, _ptr(out), n, n) == E_INVALID
    assert coset(_ptr(rows), 3, n, n, one, one, _ptr(out), 2 * n, 2 * n - 1) == E_INVALID
    for args in ((null, one, one, _ptr(out)), (_ptr(rows), null, one, _ptr(out)), (_ptr(rows), one, null, _ptr(out)),
                 (_ptr(rows), one, one, null)):
        assert coset(args[0], 3, n, n, args[1], args[2], args[3], n, n) == E_INVALID
    assert coset(_ptr(rows), 3, n, n, one, one, _ptr(out), n, n, w=null) == E_INVALID
    assert coset(_ptr(buf[8:]), 3, n, n, one, one, _ptr(out), n, n) == E_INVALID
    assert coset(_ptr(rows), 3, n, n, one, one, _ptr(out[8:]), n, n) == E_INVALID
    assert b"aligned" in L.ozk_last_error()
    assert coset(_ptr(rows), 3, n, n, one, one, _ptr(rows[32:]), n, n) == E_INVALID
    assert b"overlap" in L.ozk_last_error()
    assert coset(_ptr(rows), 3, n, n, one, one, _ptr(rows), 2 * n, 2 * n) == E_INVALID     # in place only at equal lengths
    assert coset(_ptr(rows), 3, n, n, one, one, _ptr(rows), n, n + 1) == E_INVALID         # .. and equal strides
    wsb = L.ozk_fr_rows_coset_workspace_bytes(3, n, n)
    assert coset(_ptr(rows), 3, n, n, one, one, _ptr(out), n, n, wbytes=wsb - 1) == E_INVALID
    assert b"workspace" in L.ozk_last_error()

    wires, sigma, z = buf[:3 * n * 32], buf[3 * n * 32:6 * n * 32], buf[6 * n * 32:7 * n * 32]
    total, count = buf[7 * n * 32:7 * n * 32 + 32], buf[7 * n * 32 + 32:7 * n * 32 + 64]

    def perm(w_, s_, length, stride, om, k_, be, ga, z_, t_, c_, w=_ptr(ws), wbytes=1 << 20):
        return L.ozk_fr_perm_product_dev(w_, s_, length, stride, om, k_, be, ga, z_, t_, c_, w, wbytes, stream)

    good = [_ptr(wires), _ptr(sigma), n, n, one, ks, one, one, _ptr(z), _ptr(total), _ptr(count)]
    for bad in (0, -1, (1 << 28) + 1):
        assert L.ozk_fr_perm_product_workspace_bytes(bad) == 0
        assert perm(null, null, bad, bad, null, null, null, null, null, null, null, w=null, wbytes=0) == E_INVALID
    assert perm(*(good[:3] + [n - 1] + good[4:])) == E_INVALID
    for i in (0, 1, 4, 5, 6, 7, 8, 9, 10):
        assert perm(*(good[:i] + [null] + good[i + 1:])) == E_INVALID
    assert perm(*good, w=null) == E_INVALID
    for i, off in ((0, wires[8:]), (1, sigma[8:]), (8, z[8:]), (9, total[8:])):
        assert perm(*(good[:i] + [_ptr(off)] + good[i + 1:])) == E_INVALID
        assert b"aligned" in L.ozk_last_error()
    assert perm(*(good[:10] + [_ptr(count[1:])])) == E_INVALID
    for z_bad in (wires, sigma[(3 * n - 1) * 32:]):
        assert perm(*(good[:8] + [_ptr(z_bad)] + good[9:])) == E_INVALID
        assert b"overlap" in L.ozk_last_error()
    assert perm(*(good[:9] + [_ptr(z[32:])] + good[10:])) == E_INVALID                     # the total inside z
    assert perm(*(good[:10] + [_ptr(total)])) == E_INVALID                                  # the count inside the total
    assert perm(*good, wbytes=L.ozk_fr_perm_product_workspace_bytes(n) - 1) == E_INVALID
    assert b"workspace" in L.ozk_last_error()

    n4 = 4 * n
    wit, key, t_out = buf[:5 * n4 * 32], buf[5 * n4 * 32:15 * n4 * 32], buf[15 * n4 * 32:16 * n4 * 32]

    def quot(w_, ws_, k_, ks_, n_, al, be, ga, kk, zz, o_):
        return L.ozk_plonk_quotient_dev(w_, ws_, k_, ks_, n_, al, be, ga, kk, zz, o_, stream)

    good = [_ptr(wit), n4, _ptr(key), n4, n, one, one, one, ks, zh, _ptr(t_out)]
    for bad in (0, 1, 6, (1 << 26) + 1, 1 << 27):
        assert quot(null, n4, null, n4, bad, null, null, null, null, null, null) == E_INVALID
    assert quot(*(good[:1] + [n4 - 1] + good[2:])) == E_INVALID
    assert quot(*(good[:3] + [n4 - 1] + good[4:])) == E_INVALID
    for i in (0, 2, 5, 6, 7, 8, 9, 10):
        assert quot(*(good[:i] + [null] + good[i + 1:])) == E_INVALID
    for i, off in ((0, wit[8:]), (2, key[8:]), (10, t_out[8:])):
        assert quot(*(good[:i] + [_ptr(off)] + good[i + 1:])) == E_INVALID
        assert b"aligned" in L.ozk_last_error()
    for o_bad in (wit[(5 * n4 - 1) * 32:], key[(10 * n4 - 1) * 32:]):
        assert quot(*(good[:10] + [_ptr(o_bad)])) == E_INVALID
        assert b"overlap" in L.ozk_last_error()
    torch.cuda.synchronize()
    assert u.host(buf) == bytes([SENTINEL]) * buf.numel()


# ---------------------------------------------------------------------------- the protocol
@pytest.fixture(scope="module")
def string():
    from octopuszk_amd import kzg, srs
    s = srs.Srs.from_secrets(M, TAU, 1, 1, generator=1)
    return s, kzg.VerifyKey.from_srs(s)


def _model_string():
    _, (g2, tau_g2) = kr.string(1, TAU)
    return o.G1.to_affine(o.G1.one), g2, tau_g2


@pytest.fixture(scope="module", params=[(8, 1), (1024, 3)], ids=["n8", "n1024"])
def proved(request, string):
    """one circuit set up and proved by the package and by the model"""
    from octopuszk_amd import kzg, plonk
    n, n_public = request.param
    s, kvk = string
    model, assignment = pm.chain(n, n_public, random.Random(2960 + n))
    circuit = plonk.Circuit(n, model.selectors, model.wires, n_public)
    pk, vk = plonk.setup(circuit, kzg.CommitKey.from_srs(s, n))
    st = pm.setup(model, TAU)
    return {"model": model, "assignment": assignment, "pk": pk, "vk": vk, "kvk": kvk, "st": st,
            "proof": plonk.prove(pk, assignment), "want": pm.prove(model, assignment, TAU, st)}


def test_setup_and_proof_are_the_models(proved):
    from octopuszk_amd import plonk
    vk, proof, want = proved["vk"], proved["proof"], proved["want"]
    assert vk.to_bytes() == proved["st"]["vk"]                           # eight commitments [p(tau)] g1
    assert list(proof.commitments) == want["commitments"] and list(proof.values) == want["values"]
    assert proof.to_bytes() == want["bytes"] and len(proof.to_bytes()) == plonk.PROOF_BYTES == 800
    assert plonk.verify(vk, proved["kvk"], want["public"], proof)
    again = plonk.Proof.from_bytes(proof.to_bytes())
    assert plonk.verify(plonk.VerifyingKey.from_bytes(vk.to_bytes()), proved["kvk"], want["public"], again)
    assert plonk.verify(vk, proved["kvk"], want["public"], proof.to_bytes())
    assert pm.verify_bytes(vk.to_bytes(), want["public"], proof.to_bytes(), *_model_string())


def test_a_wrong_public_input_is_refused(proved):
    from octopuszk_amd import plonk
    public = list(proved["want"]["public"])
    public[-1] = (public[-1] + 1) % R
    assert not plonk.verify(proved["vk"], proved["kvk"], public, proved["proof"])
    assert not plonk.verify(proved["vk"], proved["kvk"], public[:-1], proved["proof"])


@pytest.mark.parametrize("section", range(7 + 16 + 2))
def test_a_flipped_bit_is_refused(proved, section):
    from octopuszk_amd import plonk
    raw = bytearray(proved["proof"].to_bytes())
    raw[32 * section + 1] ^= 4
    assert not plonk.verify(proved["vk"], proved["kvk"], proved["want"]["public"], bytes(raw))


def test_z_replaced_by_a_is_refused(proved):
    from octopuszk_amd import plonk
    p = proved["proof"]
    cs = list(p.commitments)
    cs[3] = cs[0]
    assert not plonk.verify(proved["vk"], proved["kvk"], proved["want"]["public"], plonk.Proof(cs, p.values, p.w, p.w2))


def test_an_honest_opening_of_an_altered_value_fails_the_identity(proved):
    """t_lo opened honestly with 1 added: verify_multi passes, the identity does not"""
    from octopuszk_amd import kzg, plonk
    from octopuszk_amd.plonk import protocol
    vk, kvk = proved["vk"], proved["kvk"]
    bad = pm.prove(proved["model"], proved["assignment"], TAU, proved["st"], tamper_t=True)
    proof = plonk.Proof.from_bytes(bad["bytes"])
    assert not plonk.verify(vk, kvk, bad["public"], proof)
    cs = list(proof.commitments)
    ch = plonk.challenges(vk.to_bytes(), bad["public"], cs[:3], cs[3], cs[4:])
    assert ch == (bad["beta"], bad["gamma"], bad["alpha"], bad["z"])
    assert not protocol.identity_holds(vk, bad["public"], proof.values, *ch)
    values = [[v] for v in proof.values[:14]] + [list(proof.values[14:])]
    mo = kzg.MultiOpening(cs[:3] + cs[4:] + list(vk.commitments) + [cs[3]], pm.sets_of(vk.n, ch[3]), values, proof.w, proof.w2)
    assert kzg.verify_multi(kvk, mo)


def test_a_proof_for_another_circuit_is_refused(proved, string):
    from octopuszk_amd import kzg, plonk
    n = proved["vk"].n
    model, assignment = pm.chain(n, proved["vk"].n_public, random.Random(2970 + n), shared=False)
    other = plonk.Circuit(n, model.selectors, model.wires, model.n_public)
    pk, vk = plonk.setup(other, proved["pk"].commit_key)
    proof = plonk.prove(pk, assignment)
    public = model.public_inputs(assignment)
    assert plonk.verify(vk, proved["kvk"], public, proof)
    assert not plonk.verify(proved["vk"], proved["kvk"], public, proof)


def test_prove_names_the_broken_constraint(proved):
    from octopuszk_amd import plonk
    pk, model, assignment = proved["pk"], proved["model"], proved["assignment"]
    bad = list(assignment)
    bad[-1] = (bad[-1] + 1) % R                                           # the last gate's output: in one cell only
    with pytest.raises(ValueError, match="gate"):
        plonk.prove(pk, bad)
    wires = model.wire_values(assignment)
    wires[1][model.n_public] = (wires[1][model.n_public] + 1) % R        # one cell of a variable in many cells
    with pytest.raises(ValueError, match="copy"):
        plonk.prove(pk, wire_values=wires)
    assert plonk.prove(pk, wire_values=model.wire_values(assignment)).to_bytes() == proved["want"]["bytes"]
    # the assignment as 32-byte records, one of them written as v + r
    records = [kr.le(v) for v in assignment]
    records[0] = kr.le(assignment[0] + R)
    assert plonk.prove(pk, b"".join(records)).to_bytes() == proved["want"]["bytes"]
