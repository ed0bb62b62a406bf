"""GPU tests of zero-knowledge PLONK proofs: the two entry points of csrc/plonk_zk.cuh against
the integer model (tests/plonk_zk_ref.py), word for word over poisoned buffers, and octopuszk_amd/plonk under keys of
setup(zk=True) over the string of known tau that tests/test_plonk_gpu.py uses: with pinned blinders every proof is the
model's, byte for byte, and the verifier and verifying key are those of a key without zk."""
import ctypes
import random

import pytest

import fr_gpu_util as fu
import plonk_lookup_ref as lm
import plonk_ref as pm
import plonk_zk_ref as zm

pytestmark = pytest.mark.gpu

R = pm.R
E_INVALID = -1
TAU = 0x5eed0123456789abcdef0123456789abcdef0123456789abcdef % R
M = 512                        # 2 M + 1 >= 64 + 8 powers in G1
PAD = zm.ZK_PAD


# ---------------------------------------------------------------------------- the blinders of rows
def _blind(rows, n, stride, blinders):
    """ozk_fr_rows_blind_dev over rows written at `stride` with a poisoned guard -> (every word of the buffer, its
    guard untouched)"""
    L = fu.lib()
    k = len(rows)
    d = fu.dev_from_ints(fu.flat(rows, stride, fill=fu.POISON_INT), guard=64)
    keep, p_b = fu.host_ints([r for row in blinders for r in row] or [0])
    counts = (ctypes.c_int32 * k)(*[len(row) for row in blinders])
    rc = L.ozk_fr_rows_blind_dev(fu.ptr(d), k, n, stride, p_b, ctypes.cast(counts, ctypes.c_void_p), fu.stream())
    assert rc == 0, L.ozk_last_error()
    raw = fu.host_bytes(d)
    return fu.words(raw[:-64]), raw[-64:] == bytes([fu.POISON]) * 64


def _blind_case(n, seed):
    """six rows of n + 4 words as written (the slots n .. n + 3 poisoned: they are not read) and their blinders, 0, 2,
    3 and 4 of them mixed, with both wraps of the subtraction"""
    rng = random.Random(seed)
    rows = [[rng.randrange(R) for _ in range(n)] + [fu.POISON_INT] * 4 for _ in range(6)]
    blinders = [[rng.randrange(1, R) for _ in range(c)] for c in (0, 2, 3, 4, 2, 3)]
    rows[1][0], rows[1][1], blinders[1] = 0, R - 1, [1, R - 1]            # 0 - 1 = r - 1; (r - 1) - (r - 1) = 0
    rows[2][0], rows[2][1], blinders[2][:2] = R - 1, 0, [1, R - 1]        # (r - 1) - 1; 0 - (r - 1) = 1
    rows[3][2] += R                                                       # a head written as x + r
    rows[4][n - 1] = fu.ALL_ONES                                          # the last coefficient: left as written
    return rows, blinders


@pytest.mark.parametrize("extra", [0, 7], ids=["stride_n4", "stride_n11"])
@pytest.mark.parametrize("n", [8, 1024, 1025])
def test_rows_blind_matches_the_model(n, extra):
    rows, blinders = _blind_case(n, 3800 + n + extra)
    stride = n + 4 + extra
    got, guard = _blind(rows, n, stride, blinders)
    want = fu.flat(zm.rows_blind(rows, n, blinders), stride, fill=fu.POISON_INT)
    assert not fu.mismatches(got, want)[:4] and guard
    assert got[stride:stride + n + 4] == want[stride:stride + n + 4] == [R - 1, 0] + rows[1][2:n] + [1, R - 1] + [fu.POISON_INT] * 2
    assert got[2 * stride:2 * stride + 2] == [R - 2, 1]
    assert got[:stride] == fu.flat(rows[:1], stride, fill=fu.POISON_INT)  # no blinders: the row as written, bit for bit
    touched = {y * stride + at + j for y, row in enumerate(blinders) for j in range(len(row)) for at in (0, n)}
    written = fu.flat(rows, stride, fill=fu.POISON_INT)
    assert all(got[i] == written[i] for i in range(len(got)) if i not in touched)


def test_rows_blind_through_the_wrapper_keeps_the_values_on_the_domain():
    import kzg_ref as kr
    from octopuszk_amd import vectors
    n, rng = 8, random.Random(3810)
    evals = [rng.randrange(R) for _ in range(n)]
    rs = [rng.randrange(R) for _ in range(3)]
    d = fu.dev_from_ints(zm.padded(kr.intt(evals, kr.root(n)), n))
    assert vectors.fr_rows_blind(d.view(1, -1), 1, n, n + PAD, [rs]) is not None
    got = fu.words(fu.host_bytes(d))
    assert got == zm.blinded(kr.intt(evals, kr.root(n)), n, rs)
    assert [kr.horner(got, pow(kr.root(n), i, R)) for i in range(n)] == evals


# ---------------------------------------------------------------------------- the split of the quotient
def _split(t, n, out_stride, blinders):
    """ozk_plonk_quotient_split_dev -> (the three rows, the two elements behind them, *d_nonzero)"""
    L = fu.lib()
    d_t = fu.dev_from_ints(t, guard=64)
    out, count = fu.poisoned((3 * out_stride + 2) * 32), fu.poisoned(16)
    keep, p_b = fu.host_ints(blinders)
    rc = L.ozk_plonk_quotient_split_dev(fu.ptr(d_t), n, fu.ptr(out), out_stride, p_b, fu.ptr(count), fu.stream())
    assert rc == 0, L.ozk_last_error()
    got, tail = fu.words(fu.host_bytes(out)), fu.host_bytes(count)
    assert tail[4:] == bytes([fu.POISON]) * 12
    rows = [got[y * out_stride:(y + 1) * out_stride] for y in range(3)]
    return rows, got[3 * out_stride:], int.from_bytes(tail[:4], "little", signed=True)


@pytest.fixture(scope="module")
def quotients():
    """for every n: 3 n + 6 random coefficients, zero from there on, and four blinders"""
    out = {}
    for n in (8, 256, 2048):
        rng = random.Random(3820 + n)
        out[n] = ([rng.randrange(1, R) for _ in range(3 * n + 6)] + [0] * (n - 6), [rng.randrange(1, R) for _ in range(4)])
    return out


# the least stride; one that ends inside the columns that are only read; one past all 2 n of them
def _strides(n):
    return [n + PAD, n + PAD + 3, 2 * n + 5]


@pytest.mark.parametrize("n", [8, 256, 2048])
def test_quotient_split_matches_the_model(quotients, n):
    t, blinders = quotients[n]
    written = list(t)
    written[n + 1] += R                                                   # words written as x + r: one that a blinder
    written[4 * n - 1] = R                                                # is taken from, and a zero of the top
    for stride in _strides(n):
        rows, behind, nonzero = _split(written, n, stride, blinders)
        want, none = zm.quotient_split(t, n, stride, blinders)
        assert rows == want and nonzero == none == 0 and behind == [fu.POISON_INT] * 2
        assert all(row[n + PAD:] == [0] * (stride - n - PAD) for row in rows)
        assert zm.recombined(rows, n)[:3 * n + 6] == t[:3 * n + 6]


@pytest.mark.parametrize("n", [8, 256, 2048])
def test_quotient_split_with_zero_blinders_is_plain_slices(quotients, n):
    t, _ = quotients[n]
    rows, _, nonzero = _split(t, n, n + PAD, [0] * 4)
    assert nonzero == 0
    assert rows == [t[:n] + [0] * PAD, t[n:2 * n] + [0] * PAD, t[2 * n:3 * n + 6] + [0] * 2]


@pytest.mark.parametrize("n", [8, 256, 2048])
def test_quotient_split_counts_what_lies_past_3n_plus_6(quotients, n):
    t, blinders = quotients[n]
    for at, counted in ((3 * n + 6, 1), (4 * n - 1, 1), (3 * n + 5, 0)):
        planted = list(t)
        planted[at] = (planted[at] + 1) % R
        rows, _, nonzero = _split(planted, n, n + PAD, blinders)
        want, count = zm.quotient_split(planted, n, n + PAD, blinders)
        assert nonzero == count == counted and rows == want, at
    top = list(t)
    top[3 * n + 6:] = [1 + i for i in range(n - 6)]                       # every one of them, over every workgroup
    assert _split(top, n, n + PAD, blinders)[2] == n - 6


def test_rejected_calls_launch_nothing():
    L = fu.lib()
    n = 16
    buf = fu.poisoned(16 * n * 32)
    null, stream = ctypes.c_void_p(0), fu.stream()
    keep, blinders = fu.host_ints([1, 2, 3, 4])
    counts = (ctypes.c_int32 * 8)(2, 2, 2, 0, 0, 0, 0, 0)
    p_counts = ctypes.cast(counts, ctypes.c_void_p)

    def blind(r, k, n_, stride, b, c):
        return L.ozk_fr_rows_blind_dev(r, k, n_, stride, b, c, stream)

    good = [fu.ptr(buf), 2, n, n + 4, blinders, p_counts]
    for k, n_, stride in ((0, n, n + 4), (9, n, n + 4), (-1, n, n + 4), (2, 3, 7), (2, n, n + 3), (2, n, 1 << 28)):
        assert blind(null, k, n_, stride, null, null) == E_INVALID
    for i in (0, 4, 5):
        assert blind(*(good[:i] + [null] + good[i + 1:])) == E_INVALID
    assert blind(*([fu.ptr(buf[8:])] + good[1:])) == E_INVALID
    assert b"aligned" in L.ozk_last_error()
    for wrong in (5, -1):
        bad = (ctypes.c_int32 * 2)(2, wrong)
        assert blind(*(good[:5] + [ctypes.cast(bad, ctypes.c_void_p)])) == E_INVALID
        assert b"blinders" in L.ozk_last_error()

    t, out, count = buf[:4 * n * 32], buf[4 * n * 32:(4 * n + 3 * (n + PAD)) * 32], buf[12 * n * 32:12 * n * 32 + 4]

    def split(t_, n_, o_, stride, b, c):
        return L.ozk_plonk_quotient_split_dev(t_, n_, o_, stride, b, c, stream)

    good = [fu.ptr(t), n, fu.ptr(out), n + PAD, blinders, fu.ptr(count)]
    for bad_n in (0, 4, 12, -8, (1 << 26) + 1, 1 << 27):
        assert split(null, bad_n, null, bad_n + PAD, null, null) == E_INVALID
    assert split(*(good[:3] + [n + PAD - 1] + good[4:])) == E_INVALID
    assert split(*(good[:3] + [(1 << 28) // 3 + 1] + good[4:])) == E_INVALID
    for i in (0, 2, 4, 5):
        assert split(*(good[:i] + [null] + good[i + 1:])) == E_INVALID
    for i, off in ((0, t[8:]), (2, out[8:])):
        assert split(*(good[:i] + [fu.ptr(off)] + good[i + 1:])) == E_INVALID
        assert b"aligned" in L.ozk_last_error()
    assert split(*(good[:5] + [fu.ptr(buf[12 * n * 32 + 2:])])) == E_INVALID
    for o_bad in (t[(4 * n - 1) * 32:], buf[32:]):
        assert split(*(good[:2] + [fu.ptr(o_bad)] + good[3:])) == E_INVALID
        assert b"overlap" in L.ozk_last_error()
    assert split(*(good[:5] + [fu.ptr(out[32:])])) == E_INVALID                               # the count inside the rows
    assert split(*(good[:5] + [fu.ptr(t[64:])])) == E_INVALID                                 # .. and inside t
    assert fu.host_bytes(buf) == bytes([fu.POISON]) * buf.numel()


# ---------------------------------------------------------------------------- the protocol
@pytest.fixture(scope="module")
def string():
    from octopuszk_amd import kzg, srs
    s = srs.Srs.from_secrets(M, TAU, 1, 1, generator=1)
    return s, kzg.VerifyKey.from_srs(s)


def _vanilla(n):
    from octopuszk_amd import plonk
    rng = random.Random(3830 + n)
    model, assignment = pm.chain(n, 2, rng)
    return plonk.Circuit(n, model.selectors, model.wires, 2), model, assignment, assignment, rng


def _lookup(n):
    from octopuszk_amd import plonk
    rng = random.Random(3840 + n)
    table = [tuple(rng.randrange(R) for _ in range(3)) for _ in range(4)]
    model, assignment = lm.chain_with_lookups(n, 1, rng, table + [table[0]], n // 2 - 1)
    circuit = plonk.LookupCircuit(n, model.selectors, model.wires, 1, model.q_lookup, model.table)
    return circuit, model, assignment, assignment, rng


def _r1cs(n):
    from octopuszk_amd import plonk
    from octopuszk_amd import zksnark as z
    r1cs, primary, auxiliary = z.serial_construct(*{8: (2, 1), 64: (12, 3)}[n])
    circuit = plonk.from_r1cs(r1cs)
    assert circuit.n == n
    full = primary + auxiliary
    model = pm.Circuit(n, circuit.selectors, circuit.wires, circuit.n_public)
    return circuit, model, circuit.extend(full), full, random.Random(3850 + n)


KINDS = {"vanilla": _vanilla, "lookup": _lookup, "r1cs": _r1cs}


@pytest.fixture(scope="module", params=[(kind, n) for kind in KINDS for n in (8, 64)], ids=lambda p: "%s_n%d" % p)
def case(request, string):
    """one circuit under a key with zk and one without, proved with pinned blinders by the package and by the model.
    given: the assignment as the prover takes it (the R1CS's own for an imported one); assignment: one value per
    variable of the circuit, which the model and wire_values take"""
    from octopuszk_amd import kzg, plonk
    kind, n = request.param
    s, kvk = string
    circuit, model, assignment, given, rng = KINDS[kind](n)
    lookup = kind == "lookup"
    pk, vk = plonk.setup(circuit, kzg.CommitKey.from_srs(s, n + plonk.ZK_PAD), zk=True)
    plain_pk, plain_vk = plonk.setup(circuit, kzg.CommitKey.from_srs(s, n))
    count = plonk.ZK_LOOKUP_BLINDERS if lookup else plonk.ZK_BLINDERS
    blinders = [rng.randrange(1, R) for _ in range(count)]
    want = (zm.prove_lookup if lookup else zm.prove)(model, assignment, TAU, blinders)
    return {"kind": kind, "n": n, "model": model, "assignment": assignment, "given": given, "pk": pk, "vk": vk,
            "plain_pk": plain_pk, "plain_vk": plain_vk, "kvk": kvk, "blinders": blinders, "count": count, "want": want,
            "proof": plonk.prove(pk, given, blinders=blinders),
            "hidden": 9 if lookup else 7,                                 # the prover's commitments
            "blinded_values": (0, 1, 2, 3, 4, 5, 6, 19, 20, 21, 22) if lookup else (0, 1, 2, 3, 4, 5, 14, 15)}


def test_setup_zk_returns_the_verifying_key_of_a_key_without_zk(case):
    from octopuszk_amd import plonk
    pk, n = case["pk"], case["n"]
    assert pk.zk is True and case["plain_pk"].zk is False
    assert case["vk"].to_bytes() == case["plain_vk"].to_bytes()
    assert len(case["vk"].to_bytes()) == (plonk.LOOKUP_VK_BYTES if case["kind"] == "lookup" else 264)
    rows = 12 if case["kind"] == "lookup" else 8
    assert tuple(pk.coeffs.shape) == (rows, 32 * (n + plonk.ZK_PAD))
    assert not bool(pk.coeffs[:, 32 * n:].any().item())                   # zero-extended
    assert bool((pk.coeffs[:, :32 * n] == case["plain_pk"].coeffs).all().item())
    assert pk.table.shape == case["plain_pk"].table.shape and bool((pk.table == case["plain_pk"].table).all().item())
    assert isinstance(pk, type(case["plain_pk"]))


def test_a_proof_with_pinned_blinders_is_the_models(case):
    from octopuszk_amd import plonk
    proof, want = case["proof"], case["want"]
    assert list(proof.commitments) == want["commitments"] and list(proof.values) == want["values"]
    assert proof.to_bytes() == want["bytes"]
    assert len(proof.to_bytes()) == (plonk.LOOKUP_PROOF_BYTES if case["kind"] == "lookup" else plonk.PROOF_BYTES)


def test_the_verifier_of_a_key_without_zk_accepts_it(case):
    from octopuszk_amd import plonk
    public = case["want"]["public"]
    assert plonk.verify(case["plain_vk"], case["kvk"], public, case["proof"])
    assert plonk.verify(case["plain_vk"], case["kvk"], public, case["proof"].to_bytes())
    wrong = list(public)
    wrong[-1] = (wrong[-1] + 1) % R
    assert not plonk.verify(case["plain_vk"], case["kvk"], wrong, case["proof"])


def test_zero_blinders_give_the_proof_of_the_key_without_zk(case):
    from octopuszk_amd import plonk
    plain = plonk.prove(case["plain_pk"], case["given"])
    assert plonk.prove(case["pk"], case["given"], blinders=[0] * case["count"]).to_bytes() == plain.to_bytes()
    assert case["proof"].to_bytes() != plain.to_bytes()
    with pytest.raises(ValueError, match="zk=True"):
        plonk.prove(case["plain_pk"], case["given"], blinders=[0] * case["count"])
    with pytest.raises(ValueError, match="blinders"):
        plonk.prove(case["pk"], case["given"], blinders=[0] * (case["count"] - 1))


def test_two_proofs_of_one_witness_share_nothing_the_prover_hides(case):
    from octopuszk_amd import plonk
    public = case["want"]["public"]
    timings = {}
    one, two = plonk.prove(case["pk"], case["given"], timings), plonk.prove(case["pk"], case["given"])
    assert set(timings) == set(plonk.LOOKUP_STAGES if case["kind"] == "lookup" else plonk.protocol.STAGES)
    for proof in (one, two):
        assert plonk.verify(case["vk"], case["kvk"], public, proof)
    for other in (two, case["proof"]):
        assert len(one.commitments) == case["hidden"]
        assert all(a != b for a, b in zip(one.commitments, other.commitments))
        assert all(one.values[i] != other.values[i] for i in case["blinded_values"])
        assert one.w != other.w and one.w2 != other.w2


def test_every_form_of_the_witness_gives_the_same_bytes(case):
    from octopuszk_amd import plonk
    from octopuszk_amd.wire import le32
    pk, given, blinders, want = case["pk"], case["given"], case["blinders"], case["want"]["bytes"]
    assert plonk.prove(pk, le32(given), blinders=blinders).to_bytes() == want
    assert plonk.prove(pk, fu.dev_from_ints(given), blinders=blinders).to_bytes() == want          # on the device
    wires = case["model"].wire_values(case["assignment"])
    assert plonk.prove(pk, wire_values=wires, blinders=tuple(blinders)).to_bytes() == want


def _cell_to_break(model):
    """(a cell whose variable is in that cell alone or may move everywhere at once: the output of a gate with qO != 0
    that is not among the gate's inputs; a cell of a variable that is in other cells too), both outside lookup rows"""
    n = model.n
    looks = getattr(model, "q_lookup", [0] * n)
    cells = {}
    for j in range(3):
        for i in range(n):
            cells.setdefault(model.wires[j][i], []).append((j, i))
    rows = [i for i in range(model.n_public, n) if model.selectors[2][i] % R and not looks[i]
            and model.wires[2][i] not in (model.wires[0][i], model.wires[1][i])
            and all(not looks[r] for _, r in cells[model.wires[2][i]])]
    gate = rows[-1]
    shared = next(m[0] for v, m in cells.items() if len(m) > 1 and not looks[m[0][1]] and m[0][1] >= model.n_public)
    return cells[model.wires[2][gate]], shared


def test_a_violated_gate_and_a_violated_copy_still_raise(case):
    from octopuszk_amd import plonk
    model, pk = case["model"], case["pk"]
    moved, shared = _cell_to_break(model)
    wires = model.wire_values(case["assignment"])
    for j, i in moved:                                                    # every cell of one variable: the copies hold
        wires[j][i] = (wires[j][i] + 1) % R
    with pytest.raises(ValueError, match="a gate is violated"):
        plonk.prove(pk, wire_values=wires, blinders=case["blinders"])
    with pytest.raises(ValueError, match="a gate is violated"):
        plonk.prove(pk, wire_values=wires)
    wires = model.wire_values(case["assignment"])
    wires[shared[0]][shared[1]] = (wires[shared[0]][shared[1]] + 1) % R
    with pytest.raises(ValueError, match="copy"):
        plonk.prove(pk, wire_values=wires)


@pytest.mark.parametrize("section", [0, 3, 4, 6, 7, 10, 12, -2, -1])
def test_a_tampered_zk_proof_is_rejected(case, section):
    from octopuszk_amd import plonk
    raw = bytearray(case["proof"].to_bytes())
    raw[32 * (section % (len(raw) // 32)) + 1] ^= 4
    assert not plonk.verify(case["vk"], case["kvk"], case["want"]["public"], bytes(raw))
