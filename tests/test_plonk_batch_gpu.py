"""GPU tests of the batched PLONK verifier: the two entry points of csrc/plonk_verify.cuh word
for word over poisoned outputs (the challenges against plonk.challenges, lookup_challenges, kzg.multi_challenges and
transcript.weights; the scalars against identity_holds and kzg._multi_terms, the verifier's own host code, with the
challenges fed from the host), and plonk.verify_all / verify_each against plonk.verify over the string of known tau
that tests/test_plonk_gpu.py uses.  A handful of distinct proofs per key is cycled to fill a batch."""
import ctypes
import random

import pytest
import torch

import fr_gpu_util as fu
import plonk_batch_ref as bm
import plonk_lookup_ref as lm
import plonk_ref as pm
from oracle import bn254 as o

pytestmark = pytest.mark.gpu

R = o.R
TAU = 0x5eed0123456789abcdef0123456789abcdef0123456789abcdef % R
M = 512
SEED = bytes(range(100, 132))
KS = [1, 2, 63, 64, 65, 130]               # one lane, a pair, around one workgroup of 64 lanes, three workgroups
SMALL = [(0, 8, p) for p in range(4)] + [(1, 16, p) for p in range(4)]
WIDE = [(0, 256, p) for p in (64, 65, 130)]
E_INVALID = -1


def _le(values):
    return b"".join(int(v).to_bytes(32, "little") for v in values)


def _dev(b):
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda() if b else None


def _opt(t):
    return None if t is None else fu.ptr(t)


# ---------------------------------------------------------------------------- the verifier's host code as the reference
def _opening_rows(kind, vk_bytes, n, proof, z):
    """the commitments, point sets and values of the MultiOpening verify builds"""
    from octopuszk_amd.plonk import protocol as pp
    cs, values, _, _ = bm.parse(kind, proof)
    key = [vk_bytes[8 + 32 * i:40 + 32 * i] for i in range(bm.SHAPES[kind]["nkey"])]
    if kind:
        return (cs[:4] + cs[6:] + key + cs[4:6], pp._lookup_point_sets(n, z),
                [[v] for v in values[:19]] + [values[19:21], values[21:]])
    return cs[:3] + cs[4:] + key + [cs[3]], pp._point_sets(n, z), [[v] for v in values[:14]] + [values[14:]]


def _transcript(kind, vk_bytes, public, proof):
    from octopuszk_amd.plonk import protocol as pp
    cs = bm.parse(kind, proof)[0]
    if kind:
        return pp.lookup_challenges(vk_bytes, public, cs[:4], cs[4:6], cs[6:])
    return pp.challenges(vk_bytes, public, cs[:3], cs[3], cs[4:])


def _record(kind, vk_bytes, n, public, proof, rho, z=None):
    """the record the challenges kernel writes, from the package's host code; the multi-opening's two are zero where
    that code refuses the opening (a value >= r)"""
    from octopuszk_amd import kzg
    ch = list(_transcript(kind, vk_bytes, public, proof))
    try:
        g, u = kzg.multi_challenges(*_opening_rows(kind, vk_bytes, n, proof, ch[-1]), bm.parse(kind, proof)[2])
    except ValueError:
        g, u = 0, 0
    if z is not None:
        ch[-1] = z
    out = ch + [g, u, rho]
    return out + [0] * (bm.SHAPES[kind]["rec"] - len(out))


def _terms(kind, vk, public, proof, z=None):
    """(flags, the proof's own weights in row order, the key's, the scalars of g1, W, W') from identity_holds and
    kzg._multi_terms"""
    from octopuszk_amd import kzg
    from octopuszk_amd.plonk import protocol as pp
    shape = bm.SHAPES[kind]
    vk_bytes = vk.to_bytes()
    cs, values, w, w2 = bm.parse(kind, proof)
    ch = list(_transcript(kind, vk_bytes, public, proof))
    if z is not None:
        ch[-1] = z
    flags = (bm.VALUE if any(v >= R for v in values) else 0) | (bm.PUBLIC if any(x >= R for x in public) else 0)
    flags |= bm.DOMAIN if pow(ch[-1], vk.n, R) == 1 else 0
    if not flags:
        holds = pp.lookup_identity_holds if kind else pp.identity_holds
        if not holds(vk, public, values, *ch):
            flags |= bm.IDENTITY
    if flags:
        return flags, None
    weights, s_g1, s_w, u = kzg._multi_terms(kzg.MultiOpening(*_opening_rows(kind, vk_bytes, vk.n, proof, ch[-1]), w, w2))
    single = shape["nc"] - (2 if kind else 1)
    return 0, (weights[:single] + weights[single + shape["nkey"]:], weights[single:single + shape["nkey"]], s_g1, s_w, u)


def _fold(kind, terms, rho):
    """the expected outputs of the scalars kernel from per-proof terms"""
    nc, nkey = bm.SHAPES[kind]["nc"], bm.SHAPES[kind]["nkey"]
    own, s_w, s_w2, key, g1, rho_out, flags = [], [], [], [0] * nkey, 0, [], []
    for (f, t), r in zip(terms, rho):
        flags.append(f)
        if f:
            own += [0] * nc
            s_w.append(0)
            s_w2.append(0)
            rho_out.append(0)
            continue
        mine, keys, t_g1, t_w, u = t
        own += [r * x % R for x in mine]
        s_w.append(r * t_w % R)
        s_w2.append(r * u % R)
        key = [(a + r * x) % R for a, x in zip(key, keys)]
        g1 = (g1 + r * t_g1) % R
        rho_out.append(r)
    return own + s_w + s_w2 + key + [g1], rho_out, flags


# ---------------------------------------------------------------------------- the two entry points
def _challenges(kind, vk_bytes, n, n_public, proofs, publics, seed):
    """ozk_plonk_verify_challenges_dev over a poisoned output -> (the K records as ints, the guard is intact)"""
    L = fu.lib()
    k, rec = len(proofs), bm.SHAPES[kind]["rec"]
    d_vk, d_proofs = _dev(vk_bytes), _dev(b"".join(proofs))
    d_public = _dev(b"".join(_le(x) for x in publics))
    out = fu.poisoned(32 * rec * k + fu.GUARD)
    keep = ctypes.create_string_buffer(seed, 32)
    rc = L.ozk_plonk_verify_challenges_dev(kind, fu.ptr(d_vk), n, n_public, fu.ptr(d_proofs), _opt(d_public), k, fu.vp(keep),
                                           fu.ptr(out), fu.stream())
    assert rc == 0, L.ozk_last_error()
    got = fu.ints(out, rec * k)
    return [got[rec * m:rec * (m + 1)] for m in range(k)], fu.tail_untouched(out, 32 * rec * k)


def _scalars(kind, n, n_public, proofs, publics, records, raw=False):
    """ozk_plonk_verify_scalars_dev over poisoned outputs -> (scalars, rho, flags), each guard checked"""
    L = fu.lib()
    shape = bm.SHAPES[kind]
    k, total = len(proofs), len(proofs) * (shape["nc"] + 2) + shape["nkey"] + 1
    d_proofs, d_public = _dev(b"".join(proofs)), _dev(b"".join(_le(x) for x in publics))
    d_records = _dev(b"".join(_le(r) for r in records))
    scalars, rho, flags = fu.poisoned(32 * total + fu.GUARD), fu.poisoned(32 * k + fu.GUARD), fu.poisoned(4 * k + fu.GUARD)
    need = int(L.ozk_plonk_verify_scalars_workspace_bytes(kind, k))
    assert need > 0
    ws = fu.poisoned(need)
    rc = L.ozk_plonk_verify_scalars_dev(kind, n, n_public, fu.ptr(d_proofs), _opt(d_public), fu.ptr(d_records), k,
                                        fu.ptr(scalars), fu.ptr(rho), fu.ptr(flags), fu.ptr(ws), need, fu.stream())
    assert rc == 0, L.ozk_last_error()
    torch.cuda.synchronize()
    assert fu.tail_untouched(scalars, 32 * total) and fu.tail_untouched(rho, 32 * k) and fu.tail_untouched(flags, 4 * k)
    if raw:
        return fu.host_bytes(scalars), fu.host_bytes(rho), fu.host_bytes(flags)
    return fu.ints(scalars, total), fu.ints(rho, k), flags[:4 * k].view(torch.int32).cpu().tolist()


def _random_batch(kind, n, n_public, k, rng):
    shape = bm.SHAPES[kind]
    vk_bytes = n.to_bytes(4, "little") + n_public.to_bytes(4, "little") + rng.randbytes(32 * shape["nkey"])
    proofs = [rng.randbytes(32 * shape["nc"]) + _le(rng.randrange(R) for _ in range(shape["nv"])) + rng.randbytes(64)
              for _ in range(k)]
    publics = [[rng.randrange(R) for _ in range(n_public)] for _ in range(k)]
    return vk_bytes, proofs, publics


@pytest.mark.parametrize("kind,n,n_public", SMALL + WIDE + [(1, 256, 65)])
def test_challenges_are_the_host_transcripts(kind, n, n_public):
    """the message of the first digest is 374 + 32 p bytes (vanilla: its padding stays in one block for p < 4) or
    536 + 32 p (lookup: 56 mod 64 at p = 0 and 2, which takes a block more), so both parities of p are here"""
    from octopuszk_amd import transcript
    rng = random.Random(3950 + 100 * kind + n + n_public)
    vk_bytes, proofs, publics = _random_batch(kind, n, n_public, max(KS), rng)
    for k in KS:
        rho = transcript.weights(SEED, k, b"OZK-plonk-rho")
        rho = [int.from_bytes(rho[32 * m:32 * m + 32], "little") for m in range(k)]
        got, intact = _challenges(kind, vk_bytes, n, n_public, proofs[:k], publics[:k], SEED)
        assert intact
        for m in (range(k) if k <= 2 else sorted({0, 1, k // 2, k - 2, k - 1})):
            assert got[m] == _record(kind, vk_bytes, n, publics[m], proofs[m], rho[m]), (k, m)
        assert [rec[8 if kind else 6] for rec in got] == rho, k


def test_a_zero_half_of_the_stream_is_one_and_seeds_differ():
    rng = random.Random(3951)
    vk_bytes, proofs, publics = _random_batch(0, 8, 1, 3, rng)
    a, _ = _challenges(0, vk_bytes, 8, 1, proofs, publics, SEED)
    b, _ = _challenges(0, vk_bytes, 8, 1, proofs, publics, bytes(32))
    assert [r[:6] for r in a] == [r[:6] for r in b] and all(x[6] != y[6] for x, y in zip(a, b))
    assert all(1 <= r[6] < 1 << 128 for r in a + b)


# ---------------------------------------------------------------------------- real proofs
@pytest.fixture(scope="module")
def string():
    from octopuszk_amd import kzg, srs
    s = srs.Srs.from_secrets(M, TAU, 1, 1, generator=1)
    return s, kzg.VerifyKey.from_srs(s)


_TABLE = None


def _table():
    global _TABLE
    if _TABLE is None:
        rng = random.Random(3960)
        _TABLE = [tuple(rng.randrange(R) for _ in range(3)) for _ in range(4)]
        _TABLE.append(_TABLE[0])
    return _TABLE


def _case(kind, n, n_public, seed):
    """(circuit, assignment) of the models' chains; without public inputs, the chain of one whose first row has qL = 0"""
    p = max(n_public, 1)
    if kind:
        model, assignment = lm.chain_with_lookups(n, p, random.Random(seed), _table(), 3)
    else:
        model, assignment = pm.chain(n, p, random.Random(seed))
    if n_public == 0:
        model.selectors[0][0] = 0
        model.n_public = 0
    return model, assignment


_MADE = {}


def _made(string, kind, n, n_public, distinct=2, zk=False):
    """one key of this shape and `distinct` proofs of different assignments under it: (vk, kvk, publics, proofs as bytes)"""
    from octopuszk_amd import kzg, plonk
    name = (kind, n, n_public, distinct, zk)
    if name not in _MADE:
        s, kvk = string
        model, _ = _case(kind, n, n_public, 3970)
        if kind:
            circuit = plonk.LookupCircuit(n, model.selectors, model.wires, n_public, model.q_lookup, model.table)
        else:
            circuit = plonk.Circuit(n, model.selectors, model.wires, n_public)
        pk, vk = plonk.setup(circuit, kzg.CommitKey.from_srs(s, n + (plonk.ZK_PAD if zk else 0)), zk=zk)
        publics, proofs = [], []
        for i in range(distinct):
            _, assignment = _case(kind, n, n_public, 3971 + i)
            publics.append(model.public_inputs(assignment))
            proofs.append(plonk.prove(pk, assignment).to_bytes())
        _MADE[name] = (vk, kvk, publics, proofs)
    return _MADE[name]


def _cycled(items, k):
    return [items[m % len(items)] for m in range(k)]


@pytest.mark.parametrize("kind,n,n_public", SMALL + WIDE)
def test_scalars_are_the_verifiers_terms(string, kind, n, n_public):
    vk, kvk, publics, proofs = _made(string, kind, n, n_public)
    vk_bytes = vk.to_bytes()
    terms = [_terms(kind, vk, x, p) for x, p in zip(publics, proofs)]
    assert all(f == 0 for f, _ in terms)
    rng = random.Random(3980 + n_public)
    for k in KS:
        rho = [rng.randrange(1, 1 << 128) for _ in range(k)]
        records = [_record(kind, vk_bytes, n, x, p, r) for x, p, r in zip(_cycled(publics, k), _cycled(proofs, k), rho)]
        got = _scalars(kind, n, n_public, _cycled(proofs, k), _cycled(publics, k), records)
        assert got == _fold(kind, _cycled(terms, k), rho), k


@pytest.mark.parametrize("kind,n", [(0, 8), (1, 16)])
def test_flags_zero_scalars_and_sums_without_the_flagged(string, kind, n):
    from octopuszk_amd.fft import root_of_unity
    vk, kvk, publics, proofs = _made(string, kind, n, 1)
    vk_bytes, nc = vk.to_bytes(), bm.SHAPES[kind]["nc"]
    at = 32 * (nc + 2)
    v = int.from_bytes(proofs[0][at:at + 32], "little")
    raised = proofs[0][:at] + (v + R).to_bytes(32, "little") + proofs[0][at + 32:]          # the same value, as v + r
    changed = proofs[1][:at] + ((v + 1) % R).to_bytes(32, "little") + proofs[1][at + 32:]
    batch = [(publics[0], proofs[0], None), (publics[0], raised, None), ([R], proofs[1], None), (publics[1], changed, None),
             (publics[1], proofs[1], pow(root_of_unity(n), 3, R)), (publics[1], proofs[1], None)]
    rho = [3, 1 << 127, 5, 7, 11, (1 << 128) - 1]
    terms = [_terms(kind, vk, x, p, z) for x, p, z in batch]
    assert [f for f, _ in terms] == [0, bm.VALUE, bm.PUBLIC, bm.IDENTITY, bm.DOMAIN, 0]
    records = [_record(kind, vk_bytes, n, x, p, r, z) for (x, p, z), r in zip(batch, rho)]
    want = _fold(kind, terms, rho)
    got = _scalars(kind, n, 1, [p for _, p, _ in batch], [x for x, _, _ in batch], records)
    assert got == want
    scalars, rho_out, _ = got
    for m in (1, 2, 3, 4):
        assert scalars[nc * m:nc * (m + 1)] == [0] * nc and scalars[6 * nc + m] == 0 and scalars[6 * nc + 6 + m] == 0
        assert rho_out[m] == 0
    # the sums are those of the two unflagged proofs alone
    alone = _fold(kind, [terms[0], terms[5]], [rho[0], rho[5]])[0]
    assert scalars[6 * (nc + 2):] == alone[2 * (nc + 2):]


@pytest.mark.parametrize("kind,n,n_public", [(0, 8, 1), (1, 16, 2), (0, 256, 130)])
def test_two_runs_give_identical_bytes(string, kind, n, n_public):
    vk, kvk, publics, proofs = _made(string, kind, n, n_public)
    k = 130
    rho = [random.Random(3990).randrange(1, 1 << 128) for _ in range(k)]
    records = [_record(kind, vk.to_bytes(), n, x, p, r) for x, p, r in zip(_cycled(publics, k), _cycled(proofs, k), rho)]
    first = _scalars(kind, n, n_public, _cycled(proofs, k), _cycled(publics, k), records, raw=True)
    assert first == _scalars(kind, n, n_public, _cycled(proofs, k), _cycled(publics, k), records, raw=True)


def test_entry_points_reject_bad_shapes(string):
    L = fu.lib()
    buf = fu.zeroed(4096)
    p, st = fu.ptr(buf), fu.stream()
    keep = ctypes.create_string_buffer(bytes(32), 32)
    for kind, n, n_public, k in [(2, 8, 1, 1), (0, 12, 1, 1), (0, 8, 9, 1), (0, 8, 1, 0), (0, 8, 1, (1 << 16) + 1),
                                 (0, 1 << 20, 1 << 12, 1 << 13)]:
        assert L.ozk_plonk_verify_challenges_dev(kind, p, n, n_public, p, p, k, fu.vp(keep), p, st) == E_INVALID
        assert L.ozk_plonk_verify_scalars_dev(kind, n, n_public, p, p, p, k, p, p, p, p, 1 << 30, st) == E_INVALID
    assert L.ozk_plonk_verify_scalars_workspace_bytes(2, 1) == 0 and L.ozk_plonk_verify_scalars_workspace_bytes(0, 0) == 0
    assert L.ozk_plonk_verify_challenges_dev(0, p, 8, 1, None, p, 1, fu.vp(keep), p, st) == E_INVALID      # a null pointer
    assert L.ozk_plonk_verify_challenges_dev(0, p, 8, 1, p, p, 1, fu.vp(keep), p, st) == E_INVALID         # overlap
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- the protocol
def _r1cs(string):
    from octopuszk_amd import kzg, plonk
    from octopuszk_amd import zksnark as z
    if "r1cs" not in _MADE:
        s, kvk = string
        r1cs, primary, auxiliary = z.serial_construct(2, 1)
        circuit = plonk.from_r1cs(r1cs)
        pk, vk = plonk.setup(circuit, kzg.CommitKey.from_srs(s, circuit.n))
        proof = plonk.prove(pk, list(primary + auxiliary)).to_bytes()
        _MADE["r1cs"] = (vk, kvk, [list(primary)], [proof])
    return _MADE["r1cs"]


KEYS = {"vanilla": lambda s: _made(s, 0, 8, 1, 3), "lookup": lambda s: _made(s, 1, 16, 1), "r1cs": _r1cs,
        "zk": lambda s: _made(s, 0, 8, 1, 2, zk=True)}


@pytest.mark.parametrize("name", sorted(KEYS))
def test_honest_batches_verify(string, name):
    from octopuszk_amd import plonk
    vk, kvk, publics, proofs = KEYS[name](string)
    assert all(plonk.verify(vk, kvk, x, p) for x, p in zip(publics, proofs))
    for k in (1, 2, 65):
        assert plonk.verify_all(vk, kvk, _cycled(publics, k), _cycled(proofs, k)) is True
        assert plonk.verify_each(vk, kvk, _cycled(publics, k), _cycled(proofs, k), seed=SEED) == [True] * k


def _flip(proof, byte, bit=7):
    return proof[:byte] + bytes([proof[byte] ^ (1 << bit)]) + proof[byte + 1:]


def _tampered(how, publics, proofs, at):
    """one proof of the batch changed; (publics, proofs, the positions that no longer verify)"""
    publics, proofs = list(publics), list(proofs)
    if how == "commitment":
        proofs[at] = _flip(proofs[at], 32 + 31)                # [b] becomes -[b]: it decodes, the transcript moves
    elif how == "value":
        proofs[at] = _flip(proofs[at], 7 * 32 + 5 * 32 + 3, 0)
    elif how == "W":
        proofs[at] = _flip(proofs[at], 800 - 33)               # W becomes -W: only the pairing product sees it
    elif how == "W'":
        proofs[at] = _flip(proofs[at], 800 - 1)
    else:
        other = at - 1 if at else 1                            # neighbours hold different assignments
        publics[at], publics[other] = publics[other], publics[at]
        return publics, proofs, sorted({at, other})
    return publics, proofs, [at]


@pytest.mark.parametrize("at", [0, 63, 64])
@pytest.mark.parametrize("how", ["commitment", "value", "W", "W'", "public inputs swapped"])
def test_one_tampered_proof_is_singled_out(string, how, at):
    from octopuszk_amd import plonk
    vk, kvk, publics, proofs = KEYS["vanilla"](string)
    k = 65
    publics, proofs, wrong = _tampered(how, _cycled(publics, k), _cycled(proofs, k), at)
    assert all(not plonk.verify(vk, kvk, publics[m], proofs[m]) for m in wrong)
    assert plonk.verify_all(vk, kvk, publics, proofs) is False
    assert plonk.verify_each(vk, kvk, publics, proofs) == [m not in wrong for m in range(k)]


def test_a_tampered_lookup_proof(string):
    from octopuszk_amd import plonk
    vk, kvk, publics, proofs = KEYS["lookup"](string)
    k = 5
    publics, proofs = _cycled(publics, k), _cycled(proofs, k)
    for byte, bit in [(3 * 32 + 31, 7), (9 * 32 + 20 * 32, 0), (1088 - 33, 7), (1088 - 1, 7)]:    # [m], Z(z omega), W, W'
        bad = list(proofs)
        bad[3] = _flip(proofs[3], byte, bit)
        assert not plonk.verify(vk, kvk, publics[3], bad[3])
        assert plonk.verify_all(vk, kvk, publics, bad) is False
        assert plonk.verify_each(vk, kvk, publics, bad) == [True, True, True, False, True]


def test_malformed_proofs_are_false_not_errors(string):
    from octopuszk_amd import plonk
    vk, kvk, publics, proofs = KEYS["vanilla"](string)
    no_point = bytes([0xff] * 31 + [0x3f])                                # x >= q
    bad = [proofs[0], no_point + proofs[1][32:], proofs[2][:224] + _le([R]) + proofs[2][256:], bytes(800)]
    xs = [publics[0], publics[1], publics[2], publics[0]]
    assert [plonk.verify(vk, kvk, x, p) for x, p in zip(xs, bad)] == [True, False, False, False]
    assert plonk.verify_all(vk, kvk, xs, bad) is False
    assert plonk.verify_each(vk, kvk, xs, bad) == [True, False, False, False]
    assert plonk.verify_each(vk, kvk, [[R], [1 << 300], [-1]], proofs[:3]) == [False] * 3
    assert plonk.verify_all(vk, kvk, [publics[0], [1 << 300]], proofs[:2]) is False


def test_objects_bytes_and_tensors_agree(string):
    from octopuszk_amd import plonk
    vk, kvk, publics, proofs = KEYS["vanilla"](string)
    k = 5
    publics, proofs = _cycled(publics, k), _cycled(proofs, k)
    proofs[2] = _flip(proofs[2], 800 - 1)
    want = [True, True, False, True, True]
    forms = [([plonk.Proof.from_bytes(p) for p in proofs], publics), (proofs, publics),
             (b"".join(proofs), b"".join(_le(x) for x in publics)),
             (_dev(b"".join(proofs)), _dev(b"".join(_le(x) for x in publics))),
             (b"".join(proofs), _dev(b"".join(_le(x) for x in publics))), (_dev(b"".join(proofs)), publics)]
    for given, xs in forms:
        assert plonk.verify_each(vk, kvk, xs, given, seed=SEED) == want
        assert plonk.verify_all(vk, kvk, xs, given, seed=SEED) is False
    good = b"".join(proofs[:2])
    assert plonk.verify_all(vk, kvk, publics[:2], _dev(good)) and plonk.verify_all(vk, kvk, publics[:2], good)


def test_a_pinned_seed_reproduces_the_scalars(string):
    """verify_all's device buffers under a given seed: the kernels' outputs are those of the model's stream of weights"""
    from octopuszk_amd import transcript, vectors
    vk, kvk, publics, proofs = KEYS["vanilla"](string)
    k = 5
    publics, proofs = _cycled(publics, k), _cycled(proofs, k)
    d_proofs, d_public = _dev(b"".join(proofs)), _dev(b"".join(_le(x) for x in publics))
    runs = []
    for _ in range(2):
        records = vectors.plonk_verify_challenges(0, _dev(vk.to_bytes()), vk.n, vk.n_public, d_proofs, d_public, SEED)
        runs.append([fu.host_bytes(t) for t in vectors.plonk_verify_scalars(0, vk.n, vk.n_public, d_proofs, d_public, records)])
    assert runs[0] == runs[1]
    rho = transcript.weights(SEED, k, b"OZK-plonk-rho")
    assert runs[0][1] == rho
    rho = [int.from_bytes(rho[32 * m:32 * m + 32], "little") for m in range(k)]
    want = _fold(0, [_terms(0, vk, x, p) for x, p in zip(publics, proofs)], rho)
    assert runs[0][0] == _le(want[0]) and runs[0][2] == bytes(4 * k)
    other = vectors.plonk_verify_challenges(0, _dev(vk.to_bytes()), vk.n, vk.n_public, d_proofs, d_public, bytes(32))
    assert fu.host_bytes(vectors.plonk_verify_scalars(0, vk.n, vk.n_public, d_proofs, d_public, other)[0]) != runs[0][0]


def test_empty_batch_and_sizes(string):
    from octopuszk_amd import plonk
    vk, kvk, publics, proofs = KEYS["vanilla"](string)
    lvk, _, lpublics, lproofs = KEYS["lookup"](string)
    assert plonk.verify_all(vk, kvk, [], []) is True and plonk.verify_each(vk, kvk, [], []) == []
    with pytest.raises(ValueError):
        plonk.verify_all(vk, kvk, lpublics[:1], lproofs[:1])               # a lookup proof under a vanilla key
    with pytest.raises(ValueError):
        plonk.verify_all(lvk, kvk, publics[:1], proofs[:1])
    with pytest.raises(ValueError):
        plonk.verify_all(vk, kvk, publics[:2], _dev(proofs[0]))
    assert plonk.verify(vk, kvk, lpublics[0], lproofs[0]) is False
