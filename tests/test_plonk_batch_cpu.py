"""CPU tests of the batched PLONK verifier: the combined equation of tests/plonk_batch_ref.py in
the exponent over model proofs with a known tau, the argument checks of plonk.verify_all, which raise before any
device call, and the lane's SHA-256 (octopuszk_amd/csrc/sha256.cuh) compiled for the host against hashlib."""
import hashlib
import os
import random
import subprocess

import pytest

import plonk_batch_ref as bm
import plonk_lookup_ref as lm
import plonk_ref as pm

R = pm.R
TAU = 0x5eed0123456789abcdef0123456789abcdef0123456789abcdef % R
SEED = bytes(range(32))
HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------------------- the equation in the exponent
def _vanilla():
    circuit, _ = pm.chain(8, 1, random.Random(3900))
    st = pm.setup(circuit, TAU)
    proofs = [pm.prove(circuit, pm.chain(8, 1, random.Random(3901 + i))[1], TAU, st) for i in range(3)]
    return 0, st, proofs


def _lookup():
    rng = random.Random(3910)
    table = [tuple(rng.randrange(R) for _ in range(3)) for _ in range(4)]
    table.append(table[0])
    circuit, _ = lm.chain_with_lookups(8, 1, random.Random(3911), table, 3)
    st = lm.setup(circuit, TAU)
    proofs = [lm.prove(circuit, lm.chain_with_lookups(8, 1, random.Random(3912 + i), table, 3)[1], TAU, st) for i in range(2)]
    return 1, st, proofs


@pytest.fixture(scope="module", params=[_vanilla, _lookup], ids=["vanilla", "lookup"])
def proved(request):
    return request.param()


def _batch(proved, k):
    kind, st, proofs = proved
    picked = [proofs[m % len(proofs)] for m in range(k)]
    return kind, st, [p["public"] for p in picked], [p["bytes"] for p in picked], [list(p["logs"]) for p in picked]


def test_the_model_stream_is_the_package_stream():
    from octopuszk_amd import transcript
    for k in (1, 2, 5):
        want = transcript.weights(SEED, k, bm.RHO_TAG)
        assert bm.weights(SEED, k) == [int.from_bytes(want[32 * i:32 * i + 32], "little") for i in range(k)]


@pytest.mark.parametrize("k", [1, 2, 5])
def test_honest_batches_hold(proved, k):
    kind, st, publics, proofs, logs = _batch(proved, k)
    scalars, rho, flags = bm.folded(kind, st["vk"], publics, proofs, bm.weights(SEED, k))
    shape = bm.SHAPES[kind]
    assert flags == [0] * k and len(scalars) == k * (shape["nc"] + 2) + shape["nkey"] + 1
    assert bm.equation_holds(kind, scalars, rho, logs, st["logs"], TAU)
    assert bm.verify_all(kind, st["vk"], publics, proofs, SEED, logs, st["logs"], TAU)
    # every proof alone satisfies its own equation: the batch is their weighted sum
    for public, proof, lg in zip(publics, proofs, logs):
        assert bm.verify_all(kind, st["vk"], [public], [proof], SEED, [lg], st["logs"], TAU)


def test_the_record_is_the_transcript(proved):
    kind, st, publics, proofs, _ = _batch(proved, 2)
    want = proved[2][1]
    rec = bm.record(kind, st["vk"], publics[1], proofs[1], 77)
    names = ("beta", "gamma", "eta", "theta", "alpha", "z") if kind else ("beta", "gamma", "alpha", "z")
    assert rec[:len(names)] == [want[name] for name in names]
    assert rec[len(names) + 2:] == [77] + [0] * (bm.SHAPES[kind]["rec"] - len(names) - 3)


@pytest.mark.parametrize("k", [2, 5])
def test_a_changed_value_commitment_log_or_public_input_fails(proved, k):
    kind, st, publics, proofs, logs = _batch(proved, k)
    shape = bm.SHAPES[kind]
    nc, nv = shape["nc"], shape["nv"]
    for m in range(k):
        for i in range(nv):                                               # one opened value, in the bytes
            at = 32 * (nc + i)
            v = (int.from_bytes(proofs[m][at:at + 32], "little") + 1) % R
            changed = list(proofs)
            changed[m] = proofs[m][:at] + v.to_bytes(32, "little") + proofs[m][at + 32:]
            assert not bm.verify_all(kind, st["vk"], publics, changed, SEED, logs, st["logs"], TAU), (m, i)
        for i in range(nc + 2):                                           # the logarithm of one point of the proof
            changed = [list(lg) for lg in logs]
            changed[m][i] = (changed[m][i] + 1) % R
            assert not bm.verify_all(kind, st["vk"], publics, proofs, SEED, changed, st["logs"], TAU), (m, i)
        changed = [list(x) for x in publics]                              # its public input
        changed[m][0] = (changed[m][0] + 1) % R
        assert not bm.verify_all(kind, st["vk"], changed, proofs, SEED, logs, st["logs"], TAU), m
    for i in range(shape["nkey"]):                                        # the logarithm of one commitment of the key
        key_logs = list(st["logs"])
        key_logs[i] = (key_logs[i] + 1) % R
        assert not bm.verify_all(kind, st["vk"], publics, proofs, SEED, logs, key_logs, TAU), i


def test_flags_of_the_model(proved):
    kind, st, publics, proofs, _ = _batch(proved, 1)
    vk, public, proof = st["vk"], publics[0], proofs[0]
    nc = bm.SHAPES[kind]["nc"]
    assert bm.flags_of(kind, vk, public, proof) == 0
    v = int.from_bytes(proof[32 * nc:32 * nc + 32], "little")
    raised = proof[:32 * nc] + (v + R).to_bytes(32, "little") + proof[32 * nc + 32:]
    assert bm.flags_of(kind, vk, public, raised) == bm.VALUE
    assert bm.flags_of(kind, vk, [R], proof) == bm.PUBLIC
    other = proof[:32 * nc] + ((v + 1) % R).to_bytes(32, "little") + proof[32 * nc + 32:]
    assert bm.flags_of(kind, vk, public, other) == bm.IDENTITY
    from kzg_ref import root
    assert bm.flags_of(kind, vk, public, proof, z=pow(root(8), 3, R)) == bm.DOMAIN
    scalars, rho, flags = bm.folded(kind, vk, [public, public], [proof, other], [5, 6])
    alone, _, _ = bm.folded(kind, vk, [public], [proof], [5])
    assert flags == [0, bm.IDENTITY] and rho == [5, 0]
    assert scalars[nc:2 * nc] == [0] * nc and scalars[2 * nc + 1] == 0 and scalars[2 * nc + 3] == 0
    assert scalars[:nc] == alone[:nc] and scalars[2 * nc + 4:] == alone[nc + 2:]   # the sums leave the flagged proof out


# ---------------------------------------------------------------------------- argument checks: no device call
def _key(n=8, n_public=1, lookup=False):
    from octopuszk_amd import plonk
    cls, count = (plonk.LookupVerifyingKey, 12) if lookup else (plonk.VerifyingKey, 8)
    return cls(n, n_public, [bytes(32)] * count)


@pytest.fixture()
def no_device(monkeypatch):
    """any upload or library call fails the test"""
    from octopuszk_amd import lib
    from octopuszk_amd.plonk import protocol

    def refuse(*a, **k):
        raise AssertionError("a device call before the arguments were checked")
    monkeypatch.setattr(lib, "load", refuse)
    monkeypatch.setattr(protocol, "dev_bytes", refuse)


@pytest.mark.parametrize("fn", ["verify_all", "verify_each"])
def test_argument_checks_raise_before_any_device_call(no_device, fn):
    from octopuszk_amd import plonk
    check = getattr(plonk, fn)
    vk, lvk = _key(), _key(lookup=True)
    one = [[1]]
    with pytest.raises(ValueError):
        check(vk, None, one, bytes(799))                                  # no whole number of proofs
    with pytest.raises(ValueError):
        check(vk, None, one, bytes(1088))                                 # a lookup proof's size under a vanilla key
    with pytest.raises(ValueError):
        check(vk, None, one, [bytes(1088)])
    with pytest.raises(ValueError):
        check(lvk, None, one, [bytes(800)])
    with pytest.raises(ValueError):
        check(lvk, None, one, bytes(800))
    with pytest.raises(ValueError):
        check(vk, None, [[1], [2]], bytes(800))                           # two rows for one proof
    with pytest.raises(ValueError):
        check(vk, None, [[1, 2]], bytes(800))                             # a row of another length
    with pytest.raises(ValueError):
        check(vk, None, bytes(33), bytes(800))                            # public inputs as bytes of the wrong size
    with pytest.raises(ValueError):
        check(vk, None, bytes(64), bytes(800))
    with pytest.raises(ValueError):
        check(_key(n_public=0), None, bytes(32), bytes(800))
    with pytest.raises(ValueError, match="2\\^16"):
        check(_key(n_public=0), None, b"", bytes(800 * ((1 << 16) + 1)))
    with pytest.raises(ValueError, match="2\\^24"):
        check(_key(n=1024, n_public=1023), None, b"", bytes(800 * ((1 << 14) + 1)))
    with pytest.raises(TypeError):
        check(object(), None, one, bytes(800))


def test_an_empty_batch(no_device):
    from octopuszk_amd import plonk
    for vk in (_key(), _key(lookup=True)):
        assert plonk.verify_all(vk, None, [], []) is True and plonk.verify_each(vk, None, [], []) == []
        assert plonk.verify_all(vk, None, b"", b"") is True and plonk.verify_each(vk, None, b"", b"") == []
    with pytest.raises(ValueError):
        plonk.verify_all(_key(), None, [[1]], [])


# ---------------------------------------------------------------------------- the lane's SHA-256 on the host
SRC = os.path.join(HERE, "native", "sha256_hostcheck.cpp")
BIN = os.path.join(HERE, "native", "_sha256_hostcheck")
HDR = os.path.join(HERE, "..", "octopuszk_amd", "csrc", "sha256.cuh")


@pytest.fixture(scope="module")
def sha_prog():
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in (SRC, HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-x", "c++", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-o", BIN, SRC])
    return BIN


def test_sha256_against_hashlib(sha_prog):
    """the lengths around the padding's edges (55 fits one block with its padding, 56 does not, 63 / 64 and 119 the
    same one block on) and the 1651 bytes of a vanilla multi-opening message; by bytes, by words after prefixes of
    0 .. 3 bytes (the tags are byte-odd), and in three pieces"""
    rng = random.Random(3920)
    cases = []
    for length in (0, 1, 3, 55, 56, 57, 63, 64, 65, 119, 120, 128, 374, 536, 1651):
        msg = bytes(rng.randrange(256) for _ in range(length))
        for mode in ("b", "s", "w0", "w1", "w2", "w3"):
            cases.append((mode, msg))
    text = "".join("%s %s\n" % (mode, msg.hex() or "-") for mode, msg in cases)
    out = subprocess.run([sha_prog], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.split()
    assert len(got) == len(cases)
    for (mode, msg), digest in zip(cases, got):
        assert digest == hashlib.sha256(msg).hexdigest(), (mode, len(msg))
