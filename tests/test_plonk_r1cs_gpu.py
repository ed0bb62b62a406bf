"""GPU tests of the witness built on the device: the two entry points of csrc/plonk_r1cs.cuh
against the integer model (tests/plonk_r1cs_ref.py), byte for byte, with sentinel-filled outputs and gaps, and the
import of an R1CS through octopuszk_amd/plonk over the string of known tau that tests/test_plonk_gpu.py uses, where
every proof is also tests/plonk_ref.py's model proof of the compiled circuit."""
import ctypes
import random

import pytest
import torch

import fr_gpu_util as fu
import plonk_r1cs_ref as rm
import plonk_ref as pm

pytestmark = pytest.mark.gpu

R = pm.R
T = 1024                       # PLONK_TILE: the terms of one workgroup
LANE = 8                       # PLONK_L: the consecutive terms of one lane
SCAN = 256                     # PLONK_SCAN_WG: the tile sums one round of the scan takes
E_INVALID = -1
TAU = 0x5eed0123456789abcdef0123456789abcdef0123456789abcdef % R
M = 512
ALL_ONES = fu.ALL_ONES
NONE = rm.NONE


def _u32(values):
    import numpy as np
    return torch.from_numpy(np.array(values, dtype=np.uint32).view(np.uint8).copy()).cuda()


def _written(rng, count):
    """`count` words as a caller may write them: random elements, every third one as x + r, one as 2^256 - 1"""
    words = [rng.randrange(R) + (R if i % 3 == 1 else 0) for i in range(count)]
    words[rng.randrange(count)] = ALL_ONES
    return words


# ---------------------------------------------------------------------------- term sums
def _term_sums(index, coeff, vec, n_vec):
    """ozk_fr_term_sums_dev -> (the sums, the two elements behind them, *d_bad)"""
    L = fu.lib()
    terms = len(index)
    d_i, d_v = _u32(index), fu.dev_from_ints(vec, guard=64)
    d_c = None if coeff is None else fu.dev_from_ints(coeff)
    out, bad = fu.poisoned((terms + 2) * 32), fu.poisoned(16)
    wsb = L.ozk_fr_term_sums_workspace_bytes(terms)
    assert wsb > 0
    ws = fu.workspace(wsb)
    rc = L.ozk_fr_term_sums_dev(fu.ptr(d_i), None if d_c is None else fu.ptr(d_c), fu.ptr(d_v), n_vec, terms, fu.ptr(out),
                                fu.ptr(bad), fu.ptr(ws), wsb, fu.stream())
    assert rc == 0, L.ozk_last_error()
    got, tail = fu.words(fu.host_bytes(out)), fu.host_bytes(bad)
    assert tail[4:] == bytes([fu.POISON]) * 12
    return got[:terms], got[terms:], int.from_bytes(tail[:4], "little", signed=True)


# below, at and past a lane's 8 terms; the tile boundary; a middle tile with no edge; one term past a round of SCAN
# tile sums in the scan of the carries (the crossing of test_perm_product_past_one_round_of_the_scan)
TERMS = [1, LANE - 1, LANE, LANE + 1, T - 1, T, T + 1, 2 * T + 1, (SCAN + 1) * T + 1]


@pytest.fixture(scope="module")
def streams():
    """for every length: indices that repeat, vec and coefficient words as written, and the model's sums of both"""
    out = {}
    for terms in TERMS:
        rng = random.Random(3610 + terms)
        n_vec = min(terms, 37) + 3
        index = [rng.randrange(n_vec) for _ in range(terms)]
        vec, coeff = _written(rng, n_vec), _written(rng, terms)
        out[terms] = (index, coeff, vec, n_vec, rm.term_sums(index, None, vec, n_vec), rm.term_sums(index, coeff, vec, n_vec))
    return out


@pytest.mark.parametrize("with_coeff", [False, True], ids=["ones", "coeff"])
@pytest.mark.parametrize("terms", TERMS)
def test_term_sums_match_the_model(streams, terms, with_coeff):
    index, coeff, vec, n_vec, plain, weighted = streams[terms]
    want, none_bad = weighted if with_coeff else plain
    got, behind, bad = _term_sums(index, coeff if with_coeff else None, vec, n_vec)
    assert not fu.mismatches(got, want)[:4] and bad == none_bad == 0
    assert behind == [fu.POISON_INT] * 2
    assert all(v < R for v in got)


@pytest.mark.parametrize("with_coeff", [False, True], ids=["ones", "coeff"])
@pytest.mark.parametrize("terms", [LANE + 1, T + 1, 2 * T + 1])
def test_term_sums_with_two_indices_outside_vec(streams, terms, with_coeff):
    """one index = n_vec (the first element behind vec) and one = 0xFFFFFFFE: never read, zero, counted"""
    index, coeff, vec, n_vec, _, _ = streams[terms]
    index = list(index)
    index[terms // 2], index[terms - 1] = n_vec, 0xFFFFFFFE
    want, two = rm.term_sums(index, coeff if with_coeff else None, vec, n_vec)
    got, behind, bad = _term_sums(index, coeff if with_coeff else None, vec, n_vec)
    assert two == 2 and bad == 2
    assert not fu.mismatches(got, want)[:4] and behind == [fu.POISON_INT] * 2
    assert got[terms // 2] == got[terms // 2 - 1] and got[terms - 1] == got[terms - 2]


# ---------------------------------------------------------------------------- wires
def _wires(src, cells, length, cell_stride, out_stride):
    """ozk_plonk_wires_dev over k rows of descriptors -> (the rows, the elements of the gaps, *d_bad)"""
    L = fu.lib()
    k = len(cells)
    flat = []
    for row in cells:
        flat += [w for d in row for w in d] + [0xDEAD, 0xBEEF] * (cell_stride - length)
    d_s, d_c = fu.dev_from_ints(src, guard=64), _u32(flat)
    out, bad = fu.poisoned(k * out_stride * 32), fu.poisoned(16)
    rc = L.ozk_plonk_wires_dev(fu.ptr(d_s), len(src), fu.ptr(d_c), k, length, cell_stride, fu.ptr(out), out_stride,
                               fu.ptr(bad), fu.stream())
    assert rc == 0, L.ozk_last_error()
    got = fu.words(fu.host_bytes(out))
    tail = fu.host_bytes(bad)
    assert tail[4:] == bytes([fu.POISON]) * 12
    rows = [got[y * out_stride:y * out_stride + length] for y in range(k)]
    gaps = [v for y in range(k) for v in got[y * out_stride + length:(y + 1) * out_stride]]
    return rows, gaps, int.from_bytes(tail[:4], "little", signed=True)


@pytest.mark.parametrize("outside", [False, True], ids=["inside", "two_outside"])
@pytest.mark.parametrize("length", [1, 255, 256, 257])
def test_wires_match_the_model(length, outside):
    rng = random.Random(3620 + length)
    n_src = 50
    src = _written(rng, n_src)
    small, large = min(range(n_src), key=lambda v: src[v] % R), max(range(n_src), key=lambda v: src[v] % R)
    cells = [[(rng.randrange(n_src), NONE if rng.randrange(3) == 0 else rng.randrange(n_src)) for _ in range(length)]
             for _ in range(3)]
    cells[0][0] = (small, large)                                          # src[hi] < src[lo]: wraps mod r
    cells[1][length - 1] = (large, large)                                 # hi == lo: zero
    cells[2][length // 2] = (large, NONE)
    if outside:
        cells[1][0] = (n_src, NONE)
        cells[2][length - 1] = (small, n_src + 5)
    want, count = rm.wires(src, cells)
    assert count == (2 if outside else 0) and want[0][0] == (src[small] - src[large]) % R != 0
    rows, gaps, bad = _wires(src, cells, length, length + 3, length + 2)
    assert rows == want and bad == count
    assert all(v == fu.POISON_INT for v in gaps) and len(gaps) == 6
    if outside:
        assert rows[1][0] == 0 and rows[2][length - 1] == 0
    else:
        assert rows[1][length - 1] == 0


# ---------------------------------------------------------------------------- rejections
def test_rejected_calls_launch_nothing():
    L = fu.lib()
    n = 16
    buf = fu.poisoned(64 * n * 32)
    ws = fu.workspace(1 << 16)
    null, stream = ctypes.c_void_p(0), fu.stream()
    index, coeff, vec, out = buf[:4 * n], buf[32 * n:64 * n], buf[64 * n:96 * n], buf[96 * n:128 * n]
    bad = buf[128 * n:128 * n + 4]

    def sums(i_, c_, v_, n_vec, terms, o_, b_, w=fu.ptr(ws), wbytes=1 << 16):
        return L.ozk_fr_term_sums_dev(i_, c_, v_, n_vec, terms, o_, b_, w, wbytes, stream)

    good = [fu.ptr(index), fu.ptr(coeff), fu.ptr(vec), n, n, fu.ptr(out), fu.ptr(bad)]
    for terms in (0, -1, (1 << 28) + 1):
        assert L.ozk_fr_term_sums_workspace_bytes(terms) == 0
        assert sums(null, null, null, n, terms, null, null, w=null, wbytes=0) == E_INVALID
    for n_vec in (0, -1, 1 << 32):
        assert sums(*(good[:3] + [n_vec] + good[4:])) == E_INVALID
    for i in (0, 2, 5, 6):
        assert sums(*(good[:i] + [null] + good[i + 1:])) == E_INVALID
    assert sums(*good, w=null) == E_INVALID
    for i, off in ((0, index[8:]), (1, coeff[8:]), (2, vec[8:]), (5, out[8:])):
        assert sums(*(good[:i] + [fu.ptr(off)] + good[i + 1:])) == E_INVALID
        assert b"aligned" in L.ozk_last_error()
    assert sums(*(good[:6] + [fu.ptr(buf[128 * n + 1:])])) == E_INVALID
    for o_bad in (vec[(n - 1) * 32:], coeff, index[:16]):
        assert sums(*(good[:5] + [fu.ptr(o_bad)] + good[6:])) == E_INVALID
        assert b"overlap" in L.ozk_last_error()
    assert sums(*(good[:6] + [fu.ptr(out[32:])])) == E_INVALID                                # the count inside the sums
    assert sums(*good, wbytes=L.ozk_fr_term_sums_workspace_bytes(n) - 1) == E_INVALID
    assert b"workspace" in L.ozk_last_error()
    assert sums(*good, w=fu.ptr(out)) == E_INVALID                                            # the workspace over the sums

    src, cells, wout = buf[:32 * n], buf[32 * n:32 * n + 3 * n * 8], buf[64 * n:64 * n + 3 * n * 32]
    wbad = buf[60 * n * 32:60 * n * 32 + 4]

    def wires(s_, n_src, c_, k, length, cstride, o_, ostride, b_):
        return L.ozk_plonk_wires_dev(s_, n_src, c_, k, length, cstride, o_, ostride, b_, stream)

    good = [fu.ptr(src), n, fu.ptr(cells), 3, n, n, fu.ptr(wout), n, fu.ptr(wbad)]
    for k, length in ((0, n), (3, 0), (-1, n), (3, (1 << 28) // 3 + 1)):
        assert wires(null, n, null, k, length, length, null, length, null) == E_INVALID
    for n_src in (0, 1 << 32):
        assert wires(*(good[:1] + [n_src] + good[2:])) == E_INVALID
    assert wires(*(good[:5] + [n - 1] + good[6:])) == E_INVALID
    assert wires(*(good[:7] + [n - 1] + good[8:])) == E_INVALID
    for i in (0, 2, 6, 8):
        assert wires(*(good[:i] + [null] + good[i + 1:])) == E_INVALID
    for i, off in ((0, src[8:]), (6, wout[8:])):
        assert wires(*(good[:i] + [fu.ptr(off)] + good[i + 1:])) == E_INVALID
        assert b"aligned" in L.ozk_last_error()
    assert wires(*(good[:2] + [fu.ptr(cells[4:])] + good[3:])) == E_INVALID
    assert wires(*(good[:8] + [fu.ptr(buf[60 * n * 32 + 2:])])) == E_INVALID
    for o_bad in (src[(n - 1) * 32:], cells[(3 * n - 4) * 8:]):
        assert wires(*(good[:6] + [fu.ptr(o_bad)] + good[7:])) == E_INVALID
        assert b"overlap" in L.ozk_last_error()
    assert wires(*(good[:8] + [fu.ptr(wout[32:])])) == E_INVALID                              # the count inside the output
    assert fu.host_bytes(buf) == bytes([fu.POISON]) * buf.numel()


# ---------------------------------------------------------------------------- the protocol
@pytest.fixture(scope="module")
def string():
    from octopuszk_amd import kzg, srs
    s = srs.Srs.from_secrets(M, TAU, 1, 1, generator=1)
    return s, kzg.VerifyKey.from_srs(s)


def _on_device(values):
    return fu.dev_from_ints(values)


def _cases(name):
    from octopuszk_amd import zksnark as z
    if name == "mixed":
        return rm.mixed_relation()
    nc, ni = {"serial_6_2": (6, 2), "serial_30_3": (30, 3)}[name]
    r1cs, primary, auxiliary = z.serial_construct(nc, ni)
    return r1cs, primary + auxiliary


@pytest.fixture(scope="module", params=["serial_6_2", "serial_30_3", "mixed"])
def imported(request, string):
    """one R1CS compiled, set up and proved from the device, from a list and by the model"""
    from octopuszk_amd import kzg, plonk
    s, kvk = string
    r1cs, full = _cases(request.param)
    circuit = plonk.from_r1cs(r1cs)
    pk, vk = plonk.setup(circuit, kzg.CommitKey.from_srs(s, circuit.n))
    model = pm.Circuit(circuit.n, circuit.selectors, circuit.wires, circuit.n_public)
    return {"r1cs": r1cs, "full": full, "circuit": circuit, "pk": pk, "vk": vk, "kvk": kvk,
            "proof": plonk.prove(pk, _on_device(full)), "from_list": plonk.prove(pk, list(full)),
            "want": pm.prove(model, circuit.extend(full), TAU)}


def test_an_imported_r1cs_proves_from_the_device(imported):
    from octopuszk_amd import plonk
    from octopuszk_amd.wire import le32
    pk, vk, proof, full = imported["pk"], imported["vk"], imported["proof"], imported["full"]
    assert isinstance(pk, plonk.R1CSProvingKey) and isinstance(pk, plonk.ProvingKey) and isinstance(vk, plonk.VerifyingKey)
    assert (pk.term_coeff is None) == (imported["circuit"].term_coeff is None)
    primary = full[:imported["r1cs"].num_inputs]
    assert primary[0] == 1 and imported["want"]["public"] == primary
    assert plonk.verify(vk, imported["kvk"], primary, proof)
    assert proof.to_bytes() == imported["from_list"].to_bytes()
    assert proof.to_bytes() == imported["want"]["bytes"]
    assert plonk.prove(pk, le32(full)).to_bytes() == proof.to_bytes()
    wide = [v + R if i % 2 and v + R <= ALL_ONES else v for i, v in enumerate(full)]
    assert plonk.prove(pk, _on_device(wide)).to_bytes() == proof.to_bytes()           # words taken mod r
    timings = {}
    assert plonk.prove(pk, _on_device(full), timings).to_bytes() == proof.to_bytes()
    assert set(timings) == set(plonk.protocol.STAGES)


def test_a_changed_auxiliary_value_is_a_violated_gate(imported):
    from octopuszk_amd import plonk
    full, ni = list(imported["full"]), imported["r1cs"].num_inputs
    full[ni + 1] = (full[ni + 1] + 1) % R
    with pytest.raises(ValueError, match="a gate is violated"):
        plonk.prove(imported["pk"], _on_device(full))
    with pytest.raises(ValueError, match="a gate is violated"):
        plonk.prove(imported["pk"], full)


def test_a_changed_public_input_is_refused(imported):
    from octopuszk_amd import plonk
    primary = list(imported["full"][:imported["r1cs"].num_inputs])
    primary[-1] = (primary[-1] + 1) % R
    assert not plonk.verify(imported["vk"], imported["kvk"], primary, imported["proof"])


def test_an_assignment_of_the_wrong_length_is_refused(imported):
    from octopuszk_amd import plonk
    from octopuszk_amd.wire import le32
    pk, full = imported["pk"], imported["full"]
    for wrong in (full[:-1], full + [0], imported["circuit"].extend(full)):
        with pytest.raises(ValueError):
            plonk.prove(pk, _on_device(wrong))
        with pytest.raises(ValueError):
            plonk.prove(pk, list(wrong))
        with pytest.raises(ValueError):
            plonk.prove(pk, le32(wrong))


def test_any_circuit_proves_from_the_device(string):
    """a hand-built circuit whose public variable is not its first: the same bytes as from the list"""
    from octopuszk_amd import kzg, plonk
    s, kvk = string
    b = plonk.Builder()
    y = b.var()
    x = b.public()
    xy, out = b.var(), b.var()
    b.mul(x, y, xy)
    b.add(xy, x, out)
    b.constant(y, 7)
    circuit = b.build()
    values = [7, 5, 35, 40]
    pk, vk = plonk.setup(circuit, kzg.CommitKey.from_srs(s, circuit.n))
    assert pk.cells is None
    proof = plonk.prove(pk, _on_device(values))
    assert pk.cells is not None and proof.to_bytes() == plonk.prove(pk, values).to_bytes()
    assert plonk.verify(vk, kvk, [5], proof)
    with pytest.raises(ValueError):
        plonk.prove(pk, _on_device(values + [1]))
    with pytest.raises(ValueError, match="a gate is violated"):
        plonk.prove(pk, _on_device([7, 5, 35, 41]))
