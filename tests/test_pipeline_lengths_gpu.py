"""GPU parity of the device pipelines (device.VarMsmPipeline, VarMsmPipeline3) with a length per submission, results
in the caller's tensors, both meanings of submit(last=True) and both tail shapes — the form the Groth16 prover uses:
same bytes as the single-call path (VarMsmWorkspace) on the same inputs.  The buffers of such a pipeline are sized
for the longest MSM and laid out, submission by submission, by the plan of the length at hand."""
import random

import pytest

from oracle import bn254 as o

pytestmark = pytest.mark.gpu

LENGTHS = [300, 4097, 5, (1 << 12) + 77, 1]
SUBMISSIONS = 11        # more than twice the depth: every slot and both sorted sets serve MSMs of different plans
KINDS = ["two-stage", "three-stage-1", "three-stage-2"]


def _scalars(n, seed):
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    sc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sc[:, 31] &= 0x1F
    return torch.from_numpy(sc.reshape(-1)).cuda()


def _pipeline(kind, sizes, type_=1, **kw):
    from octopuszk_amd import device as dev
    if kind == "two-stage":
        return dev.VarMsmPipeline(sizes, type_, depth=2, **kw)
    return dev.VarMsmPipeline3(sizes, type_, depth=4, tail_streams=int(kind[-1]), **kw)


def _reference(lengths, type_, bases, count, seed):
    """`count` submissions that cycle through `lengths`: (n, scalars, bytes of the single call) each"""
    import torch
    from octopuszk_amd import device as dev
    ws = {n: dev.VarMsmWorkspace(n, type_) for n in lengths}
    subs = []
    for i in range(count):
        n = lengths[i % len(lengths)]
        d_sc = _scalars(n, seed + i)
        out = ws[n].run(bases[n], d_sc)
        torch.cuda.synchronize()
        subs.append((n, d_sc, bytes(out.cpu().numpy())))
    return subs


@pytest.fixture(scope="module")
def mixed():
    """bases of their own for each length (wire format and prepared) and the submissions over them"""
    from octopuszk_amd import device as dev
    bases = {n: dev.gen_g1_bases(n, seed=60 + i) for i, n in enumerate(LENGTHS)}
    prepared = {n: dev.prepare_bases(b, n, 1) for n, b in bases.items()}
    subs = _reference(LENGTHS, 1, bases, SUBMISSIONS, 500)
    assert len({want for _, _, want in subs}) == SUBMISSIONS
    return bases, prepared, subs


@pytest.mark.parametrize("tail_mode", [0, 1])
@pytest.mark.parametrize("prepared", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_mixed_lengths_into_callers_tensors(mixed, kind, prepared, tail_mode):
    import torch
    bases = mixed[1] if prepared else mixed[0]
    pipe = _pipeline(kind, LENGTHS, tail_mode=tail_mode)
    assert pipe.n == max(LENGTHS) and pipe.depth == (2 if kind == "two-stage" else 4)
    outs = torch.zeros(SUBMISSIONS, 192, dtype=torch.uint8, device="cuda")
    for i, (n, d_sc, _) in enumerate(mixed[2]):
        assert pipe.submit(bases[n], d_sc, prepared=prepared, n=n, out=outs[i]) == i
    torch.cuda.synchronize()
    pipe.close()
    assert [bytes(row.cpu().numpy()) for row in outs] == [want for _, _, want in mixed[2]]


@pytest.mark.parametrize("tail_mode", [0, 1])
@pytest.mark.parametrize("prepared", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_mixed_lengths_results_one_submission_late(mixed, kind, prepared, tail_mode):
    bases = mixed[1] if prepared else mixed[0]
    pipe = _pipeline(kind, LENGTHS, tail_mode=tail_mode)
    got, prev = [], None
    for n, d_sc, _ in mixed[2]:
        t = pipe.submit(bases[n], d_sc, prepared=prepared, n=n)
        if prev is not None:
            got.append(pipe.result(prev).clone())
        prev = t
    got.append(pipe.result(prev).clone())
    import torch
    torch.cuda.synchronize()
    pipe.close()
    assert [bytes(g.cpu().numpy()) for g in got] == [want for _, _, want in mixed[2]]


def test_length_and_output_are_checked(mixed):
    import torch
    pipe = _pipeline("three-stage-1", [300, 5])
    with pytest.raises(ValueError):
        pipe.submit(mixed[0][1], _scalars(1, 1), n=1)          # not a length the buffers were sized for
    with pytest.raises(ValueError):
        pipe.submit(mixed[0][5], _scalars(5, 1), n=5, out=torch.zeros(96, dtype=torch.uint8, device="cuda"))
    assert pipe.count == 0


@pytest.mark.parametrize("prepared", [False, True])
@pytest.mark.parametrize("last_lone", [False, True])
@pytest.mark.parametrize("kind", ["two-stage", "three-stage-1"])
def test_last_submission(mixed, kind, last_lone, prepared):
    """submit(last=True) as the fifth submission — a latency-shaped tail, or with last_lone the whole MSM through the
    single-call entry point — and, after a lone one, four more: the next proof's reuse of the slots."""
    import torch
    from octopuszk_amd import device as dev
    lengths = [4097, 300]
    bases = {n: (mixed[1] if prepared else mixed[0])[n] for n in lengths}
    ws = {n: dev.VarMsmWorkspace(n, 1) for n in lengths}
    count = 9 if last_lone else 5
    pipe = _pipeline(kind, lengths, last_lone=last_lone)
    assert hasattr(pipe, "full_ws") == last_lone
    subs = []
    for i in range(count):
        n = lengths[i % 2]
        d_sc = _scalars(n, 700 + i)
        ref = ws[n].run(bases[n], d_sc, prepared=prepared)
        torch.cuda.synchronize()
        subs.append((n, d_sc, bytes(ref.cpu().numpy())))
    outs = torch.zeros(count, 192, dtype=torch.uint8, device="cuda")
    for i, (n, d_sc, _) in enumerate(subs):
        pipe.submit(bases[n], d_sc, prepared=prepared, last=(i == 4), n=n, out=outs[i])
    torch.cuda.synchronize()
    want = [w for _, _, w in subs]
    pipe.close()
    assert [bytes(row.cpu().numpy()) for row in outs] == want and len(set(want)) == count


@pytest.mark.parametrize("kind", ["two-stage", "three-stage-2"])
def test_mixed_lengths_g2(kind):
    import numpy as np
    import torch
    rng = random.Random(31)
    G, lengths = o.G2, [7, 300]
    pts = [G.to_affine(G.mul(G.one, rng.randrange(1, 1 << 64))) for _ in range(48)]
    wire = lambda k, n: b"".join(o.g2_to_wire(pts[(k + i) % len(pts)]) for i in range(n))
    bases = {n: torch.from_numpy(np.frombuffer(wire(k, n), dtype=np.uint8).copy()).cuda() for k, n in enumerate(lengths)}
    subs = _reference(lengths, 2, bases, 5, 800)
    pipe = _pipeline(kind, lengths, type_=2)
    outs = torch.zeros(5, 384, dtype=torch.uint8, device="cuda")
    for i, (n, d_sc, _) in enumerate(subs):
        pipe.submit(bases[n], d_sc, n=n, out=outs[i])
    torch.cuda.synchronize()
    pipe.close()
    want = [w for _, _, w in subs]
    assert [bytes(row.cpu().numpy()) for row in outs] == want and len(set(want)) == 5


@pytest.mark.parametrize("kind", ["two-stage", "three-stage-2"])
def test_shorter_length_vs_oracle(mixed, kind):
    """n = 97 with the edge scalars and points of test_three_stage_pipeline_vs_oracle_small, in buffers sized for 300
    and right behind an MSM of that length: the oracle's bytes."""
    import numpy as np
    import torch
    rng = random.Random(77)
    n, G = 97, o.G1
    bases = [G.to_affine(G.mul(G.one, rng.randrange(1, 1 << 64))) for _ in range(n)]
    bases[3] = G.zero
    bases[10] = G.negate(bases[11])
    scalars = [rng.randrange(o.R) for _ in range(n)]
    scalars[0], scalars[1], scalars[2] = 0, 1, o.R - 1
    scalars[10] = scalars[11] = 4242
    d_bases = torch.from_numpy(np.frombuffer(b"".join(o.g1_to_wire(b) for b in bases), dtype=np.uint8).copy()).cuda()
    d_sc = torch.from_numpy(np.frombuffer(b"".join(s.to_bytes(32, "little") for s in scalars), dtype=np.uint8).copy()).cuda()
    pipe = _pipeline(kind, [300, n])
    pipe.submit(mixed[0][300], mixed[2][0][1], n=300)
    got = pipe.result(pipe.submit(d_bases, d_sc, n=n))
    torch.cuda.synchronize()
    pipe.close()
    assert bytes(got.cpu().numpy()) == o.g1_out_le(G.to_affine(o.naive_msm(G, scalars, bases)))


def test_prover_pipeline_variants(monkeypatch):
    """The prover's G1 pipeline as each OZK_PROVER_* variable selects it: the same witness proved twice by each
    prover gives one and the same proof, and the verifier accepts it."""
    from octopuszk_amd import device as dev, zksnark as z
    r1cs, primary, auxiliary = z.serial_construct(1000, 24)
    crs = z.serial_setup_generate(r1cs)
    variants = [({}, dev.VarMsmPipeline3, True, 1), ({"OZK_PROVER_PIPE3": "0"}, dev.VarMsmPipeline, True, None),
                ({"OZK_PROVER_LAST_LONE": "0"}, dev.VarMsmPipeline3, False, 1),
                ({"OZK_PROVER_TAIL_STREAMS": "2"}, dev.VarMsmPipeline3, True, 2)]
    proofs = []
    for env, cls, lone, tail_streams in variants:
        with monkeypatch.context() as m:
            for name in ("OZK_PROVER_PIPE3", "OZK_PROVER_LAST_LONE", "OZK_PROVER_TAIL_STREAMS"):
                m.delenv(name, raising=False)
            for name, value in env.items():
                m.setenv(name, value)
            prover = z.SerialProver(crs.proving_key)
        try:
            assert type(prover.pipe) is cls and prover.pipe.last_lone == lone and prover.pipe.tail_mode == 1
            if tail_streams:
                assert len(prover.pipe.tail_st) == tail_streams and not prover.pipe.split and prover.pipe.tail_cus == 0
            proofs += [prover.prove(primary, auxiliary) for _ in range(2)]
        finally:
            prover.close()
    assert len(proofs) == 8 and len({(p.g_a, p.g_b, p.g_c) for p in proofs}) == 1
    assert z.Verifier.verify(z.verification_key(crs), primary, proofs[0]) is True


def test_pipeline_is_a_context_manager(mixed):
    """close() on leaving the block destroys the confined streams, after the wrappers of them are dropped"""
    import torch
    from octopuszk_amd import device as dev
    n, d_sc, want = mixed[2][0]
    assert n == 300
    with dev.VarMsmPipeline3(300, 1, tail_cus=32) as p:
        assert len(p._owned) == 3
        with torch.cuda.stream(torch.cuda.Stream()):
            got = p.result(p.submit(mixed[0][n], d_sc)).clone()
        torch.cuda.synchronize()
    assert bytes(got.cpu().numpy()) == want
    assert p._owned == [] and p.acc is None and p.tail_st is None and p.side is None
    p.close()       # a second close is a no-op
    with dev.VarMsmPipeline(300, 1) as q:
        assert bytes(q.result(q.submit(mixed[0][n], d_sc)).cpu().numpy()) == want
    assert q.levels_done == []
    q.close()
