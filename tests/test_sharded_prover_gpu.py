"""zksnark.ShardedProver + distributed.distributed_prove on hardware: each rank proves over its slices of the key and
sends one 768-byte partial, one all-gather, one combine launch.  W = 1 in process (the single record goes through
ozk_groth16_combine_dev); W = 2 and 3 as gloo ranks sharing cuda:0 (spawned children: RCCL refuses two ranks on
one device).  Expected: the oracle's proof bytes at 2^10, SerialProver's bytes, and the known-scalar identity of
test_groth16_gpu on ragged shapes and at 2^20."""
import os
import socket
import traceback

import pytest
import torch
import torch.multiprocessing as mp

from oracle import bn254 as o
from oracle import groth16 as g

pytestmark = pytest.mark.gpu

NC, NI = 1 << 10, 15
R = o.R


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, nc, ni, witness, q):
    """One gloo rank on cuda:0: builds the (deterministic) key itself, proves its share, returns the proof bytes,
    its own record and key byte counts, and (rank 0) coefficientsH."""
    import torch.distributed as dist
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from octopuszk_amd import distributed as D
        from octopuszk_amd import zksnark as z
        r1cs, primary, auxiliary = z.serial_construct(nc, ni)
        if witness is not None:
            primary, auxiliary = witness
        crs = z.serial_setup_generate(r1cs)
        prover = z.ShardedProver(crs.proving_key, rank, world)
        del crs
        proof = D.distributed_prove(prover, primary, auxiliary, z.SEED, gather=D.all_gather_partials_host)
        rec = bytes(prover.prove_partial(primary, auxiliary, z.SEED).cpu().numpy())
        h = bytes(prover.d_h.cpu().numpy()) if rank == 0 else None
        prover.close()
        q.put((rank, "ok", dict(proof=(proof.g_a, proof.g_b, proof.g_c), rec=rec, h=h, key_bytes=prover.key_bytes)))
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        q.put((rank, "error", traceback.format_exc()))
        raise


def _run_world(world, nc, ni, witness=None, timeout=600):
    assert world <= 3   # at most 3 children beside the parent on the one device
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, nc, ni, witness, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    try:
        for _ in range(world):
            rank, status, payload = q.get(timeout=timeout)
            assert status == "ok", "rank %d:\n%s" % (rank, payload)
            got[rank] = payload
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.exitcode is None:
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    return got


@pytest.fixture(scope="module")
def oracle_2p10():
    r1cs, primary, auxiliary = g.serial_construct(NC, NI)
    crs = g.serial_setup(r1cs)
    (A, B, C), _ = g.serial_prove(crs, primary, auxiliary)
    return o.g1_out_le(o.G1.to_affine(A)), o.g2_out_le(o.G2.to_affine(B)), o.g1_out_le(o.G1.to_affine(C))


def _serial_proof(nc, ni, witness=None):
    from octopuszk_amd import zksnark as z
    r1cs, primary, auxiliary = z.serial_construct(nc, ni)
    if witness is not None:
        primary, auxiliary = witness
    crs = z.serial_setup_generate(r1cs)
    prover = z.SerialProver(crs.proving_key)
    try:
        p = prover.prove(primary, auxiliary)
    finally:
        prover.close()
    return (p.g_a, p.g_b, p.g_c), crs


def test_world_of_one_equals_serial_prover_and_oracle(oracle_2p10):
    from octopuszk_amd import distributed as D
    from octopuszk_amd import zksnark as z
    serial, crs = _serial_proof(NC, NI)
    assert serial == oracle_2p10
    r1cs, primary, auxiliary = z.serial_construct(NC, NI)
    prover = z.ShardedProver(crs.proving_key, 0, 1)
    try:
        assert prover.key_bytes["rank"] == prover.key_bytes["serial"]
        for _ in range(2):   # second call: buffers reused
            T = {}
            proof = D.distributed_prove(prover, primary, auxiliary, z.SEED, timing=T)
            assert (proof.g_a, proof.g_b, proof.g_c) == oracle_2p10
            assert {"witness_map_done_ms", "record_done_ms", "exchange_ms", "combine_ms"} <= set(T)
    finally:
        prover.close()


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_ranks_give_the_oracle_proof(world, oracle_2p10):
    got = _run_world(world, NC, NI)
    for r in range(world):
        assert got[r]["proof"] == oracle_2p10, r
        kb = got[r]["key_bytes"]
        assert kb["rank"] < kb["serial"] / world * 1.05 + (1 << 16), kb   # this rank's slices only


def _known_scalar_proof(crs, primary, auxiliary, H):
    """(A, B, C) wire-out bytes from the key's scalars (test_groth16_gpu._check_by_known_scalars), after checking the
    verification equation in the exponent."""
    from octopuszk_amd import zksnark as z
    full = primary + auxiliary
    ni = len(primary)
    q, sec, sc = crs.qap, crs.secrets, crs.scalars
    r = s = z.fr_random()
    m = q.degree
    assert H[m - 1] == 0 and H[m] == 0
    a = (sec["alpha"] + sum(x * y for x, y in zip(full, q.At)) + r * sec["delta"]) % R
    b = (sec["beta"] + sum(x * y for x, y in zip(full, q.Bt)) + s * sec["delta"]) % R
    c = (sum(x * y for x, y in zip(full[ni:], sc["delta_abc"])) + sum(x * y for x, y in zip(H, sc["ht"]))
         + a * s + b * r - r * s * sec["delta"]) % R
    acc = sum(x * y for x, y in zip(primary, sc["gamma_abc"])) % R
    assert (a * b - sec["alpha"] * sec["beta"] - acc * sec["gamma"] - c * sec["delta"]) % R == 0
    gen = sec["generator"]
    return (o.g1_out_le(o.G1.to_affine(o.G1.mul(o.G1.one, a * gen % R))),
            o.g2_out_le(o.G2.to_affine(o.G2.mul(o.G2.one, b * gen % R))),
            o.g1_out_le(o.G1.to_affine(o.G1.mul(o.G1.one, c * gen % R))))


def _check_sharded_by_known_scalars(nc, ni, world):
    from octopuszk_amd import zksnark as z
    got = _run_world(world, nc, ni, timeout=1200)
    r1cs, primary, auxiliary = z.serial_construct(nc, ni)
    crs = z.serial_setup_generate(r1cs)
    raw = got[0]["h"]
    H = [int.from_bytes(raw[k:k + 32], "little") for k in range(0, len(raw), 32)]
    want = _known_scalar_proof(crs, primary, auxiliary, H)
    for r in range(world):
        assert got[r]["proof"] == want, r


@pytest.mark.parametrize("nc,ni", [(50, 50), (257, 1), (1000, 24)])
def test_three_ranks_known_scalars_ragged(nc, ni):
    _check_sharded_by_known_scalars(nc, ni, 3)


def test_two_ranks_known_scalars_2p20():
    """BASELINE.json configs[4] size: 2^20 constraints, 1023 inputs, over two ranks."""
    logn = int(os.environ.get("OZK_TEST_GROTH16_LOGN", "20"))
    _check_sharded_by_known_scalars(1 << logn, 1023, 2)


def test_middle_rank_with_an_all_zero_slice():
    """The middle rank's slice of z is all zeros, so its A_r and B_r are infinity ((0, 1, 0) on the wire): the
    combined proof still equals SerialProver's on the same (unsatisfying) witness."""
    from octopuszk_amd import zksnark as z
    world = 3
    r1cs, primary, auxiliary = z.serial_construct(NC, NI)
    full = primary + auxiliary
    nv = len(full)
    lo, hi = z.shard_plan(nv, z.lowest_power_of_two(NC + NI), nv - NI, 1, world)["A"]
    assert 0 < lo < hi < nv
    full[lo:hi] = [0] * (hi - lo)
    witness = (full[:NI], full[NI:])
    want, _ = _serial_proof(NC, NI, witness)
    got = _run_world(world, NC, NI, witness)
    rec = got[1]["rec"]
    assert rec[:192] == o.g1_out_le((0, 1, 0))
    assert rec[192:576] == o.g2_out_le(((0, 0), (1, 0), (0, 0)))
    for r in range(world):
        assert got[r]["proof"] == want, r


def test_world_too_large_is_refused():
    from octopuszk_amd import zksnark as z
    r1cs, _, _ = z.serial_construct(50, 50)   # nw = 3: a fourth rank would own no deltaABC element
    crs = z.serial_setup_generate(r1cs)
    z.ShardedProver(crs.proving_key, 2, 3).close()
    with pytest.raises(ValueError):
        z.ShardedProver(crs.proving_key, 0, 4)
    with pytest.raises(ValueError):
        z.ShardedProver(crs.proving_key, 3, 3)
