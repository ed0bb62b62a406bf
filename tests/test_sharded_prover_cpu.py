"""CPU tests of the sharded Groth16 prover's plan and composition (zksnark.shard_plan, zksnark.c_share_scalars,
distributed.distributed_prove): gloo worlds of 2 and 3 build each rank's 768-byte partial with the oracle's MSMs
over the plan, exchange them with one all-gather and sum them on the host — the result must be the oracle's
SerialProver proof (DistributedProver.java:89-146 semantics: the proof elements are sums over the ranks)."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import bn254 as o
from oracle import groth16 as g

NC, NI = 64, 5


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_shard_plan_covers_every_index_once(world):
    from octopuszk_amd import zksnark as z
    for nv, m, nw in ((8, 16, 5), (53, 128, 3), (1027, 2048, 1024), ((1 << 20) + 3, 1 << 21, (1 << 20) - 1020)):
        plans = [z.shard_plan(nv, m, nw, r, world) for r in range(world)]
        assert set(plans[0]) == {"A", "B1", "B2", "L", "H"}
        for key, n in (("A", nv + 2), ("B1", nv + 2), ("B2", nv + 2), ("L", nw), ("H", m + 1)):
            seen = [0] * n
            for p in plans:
                lo, hi = p[key]
                for i in range(lo, hi):
                    seen[i] += 1
            assert seen == [1] * n, (key, nv, m, nw)
        assert all(p["A"] == p["B1"] == p["B2"] for p in plans)   # the same scalars z ++ [1, r | s] cut the same way


def test_rs_delta_term_on_rank_zero_only():
    from octopuszk_amd import zksnark as z
    r, s = 12345, 67890
    assert z.c_share_scalars(r, s, 0) == [s, r, (o.R - r * s) % o.R]
    for rank in (1, 2, 7):
        assert z.c_share_scalars(r, s, rank) == [s, r, 0]


class _OracleRank:
    """A ShardedProver stand-in: the same plan and the same per-rank formula, with the oracle's MSMs."""

    def __init__(self, crs, rank, world):
        self.crs, self.rank, self.world = crs, rank, world

    def prove_partial(self, primary, auxiliary, seed, timing=None, full_bytes=None):
        from octopuszk_amd import zksnark as z
        crs, G1, G2 = self.crs, o.G1, o.G2
        r1cs = crs.r1cs
        full, H, m, _ = g.r1cs_to_qap_witness(r1cs, primary, auxiliary)
        r = s = g.fr_random(seed)
        nv, ni = r1cs.num_variables, r1cs.num_inputs
        plan = z.shard_plan(nv, m, nv - ni, self.rank, self.world)

        def msm(C, key, scalars, bases):
            lo, hi = plan[key]
            return o.pippenger_msm(C, scalars[lo:hi], bases[lo:hi])

        a = msm(G1, "A", full + [1, r], crs.query_a + [crs.alpha_g1, crs.delta_g1])
        b1 = msm(G1, "B1", full + [1, s], [q[0] for q in crs.query_b] + [crs.beta_g1, crs.delta_g1])
        b2 = msm(G2, "B2", full + [1, s], [q[1] for q in crs.query_b] + [crs.beta_g2, crs.delta_g2])
        l_r = msm(G1, "L", list(auxiliary), crs.delta_abc_g1)
        h_r = msm(G1, "H", H, crs.query_h)
        share = o.pippenger_msm(G1, z.c_share_scalars(r, s, self.rank), [a, b1, crs.delta_g1])
        c = G1.add(G1.add(l_r, h_r), share)
        rec = o.g1_out_le(G1.to_affine(a)) + o.g2_out_le(G2.to_affine(b2)) + o.g1_out_le(G1.to_affine(c))
        return torch.frombuffer(bytearray(rec), dtype=torch.uint8)


def _host_gather(partial, group=None):
    out = [torch.empty(partial.numel(), dtype=torch.uint8) for _ in range(dist.get_world_size(group))]
    dist.all_gather(out, partial.contiguous(), group=group)
    return torch.cat(out)


def _host_combine(gathered, world):
    from octopuszk_amd import zksnark as z
    raw = bytes(gathered.numpy())
    assert len(raw) == world * z.RECORD_BYTES
    acc = [o.G1.zero, o.G2.zero, o.G1.zero]
    for k in range(world):
        rec = raw[768 * k:768 * (k + 1)]
        acc[0] = o.G1.add(acc[0], o.g1_from_out_le(rec[:192]))
        acc[1] = o.G2.add(acc[1], o.g2_from_out_le(rec[192:576]))
        acc[2] = o.G1.add(acc[2], o.g1_from_out_le(rec[576:]))
    return z.Proof(o.g1_out_le(o.G1.to_affine(acc[0])), o.g2_out_le(o.G2.to_affine(acc[1])),
                   o.g1_out_le(o.G1.to_affine(acc[2])))


def _worker(rank, world, port, crs, primary, auxiliary, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from octopuszk_amd import distributed as D
    # every rank but 0 passes another seed: distributed_prove must take rank 0's
    seed = g.SEED if rank == 0 else g.SEED + rank
    proof = D.distributed_prove(_OracleRank(crs, rank, world), primary, auxiliary, seed,
                                gather=_host_gather, combine=_host_combine)
    q.put((rank, (proof.g_a, proof.g_b, proof.g_c)))
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def oracle_case():
    r1cs, primary, auxiliary = g.serial_construct(NC, NI)
    crs = g.serial_setup(r1cs)
    (A, B, C), _ = g.serial_prove(crs, primary, auxiliary)
    want = (o.g1_out_le(o.G1.to_affine(A)), o.g2_out_le(o.G2.to_affine(B)), o.g1_out_le(o.G1.to_affine(C)))
    return crs, primary, auxiliary, want


def test_world_of_one_without_process_group(oracle_case):
    from octopuszk_amd import distributed as D
    crs, primary, auxiliary, want = oracle_case
    assert not dist.is_initialized()
    proof = D.distributed_prove(_OracleRank(crs, 0, 1), primary, auxiliary, g.SEED, combine=_host_combine)
    assert (proof.g_a, proof.g_b, proof.g_c) == want


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_world_gives_the_serial_proof(world, oracle_case):
    crs, primary, auxiliary, want = oracle_case
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, crs, primary, auxiliary, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        got = dict(q.get(timeout=300) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=60)
    assert all(p.exitcode == 0 for p in procs)
    for r in range(world):
        assert got[r] == want, r
