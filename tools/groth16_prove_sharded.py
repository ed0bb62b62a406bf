#!/usr/bin/env python3
"""Sharded Groth16 prove (zksnark.ShardedProver + distributed.distributed_prove) at BASELINE.json configs[4] scale:
W ranks, one process each, every rank proving over its 1/W of the key, one all-gather of the 768-byte partials,
one combine launch.  Prints one JSON line: per-rank stage times, the proof's SHA-256, how many devices ran.

    python tools/groth16_prove_sharded.py [--world W] [--logn 20] [--reps 5]

Each rank runs on its own device and exchanges over RCCL.  OZK_BENCH_REHEARSAL=1: all ranks share cuda:0 and
exchange over gloo (as bench.py --gpus N does) — a same-device rehearsal of the control path, whose times say
nothing about W GPUs.  With W = 1 the rank also runs SerialProver.prove on the same key, alternating with the
sharded prove, so that the two proof times come from one run (the difference is the combine launch)."""
import argparse
import hashlib
import json
import os
import socket
import statistics
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_main(rank, world, port, rehearsal, logn, reps, q):
    try:
        import torch
        import torch.distributed as dist
        from octopuszk_amd import distributed as D
        from octopuszk_amd import zksnark as z
        dev = 0 if rehearsal else rank
        torch.cuda.set_device(dev)
        gather = D.all_gather_partials
        if world > 1:
            os.environ["MASTER_ADDR"] = "127.0.0.1"
            os.environ["MASTER_PORT"] = str(port)
            if rehearsal:
                dist.init_process_group("gloo", rank=rank, world_size=world)
                gather = D.all_gather_partials_host
            else:
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev))
        nc, ni = 1 << logn, min(1023, 1 << logn)
        r1cs, primary, auxiliary = z.serial_construct(nc, ni)
        crs = z.serial_setup_generate(r1cs)
        full_bytes = z.assignment_bytes(primary + auxiliary)
        t0 = time.perf_counter()
        prover = z.ShardedProver(crs.proving_key, rank, world)
        t_prepare = time.perf_counter() - t0
        serial = z.SerialProver(crs.proving_key) if world == 1 else None
        rows, serial_rows, proof = [], [], None
        for k in range(reps + 1):   # the first of each is a warm-up
            if world > 1:
                dist.barrier()
            T = {}
            t0 = time.perf_counter()
            proof = D.distributed_prove(prover, primary, auxiliary, z.SEED, gather=gather, timing=T, full_bytes=full_bytes)
            T["prove_ms"] = (time.perf_counter() - t0) * 1e3
            if k:
                rows.append(T)
            if serial is not None:
                S = {}
                t0 = time.perf_counter()
                sp = serial.prove(primary, auxiliary, timing=S, full_bytes=full_bytes)
                S["prove_ms"] = (time.perf_counter() - t0) * 1e3
                assert (sp.g_a, sp.g_b, sp.g_c) == (proof.g_a, proof.g_b, proof.g_c), "sharded proof != SerialProver's"
                if k:
                    serial_rows.append(S)
        prover.close()
        if serial is not None:
            serial.close()
        best = min(rows, key=lambda r: r["prove_ms"])
        out = dict(rank=rank, device=torch.cuda.current_device(), device_name=torch.cuda.get_device_name(),
                   key_bytes=prover.key_bytes, prepare_key_s=round(t_prepare, 3),
                   stages_best_ms={k: round(v, 3) for k, v in best.items()},
                   prove_ms_all=[round(r["prove_ms"], 3) for r in rows],
                   proof_sha256=hashlib.sha256(proof.g_a + proof.g_b + proof.g_c).hexdigest())
        if serial_rows:
            out["serial_prove_ms_all"] = [round(r["prove_ms"], 3) for r in serial_rows]
            out["serial_gpu_ms_all"] = [round(r["gpu_ms"], 3) for r in serial_rows]
        q.put((rank, "ok", out))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:
        q.put((rank, "error", traceback.format_exc()))
        raise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--world", type=int, default=1)
    ap.add_argument("--logn", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    rehearsal = os.environ.get("OZK_BENCH_REHEARSAL", "0") == "1"
    import torch
    import torch.multiprocessing as mp
    if not rehearsal and args.world > torch.cuda.device_count():
        raise SystemExit("--world %d needs %d devices (%d visible); OZK_BENCH_REHEARSAL=1 runs the ranks on one device"
                         % (args.world, args.world, torch.cuda.device_count()))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_main, args=(r, args.world, port, rehearsal, args.logn, args.reps, q))
             for r in range(args.world)]
    for p in procs:
        p.start()
    ranks = {}
    try:
        for _ in range(args.world):
            rank, status, payload = q.get(timeout=900)
            if status != "ok":
                raise SystemExit("rank %d failed:\n%s" % (rank, payload))
            ranks[rank] = payload
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.exitcode is None:
                p.kill()
    shas = {r["proof_sha256"] for r in ranks.values()}
    assert len(shas) == 1, "ranks disagree on the proof"
    devices = len({r["device"] for r in ranks.values()})
    out = {"workload": "sharded Groth16 prove, synthetic R1CS 2^%d constraints, %d inputs, %d ranks"
                       % (args.logn, min(1023, 1 << args.logn), args.world),
           "world": args.world, "devices_used": devices, "rehearsal": rehearsal,
           "exchange": "none" if args.world == 1 else ("gloo (host)" if rehearsal else "RCCL"),
           "reps": args.reps, "proof_sha256": shas.pop(),
           "prove_ms_median_max_over_ranks": round(max(statistics.median(r["prove_ms_all"]) for r in ranks.values()), 3),
           "ranks": [ranks[r] for r in sorted(ranks)]}
    if args.world > 1 and devices < args.world:
        out["note"] = ("same-device rehearsal: %d ranks on %d device(s); unmeasured on multi-GPU hardware"
                       % (args.world, devices))
    if args.world == 1:
        r0 = ranks[0]
        out["serial_prove_ms_median"] = round(statistics.median(r0["serial_prove_ms_all"]), 3)
        out["sharded_prove_ms_median"] = round(statistics.median(r0["prove_ms_all"]), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
