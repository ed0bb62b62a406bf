"""Times the PLONK prover and verifier on one GPU at n = 2^k gates.  One JSON line.

The circuit is generated: a few public inputs, then a chain of multiplications and additions in which the first input
feeds every third gate, padded to 2^k rows.  The string is built from a known tau, so the proof verifies.

(a) every stage of plonk.prove (witness upload, witness transforms, grand product, coset transforms, quotient kernel,
    commitments, multi-opening) and plonk.verify, by a host clock around work that ends in a synchronise: the median of
    --reps proofs after one warm-up;
(b) the whole prove by the same clock, beside the sum of the MSM and transform calls it makes (9 MSMs of n, 5
    transforms of n, 6 of 4 n), each timed alone in the same run;
(c) the grand-product and quotient entry points alone under device events, with the bytes per second of their counted
    traffic: 32 len (12 reads + 1 write) and 32 (4 n) (16 reads + 1 write).

With --lookups FRACTION a second circuit of the same n is proved in the same run, in which that
share of the rows are lookups into a table of --table-rows rows (x, y, x xor y):
(d) every stage of its proof, the two lookup stages among them, beside the vanilla proof's;
(e) the four entry points of csrc/plonk_lookup.cuh alone under device events with their counted traffic, the counts
    also against a 256-row table (the most contended one), and against numpy on the host (np.unique over the 96-byte
    records, and the upload of m).

With --r1cs LOG_NC [--inputs NI] the circuit is the import of the synthetic R1CS that
tools/groth16_prove.py proves, serial_construct(2^LOG_NC, NI): about NI + 3.5 2^LOG_NC rows, so --r1cs 18 is n = 2^20.
With --device-assignment the assignment of any circuit is a uint8 CUDA tensor, and the wire columns are built on the
device.  The stage table is the same one; in both cases the run also reports
(f) the compile time of the import, and ozk_fr_term_sums_dev and ozk_plonk_wires_dev alone under device events with
    their counted traffic: per term and pass 4 + 32 bytes read (+ 32 with coefficients) and 32 written once; per cell
    8 + 32 read (+ 32 where the cell is a difference) and 32 written.

With --zk every circuit of the run is also set up with zk=True over n + 8 bases of the same
string and proved with drawn blinders, after its proof without zk and in the same process:
(g) the stage table and the rounds of whole proofs under the zero-knowledge key ("zk" beside the figures without), and
    the zero-knowledge proof verified under the verifying key of the key without zk.

    python tools/plonk_prove.py [--log-n 16] [--reps 5] [--public 3] [--lookups 0.5 --table-rows 256] [--zk]
    python tools/plonk_prove.py --r1cs 18 [--inputs 1023] [--device-assignment] [--zk]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import kzg_bench as kb  # noqa: E402
from octopuszk_amd import kzg, lib as _lib, plonk, vectors, wire  # noqa: E402
from octopuszk_amd.device import VarMsmWorkspace, _ptr, _stream  # noqa: E402
from octopuszk_amd.fft import FR, root_of_unity  # noqa: E402
from octopuszk_amd.plonk import protocol  # noqa: E402
from octopuszk_amd.plonk.circuit import K  # noqa: E402


def chain_columns(n, n_public, end):
    """(selector columns, wire columns, assignment) of n rows: n_public inputs, then gates alternating addition and
    multiplication in the rows up to `end`; the rows from `end` on are empty"""
    values = [(0x9e3779b97f4a7c15f39cc0605cedc835 * (i + 1)) % FR for i in range(n_public)]
    sel, wires = [[0] * n for _ in range(5)], [[0] * n for _ in range(3)]
    for v in range(n_public):
        sel[0][v] = 1
        wires[0][v] = wires[1][v] = wires[2][v] = v
    prev = 0
    for row in range(n_public, end):
        other = 0 if row % 3 == 0 else prev
        new = len(values)
        if row % 2:
            values.append(values[prev] * values[other] % FR)
            sel[3][row], sel[2][row] = 1, FR - 1
        else:
            values.append((values[prev] + values[other]) % FR)
            sel[0][row], sel[1][row], sel[2][row] = 1, 1, FR - 1
        wires[0][row], wires[1][row], wires[2][row] = prev, other, new
        prev = new
    return sel, wires, values


def chain(n, n_public):
    """(circuit, assignment): n_public inputs, n - n_public - 1 gates, one padding row"""
    sel, wires, values = chain_columns(n, n_public, n - 1)
    return plonk.Circuit(n, sel, wires, n_public), values


def xor_table(rows):
    """rows (x, y, x xor y) over x, y < 2^k: the first `rows` of them"""
    side = 1
    while side * side < rows:
        side *= 2
    return [(i // side, i % side, (i // side) ^ (i % side)) for i in range(rows)]


def chain_with_lookups(n, n_public, share, table):
    """(circuit, assignment): the chain over the first rows, then round(n * share) lookup rows (at least one, and at
    least one gate of the chain stays); the lookups of one table row share three variables"""
    lookups = max(1, min(int(round(n * share)), n - n_public - 1))
    sel, wires, values = chain_columns(n, n_public, n - lookups)
    q_lookup, cells = [0] * (n - lookups) + [1] * lookups, {}
    for k in range(lookups):
        at = (k * 2654435761) % len(table)
        if at not in cells:
            cells[at] = len(values)
            values += list(table[at])
        for j in range(3):
            wires[j][n - lookups + k] = cells[at] + j
    return plonk.LookupCircuit(n, sel, wires, n_public, q_lookup, table), values


def prove_rounds(pk, vk, kvk, public, assignment, reps, stage_names):
    """(a): `reps` whole proofs by the host clock, then `reps` proofs stage by stage, each verified.  pk has proved
    once already (the warm-up)."""
    stages, whole, verify = {name: [] for name in stage_names}, [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        plonk.prove(pk, assignment)
        torch.cuda.synchronize()
        whole.append(time.perf_counter() - t0)
    for _ in range(reps):
        timings = {}
        proof = plonk.prove(pk, assignment, timings)
        for name in stages:
            stages[name].append(timings.get(name, 0.0))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert plonk.verify(vk, kvk, public, proof)
        torch.cuda.synchronize()
        verify.append(time.perf_counter() - t0)
    res = {"stages_ms": {name: _median_ms(v) for name, v in stages.items()}}
    res["stages_ms"]["verification"] = _median_ms(verify)
    res["prove_ms"] = _median_ms(whole)
    res["prove_rounds_ms"] = [x * 1e3 for x in whole]
    res["proof_bytes"] = len(proof.to_bytes())
    return res


def zk_rounds(circuit, zk_ck, pk, vk, kvk, public, assignment, reps, stage_names):
    """(g): the circuit under a key of setup(zk=True), proved as `pk`, the key without zk, was: a ProvingKey over the
    same rows when `pk` is one of a plain circuit (the host path of an imported R1CS)"""
    t0 = time.perf_counter()
    zk_pk, zk_vk = plonk.setup(circuit, zk_ck, zk=True)
    torch.cuda.synchronize()
    res = {"row_length": zk_ck.n, "setup_s": time.perf_counter() - t0}
    assert zk_vk.to_bytes() == vk.to_bytes()
    if type(pk) is plonk.ProvingKey and type(zk_pk) is not plonk.ProvingKey:
        zk_pk = plonk.ProvingKey(pk.circuit, zk_ck, zk_pk.coeffs, zk_pk.sigma, zk_pk.table, zk_vk)
        zk_pk.zk = True
    proof = plonk.prove(zk_pk, assignment)                               # the warm-up
    assert plonk.verify(vk, kvk, public, proof)
    assert proof.to_bytes() != plonk.prove(zk_pk, assignment).to_bytes()
    res.update(prove_rounds(zk_pk, vk, kvk, public, assignment, reps, stage_names))
    return res


def run_lookup(log_n, reps, n_public, share, table_rows, ck, kvk, zk_ck=None):
    n = 1 << log_n
    L = _lib.load()
    circuit, as_ints = chain_with_lookups(n, n_public, share, xor_table(table_rows))
    public = as_ints[:n_public]
    t0 = time.perf_counter()
    pk, vk = plonk.setup(circuit, ck)
    torch.cuda.synchronize()
    res = {"lookups": sum(circuit.q_lookup), "table_rows": table_rows, "setup_s": time.perf_counter() - t0,
           "proving_key_table_bytes": pk.table.numel(), "index_bytes": pk.index.numel()}
    assignment = wire.le32(as_ints)
    proof = plonk.prove(pk, assignment)
    assert plonk.verify(vk, kvk, public, proof)
    res.update(prove_rounds(pk, vk, kvk, public, assignment, reps, plonk.LOOKUP_STAGES))
    if zk_ck is not None:
        res["zk"] = zk_rounds(circuit, zk_ck, pk, vk, kvk, public, assignment, reps, plonk.LOOKUP_STAGES)

    # (e) the entry points alone
    host_wires = np.frombuffer(wire.le32(v for col in circuit.wire_values(as_ints) for v in col), dtype=np.uint8).reshape(3, n, 32)
    wires = wire.upload(host_wires.reshape(3, 32 * n))
    keep = [wire.le32([c + n]) for c in (0x2468ace, 0x13579bd, 0x1357, 0x1234567, 0x7654321)]
    keep += [wire.le32(K), wire.le32(protocol.zh_inverses(n))]
    eta, theta, alpha, beta, gamma, ks, zh = (ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in keep)
    tail = torch.empty(64, dtype=torch.uint8, device="cuda")

    def counts_of(wires, rows4, n_rows):
        index = vectors.plonk_lookup_index(rows4[1:], n_rows, n)
        m = torch.empty(32 * n, dtype=torch.uint8, device="cuda")

        def build():
            _lib.check(L.ozk_plonk_lookup_index_dev(_ptr(rows4[1:]), n_rows, n, _ptr(index), index.numel(), _stream()))

        def count():
            _lib.check(L.ozk_plonk_lookup_counts_dev(_ptr(wires), _ptr(rows4[0]), n, n, _ptr(rows4[1:]), n_rows, n,
                                                     _ptr(index), index.numel(), _ptr(m), n, _ptr(tail), _ptr(tail[4:]),
                                                     _stream()))

        return kb._event_ms(build, reps), kb._event_ms(count, reps), m

    index_ms, counts_ms, m = counts_of(wires, pk.lookup_rows, table_rows)
    looked = res["lookups"]
    res["index"] = {"ms": index_ms, "counted_bytes": 100 * table_rows}
    bytes_counts = 32 * n + 96 * looked + 100 * looked
    res["counts"] = {"ms": counts_ms, "counted_bytes": bytes_counts, "bytes_per_s": bytes_counts / (counts_ms * 1e-3)}
    if table_rows != 256:
        small, small_ints = chain_with_lookups(n, n_public, share, xor_table(256))
        rows4 = protocol._rows([small.q_lookup] + small.table_columns())
        res["counts_256_row_table_ms"] = counts_of(protocol._rows(small.wire_values(small_ints)), rows4, 256)[1]

    def host_count():
        records = np.ascontiguousarray(host_wires[:, n - looked:, :].transpose(1, 0, 2)).reshape(looked, 96)
        keys = np.ascontiguousarray(records).view(np.dtype((np.void, 96))).ravel()
        uniq, cnt = np.unique(keys, return_counts=True)
        table = np.frombuffer(wire.le32(v for row in circuit.table for v in row), dtype=np.uint8).reshape(-1, 96)
        order = {bytes(row): i for i, row in reversed(list(enumerate(table)))}
        out = np.zeros((n, 4), dtype=np.uint64)
        for key, c in zip(uniq, cnt):
            out[order[bytes(key)], 0] = c
        return wire.upload(out.view(np.uint8).reshape(-1))

    samples = []
    for _ in range(max(1, min(reps, 3))):
        t0 = time.perf_counter()
        host_m = host_count()
        torch.cuda.synchronize()
        samples.append(time.perf_counter() - t0)
    assert torch.equal(host_m, m)
    res["counts_host_numpy_ms"] = _median_ms(samples)

    s_out = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
    ws = torch.empty(max(int(L.ozk_plonk_lookup_sum_workspace_bytes(n)), 256), dtype=torch.uint8, device="cuda")

    def lookup_sum():
        _lib.check(L.ozk_plonk_lookup_sum_dev(_ptr(wires), n, _ptr(pk.lookup_rows), n, _ptr(m), n, eta, theta, _ptr(s_out),
                                              _ptr(tail), _ptr(tail[32:]), _ptr(ws), ws.numel(), _stream()))

    ms = kb._event_ms(lookup_sum, reps)
    res["lookup_sum"] = {"ms": ms, "counted_bytes": 32 * n * 17, "bytes_per_s": 32 * n * 17 / (ms * 1e-3),
                         "products_per_s": 23 * n / (ms * 1e-3)}
    rows = kb._random_rows(1, 4 * n, log_n)
    wit = torch.cat([rows[0].view(1, -1)] * 7)
    out = torch.empty(32 * 4 * n, dtype=torch.uint8, device="cuda")

    def quotient():
        _lib.check(L.ozk_plonk_quotient_lookup_dev(_ptr(wit), 4 * n, _ptr(pk.table), 4 * n, n, alpha, beta, gamma, ks, zh,
                                                   eta, theta, _ptr(out), _stream()))

    ms = kb._event_ms(quotient, reps)
    res["quotient_lookup"] = {"ms": ms, "counted_bytes": 32 * 4 * n * 24, "bytes_per_s": 32 * 4 * n * 24 / (ms * 1e-3),
                              "products_per_s": 38 * 4 * n / (ms * 1e-3)}
    return res


def _median_ms(samples):
    return statistics.median(samples) * 1e3


def witness_kernels(pk, d_assignment, reps):
    """(f): the two entry points of csrc/plonk_r1cs.cuh alone, over the key's own term stream and cells"""
    L = _lib.load()
    circuit, n = pk.circuit, pk.circuit.n
    res = {}
    given = d_assignment.numel() // 32
    src = torch.zeros(32 * circuit.n_vars, dtype=torch.uint8, device="cuda")
    src[:32 * given].copy_(d_assignment)
    bad = torch.zeros(8, dtype=torch.uint8, device="cuda")
    terms = circuit.n_vars - given
    if terms:
        ws = pk.workspace

        def sums():
            _lib.check(L.ozk_fr_term_sums_dev(_ptr(pk.term_index), None if pk.term_coeff is None else _ptr(pk.term_coeff),
                                              _ptr(src), given, terms, _ptr(src[32 * given:]), _ptr(bad[4:]), _ptr(ws),
                                              ws.numel(), _stream()))

        ms = kb._event_ms(sums, reps)
        per_pass = 4 + 32 + (0 if pk.term_coeff is None else 32)
        counted = terms * ((2 if terms > 1024 else 1) * per_pass + 32)
        res["term_sums"] = {"terms": terms, "ms": ms, "counted_bytes": counted, "bytes_per_s": counted / (ms * 1e-3)}
    if pk.cells is None:
        pk.cells = protocol._plain_cells(circuit)
    out = torch.empty((3, 32 * n), dtype=torch.uint8, device="cuda")

    def gather():
        _lib.check(L.ozk_plonk_wires_dev(_ptr(src), circuit.n_vars, _ptr(pk.cells), 3, n, n, _ptr(out), n, _ptr(bad),
                                         _stream()))

    ms = kb._event_ms(gather, reps)
    differences = int((circuit.wire_index() >= given).sum()) if terms else 0
    counted = 3 * n * (8 + 32 + 32) + 32 * differences
    res["wires"] = {"cells": 3 * n, "differences": differences, "ms": ms, "counted_bytes": counted,
                    "bytes_per_s": counted / (ms * 1e-3)}
    assert not bad.any().item()
    return res


def run(log_n, reps, n_public, share=0.0, table_rows=256, r1cs_log=None, device_assignment=False, zk=False):
    L = _lib.load()
    t0 = time.perf_counter()
    imported = {}
    if r1cs_log is None:
        n = 1 << log_n
        circuit, assignment = chain(n, n_public)
        public = assignment[:n_public]
    else:
        from octopuszk_amd import zksnark
        r1cs, public, auxiliary = zksnark.serial_construct(1 << r1cs_log, n_public)
        assignment = public + auxiliary
        t_compile = time.perf_counter()
        circuit = plonk.from_r1cs(r1cs)
        n = circuit.n
        log_n = n.bit_length() - 1
        imported = {"constraints": 1 << r1cs_log, "variables": circuit.num_variables, "chain_terms": len(circuit.term_index),
                    "rows": sum(1 for i in range(n) if any(col[i] for col in circuit.selectors)),
                    "compile_s": time.perf_counter() - t_compile}
    s = kb._String(n // 2 + (plonk.ZK_PAD // 2 if zk else 0))
    ck = kzg.CommitKey.from_srs(s, n)
    zk_ck = kzg.CommitKey.from_srs(s, n + plonk.ZK_PAD) if zk else None
    kvk = kzg.VerifyKey.from_srs(s)
    ck.bases()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    pk, vk = plonk.setup(circuit, ck)
    torch.cuda.synchronize()
    res = {"n": n, "n_public": n_public, "circuit_and_string_s": t1 - t0, "setup_s": time.perf_counter() - t1,
           "proving_key_table_bytes": pk.table.numel(), "device_assignment": device_assignment}
    if imported:
        res["r1cs"] = imported

    # (a), (b): whole proofs
    as_ints = assignment
    assignment = wire.le32(as_ints)                                      # the 32-byte records: no per-value host work
    d_assignment = wire.dev_bytes(assignment)
    pk_device = pk
    if device_assignment:
        assignment = d_assignment                                        # already in HBM: the wires are built there
    elif imported:
        t_extend = time.perf_counter()
        extended = circuit.extend(as_ints)
        res["r1cs"]["extend_host_s"] = time.perf_counter() - t_extend     # what prove(pk, ints or bytes) adds per proof
        assignment = wire.le32(extended)                                 # the host path with the chains summed once
        plain = plonk.Circuit(n, circuit.selectors, circuit.wires, circuit.n_public)   # the same gates, every variable given
        pk_host = plonk.ProvingKey(plain, ck, pk.coeffs, pk.sigma, pk.table, vk)
        assert plonk.prove(pk_host, assignment).to_bytes() == plonk.prove(pk, d_assignment).to_bytes()
        pk = pk_host
    proof = plonk.prove(pk, assignment)                                  # the warm-up
    assert proof.to_bytes() == plonk.prove(pk_device, as_ints).to_bytes()
    assert plonk.verify(vk, kvk, public, proof)
    res.update(prove_rounds(pk, vk, kvk, public, assignment, reps, plonk.protocol.STAGES))
    if zk:
        zk_ck.bases()
        res["zk"] = zk_rounds(circuit, zk_ck, pk, vk, kvk, public, assignment, reps, plonk.protocol.STAGES)

    # (b) the MSM and the transforms alone
    rows = kb._random_rows(1, 4 * n, log_n)
    msm = VarMsmWorkspace(n, 1)
    res["msm_n_ms"] = kb._event_ms(lambda: msm.run(ck.bases(), rows[0][:32 * n], prepared=True), reps)
    out = torch.empty(32 * 4 * n, dtype=torch.uint8, device="cuda")
    res["fft_n_ms"] = kb._median_ms(lambda: vectors.fr_fft(rows[0][:32 * n], n, root_of_unity(n), out[:32 * n]), reps)
    res["fft_4n_ms"] = kb._median_ms(lambda: vectors.fr_fft(rows[0], 4 * n, root_of_unity(4 * n), out), reps)
    res["msm_and_fft_calls_ms"] = 9 * res["msm_n_ms"] + 5 * res["fft_n_ms"] + 6 * res["fft_4n_ms"]

    # (f) the witness kernels alone
    if imported or device_assignment:
        res["witness_kernels"] = witness_kernels(pk_device, d_assignment, reps)

    # (c) the two kernels alone
    wires = protocol._rows(circuit.wire_values(circuit.extend(as_ints) if imported else as_ints))
    z = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
    tail = torch.empty(48, dtype=torch.uint8, device="cuda")
    ws = torch.empty(max(int(L.ozk_fr_perm_product_workspace_bytes(n)), 256), dtype=torch.uint8, device="cuda")
    le = lambda vs: wire.le32([int(v) % FR for v in vs])
    beta, gamma, alpha = 0x1234567 + n, 0x7654321 + n, 0x1357 + n
    args = [le([root_of_unity(n)]), le(K), le([beta]), le([gamma]), le([alpha]), le(protocol.zh_inverses(n))]
    vps = [ctypes.cast(ctypes.c_char_p(b), ctypes.c_void_p) for b in args]

    def product():
        _lib.check(L.ozk_fr_perm_product_dev(_ptr(wires), _ptr(pk.sigma), n, n, vps[0], vps[1], vps[2], vps[3], _ptr(z),
                                             _ptr(tail), _ptr(tail[32:]), _ptr(ws), ws.numel(), _stream()))

    ms = kb._event_ms(product, reps)
    res["perm_product"] = {"ms": ms, "counted_bytes": 32 * n * 13, "bytes_per_s": 32 * n * 13 / (ms * 1e-3)}
    wit = torch.cat([rows[0].view(1, -1)] * 5)

    def quotient():
        _lib.check(L.ozk_plonk_quotient_dev(_ptr(wit), 4 * n, _ptr(pk.table), 4 * n, n, vps[4], vps[2], vps[3], vps[1],
                                            vps[5], _ptr(out), _stream()))

    ms = kb._event_ms(quotient, reps)
    res["quotient"] = {"ms": ms, "counted_bytes": 32 * 4 * n * 17, "bytes_per_s": 32 * 4 * n * 17 / (ms * 1e-3)}
    if share > 0:
        del pk, pk_device, wit, wires
        res["lookup"] = run_lookup(log_n, reps, n_public, share, table_rows, ck, kvk, zk_ck)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--public", type=int, default=3)
    ap.add_argument("--lookups", type=float, default=0.0, help="the share of rows that are lookups (0: none)")
    ap.add_argument("--table-rows", type=int, default=256)
    ap.add_argument("--r1cs", type=int, default=None, metavar="LOG_NC",
                    help="prove the import of serial_construct(2^LOG_NC, --inputs) instead of the generated chain")
    ap.add_argument("--inputs", type=int, default=None, help="the R1CS's num_inputs (default: min(1023, 2^LOG_NC))")
    ap.add_argument("--device-assignment", action="store_true", help="hand prove the assignment as a CUDA tensor")
    ap.add_argument("--zk", action="store_true", help="also prove every circuit under a key of setup(zk=True)")
    a = ap.parse_args()
    if a.r1cs is not None:
        if not 1 <= a.r1cs <= 20 or a.lookups:
            ap.error("1 <= --r1cs <= 20, without --lookups")
        a.public = min(1023, 1 << a.r1cs) if a.inputs is None else a.inputs
        if not 1 <= a.public <= (1 << a.r1cs) + 1:
            ap.error("1 <= --inputs <= 2^LOG_NC + 1")
        a.log_n = 16
    if not 2 <= a.log_n <= 22 or not 1 <= a.public < (1 << a.log_n) - 1:
        ap.error("2 <= --log-n <= 22 and 1 <= --public < 2^log-n - 1")
    if not 0 <= a.lookups <= 1 or not 1 <= a.table_rows <= 1 << a.log_n:
        ap.error("0 <= --lookups <= 1 and 1 <= --table-rows <= 2^log-n")
    torch.cuda.set_device(0)
    out = {"bench": "plonk_prove", "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "result": run(a.log_n, a.reps, a.public, a.lookups, a.table_rows, a.r1cs, a.device_assignment, a.zk)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
