"""Device-resident entry points on torch CUDA(HIP) tensors: torch is plumbing only (HBM
buffers, streams, torch.distributed); all arithmetic is in libozk_hip.so."""
import ctypes
import os
import sys

import torch

from . import lib as _lib


def _ptr(t):
    return int(t.data_ptr())


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


def prepare_bases(d_bases, n, type_):
    """Affine Montgomery records of the `n` bases `d_bases` (wire format) for ozk_var_msm_prepared_dev and the
    staged entry points' prepared form (submit(..., prepared=True)): done once per proving key, skips the conversion kernel in every MSM.
    Asynchronous on the current stream."""
    L = _lib.load()
    nbytes = int(L.ozk_var_msm_prepared_bytes(n, type_))
    out = torch.empty(nbytes, dtype=torch.uint8, device=d_bases.device)
    _lib.check(L.ozk_var_msm_prepare_dev(_ptr(d_bases), n, type_, _ptr(out), nbytes, _stream()))
    return out


def _close_on_del(self):
    # never call into HIP while the interpreter (and possibly the HIP runtime) is being torn down
    # (`sys` is a module-level import: an import statement here fails during interpreter shutdown)
    if sys is None or sys.is_finalizing():
        return
    try:
        self.close()
    except Exception:
        pass


class VarMsmWorkspace:
    """Pre-allocated workspace + output for repeated device-resident MSMs of size n.

    The library receives raw device pointers, so — as with any stream-ordered foreign library —
    this object (its workspace) and the input tensors must stay alive until the stream the work
    was enqueued on has been synchronised; `run` keeps references to its last inputs to help."""

    def __init__(self, n, type_=1, device="cuda"):
        L = _lib.load()
        self.n, self.type = n, type_
        self.bytes = int(L.ozk_var_msm_workspace_bytes(n, type_))
        if self.bytes == 0:
            raise _lib.OzkError("workspace size query failed")
        self.ws = torch.empty(self.bytes, dtype=torch.uint8, device=device)
        self.out = torch.zeros(192 if type_ == 1 else 384, dtype=torch.uint8, device=device)

    def run(self, d_bases, d_scalars, prepared=False):
        """d_bases: uint8 [n*96|192] wire format (or the records of ozk_var_msm_prepare_dev with
        prepared=True), d_scalars: uint8 [n*32], in HBM.
        Asynchronous on the current stream; returns the output tensor (192|384 B)."""
        L = _lib.load()
        self._inputs = (d_bases, d_scalars)
        fn = L.ozk_var_msm_prepared_dev if prepared else L.ozk_var_msm_dev
        _lib.check(fn(_ptr(d_bases), _ptr(d_scalars), self.n, self.type, _ptr(self.out), _ptr(self.ws), self.bytes,
                      _stream()))
        return self.out


class SharedBaseMsm:
    """k MSMs over the SAME n G1 bases, out_i = sum_j s_ij P_j (ozk_multi_msm_*): the window table of the bases is
    built once, here, asynchronously on the current stream; `run` then only gathers and adds.

    As for VarMsmWorkspace, this object (table, workspace) and the inputs must stay alive until the stream has been
    synchronised; references to the bases and to the last scalars are kept.  The workspace grows when k grows: the
    old one is released to torch's stream-ordered allocator, so runs must stay on one stream (or be synchronised)."""

    def __init__(self, d_bases, n):
        L = _lib.load()
        self.n = int(n)
        self.table_bytes = int(L.ozk_multi_msm_table_bytes(self.n, 1))
        if self.table_bytes == 0:
            raise _lib.OzkError("shared-base MSM: n = %d rejected (1 <= n <= 4096)" % self.n)
        if d_bases.numel() * d_bases.element_size() < self.n * 96:
            raise ValueError("d_bases holds fewer than n wire-format G1 points")
        wb, oc = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(L.ozk_multi_msm_plan(self.n, ctypes.byref(wb), ctypes.byref(oc)))
        self.window_bits, self.windows = wb.value, oc.value
        self._bases = d_bases
        self.device = d_bases.device
        self.table = torch.empty(self.table_bytes, dtype=torch.uint8, device=self.device)
        self.k_cap, self.ws_bytes, self.ws = 0, 0, None
        self._grow(1)
        _lib.check(L.ozk_multi_msm_prepare_dev(_ptr(d_bases), self.n, 1, _ptr(self.table), self.table_bytes,
                                               _ptr(self.ws), self.ws_bytes, _stream()))

    def _grow(self, k):
        L = _lib.load()
        nbytes = int(L.ozk_multi_msm_workspace_bytes(self.n, k, 1))
        if nbytes == 0:
            raise _lib.OzkError("shared-base MSM: shape n = %d, k = %d rejected (k >= 1, k * n <= 2^28)" % (self.n, k))
        if nbytes > self.ws_bytes:
            self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self.ws_bytes = nbytes
        self.k_cap = max(self.k_cap, k)

    def run(self, d_scalars, k):
        """d_scalars: uint8 [k * n * 32], k rows of n little-endian scalars, in HBM.  Asynchronous on the current
        stream; returns a new uint8 tensor [k * 192] of wire-out points."""
        L = _lib.load()
        k = int(k)
        if k < 1 or d_scalars.numel() * d_scalars.element_size() < k * self.n * 32:
            raise ValueError("d_scalars holds fewer than k rows of n 32-byte scalars")
        # (the workspace size is not monotonic in k: the lanes-per-output split changes with it)
        self._grow(k)
        out = torch.empty(k * 192, dtype=torch.uint8, device=self.device)
        self._inputs = d_scalars
        _lib.check(L.ozk_multi_msm_dev(_ptr(self.table), _ptr(d_scalars), self.n, k, 1, _ptr(out), _ptr(self.ws),
                                       self.ws_bytes, _stream()))
        return out


class _MsmPipeline:
    """What the two schedules below share: the lengths a pipeline is sized for, its result slots (tail buffer, output
    and tail-done event per slot), the lone last MSM, and the lifetime of the object.

    `n` is one length or a sequence of lengths: submit(..., n=) then takes any of them, and every buffer holds the
    largest of its byte query over the lengths (the queries are not monotonic in n, so not the query at the largest).
    `tail_mode` is the shape of the window sums of the tails (include/ozk.h, ozk_var_msm_tail_dev): 0 latency,
    1 throughput.  `last_lone` chooses what submit(last=True) means: see the two submit methods."""

    def __init__(self, n, type_, depth, tail_mode, last_lone, device):
        L = _lib.load()
        self.sizes = [int(x) for x in n] if isinstance(n, (list, tuple)) else [n]
        self.n, self.type, self.depth = max(self.sizes), type_, depth
        self.tail_mode, self.last_lone, self.device = int(tail_mode), bool(last_lone), device
        self.tail_bytes = self._max_bytes(L.ozk_var_msm_tail_bytes)
        self.tails = [self._buf(self.tail_bytes) for _ in range(depth)]
        self.outs = [torch.zeros(192 if type_ == 1 else 384, dtype=torch.uint8, device=device) for _ in range(depth)]
        self._results = list(self.outs)     # where each slot's result goes: outs[slot], or the caller's `out`
        self.tail_done = [torch.cuda.Event() for _ in range(depth)]
        if self.last_lone:                  # a whole MSM's workspace, for submit(last=True)
            self.full_ws_bytes = self._max_bytes(L.ozk_var_msm_workspace_bytes)
            self.full_ws = self._buf(self.full_ws_bytes)
        self.count = 0
        self._inputs = None

    def _buf(self, nbytes):
        return torch.empty(nbytes, dtype=torch.uint8, device=self.device)

    def _max_bytes(self, query):
        return max(int(query(n, self.type)) for n in self.sizes)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    __del__ = _close_on_del

    def prepare(self, d_bases, n=None):
        return prepare_bases(d_bases, self.n if n is None else n, self.type)

    def _begin(self, d_bases, d_scalars, n, out):
        """slot, length and output tensor of the submission that starts"""
        n = self.n if n is None else int(n)
        if n not in self.sizes:
            raise ValueError(f"n={n}: the pipeline is sized for the lengths {self.sizes}")
        slot = self.count % self.depth
        if out is None:
            out = self.outs[slot]
        elif out.numel() * out.element_size() != self.outs[slot].numel() or not out.is_contiguous():
            raise ValueError(f"out must be {self.outs[slot].numel()} contiguous bytes")
        self._inputs = (d_bases, d_scalars)
        self._results[slot] = out
        return slot, n, out

    def _end(self, stream, slot):
        self.tail_done[slot].record(stream)
        self.count += 1
        return self.count - 1

    def _lone(self, stream, d_bases, d_scalars, prepared, n, out, slot):
        """submit(last=True) of a last_lone pipeline: nothing follows this MSM, so most of its bucket accumulation and
        all of its tail run with the chip to themselves — the single-call entry point then does better than the stages:
        its level-1 launch is a whole number of rounds of the chip and its tail has the latency shape (a
        2^20-constraint proof's H MSM: 2.49 + 0.22 + 1.1 ms -> see DESIGN.md section 8)."""
        L = _lib.load()
        msm = L.ozk_var_msm_prepared_dev if prepared else L.ozk_var_msm_dev
        _lib.check(msm(_ptr(d_bases), _ptr(d_scalars), n, self.type, _ptr(out), _ptr(self.full_ws), self.full_ws_bytes,
                       int(stream.cuda_stream)))
        return self._end(stream, slot)

    def done(self, ticket):
        """The event that fires when `ticket`'s result is complete (re-recorded by the slot's next submission): for
        callers that queue the wait on a stream of their own."""
        assert self.count - ticket <= self.depth, "result buffer already reused"
        return self.tail_done[ticket % self.depth]

    def result(self, ticket):
        """Output tensor of `ticket` (outs[slot], valid until `depth` more submissions, or the `out` it was submitted
        with); the current stream waits for its tail."""
        torch.cuda.current_stream().wait_event(self.done(ticket))
        return self._results[ticket % self.depth]


class VarMsmPipeline(_MsmPipeline):
    """Several device-resident MSMs in flight: heads (throughput-bound) run back to back on the
    caller's stream and share ONE workspace; each tail (latency-bound: upper window-sum levels,
    Horner, normalisation) runs on a side stream out of its own small tail buffer, overlapping the
    next head.  This is how a prover issues its six independent MSMs.

        pipe = VarMsmPipeline(n, depth=2)
        t = pipe.submit(d_bases, d_scalars)      # returns a ticket
        out = pipe.result(t)                     # makes the current stream wait for that tail
    """

    def __init__(self, n, type_=1, depth=2, device="cuda", tail_mode=0, last_lone=False):
        super().__init__(n, type_, depth, tail_mode, last_lone, device)
        L = _lib.load()
        self.ws_bytes = self._max_bytes(L.ozk_var_msm_head_workspace_bytes)
        self.ws = self._buf(self.ws_bytes)
        self.side = torch.cuda.Stream(device=device)
        self.head_done = [torch.cuda.Event() for _ in range(depth)]
        # ordering hint (include/ozk.h): the next head's bucket accumulation is dispatched after the
        # previous tail's multi-wave levels, so that its single-wave Horner kernel is resident first
        self.levels_done = []
        for _ in range(depth):
            ev = ctypes.c_void_p()
            _lib.check(L.ozk_order_event_create(ctypes.byref(ev)))
            self.levels_done.append(ev)

    def close(self):
        """Destroy the ordering events (after the work that uses them has drained)."""
        if self.levels_done:
            L = _lib.load()
            torch.cuda.synchronize()
            for ev in self.levels_done:
                L.ozk_order_event_destroy(ev)
            self.levels_done = []

    def submit(self, d_bases, d_scalars, prepared=False, last=False, n=None, out=None):
        """last=True: the caller knows that no MSM follows this one.  A last_lone pipeline then runs the whole MSM
        through the single-call entry point on the caller's stream (_lone); any other treats it like the rest."""
        L = _lib.load()
        slot, n, out = self._begin(d_bases, d_scalars, n, out)
        main = torch.cuda.current_stream()
        if self.count >= self.depth:
            main.wait_event(self.tail_done[slot])      # the tail that last used this slot's buffers
        if last and self.last_lone:
            return self._lone(main, d_bases, d_scalars, prepared, n, out, slot)
        prev = self.levels_done[(self.count - 1) % self.depth] if (self.count and self.depth > 1) else None
        _lib.check(L.ozk_var_msm_head_dev(_ptr(d_bases), int(prepared), _ptr(d_scalars), n, self.type, _ptr(self.ws),
                                          self.ws_bytes, _ptr(self.tails[slot]), self.tail_bytes,
                                          int(main.cuda_stream), prev))
        self.head_done[slot].record(main)
        self.side.wait_event(self.head_done[slot])
        _lib.check(L.ozk_var_msm_tail_dev(n, self.type, _ptr(self.tails[slot]), self.tail_bytes, _ptr(out),
                                          int(self.side.cuda_stream), self.levels_done[slot], self.tail_mode))
        return self._end(self.side, slot)


class VarMsmPipeline3(_MsmPipeline):
    """Three-stage schedule of consecutive device-resident MSMs: SORT of MSM k+1 (base conversion, digits, counting
    sort: HBM / LDS-bound) on the caller's stream | ACCUMULATE of MSM k (bucket accumulation, run merge: vector-ALU
    bound) on a second stream | TAIL of MSM k-1 (window sums, Horner, normalisation: latency-bound) on one or two more.
    The sort writes a double-buffered "sorted set"; each stage has private scratch (include/ozk.h,
    ozk_var_msm_sort_dev / _accum_dev / _tail_dev).  The sort kernels are sized to be resident beside three
    accumulation blocks per CU (csrc/msm_var.cuh, k_sort2), which is what lets the multiplier run back to back.
    Same interface as VarMsmPipeline (submit -> ticket, result(ticket))."""

    def __init__(self, n, type_=1, depth=3, tail_streams=2, device="cuda", split_accum=None, tail_cus=None,
                 tail_mode=1, last_lone=False):
        L = _lib.load()
        ts = max(1, tail_streams)
        # tail_cus = N > 0: the tail streams are confined to N compute units and the accumulate stream to the others
        # (ozk_stream_create_cu_range): the latency-bound tail waves no longer sit on the accumulation's SIMDs.  Such
        # streams are BLOCKING streams — they synchronise with the null stream — so submit() refuses to run on it.
        self.tail_cus = int(os.environ.get("OZK_P3_TAIL_CUS", "0")) if tail_cus is None else int(tail_cus)
        self._owned = []
        # split_accum: level 1 alone on the accumulate stream, the rest of the stage (run merge, generic levels) at the
        # head of the tail stream (ozk_var_msm_accum_dev, part 1 | 2); the accumulate scratch is then double-buffered too
        self.split = bool(int(os.environ.get("OZK_P3_SPLIT_ACCUM", "0"))) if split_accum is None else bool(split_accum)
        # a result slot is always served by the same tail stream (slot = k mod depth, stream = k mod ts), so whatever a
        # caller enqueues on stream_of(ticket) after result(ticket) is ordered before the slot's next tail
        super().__init__(n, type_, (max(2, depth) + ts - 1) // ts * ts, tail_mode, last_lone, device)
        self.sorted_bytes = self.sort_ws_bytes = self.accum_ws_bytes = 0
        for k in self.sizes:
            sb, swb, awb = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
            _lib.check(L.ozk_var_msm_stage_bytes(k, type_, ctypes.byref(sb), ctypes.byref(swb), ctypes.byref(awb)))
            self.sorted_bytes = max(self.sorted_bytes, sb.value)
            self.sort_ws_bytes = max(self.sort_ws_bytes, swb.value)
            self.accum_ws_bytes = max(self.accum_ws_bytes, awb.value)
        self.sorted = [self._buf(self.sorted_bytes) for _ in range(2)]
        self.sort_ws, self.accum_ws = self._buf(self.sort_ws_bytes), self._buf(self.accum_ws_bytes)
        self.accum_ws2 = [self.accum_ws, self._buf(self.accum_ws_bytes)] if self.split else None
        # never set in here: tools/sched_probe.py assigns a stream of its own for the second part of a split
        # accumulate stage (submit: `R`)
        self.rest_st = None
        if self.tail_cus > 0:
            total = int(L.ozk_device_cu_count())
            if not 0 < self.tail_cus < total:
                raise ValueError(f"tail_cus={self.tail_cus}: the device has {total} compute units")

            def confined(first, count):
                h = ctypes.c_void_p()
                _lib.check(L.ozk_stream_create_cu_range(first, count, ctypes.byref(h)))
                self._owned.append(h.value)
                return torch.cuda.ExternalStream(h.value)
            self.acc = confined(self.tail_cus, total - self.tail_cus)
            self.tail_st = [confined(0, self.tail_cus) for _ in range(ts)]
        else:
            self.acc = torch.cuda.Stream(device=device)
            self.tail_st = [torch.cuda.Stream(device=device) for _ in range(ts)]
        self.side = self.tail_st[0]
        ev = lambda k: [torch.cuda.Event() for _ in range(k)]
        self.sort_done, self.accum_done = ev(2), ev(2)
        self.l1_done = ev(2)

    def close(self):
        """Destroy the confined streams (after their work has drained); the pipeline cannot be used afterwards."""
        if self._owned:
            torch.cuda.synchronize()
            L = _lib.load()
            owned, self._owned = self._owned, []
            self.acc = self.tail_st = self.side = None     # no wrapper outlives the stream it wraps
            for h in owned:
                L.ozk_stream_destroy(h)

    def _check_stream(self, main):
        if self.tail_cus > 0 and int(main.cuda_stream) == 0:
            raise RuntimeError("VarMsmPipeline3(tail_cus > 0) on the null stream: the confined streams are blocking "
                               "streams and would serialise against it; submit under torch.cuda.stream(<a stream>)")

    def submit(self, d_bases, d_scalars, prepared=False, last=False, n=None, out=None):
        """last=True: the caller knows that no MSM follows this one (the end of a burst, a prover's final MSM).
        LATENCY TAIL (last_lone=False): it goes through the stages, and its tail, which runs with the chip to itself,
        takes the latency shape of the window sums (fused first level + wave levels: ~40 dependent additions shorter)
        whatever tail_mode says.  LONE (last_lone=True): the whole MSM runs through the single-call entry point on
        the accumulate stream, behind the accumulations already queued (_lone)."""
        L = _lib.load()
        k = self.count
        s = k % 2
        main = torch.cuda.current_stream()
        self._check_stream(main)
        slot, n, out = self._begin(d_bases, d_scalars, n, out)
        if last and self.last_lone:
            ready = torch.cuda.Event()
            ready.record(main)
            self.acc.wait_event(ready)
            if k >= self.depth:
                self.acc.wait_event(self.tail_done[slot])
            return self._lone(self.acc, d_bases, d_scalars, prepared, n, out, slot)
        if k >= 2:
            main.wait_event(self.accum_done[s])        # sorted set s (and, split, accumulate scratch s) is free again
        _lib.check(L.ozk_var_msm_sort_dev(_ptr(d_bases), int(prepared), _ptr(d_scalars), n, self.type,
                                          _ptr(self.sorted[s]), self.sorted_bytes, _ptr(self.sort_ws),
                                          self.sort_ws_bytes, int(main.cuda_stream)))
        self.sort_done[s].record(main)
        self.acc.wait_event(self.sort_done[s])
        if k >= self.depth:
            self.acc.wait_event(self.tail_done[slot])  # the tail that last used this slot's buffers
        T = self.tail_st[k % len(self.tail_st)]
        accum_ws = self.accum_ws2[s] if self.split else self.accum_ws
        # part 0: all of the stage, 1: level 1, 2: the rest
        accum = lambda stream, part: _lib.check(L.ozk_var_msm_accum_dev(
            _ptr(d_bases) if prepared else None, n, self.type, _ptr(self.sorted[s]), self.sorted_bytes, _ptr(accum_ws),
            self.accum_ws_bytes, _ptr(self.tails[slot]), self.tail_bytes, int(stream.cuda_stream), part))
        if self.split:
            # the accumulate stage in two parts: sorted set s and accumulate scratch s are free again once the REST of
            # MSM k has run, which is where accum_done[s] is recorded (the next accumulate on scratch s is ordered
            # after it through the sort's wait above)
            accum(self.acc, 1)
            self.l1_done[s].record(self.acc)
            R = self.rest_st or T     # (the rest on a stream of its own when the tail streams are confined to a few CUs)
            R.wait_event(self.l1_done[s])
            accum(R, 2)
            self.accum_done[s].record(R)
            if R is not T:
                T.wait_event(self.accum_done[s])
        else:
            accum(self.acc, 0)
            self.accum_done[s].record(self.acc)
            T.wait_event(self.accum_done[s])
        _lib.check(L.ozk_var_msm_tail_dev(n, self.type, _ptr(self.tails[slot]), self.tail_bytes, _ptr(out),
                                          int(T.cuda_stream), None, 0 if last else self.tail_mode))
        return self._end(T, slot)

    def stream_of(self, ticket):
        """the stream ticket's tail ran on: consumers of result(ticket) that must not stall the caller's (sort)
        stream enqueue there.  (A lone last MSM ran on the accumulate stream instead: take it through result().)"""
        return self.tail_st[ticket % len(self.tail_st)]


def gen_g1_bases(n, seed, device="cuda"):
    L = _lib.load()
    out = torch.empty(n * 96, dtype=torch.uint8, device=device)
    _lib.check(L.ozk_gen_bases_dev(seed, n, 1, _ptr(out), _stream()))
    return out


def points_sum(d_points, k, type_=1):
    L = _lib.load()
    out = torch.zeros(192 if type_ == 1 else 384, dtype=torch.uint8, device=d_points.device)
    _lib.check(L.ozk_points_sum_dev(_ptr(d_points), k, type_, _ptr(out), _stream()))
    return out


def groth16_combine(d_records, world):
    """The sharded Groth16 proof (zksnark.ShardedProver) from `world` gathered 768-byte partials A_r | B_r | C_r in
    one launch (ozk_groth16_combine_dev) -> zksnark.Proof of wire-out bytes.  Synchronises the current stream."""
    from .zksnark import Proof
    L = _lib.load()
    if d_records.numel() != world * 768:
        raise ValueError("%d bytes are not %d records of 768" % (d_records.numel(), world))
    d_records = d_records.contiguous()
    out = torch.zeros(768, dtype=torch.uint8, device=d_records.device)
    _lib.check(L.ozk_groth16_combine_dev(_ptr(d_records), world, _ptr(out), _stream()))
    raw = bytes(out.cpu().numpy())
    return Proof(raw[:192], raw[192:576], raw[576:])


SPLITMIX_MASK = (1 << 64) - 1


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & SPLITMIX_MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & SPLITMIX_MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & SPLITMIX_MASK
    return x ^ (x >> 31)


def gen_base_logs(n, seed):
    """the k_i of gen_g1_bases, for CPU-side checking"""
    out = []
    for i in range(n):
        k = splitmix64((seed + i) & SPLITMIX_MASK)
        out.append(k if k else 1)
    return out
