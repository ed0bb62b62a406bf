"""Running the three staged entries of the variable-base MSM (ozk_var_msm_sort_dev, _accum_dev, _tail_dev) one by one
over poisoned buffers, and reading back what each leaves; shared by test_msm_sort_stage_gpu.py and
test_msm_accum_stage_gpu.py.  The buffers are laid out by the library's own query (msm_stage_ref.stage_layout)."""
import ctypes
import time

import numpy as np

import msm_stage_ref as ref
from oracle import bn254 as o


def with_knobs(monkeypatch, env, body):
    """body() under the tuning knobs `env`, the defaults restored whatever happens"""
    from octopuszk_amd import lib
    L = lib.load()
    try:
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        L.ozk_tuning_reload()
        return body()
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)
        L.ozk_tuning_reload()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


class Stages:
    """The buffers of one MSM size under the knobs in force, and the stages over them."""

    def __init__(self, n_in, type_=1, prepared=0):
        import torch
        from octopuszk_amd import lib
        self.torch, self.lib, self.L = torch, lib, lib.load()
        self.n_in, self.type = n_in, type_
        self.lay = lay = ref.stage_layout(self.L, n_in, type_, prepared)
        new = lambda k: torch.empty(k, dtype=torch.uint8, device="cuda")
        self.sorted, self.sort_ws = new(lay["sorted_bytes"]), new(lay["sort_ws_bytes"])
        self.accum_ws, self.tail_buf = new(lay["accum_ws_bytes"]), new(lay["tail_bytes"])
        self.out = new(192 * type_)
        self.d_prepared = None

    def _stream(self):
        return ctypes.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def upload(self, arr):
        return self.torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint8).reshape(-1)).cuda()

    def prepare(self, d_bases):
        """the prepared records of the bases (ozk_var_msm_prepare_dev); the sort and the accumulation then read these"""
        k = int(self.L.ozk_var_msm_prepared_bytes(self.n_in, self.type))
        self.d_prepared = self.torch.empty(k, dtype=self.torch.uint8, device="cuda")
        self.lib.check(self.L.ozk_var_msm_prepare_dev(_p(d_bases), self.n_in, self.type, _p(self.d_prepared), k, self._stream()))
        self.torch.cuda.synchronize()
        return self.d_prepared

    def sort(self, d_bases, d_scalars, poison=True):
        """SORT over poisoned buffers -> the sorted set as host bytes"""
        if poison:
            self.sorted.fill_(ref.POISON)
            self.sort_ws.fill_(ref.POISON)
        lay = self.lay
        src = self.d_prepared if lay["prepared"] else d_bases
        self.lib.check(self.L.ozk_var_msm_sort_dev(_p(src), lay["prepared"], _p(d_scalars), self.n_in, self.type, _p(self.sorted),
                                                   lay["sorted_bytes"], _p(self.sort_ws), lay["sort_ws_bytes"], self._stream()))
        self.torch.cuda.synchronize()
        return self.sorted.cpu().numpy()

    def accum(self, part=0, poison=True):
        """ACCUMULATE over a poisoned scratch and tail buffer -> (tail buffer, sorted set after the stage, level-1 path)"""
        if poison:
            self.accum_ws.fill_(ref.POISON)
            self.tail_buf.fill_(ref.POISON)
        lay = self.lay
        prep = _p(self.d_prepared) if lay["prepared"] else None
        for pt in ((1, 2) if part == 12 else (part,)):
            self.lib.check(self.L.ozk_var_msm_accum_dev(prep, self.n_in, self.type, _p(self.sorted), lay["sorted_bytes"],
                                                        _p(self.accum_ws), lay["accum_ws_bytes"], _p(self.tail_buf),
                                                        lay["tail_bytes"], self._stream(), pt))
        self.torch.cuda.synchronize()
        path = self.L.ozk_var_msm_last_l1_path()
        return self.tail_buf.cpu().numpy(), self.sorted.cpu().numpy(), path

    def tail(self, mode=1):
        self.out.zero_()
        self.lib.check(self.L.ozk_var_msm_tail_dev(self.n_in, self.type, _p(self.tail_buf), self.lay["tail_bytes"], _p(self.out),
                                                   self._stream(), None, mode))
        self.torch.cuda.synchronize()
        return bytes(self.out.cpu().numpy())


# ---------------------------------------------------------------------------------------------------- bases
def g1_wire(points):
    return np.frombuffer(b"".join(o.g1_to_wire(P) for P in points), dtype=np.uint8).reshape(len(points), 96)


def g2_wire(points):
    return np.frombuffer(b"".join(o.g2_to_wire(P) for P in points), dtype=np.uint8).reshape(len(points), 192)


def tiled(points, n, type_=1):
    """n bases that repeat a few points: (the oracle points, base by base; their wire records)"""
    wire = (g1_wire if type_ == 1 else g2_wire)(points)
    idx = np.arange(n) % len(points)
    return [points[i] for i in idx], wire[idx].copy()


def g1_points(k, seed, edges=True):
    """k G1 points in Jacobian form with Z != 1; with `edges`: O, a Z that reduces to zero (Z = q), an affine point"""
    import random
    rng = random.Random(seed)
    pts = [o.G1.mul(o.G1.one, rng.randrange(1, 1 << 64)) for _ in range(k)]
    if edges:
        pts[1] = o.G1.zero
        pts[2] = (pts[2][0], pts[2][1], o.Q)
        pts[3] = o.G1.to_affine(pts[3])
    return pts


def g2_points(k, seed, edges=True):
    import random
    rng = random.Random(seed)
    pts = [o.G2.mul(o.G2.one, rng.randrange(1, 1 << 32)) for _ in range(k)]
    if edges:
        pts[1] = o.G2.zero
        pts[2] = (pts[2][0], pts[2][1], (o.Q, o.Q))
        pts[3] = o.G2.to_affine(pts[3])
    return pts


def g2_dlog_bases(n, seed):
    """n G2 bases k_i G2 (k_i < 2^64) from the fixed-base path, as test_msm_plans_gpu.py builds them: (wire rows, k_i)"""
    import torch
    from octopuszk_amd import lib
    L = lib.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ks = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    ks[:, 8:] = 0
    base = torch.from_numpy(np.frombuffer(o.g2_to_wire(o.G2.one), dtype=np.uint8).copy()).cuda()
    out_be = torch.empty(n * 384, dtype=torch.uint8, device="cuda")
    wsb = int(L.ozk_fixed_batch_msm_workspace_bytes(4, 16, n, 2))
    wsf = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    lib.check(L.ozk_fixed_batch_msm_dev(4, 16, n, _p(base), _p(torch.from_numpy(ks.reshape(-1)).cuda()), 2, _p(out_be),
                                        _p(wsf), wsb, st))
    torch.cuda.synchronize()
    be = out_be.cpu().numpy().reshape(n, 6, 64)
    assert not be[:, :, :32].any()
    wire = np.ascontiguousarray(be[:, :, ::-1][:, :, :32]).reshape(n, -1).copy()
    return wire, [int.from_bytes(k.tobytes(), "little") for k in ks]


class Timer:
    """prints what a case spent where (host model against device and read-back), for the record of the slowest cases"""

    def __init__(self, name):
        self.name, self.t0, self.parts = name, time.perf_counter(), []

    def lap(self, what):
        t = time.perf_counter()
        self.parts.append("%s %.2f s" % (what, t - self.t0))
        self.t0 = t

    def show(self):
        print("[stage-time] %s: %s" % (self.name, ", ".join(self.parts)))
