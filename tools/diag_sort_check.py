"""Diagnostic: full validity check of the SORT stage on the profiler-shaped (skewed) 2^20 input against the host model
of the GLV split + recoding that the tests use (tests/msm_stage_ref.py): every (virtual point, window) with a non-zero
digit must appear exactly once, in the right bucket, with the right sign, every bucket's entries adjacent, hist right
for every bucket.  The buffers are laid out by the library's own query (ozk_var_msm_stage_layout).

    DIAG_LOGN=20 DIAG_REPS=12 python tools/diag_sort_check.py"""
import ctypes, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from octopuszk_amd import lib as ozk
from oracle import bn254 as o
import msm_stage_ref as ref
L = ozk.load()
def ptr(t): return ctypes.c_void_p(t.data_ptr())
n = 1 << int(os.environ.get("DIAG_LOGN", "20"))
rng = np.random.default_rng(10)
lows = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
neg = rng.integers(0, 2, size=n).astype(bool)
vals = [(o.R - int(v)) if ng else int(v) for v, ng in zip(lows, neg)]
base = o.G1.to_affine(o.G1.mul(o.G1.one, 987654321))
bases = np.frombuffer(o.g1_to_wire(base) * n, dtype=np.uint8).copy()
d_bases, d_scalars = torch.from_numpy(bases).cuda(), torch.from_numpy(ref.scalar_bytes(vals).reshape(-1)).cuda()
lay = ref.stage_layout(L, n, 1)
print("plan:", {k: lay[k] for k in ref.FIELDS[:13]}, flush=True)
model = ref.Model(lay, vals)
print("host model done; non-zero digits %d; coarse bins above big_thresh: %d" % (
    model.total, 0 if lay["small_sort"] else int((model.bin_sizes() > lay["big_thresh"]).sum())), flush=True)
d_sorted = torch.empty(lay["sorted_bytes"], dtype=torch.uint8, device="cuda")
d_sortws = torch.empty(lay["sort_ws_bytes"], dtype=torch.uint8, device="cuda")
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
fillv = int(os.environ.get("DIAG_FILLV", "255"))
for rep in range(int(os.environ.get("DIAG_REPS", "12"))):
    d_sorted.fill_(fillv); d_sortws.fill_(fillv)
    ozk.check(L.ozk_var_msm_sort_dev(ptr(d_bases), 0, ptr(d_scalars), n, 1, ptr(d_sorted), lay["sorted_bytes"], ptr(d_sortws), lay["sort_ws_bytes"], st))
    torch.cuda.synchronize()
    try:
        ref.check_sorted_set(lay, d_sorted.cpu().numpy(), vals, [base] * n, model=model)
        print("rep", rep, "OK", flush=True)
    except ref.StageError as e:
        print("rep", rep, "BROKEN:", e, flush=True)
