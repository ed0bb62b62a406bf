"""Diagnostic: on the profiler-shaped 2^20 input (ONE base k G), run sort + accumulate + tail through the staged
entries and check what each stage hands on with the checkers of the tests (tests/msm_stage_ref.py): the sorted set
against the host model, every non-empty bucket record against [net count of the first half + lambda net count of the
second] k G, the final point against the oracle.  The buffers are laid out by the library's own query
(ozk_var_msm_stage_layout).

    DIAG_LOGN=20 DIAG_REPS=12 DIAG_FILLV=255 python tools/diag_buckets.py"""
import ctypes, os, sys, time
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
from octopuszk_amd import lib as ozk
from oracle import bn254 as o
import msm_stage_ref as ref
L = ozk.load()
def ptr(t): return ctypes.c_void_p(t.data_ptr())
n = 1 << int(os.environ.get("DIAG_LOGN", "20"))
K = 987654321
rng = np.random.default_rng(10)
lows = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
neg = rng.integers(0, 2, size=n).astype(bool)
vals = [(o.R - int(v)) if ng else int(v) for v, ng in zip(lows, neg)]
base = o.G1.to_affine(o.G1.mul(o.G1.one, K))
bases = np.frombuffer(o.g1_to_wire(base) * n, dtype=np.uint8).copy()
d_bases, d_scalars = torch.from_numpy(bases).cuda(), torch.from_numpy(ref.scalar_bytes(vals).reshape(-1)).cuda()
want = o.g1_out_le(o.G1.to_affine(o.G1.mul(base, sum(vals) % o.R)))
lay = ref.stage_layout(L, n, 1)
print("plan:", {k: lay[k] for k in ref.FIELDS[:13]}, flush=True)
model = ref.Model(lay, vals)
print("host model done", flush=True)
fillv = int(os.environ.get("DIAG_FILLV", "255"))
new = lambda k: torch.empty(lay[k], dtype=torch.uint8, device="cuda")
d_sorted, d_sortws, d_acc, d_tail = new("sorted_bytes"), new("sort_ws_bytes"), new("accum_ws_bytes"), new("tail_bytes")
d_out = torch.zeros(192, dtype=torch.uint8, device="cuda")
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
expected = None
for attempt in range(int(os.environ.get("DIAG_REPS", "12"))):
    for t in (d_sorted, d_sortws, d_acc, d_tail):
        t.fill_(fillv)
    ozk.check(L.ozk_var_msm_sort_dev(ptr(d_bases), 0, ptr(d_scalars), n, 1, ptr(d_sorted), lay["sorted_bytes"], ptr(d_sortws), lay["sort_ws_bytes"], st))
    torch.cuda.synchronize()
    sorted0 = d_sorted.cpu().numpy()
    ozk.check(L.ozk_var_msm_accum_dev(None, n, 1, ptr(d_sorted), lay["sorted_bytes"], ptr(d_acc), lay["accum_ws_bytes"], ptr(d_tail), lay["tail_bytes"], st, 0))
    torch.cuda.synchronize()
    path = L.ozk_var_msm_last_l1_path()
    sorted1, tail = d_sorted.cpu().numpy(), d_tail.cpu().numpy()
    ozk.check(L.ozk_var_msm_tail_dev(n, 1, ptr(d_tail), lay["tail_bytes"], ptr(d_out), st, None, 1))
    torch.cuda.synchronize()
    msgs = []
    try:
        ref.check_sorted_set(lay, sorted0, vals, model=model)
    except ref.StageError as e:
        msgs.append("sorted set: %s" % e)
    for name, k in (("hist", 4 * lay["NB"]), ("sent", 8 * model.total)):
        if not np.array_equal(sorted0[lay[name]:lay[name] + k], sorted1[lay[name]:lay[name] + k]):
            msgs.append("%s changed by the accumulate stage" % name)
    if not msgs:    # (the bucket checker reads the entries of the sorted set: only a valid one says what a bucket holds)
        t0 = time.time()
        try:
            expected = ref.check_buckets(lay, tail, sorted0, [K] * n, expected=expected)
        except ref.StageError as e:
            msgs.append("buckets: %s" % e)
        print("  buckets checked in %.0f s" % (time.time() - t0), flush=True)
    ok = bytes(d_out.cpu().numpy()) == want
    print("attempt", attempt, "level-1 path", path, "| result ok:", ok, "|", "; ".join(msgs) if msgs else "every stage OK", flush=True)
    if msgs or not ok:
        break
