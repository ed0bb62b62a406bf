"""Level 1 of the G1 MSM by whole buckets on lane groups (msm_var.cuh k_bucket_items / k_l1_whole) against the chunked
level 1 + run merge it replaces (OZK_MSM_L1_WHOLE=0), both against the C oracle's bytes.

Shapes: the smallest that still take the two-level sort (more than 4096 pairs) with a window size forced so that the
mean bucket holds about 2, 16 or 64 entries and the TOP window's buckets — whose digits have fewer significant bits —
stay under their four-lane limit:  n = 2^14, c = 15 (mean 2);  n = 2^13, c = 11 (mean 16);  n = 2^14, c = 10 (mean 64).
The group-limit cases use scalars below 2^15 at c = 16: the GLV split of such a scalar is (k, 0) (glv.cuh: both
quotients are 0), so every entry lands in window 0, in the bucket of its own value, and all other windows — the top
one included — are empty.

Every case asserts which path ran (ozk_var_msm_last_l1_path): a case meant for the whole-bucket path that falls back
fails, and so does a skewed case that does not.

Bite check (scratch builds, not committed): recorded in DESIGN.md, "Level 1 by whole buckets".
"""
import numpy as np
import pytest

from oracle import bn254 as o

pytestmark = pytest.mark.gpu

WHOLE, CHUNKED = 1, 0
N_MAX = 1 << 14
SEED = 47
LIMIT = 2 * 255          # l1_whole.h: WHOLE_G * WHOLE_LANE_MAX


@pytest.fixture(scope="module")
def g1():
    """bases k_i G in wire form, on the device and as host bytes"""
    import torch
    from octopuszk_amd import device as dev
    d = dev.gen_g1_bases(N_MAX, SEED)
    torch.cuda.synchronize()
    return d, d.cpu().numpy().copy()


def _uniform(n, seed):
    rng = np.random.default_rng(seed)
    sc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sc[:, 31] &= 0x1F
    return sc


def _scalars(values):
    return np.frombuffer(b"".join(int(v % o.R).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(-1, 32).copy()


def _want(bases_np, sc, n):
    from oracle import coracle
    return coracle.pippenger_g1(bases_np[:n * 96].tobytes(), np.ascontiguousarray(sc).tobytes(), n)


def _run(bases_np, sc, n):
    import torch
    from octopuszk_amd import device as dev, lib
    ws = dev.VarMsmWorkspace(n, 1)
    out = ws.run(torch.from_numpy(bases_np[:n * 96].copy()).cuda(), torch.from_numpy(np.ascontiguousarray(sc).reshape(-1)).cuda())
    torch.cuda.synchronize()
    return bytes(out.cpu().numpy()), lib.load().ozk_var_msm_last_l1_path()


def _both_paths(monkeypatch, c, bases_np, sc, n, path):
    """the MSM with the whole-bucket path allowed (it must take `path`) and forbidden, each against the oracle"""
    from octopuszk_amd import lib
    L = lib.load()
    want = _want(bases_np, sc, n)
    try:
        if c:
            monkeypatch.setenv("OZK_MSM_C", str(c))
        for knob, expect in (("1", path), ("0", CHUNKED)):
            monkeypatch.setenv("OZK_MSM_L1_WHOLE", knob)
            L.ozk_tuning_reload()
            got, took = _run(bases_np, sc, n)
            print("OZK_MSM_L1_WHOLE=%s c=%s n=%d: path %d (expected %d), bytes %s" % (knob, c, n, took, expect, got == want))
            assert took == expect, (knob, took)
            assert got == want, knob
    finally:
        monkeypatch.delenv("OZK_MSM_C", raising=False)
        monkeypatch.delenv("OZK_MSM_L1_WHOLE", raising=False)
        L.ozk_tuning_reload()


@pytest.mark.parametrize("n,c", [(1 << 14, 15), (1 << 13, 11), (1 << 14, 10)], ids=["mean2", "mean16", "mean64"])
def test_random_scalars(n, c, g1, monkeypatch):
    """counts 0, 1 (an empty second lane), 2, 3 (odd split) ... ~100; four-lane groups in the top window"""
    _, bases = g1
    _both_paths(monkeypatch, c, bases, _uniform(n, 100 + c), n, WHOLE)


@pytest.mark.parametrize("extra,path", [(0, WHOLE), (1, CHUNKED)], ids=["limit", "limit_plus_1"])
def test_one_bucket_at_the_group_limit(extra, path, g1, monkeypatch):
    """one bucket of window 0 holds exactly 2 x 255 entries (whole buckets), or one more (the flag sends the MSM down
    the chunked path); the other entries sit two to a bucket; every other window is empty"""
    _, bases = g1
    n = 1 << 13
    long_run = LIMIT + extra
    vals = [5] * long_run + [100 + (i % ((n - long_run + 1) // 2)) for i in range(n - long_run)]
    _both_paths(monkeypatch, 16, bases, _scalars(vals), n, path)


@pytest.mark.parametrize("distinct", [1, 2])
def test_skewed_scalars_take_the_chunked_path(distinct, g1, monkeypatch):
    _, bases = g1
    n = 1 << 13
    cs = [0x1234567890abcdef1234567890abcdef1234567890abcdef1234567890abcd, 0x0fedcba987654321fedcba987654321fedcba987654321fedcba9876543210f]
    _both_paths(monkeypatch, 0, bases, _scalars([cs[i % distinct] for i in range(n)]), n, CHUNKED)


@pytest.mark.parametrize("arrangement", ["same_point", "plus_minus"])
def test_group_law_corners_inside_the_merge(arrangement, g1, monkeypatch):
    """every base the same point P, groups of four pairs sharing a scalar: the lanes of a bucket hold 2P and 2P (the
    doubling branch of the in-register xyzz_add); with bases P, -P alternating they hold O and O, or 2P and -2P"""
    _, bases = g1
    n = 1 << 13
    rec = bases[:96].copy()
    recs = np.tile(rec, (n, 1))
    if arrangement == "plus_minus":
        y = int.from_bytes(rec[32:64].tobytes(), "little")
        neg = rec.copy()
        neg[32:64] = np.frombuffer((o.Q - y).to_bytes(32, "little"), dtype=np.uint8)
        recs[1::2] = neg
    sc = np.repeat(_uniform(n // 4, 9), 4, axis=0)
    if arrangement == "plus_minus":
        assert _want(recs.reshape(-1), sc, n) == o.g1_out_le(o.G1.zero_affine)
    _both_paths(monkeypatch, 16, recs.reshape(-1), sc, n, WHOLE)


def test_infinity_bases_and_edge_scalars(g1, monkeypatch):
    """bases with wire Z = 0 mixed in; scalars 0, 1 and r - 1 among random ones"""
    _, bases = g1
    n = 1 << 13
    b = bases[:n * 96].copy().reshape(n, 96)
    b[::7, 64:96] = 0
    sc = _uniform(n, 12)
    edge = _scalars([0, 1, o.R - 1])
    for k in range(3):
        sc[k:k + 11 * 40:11] = edge[k]       # 40 of each: their buckets stay far below the group limit
    _both_paths(monkeypatch, 11, b.reshape(-1), sc, n, WHOLE)


def test_empty_top_window(g1, monkeypatch):
    """scalars below 2^87: the split of so short a scalar is (k, 0), and 87 bits are eight windows of 11 with the top bit
    clear, so no signed digit carries out of window 7 — windows 8 to 11 hold no entry at all: every item of those
    windows has count 0 and writes nothing"""
    _, bases = g1
    n = 1 << 13
    sc = _uniform(n, 13)
    sc[:, 11:] = 0
    sc[:, 10] &= 0x7F
    _both_paths(monkeypatch, 11, bases, sc, n, WHOLE)


def test_pipeline3_gives_the_same_bytes(g1, monkeypatch):
    """the staged entries (sort | accumulate | tail on their own streams) at one size"""
    import torch
    from octopuszk_amd import device as dev, lib
    d_bases, bases = g1
    L = lib.load()
    n = 1 << 13
    sc = _uniform(n, 14)
    want = _want(bases, sc, n)
    try:
        monkeypatch.setenv("OZK_MSM_C", "11")
        monkeypatch.setenv("OZK_MSM_L1_WHOLE", "1")
        L.ozk_tuning_reload()
        d_sc = torch.from_numpy(sc.reshape(-1)).cuda()
        pipe = dev.VarMsmPipeline3(n, 1)
        tickets = [pipe.submit(d_bases[:n * 96], d_sc) for _ in range(3)]
        outs = [bytes(pipe.result(t).cpu().numpy())[:192] for t in tickets]
        torch.cuda.synchronize()
        assert L.ozk_var_msm_last_l1_path() == WHOLE
        assert outs == [want] * 3
        pipe.close()
    finally:
        monkeypatch.delenv("OZK_MSM_C", raising=False)
        monkeypatch.delenv("OZK_MSM_L1_WHOLE", raising=False)
        L.ozk_tuning_reload()
