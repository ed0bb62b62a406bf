"""The THROUGHPUT window sums of G1 by bucket rows and columns (msm_var.cuh k_rc_partial / k_rc_reduce / k_rc_wave,
wsum_rc.h) against the serial levels they replace (OZK_MSM_TAIL_RC=0), both against the C oracle's bytes.  Every case
asserts which form ran (ozk_var_msm_last_tail_form), so a case that silently fell back to the serial levels fails.

Window sizes: c = 10 (cb = 9: 16 rows of 32, half as many rows as columns, so the row list is padded; two parts per
row, one per column), c = 11 (cb = 10: 32 x 32) and c = 16 (cb = 15: 128 rows of 256, the workload's shape), at 2^13
pairs.  OZK_MSM_TAIL_RC is opt-in (unset keeps the serial levels: the last test).
The shaped cases use small scalars: a scalar v <= 2^(c-1) splits as (v, 0) and has the one signed digit v, in window
0, bucket v - 1 (weight v), so a bucket, a row or a column can be filled at will.  Such buckets are far longer than
the whole-bucket level 1 takes, so these MSMs run the chunked level 1, whose higher levels leave JACOBIAN bucket
records: the tail converts them; the random cases leave XYZZ records.
"""
import numpy as np
import pytest

from oracle import bn254 as o

pytestmark = pytest.mark.gpu

N = 1 << 13
SEED = 59
CS = [10, 11, 16]


@pytest.fixture(scope="module")
def g1():
    import torch
    from octopuszk_amd import device as dev
    d = dev.gen_g1_bases(N, SEED)
    torch.cuda.synchronize()
    return d.cpu().numpy().copy().reshape(N, 96)


def _scalars(values):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in values), dtype=np.uint8).reshape(-1, 32).copy()


def _negated(rec):
    y = int.from_bytes(rec[32:64].tobytes(), "little")
    out = rec.copy()
    out[32:64] = np.frombuffer(((o.Q - y) % o.Q).to_bytes(32, "little"), dtype=np.uint8)
    return out


def _geom(c):
    cb = c - 1
    s = (cb + 1) // 2
    return cb, s, 1 << (cb - s), 1 << s


def _both_forms(monkeypatch, c, recs, sc):
    """the single-call MSM with the throughput tail forced, by rows and columns and by the serial levels"""
    import torch
    from oracle import coracle
    from octopuszk_amd import device as dev, lib
    L = lib.load()
    n = len(sc)
    want = coracle.pippenger_g1(recs.tobytes(), np.ascontiguousarray(sc).tobytes(), n)
    d_b, d_s = torch.from_numpy(recs.reshape(-1).copy()).cuda(), torch.from_numpy(np.ascontiguousarray(sc).reshape(-1)).cuda()
    try:
        monkeypatch.setenv("OZK_MSM_C", str(c))
        monkeypatch.setenv("OZK_MSM_TAIL_MODE", "1")
        for knob in ("1", "0"):
            monkeypatch.setenv("OZK_MSM_TAIL_RC", knob)
            L.ozk_tuning_reload()
            ws = dev.VarMsmWorkspace(n, 1)
            got = bytes(ws.run(d_b, d_s).cpu().numpy())
            torch.cuda.synchronize()
            form = L.ozk_var_msm_last_tail_form()
            print("OZK_MSM_TAIL_RC=%s c=%d n=%d: form %d, bytes %s" % (knob, c, n, form, got == want))
            assert form == int(knob)
            assert got == want, knob
    finally:
        for k in ("OZK_MSM_C", "OZK_MSM_TAIL_MODE", "OZK_MSM_TAIL_RC"):
            monkeypatch.delenv(k, raising=False)
        L.ozk_tuning_reload()
    return want


@pytest.mark.parametrize("c", CS)
def test_random_scalars(c, g1, monkeypatch):
    rng = np.random.default_rng(300 + c)
    sc = rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
    sc[:, 31] &= 0x1F
    _both_forms(monkeypatch, c, g1, sc)


@pytest.mark.parametrize("c", CS)
def test_all_scalars_equal(c, g1, monkeypatch):
    """one bucket per window: every other row and column is empty"""
    k = 0x0b5f1c7d2e3a49586776859403a2b1c0d9e8f7061524334251607f8e9dacbbca % o.R
    _both_forms(monkeypatch, c, g1, _scalars([k] * N))


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("which", ["first", "last"])
def test_one_extreme_bucket(which, c, g1, monkeypatch):
    """only bucket 0 (weight 1: row 0, column 0), or only bucket 2^cb - 1 (the largest weight: last row, last column)"""
    v = 1 if which == "first" else 1 << (c - 1)
    _both_forms(monkeypatch, c, g1, _scalars([v] * N))


def _two_buckets(c, line, gap, g1, signs):
    """N / 2 copies of +-P in each of two buckets of one row (line = "row") or of one column, `gap` places apart"""
    cb, s, rows, cols = _geom(c)
    if line == "row":
        r, q = rows - 1, 1
        b1, b2 = (r << s) + q, (r << s) + q + gap
        assert q + gap < cols
    else:
        r, q = 1, cols - 2
        b1, b2 = (r << s) + q, ((r + gap) << s) + q
        assert r + gap < rows
    p = g1[0]
    recs = np.stack([p if signs[i % 2] > 0 else _negated(p) for i in range(N)])
    return recs, _scalars([(b1, b2)[i % 2] + 1 for i in range(N)])


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("gap", [1, 17], ids=["same_part", "two_parts"])
@pytest.mark.parametrize("line", ["row", "column"])
def test_equal_points_double_inside_a_plain_sum(line, gap, c, g1, monkeypatch):
    """two buckets of one row (column) hold the same point: the doubling branch of xyzz_add, inside one partial sum
    (gap 1) or where the partial sums meet (gap 17, where the row or column is long enough to have two parts)"""
    cb, s, rows, cols = _geom(c)
    if gap >= (cols if line == "row" else rows) - 2:
        gap = 3   # c = 10: a column has 16 buckets, one part; three places apart
    recs, sc = _two_buckets(c, line, gap, g1, (1, 1))
    _both_forms(monkeypatch, c, recs, sc)


@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("line", ["row", "column"])
def test_opposite_points_cancel_in_one_line_only(line, c, g1, monkeypatch):
    """two buckets of one row hold P and -P: that row sum is infinity while their two column sums are not (and the
    same with rows and columns exchanged); the weights differ, so the MSM is not infinity"""
    recs, sc = _two_buckets(c, line, 2, g1, (1, -1))
    want = _both_forms(monkeypatch, c, recs, sc)
    assert want != o.g1_out_le(o.G1.zero_affine)


@pytest.mark.parametrize("knob,form", [("1", 1), (None, 0)], ids=["rows_columns", "unset"])
def test_pipeline3_at_the_workload_window(knob, form, g1, monkeypatch):
    """the staged entries (throughput tail) at c = 16: rows and columns when asked for; unset keeps the serial levels
    (the form measured 5 % slower in the three-stage schedule, profiles/r09_ab_tail_rowcol.txt)"""
    import torch
    from oracle import coracle
    from octopuszk_amd import device as dev, lib
    L = lib.load()
    rng = np.random.default_rng(77)
    sc = rng.integers(0, 256, size=(N, 32), dtype=np.uint8)
    sc[:, 31] &= 0x1F
    want = coracle.pippenger_g1(g1.tobytes(), sc.tobytes(), N)
    try:
        monkeypatch.setenv("OZK_MSM_C", "16")
        if knob is not None:
            monkeypatch.setenv("OZK_MSM_TAIL_RC", knob)
        L.ozk_tuning_reload()
        pipe = dev.VarMsmPipeline3(N, 1)
        d_b, d_s = torch.from_numpy(g1.reshape(-1).copy()).cuda(), torch.from_numpy(sc.reshape(-1)).cuda()
        tickets = [pipe.submit(d_b, d_s) for _ in range(3)]
        outs = [bytes(pipe.result(t).cpu().numpy())[:192] for t in tickets]
        torch.cuda.synchronize()
        assert L.ozk_var_msm_last_tail_form() == form
        assert outs == [want] * 3
        pipe.close()
    finally:
        monkeypatch.delenv("OZK_MSM_C", raising=False)
        monkeypatch.delenv("OZK_MSM_TAIL_RC", raising=False)
        L.ozk_tuning_reload()
