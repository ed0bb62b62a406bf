"""The length order of the whole-bucket level 1 and its dense-merge test (octopuszk_amd/csrc/l1_whole.h: whole_key,
whole_class_bases, whole_lane_map_len, whole_block_interleave, whole_block_dense), compiled for the host with the
address and undefined-behaviour sanitizers and compared with a Python model.

For every geometry and class table:
  * every non-padding lane maps to exactly one (item, g), and every item is covered by exactly G lanes g = 0 .. G-1
    that lie inside one aligned quad;
  * the class bases descend by key (base[k] = items with a key above k);
  * the keys along a region's lanes never rise, and 64 consecutive lanes of a region hold at most two NEIGHBOURING
    non-empty classes, plus whatever classes lie wholly inside the 64 lanes (a class of fewer than 64 / G items: the
    tiny geometries and the table with every class non-empty have such).  Where no class is that small this is the
    plain statement "the keys of a wave differ by at most one class";
  * the launch-order map is a bijection that spreads the late workgroups evenly among the early ones;
  * a workgroup the dense test accepts has 256 existing lanes, all pairs; under the length order it accepts exactly
    the workgroups that lie wholly in region 0.
The rank order's functions keep their own check (test_l1_items_cpu.py)."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "l1_order_hostcheck.cpp")
BIN = os.path.join(HERE, "native", "_l1_order_hostcheck")
HDR = os.path.join(HERE, "..", "octopuszk_amd", "csrc", "l1_whole.h")
KEYS, WAVE, TB = 128, 64, 256
NO_ITEM = 0xFFFFFFFF
TABLES = ["zero", "empty", "one_class", "clamp", "every_class"]


@pytest.fixture(scope="module")
def prog():
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in (SRC, HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", BIN, SRC])
    return BIN


def _region_items(W, NH, nb, g_top):
    if g_top == 2:
        return [W * NH * nb, 0]
    return [(W - 1) * NH * nb, NH * nb]


def _table(kind, items):
    """a class table of one region with `items` items"""
    T = np.zeros(KEYS, dtype=np.int64)
    if kind == "zero" or items == 0:
        return T                      # (no item counted yet: every base is 0)
    if kind == "empty":
        T[0] = items                  # every bucket empty
    elif kind == "one_class":
        T[37] = items
    elif kind == "clamp":
        T[KEYS - 1] = items
    else:                             # as many classes as there are items to give them, from the longest down
        k = min(items, KEYS)
        T[KEYS - k:] = items // k
        T[KEYS - k:KEYS - k + items % k] += 1
    assert T.sum() == items
    return T


def _run(prog, W, NH, nb, g_top, T):
    text = "%d %d %d %d\n%s\n" % (W, NH, nb, g_top, " ".join(str(int(v)) for v in np.concatenate(T)))
    out = subprocess.run([prog], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return {l[0]: np.array(l[2:].split(), dtype=np.int64) for l in out.stdout.splitlines()}


def _check(prog, W, NH, nb, g_top, kind):
    items = _region_items(W, NH, nb, g_top)
    G = [2, g_top]
    T = [_table(kind, n) for n in items]
    got = _run(prog, W, NH, nb, g_top, T)
    assert list(got["C"]) == [KEYS, WAVE, TB, 4 * KEYS]
    pad = lambda x: (x + WAVE - 1) // WAVE * WAVE
    lanes_r = [pad(G[r] * items[r]) for r in range(2)]
    assert list(got["R"]) == [2, items[0], lanes_r[0], g_top, items[1], lanes_r[1]]
    # class bases: items with a key above k, descending by key
    bases = got["B"].reshape(2, KEYS)
    for r in range(2):
        want = np.concatenate([np.cumsum(T[r][::-1])[::-1][1:], [0]])
        assert np.array_equal(bases[r], want)
        assert (np.diff(bases[r]) <= 0).all() and bases[r][KEYS - 1] == 0
    # lanes
    n_lanes = sum(lanes_r)
    blocks = (n_lanes + TB - 1) // TB
    nb0 = lanes_r[0] // TB
    assert list(got["N"]) == [nb0, blocks - nb0, n_lanes]
    L = got["L"].reshape(-1, 3)
    assert len(L) == n_lanes
    u = np.arange(n_lanes)
    region = (u >= lanes_r[0]).astype(np.int64)
    q = u - region * lanes_r[0]
    Gl = np.where(region == 1, g_top, 2)
    idx = q // Gl
    want_item = np.where(idx < np.where(region == 1, items[1], items[0]), idx + region * items[0], NO_ITEM)
    assert np.array_equal(L[:, 0], want_item) and np.array_equal(L[:, 1], q % Gl) and np.array_equal(L[:, 2], Gl)
    live = L[:, 0] != NO_ITEM
    # every non-padding lane maps to exactly one (item, g); every item has its G lanes, in order, inside one aligned quad
    pairs = L[live, 0] * 4 + L[live, 1]
    assert len(np.unique(pairs)) == len(pairs) == 2 * items[0] + g_top * items[1]
    first = np.nonzero(live & (L[:, 1] == 0))[0]
    assert np.array_equal(np.sort(L[first, 0]), np.arange(sum(items)))
    for k in range(4):
        sel = first[L[first, 2] > k]
        assert np.array_equal(L[sel + k, 0], L[sel, 0]) and (L[sel + k, 1] == k).all()
        assert ((sel + k) // 4 == sel // 4).all()
    # keys along the lanes of a region
    if kind != "zero":
        for r in range(2):
            if items[r] == 0:
                continue
            cls = np.nonzero(T[r])[0][::-1]                       # the non-empty classes, longest first
            sizes = T[r][cls]
            key_rank = np.repeat(np.arange(len(cls)), sizes)      # class rank of every item of the region, in item order
            lane_rank = np.repeat(key_rank, G[r])                 # ... of every live lane
            assert (np.diff(cls[lane_rank]) <= 0).all()           # the keys never rise
            small = np.concatenate([[0], np.cumsum(sizes * G[r] < WAVE)])     # small[i] = classes of rank < i that fit inside a wave
            lo = lane_rank
            hi = lane_rank[np.minimum(np.arange(len(lane_rank)) + WAVE - 1, len(lane_rank) - 1)]
            inside = np.where(hi > lo, small[hi] - small[np.minimum(lo + 1, hi)], 0)   # small classes strictly between
            assert (hi - lo <= 1 + inside).all()
            if not (sizes * G[r] < WAVE).any():
                assert (hi - lo <= 1).all()
                if kind == "every_class":
                    assert (cls[lo] - cls[hi] <= 1).all()         # neighbouring classes are neighbouring keys
    # launch order -> lane order
    V = got["V"]
    assert np.array_equal(np.sort(V), np.arange(blocks))
    late = V >= nb0
    seen = np.concatenate([[0], np.cumsum(late)])                  # late workgroups among the first p launched
    p = np.arange(blocks + 1)
    assert np.array_equal(seen, p * (blocks - nb0) // max(blocks, 1))
    assert (np.diff(V[late]) > 0).all() and (np.diff(V[~late]) > 0).all()     # each kind keeps its own order
    # dense workgroups
    D = got["D"]
    b0 = int(D[0])
    d0 = D[1:1 + 2 * b0].reshape(b0, 2)
    b1 = int(D[1 + 2 * b0])
    d1 = D[2 + 2 * b0:].reshape(b1, 2)
    assert b1 == blocks
    assert (d0[:, 0] <= d0[:, 1]).all() and (d1[:, 0] <= d1[:, 1]).all()     # accepted => 256 lanes, all pairs
    assert np.array_equal(d1[:, 0], (np.arange(blocks) < nb0).astype(np.int64))
    if g_top == 4:       # the rank order: every workgroup of pairs is accepted (with g_top = 2 the top section's are not)
        assert np.array_equal(d0[:, 0], d0[:, 1])
    return got


@pytest.mark.parametrize("kind", TABLES)
@pytest.mark.parametrize("g_top", [2, 4])
@pytest.mark.parametrize("nb", [1, 2, 128])
@pytest.mark.parametrize("NH", [1, 3, 256])
@pytest.mark.parametrize("W", [1, 2, 8])
def test_lane_map_and_class_bases(prog, W, NH, nb, g_top, kind):
    _check(prog, W, NH, nb, g_top, kind)


def test_the_workload_geometry(prog):
    """W = 8, NH = 256, nb = 128, four lanes in the top window: 2^18 buckets, 1792 + 512 workgroups"""
    got = _check(prog, 8, 256, 128, 4, "every_class")
    assert list(got["N"]) == [1792, 512, 2304 * 256]


def test_key(prog):
    got = _run(prog, 1, 1, 1, 2, [np.zeros(KEYS, dtype=np.int64)] * 2)
    K = got["K"].reshape(2, 1101)
    for row, G in zip(K, (2, 4)):
        c = np.arange(1101)
        assert np.array_equal(row, np.minimum((c + G - 1) // G, KEYS - 1))
        assert row[0] == 0 and row[1] == 1 and row[G * 127] == 127 and row[G * 255] == 127     # the lane limit shares the clamp class
