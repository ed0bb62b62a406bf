"""The item order of the whole-bucket level 1 (octopuszk_amd/csrc/l1_whole.h), compiled for the host and compared with
a Python model: the items are a permutation of the buckets, rank-ordered inside a bin by descending count with ties
by index, laid out rank-major (rank * nbins + bin); every item is served by G adjacent lanes (2, g_top in the top
window); the lanes' parts of a bucket are contiguous, nearly equal and cover it."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "l1_items_hostcheck.cpp")
BIN = os.path.join(HERE, "native", "_l1_items_hostcheck")
HDR = os.path.join(HERE, "..", "octopuszk_amd", "csrc", "l1_whole.h")


@pytest.fixture(scope="module")
def prog():
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in (SRC, HDR)):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-o", BIN, SRC])
    return BIN


def _run(prog, W, NH, nb, g_top, counts):
    text = "%d %d %d %d\n" % (W, NH, nb, g_top) + "\n".join(" ".join(str(int(c)) for c in row) for row in counts) + "\n"
    out = subprocess.run([prog], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [l.split() for l in out.stdout.splitlines()]
    return {k: [[int(x) for x in r[1:]] for r in rows if r[0] == k] for k in "ILPG"}


# (W, NH, nb, g_top): the workload's geometry in miniature, one bin per window, tiny bins, a two-lane top window
GEOMETRIES = [(8, 4, 128, 4), (3, 1, 128, 4), (2, 3, 8, 2), (4, 2, 1, 4), (1, 2, 16, 4), (5, 1, 2, 2), (2, 1, 4, 4)]


@pytest.mark.parametrize("W,NH,nb,g_top", GEOMETRIES)
def test_items_and_lanes_against_the_model(prog, W, NH, nb, g_top):
    rng = np.random.default_rng(1000 * W + 10 * NH + nb)
    nbins = W * NH
    # Poisson counts around 4 (many ties, zeros), around 64 (the workload), and a few constant bins (all ties)
    counts = [rng.poisson([4, 64][b % 2], size=nb) if b % 5 else np.full(nb, b % 3) for b in range(nbins)]
    got = _run(prog, W, NH, nb, g_top, counts)
    seen = set()
    for bin_, row in enumerate(got["I"]):
        assert row[0] == bin_
        idx = row[1:]
        # the model: stable sort by descending count = descending count, ties by index
        order = sorted(range(nb), key=lambda i: (-int(counts[bin_][i]), i))
        want = [0] * nb
        for rank, i in enumerate(order):
            want[i] = rank * nbins + bin_
        assert idx == want
        ranks = [(x - bin_) // nbins for x in idx]
        assert all((x - bin_) % nbins == 0 for x in idx) and sorted(ranks) == list(range(nb))
        by_rank = sorted(range(nb), key=lambda i: ranks[i])
        for a, b in zip(by_rank, by_rank[1:]):
            assert counts[bin_][a] > counts[bin_][b] or (counts[bin_][a] == counts[bin_][b] and a < b)
        seen.update(idx)
    assert seen == set(range(nb * nbins))          # a permutation of the buckets
    groups = {bin_: G for bin_, G, _ in got["G"]}
    assert all(lim == 255 * G for _, G, lim in got["G"])
    assert all(groups[b] == (g_top if b // NH == W - 1 else 2) for b in range(nbins))
    # lanes: numbered densely, each item served by its bin's G adjacent lanes g = 0 .. G-1, groups aligned to G
    # (each rank's ordinary and top sections are padded to whole quads with lanes that have no item: a group never
    # straddles an aligned quad, which is what the kernel's quad permutes need)
    lanes = got["L"]
    pad4 = lambda x: (x + 3) // 4 * 4
    assert [l[0] for l in lanes] == list(range(nb * (pad4(2 * NH * (W - 1)) + pad4(g_top * NH))))
    t = 0
    served = []
    NO_ITEM = 0xffffffff
    while t < len(lanes):
        _, item, g, G = lanes[t]
        assert g == 0 and t % G == 0 and t // 4 == (t + G - 1) // 4
        assert [l[1:] for l in lanes[t:t + G]] == [[item, k, G] for k in range(G)]
        if item != NO_ITEM:
            assert G == groups[item % nbins]
            served.append(item)
        t += G
    assert sorted(served) == list(range(nb * nbins))
    assert [s // nbins for s in served] == sorted(s // nbins for s in served)   # rank-major: the grid runs longest-first


def test_parts_cover_the_bucket(prog):
    got = _run(prog, 1, 1, 1, 1, [[0]])
    parts = {}
    for count, g, G, first, ln in got["P"]:
        parts.setdefault((count, G), []).append((g, first, ln))
    assert len(parts) == 3 * 601
    for (count, G), ps in parts.items():
        ps.sort()
        assert [p[0] for p in ps] == list(range(G)) and ps[0][1] == 0
        assert all(a[1] + a[2] == b[1] for a, b in zip(ps, ps[1:])) and ps[-1][1] + ps[-1][2] == count
        lens = [p[2] for p in ps]
        assert max(lens) - min(lens) <= 1 and lens[0] == max(lens)
        assert max(lens) <= 255 or count > 255 * G
