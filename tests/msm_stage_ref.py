"""The variable-base MSM stage by stage: an exact host model of what SORT hands to ACCUMULATE (the sorted set) and of
what ACCUMULATE hands to the tail (the bucket records), and the checkers of both contracts.

Where everything lies comes from the library's own layout query (ozk_var_msm_stage_layout, include/ozk.h): nothing here
repeats the workspace arithmetic.  The recoding is restated from the definitions in csrc/msm_var.cuh (scalar_digit,
signed_digit_codes, digit_decode, k_digits, k_digits_glv); the GLV split is the model of tests/multi_msm_ref.py.

The sorted set (as the producers k_sort_small, k_sort2, k_sortbig_scan / _scatter write it and the consumers
k_segreduce, k_bin_sums, k_bucket_items read it):
    total[0]   the number of non-zero digits
    sent[j]    j < total[0]: (virtual point | sign << 31, bucket id), bucket id = window << cb | bucket; every non-zero
               digit exactly once; the entries of a bucket adjacent, in any order
    hist[b]    the number of entries of bucket b, for EVERY b < W << cb (no memset precedes the sort)
    two-level sort: buckets ascending, so bucket b's run starts at the exclusive prefix sum of hist (k_bucket_items
               computes the runs from hist alone); one-launch sort: a window's piece is contiguous and bucket-ascending,
               the pieces in any order (k_segreduce only compares neighbouring bucket ids)
    aff[i]     canonical Montgomery (x, y) of base i, aff[n_in + i] = (beta x, y); O is (0, 0); unsigned GLV plans
               negate y by the half scalar's sign; untouched over prepared bases
The bucket records: hist_t == hist; for every bucket with hist[b] > 0 a record tagged XYZZ or Jacobian (raw 29-bit
limbs, Montgomery radix 2^261) that is the bucket's sum as a group element; records of empty buckets are never read."""
import ctypes

import numpy as np

from multi_msm_ref import LAM, glv_split
from oracle import bn254 as o

FIELDS = ("n", "glv", "sd", "c", "cb", "W", "small_sort", "L1", "l1_whole", "lo_bits", "NH", "nblk", "big_thresh",
          "aff", "hist", "total", "sent", "buckets", "hist_t", "AFF_WORDS", "REC_WORDS", "REC_TAG")
TAG_XYZZ, TAG_JAC = 0, 1
POISON = 0xFF
RBITS = 261
RINV = pow(1 << RBITS, -1, o.Q)
MONT = pow(2, RBITS, o.Q)
BETA_G1 = 2203960485148121921418603742825762020974279258880205651966    # (beta x, y) = [LAM] (x, y) on G1
BETA_G2 = BETA_G1 * BETA_G1 % o.Q                                       # and on the twist (glv.cuh)
S2_TILE = 8704          # msm_var.cuh: entries per register tile of k_sort2
SORTBIG_CHUNK = 1 << 13
SORT2_CASES = {S2_TILE: 0, S2_TILE + 1: 0, 2 * S2_TILE + 1: 2048}   # bin size at 2^14 pairs -> pairs with both halves in the bin
SORTS_MAX_N = 8192


class StageError(AssertionError):
    """a broken clause of a stage contract; `clause` names it"""

    def __init__(self, clause, detail=""):
        super().__init__("%s: %s" % (clause, detail) if detail else clause)
        self.clause = clause


def _need(ok, clause, detail=""):
    if not ok:
        raise StageError(clause, detail() if callable(detail) else detail)


# ---------------------------------------------------------------------------------------------------- the layout
def stage_layout(L, n_in, type_, prepared=0):
    """ozk_var_msm_stage_layout as a dict, with the sizes of the buffers (ozk_var_msm_stage_bytes, _tail_bytes)"""
    out = (ctypes.c_int64 * len(FIELDS))()
    rc = L.ozk_var_msm_stage_layout(n_in, type_, prepared, out, len(FIELDS))
    assert rc == 0, L.ozk_last_error()
    lay = dict(zip(FIELDS, (int(v) for v in out)))
    sizes = [ctypes.c_size_t() for _ in range(3)]
    assert L.ozk_var_msm_stage_bytes(n_in, type_, *[ctypes.byref(s) for s in sizes]) == 0
    lay.update(n_in=n_in, type=type_, prepared=int(bool(prepared)), NB=lay["W"] << lay["cb"],
               sorted_bytes=sizes[0].value, sort_ws_bytes=sizes[1].value, accum_ws_bytes=sizes[2].value,
               tail_bytes=int(L.ozk_var_msm_tail_bytes(n_in, type_)))
    if prepared:   # where the sort would have put the records, to see that it left them alone
        lay["aff_area"] = stage_layout(L, n_in, type_, 0)["aff"]
    else:
        lay["aff_area"] = lay["aff"]
    return lay


def plan_layout(n_in, c, glv=1, signed=1, small_sort=None, type_=1):
    """A layout dict for the model alone (no library): the plan fields as make_plan derives them from c and the modes."""
    sd = int(bool(glv and signed and c >= 2))
    cb = c - sd
    n = 2 * n_in if glv else n_in
    W = ((128 if glv else 256) + c - 1) // c
    lo_bits = min(cb, 7 if sd else 8)
    if small_sort is None:
        small_sort = int(n <= SORTS_MAX_N and cb <= 10)
    return dict(n=n, n_in=n_in, glv=int(glv), sd=sd, c=c, cb=cb, W=W, NB=W << cb, small_sort=int(small_sort),
                lo_bits=lo_bits, NH=1 << (cb - lo_bits), type=type_, prepared=0)


# ---------------------------------------------------------------------------------------------------- the model
def scalar_ints(sc):
    """(n, 32) uint8 rows, 32 n bytes, or a list of integers -> list of integers"""
    if isinstance(sc, (bytes, bytearray)):
        sc = np.frombuffer(bytes(sc), dtype=np.uint8).reshape(-1, 32)
    if isinstance(sc, np.ndarray):
        raw = np.ascontiguousarray(sc, dtype=np.uint8).reshape(-1, 32).tobytes()
        return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(raw) // 32)]
    return [int(s) for s in sc]


def scalar_bytes(ints):
    return np.frombuffer(b"".join(int(s).to_bytes(32, "little") for s in ints), dtype=np.uint8).reshape(-1, 32).copy()


def half_scalars(scalars, glv):
    """The signed integers whose digits the sort sees, one per virtual point: k1 of every pair, then k2 of every pair
    (virtual point n_in + i), with k1 + LAM k2 = s mod r; without GLV the 256-bit values as they are."""
    s = scalar_ints(scalars)
    if not glv:
        return s
    # a value below 2^63 splits into (s, 0): both quotient estimates of the split are zero
    pairs = [(v, 0) if v < (1 << 63) else glv_split(v) for v in s]
    return [p[0] for p in pairs] + [p[1] for p in pairs]


def _words(mags, nbytes):
    raw = b"".join(m.to_bytes(nbytes, "little") for m in mags)
    w = np.frombuffer(raw, dtype="<u4").reshape(len(mags), nbytes // 4).astype(np.uint64)
    return np.concatenate([w, np.zeros((len(mags), 1), dtype=np.uint64)], axis=1)   # one guard word


def _raw_digits(words, w, c):
    """scalar_digit for every row: the c bits from bit w c on"""
    bit = w * c
    wi, sh = bit >> 5, bit & 31
    if wi >= words.shape[1] - 1:
        return np.zeros(words.shape[0], dtype=np.int64)
    v = (words[:, wi] | (words[:, wi + 1] << np.uint64(32))) >> np.uint64(sh)
    return (v & np.uint64((1 << c) - 1)).astype(np.int64)


class Model:
    """The entries the sort must produce.  Flat arrays over the non-zero digits: vp (virtual point), w (window),
    b (bucket inside the window), neg (sign bit of the entry), bid = w << cb | b; counts[bid]; half_neg per virtual
    point (the neg_flags of an unsigned GLV plan); codes (virtual points x W, the u16 digit codes)."""

    def __init__(self, lay, scalars):
        c, cb, W, sd, glv = lay["c"], lay["cb"], lay["W"], lay["sd"], lay["glv"]
        halves = half_scalars(scalars, glv)
        self.lay, self.halves = lay, halves
        nv = len(halves)
        assert nv == lay["n"], (nv, lay["n"])
        self.half_neg = np.fromiter((h < 0 for h in halves), dtype=bool, count=nv)
        words = _words([-h if h < 0 else h for h in halves], 16 if glv else 32)
        codes = np.zeros((nv, W), dtype=np.int64)
        if sd:
            half = 1 << (c - 1)
            thr = np.where(self.half_neg & (c == 16), half - 1, half)     # signed_digit_codes: [-2^15, 2^15) at c = 16
            cy = np.zeros(nv, dtype=np.int64)
            for w in range(W):
                d = _raw_digits(words, w, c) + cy
                cy = (d > thr).astype(np.int64)
                m = np.where(cy == 1, (1 << c) - d, d)
                codes[:, w] = np.where(m != 0, (((m - 1) << 1) | (cy ^ self.half_neg)) + 1, 0)
            assert not cy.any(), "a carry left the top window"
        else:
            for w in range(W):
                codes[:, w] = _raw_digits(words, w, c)
        self.codes = codes
        vp, w = np.nonzero(codes)
        code = codes[vp, w]
        if sd:   # digit_decode
            self.b, self.neg = (code - 1) >> 1, (code - 1) & 1
        else:
            self.b, self.neg = code, np.zeros_like(code)
        self.vp, self.w = vp.astype(np.int64), w.astype(np.int64)
        self.bid = (self.w << cb) | self.b
        self.counts = np.bincount(self.bid, minlength=lay["NB"]).astype(np.int64)
        self.total = len(self.vp)

    def keys(self):
        return _keys(self.vp, self.neg, self.bid)

    def bin_sizes(self):
        """entries per coarse bin of the two-level sort, (W, NH)"""
        lay = self.lay
        return self.counts.reshape(lay["W"], lay["NH"], 1 << lay["lo_bits"]).sum(axis=2)

    def reconstruct(self, i):
        """the integer the entries of virtual point i stand for"""
        lay = self.lay
        sel = self.vp == i
        wt = self.b[sel] + 1 if lay["sd"] else self.b[sel]
        v = sum((-int(x) if s else int(x)) << (lay["c"] * int(w)) for x, s, w in zip(wt, self.neg[sel], self.w[sel]))
        return -v if (lay["glv"] and not lay["sd"] and self.half_neg[i]) else v


def _keys(vp, neg, bid):
    return np.sort((vp.astype(np.int64) << 25 | bid.astype(np.int64)) << 1 | neg.astype(np.int64))


# ---------------------------------------------------------------------------------------------------- field codecs
def _mont32(v):
    return (v * MONT % o.Q).to_bytes(32, "little")


def affine_or_none(type_, P):
    """affine (x, y) of a wire point (X, Y, Z) as k_convert_bases reads it; None for O and for a Z that reduces to zero"""
    F = (o.G1 if type_ == 1 else o.G2).F
    Z = P[2] % o.Q if type_ == 1 else (P[2][0] % o.Q, P[2][1] % o.Q)
    if F.is_zero(Z):
        return None
    zi = F.inv(Z)
    zi2 = F.sqr(zi)
    red = (lambda v: v % o.Q) if type_ == 1 else (lambda v: (v[0] % o.Q, v[1] % o.Q))
    return F.mul(red(P[0]), zi2), F.mul(red(P[1]), F.mul(zi2, zi))


def aff_records(type_, P, neg1=False, neg2=False):
    """(record of P, record of phi(P)) as CurveIO::store_aff packs them; y negated where an unsigned plan says so"""
    F = (o.G1 if type_ == 1 else o.G2).F
    a = affine_or_none(type_, P)
    if a is None:
        return bytes(64 * type_), bytes(64 * type_)
    x, y = a
    ys = [F.neg(y) if ng else y for ng in (neg1, neg2)]
    if type_ == 1:
        return _mont32(x) + _mont32(ys[0]), _mont32(BETA_G1 * x % o.Q) + _mont32(ys[1])
    bx = (BETA_G2 * x[0] % o.Q, BETA_G2 * x[1] % o.Q)
    pk = lambda e: _mont32(e[0]) + _mont32(e[1])
    return pk(x) + pk(ys[0]), pk(bx) + pk(ys[1])


def expected_aff(lay, bases, half_neg=None):
    """the aff area of the sorted set, as bytes"""
    t, n_in = lay["type"], lay["n_in"]
    flip = lay["glv"] and not lay["sd"]
    seen = {}   # (the large cases repeat a few points)

    def rec(P, n1, n2):
        key = (P, n1, n2)
        if key not in seen:
            seen[key] = aff_records(t, P, n1, n2)
        return seen[key]
    recs = [rec(P, bool(flip and half_neg[i]), bool(flip and half_neg[n_in + i])) for i, P in enumerate(bases)]
    return b"".join(r[0] for r in recs) + (b"".join(r[1] for r in recs) if lay["glv"] else b"")


def _limbs(v):
    return [(v >> (29 * i)) & ((1 << 29) - 1) for i in range(9)]


def encode_record(lay, P, tag):
    """A bucket record of REC_WORDS words holding the Jacobian point P = (X, Y, Z): as Jacobian, or as XYZZ
    (X, Y, Z^2, Z^3); raw 29-bit limbs of the Montgomery values, the tag in word REC_TAG, the padding poisoned."""
    t = lay["type"]
    F = (o.G1 if t == 1 else o.G2).F
    X, Y, Z = P
    coords = [X, Y, Z] if tag == TAG_JAC else [X, Y, F.sqr(Z), F.mul(F.sqr(Z), Z)]
    rec = np.full(lay["REC_WORDS"], 0xFFFFFFFF, dtype=np.uint32)
    words = []
    for e in coords:
        for v in ((e,) if t == 1 else e):
            words += _limbs(v % o.Q * MONT % o.Q)
    rec[:len(words)] = words
    rec[lay["REC_TAG"]] = tag
    return rec


def _decode_fq(words):
    """(k, 9) raw limbs -> list of k field values (out of Montgomery form)"""
    acc = np.zeros(words.shape[0], dtype=object)
    for j in range(9):
        acc = acc + (words[:, j].astype(object) << (29 * j))
    return [int(v) * RINV % o.Q for v in acc]


def decode_records(lay, recs):
    """(k, REC_WORDS) uint32 -> list of (tag, coordinates): 4 (XYZZ) or 3 (Jacobian) field elements, Fq2 as (c0, c1)"""
    t = lay["type"]
    assert 4 * 9 * t == lay["REC_TAG"]
    cols = [_decode_fq(recs[:, 9 * j:9 * j + 9]) for j in range(4 * t)]
    out = []
    for k in range(recs.shape[0]):
        el = [cols[j][k] for j in range(4 * t)]
        coords = el if t == 1 else [(el[2 * j], el[2 * j + 1]) for j in range(4)]
        out.append((int(recs[k, lay["REC_TAG"]]), coords))
    return out


# ---------------------------------------------------------------------------------------------------- the sorted set
def read_sorted(lay, buf):
    """(total words, hist, idx, sign, bid) of a sorted set; the entries as far as total[0] and the buffer allow"""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    u32 = lambda off, k: buf[off:off + 4 * k].view("<u4").astype(np.int64)
    total = u32(lay["total"], 4)
    hist = u32(lay["hist"], lay["NB"])
    cap = lay["n"] * lay["W"]
    m = int(min(total[0], cap))
    sent = u32(lay["sent"], 2 * m).reshape(m, 2)
    return total, hist, sent[:, 0] & 0x7FFFFFFF, sent[:, 0] >> 31, sent[:, 1]


def check_sorted_set(lay, sorted_bytes, scalars, bases=None, model=None):
    """Raises StageError naming the first clause of the sorted-set contract that `sorted_bytes` breaks."""
    m = model if model is not None else Model(lay, scalars)
    buf = np.ascontiguousarray(sorted_bytes, dtype=np.uint8)
    total, hist, idx, sign, bid = read_sorted(lay, buf)
    NB, cb = lay["NB"], lay["cb"]
    _need(total[0] == m.total, "total", lambda: "total[0] = %d, non-zero digits %d" % (total[0], m.total))
    _need(bool((idx < lay["n"]).all()) and bool((bid < NB).all()), "range",
          lambda: "%d entries with an index >= %d or a bucket id >= %d" % (int(((idx >= lay["n"]) | (bid >= NB)).sum()), lay["n"], NB))
    got, want = _keys(idx, sign, bid), m.keys()
    if not np.array_equal(got, want):
        missing = np.setdiff1d(want, got)
        extra = np.setdiff1d(got, want)
        twice = len(got) - len(np.unique(got))
        name = lambda k: "(point %d, bucket %#x, sign %d)" % (k >> 26, (k >> 1) & ((1 << 25) - 1), k & 1)
        raise StageError("multiset", "%d missing (first %s), %d not in the model (first %s), %d twice" % (
            len(missing), name(int(missing[0])) if len(missing) else "-", len(extra),
            name(int(extra[0])) if len(extra) else "-", twice))
    bad = np.nonzero(hist != m.counts)[0]
    _need(len(bad) == 0, "hist", lambda: "%d buckets, first %#x: hist %d, model %d (%s)" % (
        len(bad), bad[0], hist[bad[0]], m.counts[bad[0]], "an empty bucket" if m.counts[bad[0]] == 0 else "not empty"))
    if len(bid):
        starts = np.concatenate([[0], np.nonzero(bid[1:] != bid[:-1])[0] + 1])
        run_bids = bid[starts]
        _need(len(np.unique(run_bids)) == len(run_bids), "adjacent",
              lambda: "bucket %#x is in more than one run" % int(_first_repeat(run_bids)))
        if lay["small_sort"]:
            win = bid >> cb
            wstarts = np.concatenate([[0], np.nonzero(win[1:] != win[:-1])[0] + 1])
            _need(len(np.unique(win[wstarts])) == len(wstarts), "window pieces", "a window's entries are not contiguous")
            inside = win[1:] == win[:-1]
            _need(bool((bid[1:][inside] >= bid[:-1][inside]).all()), "window pieces",
                  "a window's piece is not bucket-ascending")
        else:
            _need(np.array_equal(bid, np.repeat(np.arange(NB, dtype=np.int64), m.counts)), "prefix sum",
                  lambda: "a bucket's run does not start at the exclusive prefix sum of hist (first at entry %d)" % int(
                      np.nonzero(bid != np.repeat(np.arange(NB, dtype=np.int64), m.counts))[0][0]))
    area = lay["n"] * lay["AFF_WORDS"] * 4
    if lay["prepared"]:
        a0 = lay["aff_area"]
        _need(bool((buf[a0:a0 + area] == POISON).all()), "aff untouched", "the sort wrote affine records over prepared bases")
    elif bases is not None:
        want_aff = np.frombuffer(expected_aff(lay, bases, m.half_neg), dtype=np.uint8)
        got_aff = buf[lay["aff"]:lay["aff"] + area]
        if not np.array_equal(got_aff, want_aff):
            rec = lay["AFF_WORDS"] * 4
            k = int(np.nonzero(got_aff != want_aff)[0][0]) // rec
            raise StageError("aff", "record %d (%s of base %d)" % (k, "(beta x, y)" if k >= lay["n_in"] else "(x, y)", k % lay["n_in"]))
    return m


def _first_repeat(a):
    s = np.sort(a)
    return s[np.nonzero(s[1:] == s[:-1])[0][0]]


def build_sorted_set(lay, scalars, bases=None, rng=None, model=None):
    """A valid sorted set on the host, laid out by `lay`, in a buffer poisoned with 0xFF: entries bucket-major (the
    two-level order), or with the windows' pieces shuffled (the one-launch sort); inside a bucket the order is random."""
    m = model if model is not None else Model(lay, scalars)
    rng = rng or np.random.default_rng(1)
    buf = np.full(lay["sorted_bytes"], POISON, dtype=np.uint8)
    perm = rng.permutation(m.total)
    order = perm[np.argsort(m.bid[perm], kind="stable")]
    if lay["small_sort"]:
        pieces = [order[(m.w[order] == w)] for w in rng.permutation(lay["W"])]
        order = np.concatenate(pieces) if pieces else order
    sent = np.stack([m.vp[order] | (m.neg[order] << 31), m.bid[order]], axis=1).astype("<u4")
    put = lambda off, arr: buf.__setitem__(slice(off, off + arr.nbytes), np.frombuffer(arr.tobytes(), dtype=np.uint8))
    put(lay["sent"], sent)
    put(lay["hist"], m.counts.astype("<u4"))
    put(lay["total"], np.array([m.total, 0, 0, 0], dtype="<u4"))
    if bases is not None and not lay["prepared"]:
        put(lay["aff"], np.frombuffer(expected_aff(lay, bases, m.half_neg), dtype=np.uint8))
    return buf, m


# ---------------------------------------------------------------------------------------------------- the bucket records
def bucket_logs(lay, sorted_bytes, logs, half_neg=None):
    """For bases k_i G: the discrete logs (mod r) of what every bucket must hold, from the entries of the sorted set.
    |log| < 2^64; a negative log stands for the negated point.  An unsigned GLV plan carries the half scalars' signs in
    the records (half_neg)."""
    _, hist, idx, sign, bid = read_sorted(lay, sorted_bytes)
    n_in, NB = lay["n_in"], lay["NB"]
    k = np.array([abs(int(v)) for v in logs[:n_in]], dtype=np.uint64)
    ksign = np.array([-1 if int(v) < 0 else 1 for v in logs[:n_in]], dtype=np.int64)
    base = idx % n_in if lay["glv"] else idx
    sg = (1 - 2 * sign) * ksign[base]
    if half_neg is not None and lay["glv"] and not lay["sd"]:
        sg = sg * (1 - 2 * np.asarray(half_neg, dtype=np.int64)[idx])
    lo = (k[base] & np.uint64(0xFFFFFFFF)).astype(np.int64) * sg
    hi = (k[base] >> np.uint64(32)).astype(np.int64) * sg
    second = (idx >= n_in) if lay["glv"] else np.zeros(len(idx), dtype=bool)
    acc = np.zeros((2, 2, NB), dtype=np.int64)      # [half][lo | hi][bucket]; |sum| < 2^21 entries x 2^32
    for h, sel in ((0, ~second), (1, second)):
        np.add.at(acc[h, 0], bid[sel], lo[sel])
        np.add.at(acc[h, 1], bid[sel], hi[sel])
    val = lambda h, b: int(acc[h, 0, b]) + (int(acc[h, 1, b]) << 32)
    return hist, [(val(0, b) + LAM * val(1, b)) % o.R if hist[b] else None for b in range(NB)]


def expected_points(type_, dlogs):
    """[k] G for every k that is not None, as oracle Jacobian points: G1 in bulk through the C oracle"""
    live = [k for k in dlogs if k is not None]
    if type_ == 1:
        from concurrent.futures import ThreadPoolExecutor
        from oracle import coracle
        coracle.load()
        gen = o.g1_to_wire(o.G1.one)
        # (the C call releases the interpreter lock and keeps no state: a few threads share the multiplications)
        chunks = [live[i:i + 256] for i in range(0, len(live), 256)]
        with ThreadPoolExecutor(max_workers=8) as pool:
            raw = b"".join(pool.map(lambda ch: coracle.fixed_base_g1(gen, b"".join(k.to_bytes(32, "little") for k in ch), len(ch), 16, 16), chunks))
        pts = [tuple(int.from_bytes(raw[192 * i + 64 * j:192 * i + 64 * j + 64], "big") for j in range(3)) for i in range(len(live))]
    else:
        pts = [o.G2.mul(o.G2.one, k) for k in live]
    it = iter(pts)
    return [next(it) if k is not None else None for k in dlogs]


def record_point(lay, tag, coords):
    """(Jacobian point of a decoded record, or None where its coordinates are inconsistent)"""
    C = o.G1 if lay["type"] == 1 else o.G2
    F = C.F
    if tag == TAG_JAC:
        return (coords[0], coords[1], coords[2])
    X, Y, ZZ, ZZZ = coords
    if not F.eq(F.mul(F.sqr(ZZ), ZZ), F.sqr(ZZZ)):
        return None
    return (F.mul(X, ZZ), F.mul(Y, ZZZ), ZZ)     # x = X / ZZ = X ZZ / ZZ^2, y = Y / ZZZ = Y ZZZ / ZZ^3


def check_buckets(lay, tail_bytes, sorted_bytes, logs, half_neg=None, expected=None):
    """Raises StageError naming the first clause of the bucket-record contract that `tail_bytes` breaks.  `expected`
    (the result of a previous call's expected_points on the same sorted set) saves computing the points again."""
    C = o.G1 if lay["type"] == 1 else o.G2
    tail = np.ascontiguousarray(tail_bytes, dtype=np.uint8)
    NB, RW = lay["NB"], lay["REC_WORDS"]
    hist, dlogs = bucket_logs(lay, sorted_bytes, logs, half_neg)
    hist_t = tail[lay["hist_t"]:lay["hist_t"] + 4 * NB].view("<u4").astype(np.int64)
    bad = np.nonzero(hist_t != hist)[0]
    _need(len(bad) == 0, "hist_t", lambda: "%d buckets, first %#x: hist_t %d, hist %d" % (len(bad), bad[0], hist_t[bad[0]], hist[bad[0]]))
    recs = tail[lay["buckets"]:lay["buckets"] + 4 * NB * RW].view("<u4").reshape(NB, RW)
    live = np.nonzero(hist > 0)[0]
    tags = recs[live, lay["REC_TAG"]]
    badt = np.nonzero((tags != TAG_XYZZ) & (tags != TAG_JAC))[0]
    _need(len(badt) == 0, "tag", lambda: "%d non-empty buckets, first %#x: tag %#x" % (len(badt), live[badt[0]], tags[badt[0]]))
    want = expected if expected is not None else expected_points(lay["type"], dlogs)
    got = decode_records(lay, recs[live])
    for b, (tag, coords) in zip(live, got):
        P = record_point(lay, tag, coords)
        _need(P is not None, "point", lambda: "bucket %#x: ZZ^3 != ZZZ^2" % b)
        exp = want[b]
        if C.is_zero(exp):
            _need(C.is_zero(P), "infinity", lambda: "bucket %#x (%d entries that cancel) is not O" % (b, hist[b]))
        else:
            _need(not C.is_zero(P) and C.equals(P, exp), "point",
                  lambda: "bucket %#x (window %d, %d entries, tag %d) is not [%#x] G" % (b, b >> lay["cb"], hist[b], tag, dlogs[b]))
    return want


# ---------------------------------------------------------------------------------------------------- shape builders
def uniform_scalars(n, seed):
    """n values below 2^253, as integers"""
    rng = np.random.default_rng(seed)
    sc = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sc[:, 31] &= 0x1F
    return scalar_ints(sc)


def neg_split_constants():
    """(K, k2): the split of r - v is (K - v, k2), k2 < 0 the same for every small v (the model says so: the CPU test)"""
    k1, k2 = glv_split(o.R - 1)
    return k1 + 1, k2


def skewed_bin_scalars(lay, target, seed, doubles=0):
    """n_in scalars of which one coarse bin of window 0 holds exactly `target` entries under the signed GLV plan `lay`.
    Returns (scalars, model, hi): the bin is (window 0, hi).
      doubles = 0: hi = 0.  The first m scalars are 1..2^lo_bits: such a value splits into (s, 0) and is one entry of
        that bin; the rest are uniform, and m is moved against the model until the bin is exact.
      doubles > 0 (a bin of more entries than pairs): hi is where the first digit of the k2 shared by every r - v
        lands.  The first `doubles` scalars are r - v with v chosen so that the first digit of k1 = K - v lands in the
        same bin: two entries each; then m values (hi << lo_bits) + 1.. of one entry each; the rest uniform."""
    assert lay["glv"] and lay["sd"]
    n_in, c, lo_bits = lay["n_in"], lay["c"], lay["lo_bits"]
    nlo = 1 << lo_bits
    hi, first = 0, []
    if doubles:
        K, _ = neg_split_constants()
        one = Model(dict(lay, n_in=1, n=2, NB=lay["NB"]), [o.R - 1])
        hi = int(one.b[(one.vp == 1) & (one.w == 0)][0]) >> lo_bits
        assert ((hi + 1) << lo_bits) <= 1 << (c - 1)              # the digits below stay at or under 2^(c-1): no carry
        for j in range(doubles):
            d = (hi << lo_bits) + (j % nlo) + 1                    # the first digit K - v is to have
            v = ((K - d) % (1 << c)) + ((j // nlo) << c)
            first.append(o.R - (v if v else 1 << c))
        assert len(set(first)) == doubles and all(o.R - s < 1 << 30 for s in first)
    uni = uniform_scalars(n_in, seed)
    rng = np.random.default_rng(seed + 1)
    small = [(hi << lo_bits) + int(v) + 1 for v in rng.integers(0, nlo, size=n_in)]
    mu = Model(lay, first + uni[doubles:])
    in_bin = (mu.w == 0) & ((mu.b >> lo_bits) == hi)
    per_pair = np.bincount(mu.vp[in_bin] % n_in, minlength=n_in)      # what scalar i puts into the bin
    assert not doubles or (per_pair[:doubles] == 2).all()
    suffix = np.concatenate([np.cumsum(per_pair[::-1])[::-1], [0]])    # ... what scalars m.. put into it
    f = int(per_pair[:doubles].sum()) + np.arange(n_in + 1) - doubles + suffix   # with scalars doubles..m-1 small
    hit = np.nonzero(f[doubles:] == target)[0]
    assert len(hit), "no mix of %d pairs gives a bin of %d entries" % (n_in, target)
    m = doubles + int(hit[0])
    sc = first + small[doubles:m] + uni[m:]
    model = Model(lay, sc)
    assert int(model.bin_sizes()[0, hi]) == target
    return sc, model, hi


def low_window_scalars(lay, seed, windows=3):
    """n_in values in [1, 2^(c windows - 1)): under a GLV plan they split into (s, 0), their digits end below window
    `windows` (the top digit stays below 2^(c-1): no carry), so every bucket from that window on is empty"""
    rng = np.random.default_rng(seed)
    bits = lay["c"] * windows - 1
    assert 1 <= bits <= 62
    return [int(v) + 1 for v in rng.integers(0, (1 << bits) - 1, size=lay["n_in"])]


def negative_half_scalars(lay, seed):
    """Every second scalar r - v with a small v, the others uniform.  The split of r - v is (K - v, k2) with the same
    negative k2 for every v, so in every window one bucket — one coarse bin — takes an entry from half the pairs."""
    rng = np.random.default_rng(seed)
    sc = uniform_scalars(lay["n_in"], seed + 1)
    for i, v in zip(range(0, lay["n_in"], 2), rng.integers(1, 1 << 20, size=(lay["n_in"] + 1) // 2)):
        sc[i] = o.R - int(v)
    return sc
