"""Exact-integer model of the shared-base batched MSM (octopuszk_amd/csrc/msm_multi.cuh, msm_multi.hip) over
oracle.bn254: the table plan, the table layout, the GLV split and the signed-digit recoding, restated in Python.

    table of base P, window size ws:  T[w][d - 1] = d * 2^(w*ws) * P,  w < ceil(128 / ws),  1 <= d <= 2^(ws-1)
    s P = sum_w sgn1 d1_w-th entry + phi(sum_w sgn2 d2_w-th entry),    phi(x, y) = (beta x, y)
"""
from oracle import bn254 as o

# lattice basis of the GLV split (octopuszk_amd/csrc/glv.cuh; tools/gen_glv.py)
LAM = 4407920970296243842393367215006156084916469457145843978461
A1 = 9931322734385697763
B1 = -147946756881789319000765030803803410728
A2 = 147946756881789319010696353538189108491
B2 = 9931322734385697763

MAX_N = 4096
MAX_KN = 1 << 28
WS_MIN, WS_MAX = 4, 8
TABLE_BUDGET = 160 << 20
RECORD_BYTES = 64


def windows(ws):
    return (128 + ws - 1) // ws


def records_per_base(ws):
    return windows(ws) << (ws - 1)


def window_bits(n):
    """ozk_multi_msm_plan's rule: the widest window whose table of n bases fits the budget"""
    for ws in range(WS_MAX, WS_MIN, -1):
        if n * records_per_base(ws) * RECORD_BYTES <= TABLE_BUDGET:
            return ws
    return WS_MIN


def glv_split(s):
    """glv_decompose: (k1, k2) signed with k1 + k2 LAM = s mod r; a value >= r is reduced first"""
    k = s % o.R
    g1 = (B2 << 256) // o.R
    g2 = ((-B1) << 256) // o.R
    c1 = (k * g1) >> 256
    c2 = (k * g2) >> 256
    return k - c1 * A1 - c2 * A2, -c1 * B1 - c2 * B2


def recode(mag, ws):
    """mm_signed_digit over all windows: digits in [-(half - 1), half] and the carry out of the top window"""
    half = 1 << (ws - 1)
    digits, carry = [], 0
    for w in range(windows(ws)):
        raw = ((mag >> (w * ws)) & ((1 << ws) - 1)) + carry
        carry = 1 if raw > half else 0
        digits.append(raw - (carry << ws))
    return digits, carry


def _beta():
    """the cube root of unity in Fq with (beta x, y) = LAM (x, y) on G1"""
    P = o.G1.to_affine(o.G1.mul(o.G1.one, 0xdecafbad12345))
    target = o.G1.to_affine(o.G1.mul(P, LAM))
    for g in range(2, 20):
        b = pow(g, (o.Q - 1) // 3, o.Q)
        if b != 1 and (b * P[0] % o.Q, P[1], 1) == target:
            return b
    raise AssertionError("no cube root of unity matches lambda")


BETA = _beta()


class Table:
    """The window table of one base; entries are computed on demand (the model only ever needs the selected ones).
    An entry is an affine triple (x, y, 1), or None for infinity (the kernel's (0, 0) record)."""

    def __init__(self, base, ws):
        self.base, self.ws = base, ws
        self._rows = {}
        self._e = {}

    def entry(self, w, index):
        """record `index` (= d - 1) of window w"""
        assert 0 <= w < windows(self.ws) and 0 <= index < (1 << (self.ws - 1))
        key = (w, index)
        if key not in self._e:
            if w not in self._rows:
                p = self.base
                for _ in range(w * self.ws):
                    p = o.G1.twice(p)
                self._rows[w] = p
            p = o.G1.mul(self._rows[w], index + 1)
            self._e[key] = None if o.G1.is_zero(p) else o.G1.to_affine(p)
        return self._e[key]


def _madd(acc, q, negate):
    if q is None:
        return acc
    if negate:
        q = (q[0], (o.Q - q[1]) % o.Q, 1)
    return o.G1.add(acc, q)


def model_output(tables, scalars):
    """one output of the evaluation: per (base, half) the gathered entries, phi on the second halves' sum"""
    ws = tables[0].ws
    half_sum = [o.G1.zero, o.G1.zero]
    for tab, s in zip(tables, scalars):
        for h, kh in enumerate(glv_split(s)):
            digits, carry = recode(abs(kh), ws)
            assert carry == 0, "top carry: |k| >= 2^127 ?"
            for w, d in enumerate(digits):
                if d:
                    half_sum[h] = _madd(half_sum[h], tab.entry(w, abs(d) - 1), (d < 0) != (kh < 0))
    x, y, z = half_sum[1]
    return o.G1.to_affine(o.G1.add(half_sum[0], (BETA * x % o.Q, y, z)))


def model_msm(scalar_rows, bases, ws=None):
    ws = ws or window_bits(len(bases))
    tables = [Table(b, ws) for b in bases]
    return [model_output(tables, row) for row in scalar_rows]


def edge_scalars():
    """the scalars every check of the batched MSM places somewhere (all canonical, < r)"""
    r = o.R
    carry_k = int("5f" + "c1" * 15, 16)   # every window's raw digit exceeds half: carries through all windows
    return [0, 1, 2, r - 1, r - 2, 1 << 253, (r - 1) // 2, (r - 1) // 2 - 1, (r - 1) // 2 + 1,
            0xfedcba9876543210, r - 0xfedcba9876543210,          # the Fp.random shapes: 64 bits, r minus 64 bits
            (carry_k - carry_k * LAM) % r,                       # halves (+carry_k, -carry_k): opposite signs, all carries
            (3 + (1 << 100) * LAM) % r]


def carry_patterns(ws):
    """(never, always): magnitudes whose raw digit is `half` in every window wholly below bit 125 (the recoding never
    carries there) and `half + 1` in every such window (it always carries), as test_multi_msm_cpu.test_recode_exact
    builds them, with bit 125 set above: a half below 2^124.4 is not sure to come back from the split as written"""
    half = 1 << (ws - 1)
    whole = 125 // ws
    return tuple(sum(d << (ws * w) for w in range(whole)) | 1 << 125 for d in (half, half + 1))


def carry_pattern_scalars(ws):
    """[(s, k1, k2)]: s = k1 + k2 LAM mod r with the patterns of carry_patterns(ws) as halves, each in both places"""
    never, always = carry_patterns(ws)
    return [((k1 + k2 * LAM) % o.R, k1, k2) for k1, k2 in ((never, -always), (always, -never), (never, -never),
                                                           (always, -always))]


def assert_carry_patterns_realised(ws):
    """the split gives back the halves the scalars were built from, and their recoding is what the names say"""
    half = 1 << (ws - 1)
    whole = 125 // ws
    never, always = carry_patterns(ws)
    d, c = recode(never, ws)
    assert c == 0 and d[:whole] == [half] * whole
    d, c = recode(always, ws)
    assert c == 0 and d[0] == half + 1 - (1 << ws) and d[1:whole] == [half + 2 - (1 << ws)] * (whole - 1)
    for s, k1, k2 in carry_pattern_scalars(ws):
        assert glv_split(s) == (k1, k2), (ws, hex(s))
