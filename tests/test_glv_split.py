"""The GLV split as the digit kernel runs it (glv.cuh glv_decompose: branch-free reduction mod r, multiply-add
products modulo 2^128; msm_var.cuh signed_digit_codes), compiled for the host, against exact integers: every output
word, both signs (the neg_flags of the unsigned plan) and every digit code, for 10^5 random 256-bit values, the edge
values of tests/test_glv.py and the values around every multiple of r that fits 256 bits (the quotient estimate of
the reduction steps there)."""
import ctypes
import random

from oracle import bn254 as o
from test_glv import A1, A2, LAM, decompose, model
from test_host_arith import hc  # noqa: F401  (fixture)

EDGE = [0, 1, 2, o.R - 1, o.R - 2, o.R, o.R + 1, (1 << 256) - 1, LAM, LAM - 1, LAM + 1, o.R - LAM,
        1 << 127, (1 << 127) - 1, 1 << 128, (1 << 253), 5 * o.R + 3, A1, A2, o.R // 2, o.R // 3]
UNREDUCED = [o.R, o.R + 1, (1 << 256) - 1, 5 * o.R + 7, (1 << 256) - 2, 1 << 255]
for _k in range(1, 6):
    UNREDUCED += [_k * o.R + d for d in (-2, -1, 0, 1, 2)]
# where the top-word quotient estimate of reduce_mod_r steps: k7 a multiple of r7 + 1, low words all ones / all zeros
_D = ((o.R >> 224) + 1) << 224
for _k in range(1, 6):
    UNREDUCED += [v for v in (_k * _D - 1, _k * _D, _k * _D + (1 << 224) - 1) if v < (1 << 256)]


def code_model(k, c, W, neg):
    """signed_digit_codes from its definition: digits in (-2^(c-1), 2^(c-1)] (at c = 16 and neg: [-2^15, 2^15)),
    code = (((|d| - 1) << 1) | (d < 0) ^ neg) + 1, 0 for a zero digit"""
    half = 1 << (c - 1)
    thr = half - 1 if (c == 16 and neg) else half
    out, cy = [], 0
    for w in range(W):
        d = ((k >> (c * w)) & ((1 << c) - 1)) + cy
        cy = 1 if d > thr else 0
        m = (1 << c) - d if cy else d
        out.append((((m - 1) << 1) | (cy ^ neg)) + 1 if m else 0)
    return out


def codes(hc, k, c, W, neg):
    buf = (ctypes.c_uint16 * W)()
    words = (ctypes.c_uint32 * 4)(*[(k >> (32 * i)) & 0xffffffff for i in range(4)])
    hc.hc_signed_digits(words, c, W, neg, buf)
    return list(buf)


def test_split_and_digit_codes_equal_the_model(hc):
    rng = random.Random(2024)
    ks = EDGE + UNREDUCED + [rng.randrange(1 << 256) for _ in range(100000)]
    out = (ctypes.c_uint32 * 10)()
    kw = (ctypes.c_uint32 * 8)()
    for n, k in enumerate(ks):
        for i in range(8):
            kw[i] = (k >> (32 * i)) & 0xffffffff
        hc.hc_glv(kw, out)
        m1, m2 = model(k)
        got = [int(out[i]) for i in range(10)]
        want = [(abs(m1) >> (32 * i)) & 0xffffffff for i in range(4)] + \
               [(abs(m2) >> (32 * i)) & 0xffffffff for i in range(4)] + [int(m1 < 0), int(m2 < 0)]
        assert got == want, hex(k)
        assert abs(m1) < 1 << 127 and abs(m2) < 1 << 127
        # the digit codes of both halves: the workload's window size for every value, the others for a sample
        for c in ((16,) if n % 50 else (16, 13, 8, 5, 2)):
            W = (128 + c - 1) // c
            for m in (m1, m2):
                assert codes(hc, abs(m), c, W, int(m < 0)) == code_model(abs(m), c, W, int(m < 0)), (hex(k), c)


def test_reduction_accepts_every_256_bit_value(hc):
    """k and k mod r split alike, for unreduced inputs up to 2^256 - 1"""
    for k in UNREDUCED:
        assert decompose(hc, k) == decompose(hc, k % o.R) == model(k), hex(k)
