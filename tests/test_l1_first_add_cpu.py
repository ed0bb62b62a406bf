"""The peeled first two entries of the whole-bucket level 1 (ec.cuh xyzz_from_affine_signed, xyzz_add_affine2_lazy)
on the host: every ordered pair of k G (k = 1 .. 12) and the infinity marker, under all four sign combinations, against
the carried mixed addition xyzz_madd, and again after three further xyzz_madd_lazy additions (the outputs must be valid
loop values).  The pairs include P + P (doubling), P - P (infinity) and infinity on either side.  The program is
compiled with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "first_add_hostcheck.cpp")
BIN = os.path.join(HERE, "native", "_first_add_hostcheck")
CSRC = os.path.join(HERE, "..", "octopuszk_amd", "csrc")
HDRS = [os.path.join(CSRC, h) for h in ("ec.cuh", "fp29.cuh", "consts_gen.h")]


@pytest.fixture(scope="module")
def prog():
    if not os.path.exists(BIN) or any(os.path.getmtime(d) > os.path.getmtime(BIN) for d in [SRC] + HDRS):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-x", "c++", "-o", BIN, SRC])
    return BIN


def test_first_two_entries_against_the_carried_addition(prog):
    out = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:])
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    # 13 x 13 pairs x 4 sign combinations; 12 equal pairs x 2 sign combinations each double / cancel
    assert out.stdout.strip().splitlines()[-1] == "cases 676 doublings 24 cancellations 24 bad 0"
