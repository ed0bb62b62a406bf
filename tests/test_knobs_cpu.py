"""The table of tuning switches (octopuszk_amd/csrc/knobs.h), compiled for the host: defaults, parsing, and the
promise that values are PROCESS-WIDE per generation — a change of the environment is invisible to every thread, one
started after the change included, until ozk_tuning_reload (env_reload).  The per-thread cache this table replaced
let such a thread plan an MSM differently from the thread that had sized its buffers."""
import ctypes
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "knobs_hostcheck.cpp")
LIB = os.path.join(HERE, "native", "_knobs_hostcheck.so")
RACE_SRC = os.path.join(HERE, "native", "knobs_race_main.cpp")
RACE_BIN = os.path.join(HERE, "native", "_knobs_race")
HDR = os.path.join(HERE, "..", "octopuszk_amd", "csrc", "knobs.h")

COMPUTED = {"OZK_MSM_C", "OZK_MSM_L1", "OZK_FB_WS", "OZK_MM_WS", "OZK_MSM_S_LAT"}


def _stale(out, deps):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps)


@pytest.fixture(scope="module")
def kh():
    if _stale(LIB, [SRC, HDR]):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-pthread", "-shared", "-fPIC", "-o", LIB, SRC])
    L = ctypes.CDLL(LIB)
    for f in ("kh_env", "kh_doc", "kh_knob_str"):
        getattr(L, f).restype = ctypes.c_char_p
    L.kh_index.argtypes = [ctypes.c_char_p]
    return L


@pytest.fixture
def env(kh):
    """set / unset variables; whatever the test left is gone, and reloaded, behind it"""
    touched = set()

    def put(name, value):
        assert name.startswith("OZK_")
        touched.add(name)
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value
    for k in range(kh.kh_count()):
        assert kh.kh_env(k).decode() not in os.environ
    kh.kh_reload()
    yield put
    for name in touched:
        os.environ.pop(name, None)
    kh.kh_reload()


def _k(kh, name):
    k = kh.kh_index(name.encode())
    assert k >= 0, name
    return k


def test_table_is_well_formed(kh):
    names = [kh.kh_env(k).decode() for k in range(kh.kh_count())]
    assert len(set(names)) == len(names) and all(n.startswith("OZK_") for n in names)
    assert all(kh.kh_doc(k) for k in range(kh.kh_count()))
    assert {n for k, n in enumerate(names) if kh.kh_default(k) == kh.kh_computed()} == COMPUTED
    assert [n for k, n in enumerate(names) if kh.kh_default(k) == kh.kh_string()] == ["OZK_FFT_KS"]


def test_integration_guide_lists_every_knob(kh):
    with open(os.path.join(HERE, "..", "INTEGRATION.md")) as f:
        rows = dict(l.split(" | ", 1) for l in f if l.startswith("| `OZK_"))
    assert len(rows) == kh.kh_count()
    for k in range(kh.kh_count()):
        d = kh.kh_default(k)
        dflt = {kh.kh_computed(): "computed", kh.kh_string(): "unset", 1 << 21: "2^21"}.get(d, str(d))
        assert rows["| `%s`" % kh.kh_env(k).decode()] == "%s | %s |\n" % (dflt, kh.kh_doc(k).decode())


def test_default_when_unset_or_empty(kh, env):
    fin, glv, mode = _k(kh, "OZK_MSM_FIN_MAX"), _k(kh, "OZK_MSM_GLV"), _k(kh, "OZK_MSM_TAIL_MODE")
    assert (kh.kh_knob(fin), kh.kh_knob(glv), kh.kh_knob(mode)) == (4, 1, -1)
    assert kh.kh_knob(_k(kh, "OZK_SHARD_MIN_N")) == 1 << 21
    env("OZK_MSM_FIN_MAX", "")
    env("OZK_MSM_TAIL_MODE", "")
    kh.kh_reload()
    assert (kh.kh_knob(fin), kh.kh_knob(mode)) == (4, -1)
    assert kh.kh_knob_str(_k(kh, "OZK_FFT_KS")) is None


@pytest.mark.parametrize("text,want", [("7", 7), ("0", 0), ("-3", -3), (" 12", 12), ("9x", 9), ("x", 0), ("2097152", 1 << 21)])
def test_values_parse_as_atoi(kh, env, text, want):
    env("OZK_MSM_FIN_MAX", text)
    kh.kh_reload()
    assert kh.kh_knob(_k(kh, "OZK_MSM_FIN_MAX")) == want


def test_computed_default(kh, env):
    c = _k(kh, "OZK_MSM_C")
    assert kh.kh_knob_or(c, 13) == 13 and kh.kh_knob_or(c, 16) == 16
    env("OZK_MSM_C", "7")
    kh.kh_reload()
    assert kh.kh_knob_or(c, 13) == 7
    env("OZK_MSM_C", "")
    kh.kh_reload()
    assert kh.kh_knob_or(c, 13) == 13


def test_string_knob(kh, env):
    env("OZK_FFT_KS", "8,6,8")
    kh.kh_reload()
    assert kh.kh_knob_str(_k(kh, "OZK_FFT_KS")) == b"8,6,8"


def test_change_is_invisible_until_reload_on_every_thread(kh, env):
    glv = _k(kh, "OZK_MSM_GLV")
    assert kh.kh_knob(glv) == 1
    env("OZK_MSM_GLV", "0")
    assert kh.kh_knob(glv) == 1                       # no reload yet
    assert kh.kh_knob_in_new_thread(glv) == 1         # ... and a thread started after the change reads the same
    kh.kh_reload()
    assert kh.kh_knob(glv) == 0 and kh.kh_knob_in_new_thread(glv) == 0
    env("OZK_MSM_GLV", None)
    assert kh.kh_knob(glv) == 0 and kh.kh_knob_in_new_thread(glv) == 0
    kh.kh_reload()
    assert kh.kh_knob(glv) == 1 and kh.kh_knob_in_new_thread(glv) == 1


@pytest.mark.timeout(120)
def test_readers_beside_reloads_under_thread_sanitizer():
    """eight readers against 4000 setenv + reload rounds, as a program of its own built with -fsanitize=thread"""
    if _stale(RACE_BIN, [RACE_SRC, HDR]):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=thread", "-o", RACE_BIN, RACE_SRC])
    clean = {k: v for k, v in os.environ.items() if not k.startswith("OZK_")}
    r = subprocess.run([RACE_BIN], env=clean, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=100)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "ThreadSanitizer" not in out and " bad 0" in out, out
