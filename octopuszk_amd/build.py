"""Build the HIP library (libozk_hip.so) and the JNI shim libraries in-tree for gfx950.

    python -m octopuszk_amd.build [--force]

hipcc cross-compiles without a GPU.  Outputs land next to this file (git-ignored).  What a translation unit depends on
is what the compiler says it read: every object is compiled with -MD -MF <object>.d, and an object is stale when it or
its depfile is missing, when a file of this repository named there is newer than it, or when the depfile was written
for a tree in another place.
"""
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "libozk_hip.so")

HIP_SOURCES = ["msm_var.hip", "msm_var_g2.hip", "msm_fixed.hip", "fft.hip", "bace.hip", "kzg.hip", "plonk.hip",
               "host_ctx.hip", "pairing.hip", "msm_multi.hip", "point_codec.hip", "points_scale.hip", "ec_fft.hip",
               "points_mul.hip", "points_mac.hip"]
HIPCC_JOBS = 16   # hipcc processes at a time
# hipcc flags of every device translation unit (after the hipcc path); the test harness tests/native/devcheck.hip
# is compiled with the same list, so that it runs the arithmetic exactly as the library compiles it
HIPCC_FLAGS = ["-std=c++17", "-O3", "--offload-arch=gfx950", "-fPIC", "-fno-gpu-rdc", "-Wno-unused-result",
               "-Wno-pass-failed"]

JNI_LIBS = {
    "libAlgebraMSMVariableBaseMSM.so": "jni_var_msm.c",
    "libAlgebraMSMFixedBaseMSM.so": "jni_fixed_msm.c",
    "libAlgebraFFTAuxiliary.so": "jni_fft.c",
}


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the HIP library cannot be built (there is no CPU path)")


def depfile_deps(path, root=ROOT):
    """The files under `root` that the make-style depfile `path` names as prerequisites, as normalised absolute
    paths, or None when there is no depfile.  Whatever lies outside `root` (system headers) is not listed."""
    try:
        with open(path) as f:
            text = f.read()
    except OSError:
        return None
    deps = []
    for rule in text.replace("\\\n", " ").splitlines():
        _, colon, rest = rule.partition(": ")
        if not colon:
            continue
        for word in re.split(r"(?<!\\)\s+", rest.strip()):   # (a space inside a path is written "\ ")
            if word:
                d = os.path.abspath(word.replace("\\ ", " ").replace("$$", "$"))
                if d.startswith(os.path.join(root, "")):
                    deps.append(d)
    return deps


def object_is_stale(obj, src, root=ROOT):
    deps = depfile_deps(obj + ".d", root)
    # (a depfile that does not name the source where it lies now was written in another place: the tree was moved)
    if deps is None or src not in deps or not os.path.exists(obj):
        return True
    t = os.path.getmtime(obj)
    return any(not os.path.exists(d) or os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    srcs = [os.path.join(CSRC, s) for s in HIP_SOURCES if os.path.exists(os.path.join(CSRC, s))]
    defs = []
    if os.path.exists(os.path.join(CSRC, "fq2.cuh")):
        defs.append("-DOZK_WITH_G2")
    # one object per translation unit, compiled in parallel, then one device link
    objdir = os.path.join(HERE, "_obj")
    os.makedirs(objdir, exist_ok=True)
    common = [hipcc()] + HIPCC_FLAGS + defs
    objs = [os.path.join(objdir, os.path.basename(src) + ".o") for src in srcs]
    cmds = [common + ["-MD", "-MF", obj + ".d", "-c", "-o", obj, src]
            for src, obj in zip(srcs, objs) if force or object_is_stale(obj, src)]

    def compile_one(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)

    if cmds:
        with ThreadPoolExecutor(min(len(srcs), HIPCC_JOBS)) as pool:
            for cmd, done in zip(cmds, list(pool.map(compile_one, cmds))):
                if done.returncode != 0:
                    sys.stderr.write(done.stdout.decode(errors="replace"))
                    raise subprocess.CalledProcessError(done.returncode, cmd)
    if force or _newer(LIB, objs):
        cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    elif verbose:
        print("libozk_hip.so is up to date: nothing to do", flush=True)
    # JNI shims: plain C++ (g++), forward to libozk_hip.so through the C ABI
    for lib, src in JNI_LIBS.items():
        s = os.path.join(CSRC, src)
        if not os.path.exists(s):
            continue
        out = os.path.join(HERE, lib)
        if force or _newer(out, [s, os.path.join(CSRC, "jni_common.h"), os.path.join(ROOT, "include", "ozk_jni.h"),
                                 os.path.join(ROOT, "include", "ozk.h")]):
            cmd = ["gcc", "-std=c11", "-O2", "-Wall", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"),
                   "-o", out, s, "-L", HERE, "-lozk_hip", "-Wl,-rpath,$ORIGIN"]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
