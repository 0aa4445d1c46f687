"""Builds libsbr_amd.so (HIP, gfx950 only) in-tree: gym_sbr2_amd/lib/libsbr_amd.so.

The library's source is one translation unit per kernel family (SOURCES; DESIGN.md, "Source layout"); compile_library() is the one
place that turns them into a shared library or into device assembly, one hipcc process per unit, side by side.  Everything that
compiles the library - build_library(), tests/isa.py, the sanitizer build of the host half, the probes under scripts/ - calls it
with its own extra flags.

Staleness is decided by CONTENT, not by mtime: the hash of the sources and flags the library was built from is kept next to
it (libsbr_amd.so.srchash).  A copied tree (e.g. the snapshot sent to a GPU box) has arbitrary mtimes, and eight ranks that
all thought the library stale would otherwise run hipcc into the same file at once.  The build itself is serialised with a
file lock and published with an atomic rename, so a concurrent loader sees either the old library or the new one."""
import concurrent.futures
import fcntl
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile
import time

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
SOURCES = [os.path.join(_CSRC, n) for n in ("sbr_core.hip", "sbr_rollout.hip", "sbr_tape.hip", "sbr_sampled.hip", "sbr_policy.hip",
                                            "sbr_policy_lookahead.hip", "sbr_policy_collect.hip", "sbr_policy_collect_models.hip",
                                            "sbr_cycle_lookahead.hip", "sbr_cycle_scenarios.hip", "sbr_cycle_models.hip",
                                            "sbr_lookahead_models.hip")]
SRC = os.path.join(_CSRC, "sbr_amd.hip")      # the units of SOURCES as one translation unit (#include lines only), for one-file tools
DEPS = SOURCES + [os.path.join(_CSRC, n) for n in ("sbr_kernels.h", "sbr_host.h", "sbr_policy.h", "sbr_device.h")] + [
    os.path.join(os.path.dirname(_HERE), "include", "sbr_amd.h")]
LIB = os.path.join(_HERE, "lib", "libsbr_amd.so")
HASH = LIB + ".srchash"
# -amdgpu-kernarg-preload-count: the first 16 dwords of a kernel's argument segment arrive in SGPRs at wave launch (gfx940+);
# k_step's leading arguments are the pointers its first loads need (-0.5 us per launch at small batches, profiles/r02_notes.md)
# -ffp-contract=off: a multiply-add is fused where the source says __builtin_fma and nowhere else.  hipcc's default lets the
# backend fuse a * b + c when it sees fit, which depends on the shape of the surrounding code: the two register budgets of
# k_step (round 5) differed in three such places - by one ulp in the NO3-PID's integral from the first aerobic call on - where
# the library promises the same bits for an env whatever batch it is stepped in.  No measurable cost (profiles/r05_notes.md).
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-fno-fast-math", "-ffp-contract=off",
         "-mllvm", "-amdgpu-kernarg-preload-count=16"]
MAX_PARALLEL = 16       # hipcc processes side by side, at the most


def hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: libsbr_amd.so cannot be built (and there is no CPU fallback)")
    return exe


def source_hash():
    h = hashlib.sha256(" ".join(FLAGS).encode())
    for d in DEPS:
        with open(d, "rb") as f:
            h.update(b"\0" + os.path.basename(d).encode() + b"\0" + f.read())
    return h.hexdigest()


def is_stale():
    if not os.path.exists(LIB) or not os.path.exists(HASH):
        return True
    with open(HASH) as f:
        return f.read().strip() != source_hash()


def parallel_jobs():
    limits = [len(SOURCES), os.cpu_count() or 1, MAX_PARALLEL]
    if os.environ.get("MAX_JOBS", "").isdigit():
        limits.append(int(os.environ["MAX_JOBS"]))
    return max(1, min(limits))


def compile_library(extra_flags=(), out=None, verbose=False):
    """Every unit of SOURCES under FLAGS + extra_flags (later flags win: "-O1" replaces FLAGS' -O3), as concurrent hipcc processes.
    out = a path: the units are compiled to objects and linked into that shared library.  out = None: the device assembly
    (hipcc -S --cuda-device-only) of each unit, a list of texts in SOURCES order - "".join() of it is the library's assembly.
    A unit that fails raises RuntimeError with its hipcc output.  Objects and assemblies live in a temporary directory that is
    gone when the function returns, however it returns."""
    asm = out is None
    base = [hipcc()] + [f for f in FLAGS if f != "-shared"] + list(extra_flags) + (["-S", "--cuda-device-only"] if asm else ["-c"])
    with tempfile.TemporaryDirectory(prefix="sbr_amd_build") as tmp:
        outs = [os.path.join(tmp, os.path.splitext(os.path.basename(s))[0] + (".s" if asm else ".o")) for s in SOURCES]

        def one(src, dst):
            t0 = time.monotonic()
            p = subprocess.run(base + ["-o", dst, src], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            return p.returncode, p.stdout, time.monotonic() - t0

        if verbose:
            print("%s <unit>   x %d units, %d at a time" % (" ".join(base), len(SOURCES), parallel_jobs()))
        with concurrent.futures.ThreadPoolExecutor(parallel_jobs()) as pool:
            done = list(pool.map(one, SOURCES, outs))
        for src, (code, log, seconds) in zip(SOURCES, done):
            if code != 0:
                raise RuntimeError("hipcc failed on %s (exit status %d):\n%s" % (src, code, log))
            if verbose:
                print("  %-18s %6.1f s" % (os.path.basename(src), seconds))
                if log.strip():                      # a successful unit's warnings
                    print(log.rstrip())
        if asm:
            texts = []
            for o in outs:
                with open(o) as f:
                    texts.append(f.read())
            return texts
        link = [hipcc()] + FLAGS + list(extra_flags) + ["-o", out] + outs
        if verbose:
            print(" ".join(link))
        subprocess.check_call(link)
    return out


def build_library(force=False, verbose=False):
    if not force and not is_stale():
        return LIB
    os.makedirs(os.path.dirname(LIB), exist_ok=True)
    with open(LIB + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and not is_stale():          # another process built it while this one waited
                return LIB
            tmp = "%s.tmp.%d" % (LIB, os.getpid())
            try:
                compile_library(out=tmp, verbose=verbose)
                os.replace(tmp, LIB)
            finally:
                if os.path.exists(tmp):
                    os.remove(tmp)
            with open(HASH + ".tmp", "w") as f:
                f.write(source_hash() + "\n")
            os.replace(HASH + ".tmp", HASH)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return LIB


if __name__ == "__main__":
    # no argument: the library, rebuilt.  `-o PATH [flag ...]`: a variant under extra flags next to it (scripts/build_variants.sh)
    if len(sys.argv) > 2 and sys.argv[1] == "-o":
        print(compile_library(sys.argv[3:], out=sys.argv[2], verbose=True))
    else:
        print(build_library(force=True, verbose=True))
