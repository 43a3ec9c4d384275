"""Build libsatools_hip.so (gfx950) in-tree with hipcc.  `python sa-toolkit_amd/build.py`
or `satools_amd.build.build()`; hipcc cross-compiles without a GPU."""
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libsatools_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function"]


def components():
    """names of the components besides the core: a sub-directory csrc/<name>/ with at least one .hip file is one, and its entry
    points are declared in include/satools_hip_<name>.h (the core is csrc/*.hip with include/satools_hip.h)"""
    csrc = os.path.join(HERE, "csrc")
    return sorted(d for d in os.listdir(csrc) if glob.glob(os.path.join(csrc, d, "*.hip")))


def sources():
    """the kernels of the core, then those of every component, each directory's in sorted order: one library"""
    csrc = os.path.join(HERE, "csrc")
    return [s for d in [csrc] + [os.path.join(csrc, c) for c in components()] for s in sorted(glob.glob(os.path.join(d, "*.hip")))]


def headers():
    """what every object depends on besides its own source: every header under csrc/ and the public ones"""
    return (glob.glob(os.path.join(HERE, "csrc", "**", "*.h"), recursive=True)
            + glob.glob(os.path.join(HERE, "..", "include", "satools_hip*.h")))


def object_name(src):
    """csrc/x.hip -> x.hip.o, csrc/<name>/x.hip -> <name>_x.hip.o: a file name may repeat between the directories"""
    rel = os.path.relpath(src, os.path.join(HERE, "csrc"))
    return rel.replace(os.sep, "_") + ".o"


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = sources() + headers()
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True, jobs=None):
    if not force and not needs_build():
        return LIB
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    jobs = jobs or min(4, os.cpu_count() or 1)
    procs, objs = [], []
    for src in sources():
        obj = os.path.join(objdir, object_name(src))
        objs.append(obj)
        hdrs = headers()
        if not force and os.path.exists(obj) and all(os.path.getmtime(obj) > os.path.getmtime(d) for d in [src] + hdrs):
            continue
        cmd = [HIPCC] + FLAGS + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((src, subprocess.Popen(cmd)))
        while len([p for _, p in procs if p.poll() is None]) >= jobs:
            for _, p in procs:
                if p.poll() is None:
                    p.wait()
                    break
    for src, p in procs:
        if p.wait() != 0:
            raise RuntimeError(f"hipcc failed on {src}")
    cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
