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


def sources():
    """the kernels directly in csrc/ (include/satools_hip.h), those of csrc/stats/ (include/satools_hip_stats.h), those of
    csrc/conv2d16/ (include/satools_hip_conv2d16.h), those of csrc/ragged/ (include/satools_hip_ragged.h), those of csrc/ragged2d/
    (include/satools_hip_ragged2d.h), those of csrc/ragged2d16/ (include/satools_hip_ragged2d16.h), those of csrc/yaapt_long/
    (include/satools_hip_yaapt_long.h) and those of csrc/geninput/ (include/satools_hip_geninput.h): one library"""
    return (sorted(glob.glob(os.path.join(HERE, "csrc", "*.hip"))) + sorted(glob.glob(os.path.join(HERE, "csrc", "stats", "*.hip")))
            + sorted(glob.glob(os.path.join(HERE, "csrc", "conv2d16", "*.hip"))) + sorted(glob.glob(os.path.join(HERE, "csrc", "ragged", "*.hip")))
            + sorted(glob.glob(os.path.join(HERE, "csrc", "ragged2d", "*.hip"))) + sorted(glob.glob(os.path.join(HERE, "csrc", "ragged2d16", "*.hip")))
            + sorted(glob.glob(os.path.join(HERE, "csrc", "yaapt_long", "*.hip"))) + sorted(glob.glob(os.path.join(HERE, "csrc", "geninput", "*.hip"))))


def headers():
    """what every object depends on besides its own source"""
    inc = os.path.join(HERE, "..", "include")
    return (glob.glob(os.path.join(HERE, "csrc", "*.h")) + glob.glob(os.path.join(HERE, "csrc", "stats", "*.h"))
            + glob.glob(os.path.join(HERE, "csrc", "conv2d16", "*.h")) + glob.glob(os.path.join(HERE, "csrc", "ragged", "*.h"))
            + glob.glob(os.path.join(HERE, "csrc", "ragged2d", "*.h")) + glob.glob(os.path.join(HERE, "csrc", "ragged2d16", "*.h")) + glob.glob(os.path.join(HERE, "csrc", "yaapt_long", "*.h"))
            + glob.glob(os.path.join(HERE, "csrc", "geninput", "*.h"))
            + [os.path.join(inc, "satools_hip.h"), os.path.join(inc, "satools_hip_stats.h"), os.path.join(inc, "satools_hip_conv2d16.h"),
               os.path.join(inc, "satools_hip_ragged.h"), os.path.join(inc, "satools_hip_ragged2d.h"), os.path.join(inc, "satools_hip_ragged2d16.h"),
               os.path.join(inc, "satools_hip_yaapt_long.h"), os.path.join(inc, "satools_hip_geninput.h")])


def object_name(src):
    """csrc/x.hip -> x.hip.o, csrc/stats/x.hip -> stats_x.hip.o, csrc/conv2d16/x.hip -> conv2d16_x.hip.o, csrc/ragged/x.hip ->
    ragged_x.hip.o, csrc/ragged2d/x.hip -> ragged2d_x.hip.o, csrc/ragged2d16/x.hip -> ragged2d16_x.hip.o, csrc/yaapt_long/x.hip -> yaapt_long_x.hip.o,
    csrc/geninput/x.hip -> geninput_x.hip.o: a file name may repeat between the directories"""
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
