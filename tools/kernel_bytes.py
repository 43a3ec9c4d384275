#!/usr/bin/env python3
"""Are the kernels of two sets of objects the same machine code?  No GPU needed.

    python tools/kernel_bytes.py OLD.o [OLD.o ...] -- NEW.o [NEW.o ...]

Every object is the output of `hipcc <FLAGS of build.py> --cuda-device-only -c` (a gfx950 code object, bare or in an offload
bundle) or of a plain `-c` (a host object with the bundle in .hip_fatbin).  For every kernel symbol (a FUNC with a 64-byte
`<name>.kd` descriptor beside it) two things are compared between the union of the old objects and the union of the new ones:
the bytes of its code, and the bytes of its descriptor without bytes 16-23 (KERNEL_CODE_ENTRY_BYTE_OFFSET: where the kernel
lies in its object).  One line per symbol; exit status 1 on any difference and on a kernel that is missing or extra.
Reads sizes and bytes only: nothing is disassembled."""
import os
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def tool(name):
    for d in (os.path.join(ROCM, "llvm", "bin"), os.path.join(ROCM, "lib", "llvm", "bin")):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    raise SystemExit(f"{name} not found under {ROCM}")


def readelf(path, flag):
    return subprocess.check_output([tool("llvm-readelf"), flag, "--wide", path], text=True)


def sections(path):
    """index -> (name, address, file offset, size)"""
    out = {}
    for line in readelf(path, "--sections").splitlines():
        line = line.strip()
        if not line.startswith("["):
            continue
        idx, rest = line[1:].split("]", 1)
        f = rest.split()
        if not idx.strip().isdigit() or len(f) < 5 or f[1] == "NULL" or f[0] == "NULL":
            continue
        out[int(idx)] = (f[0], int(f[2], 16), int(f[3], 16), int(f[4], 16))
    return out


def symbols(path):
    """name -> (value, size, type, section index)"""
    out = {}
    for line in readelf(path, "--symbols").splitlines():
        f = line.split()
        if len(f) < 8 or not f[0].endswith(":") or not f[0][:-1].isdigit() or not f[6].isdigit():
            continue
        out[f[7]] = (int(f[1], 16), int(f[2], 0), f[3], int(f[6]))
    return out


def code_object(path, tmp):
    """the gfx950 ELF inside `path`, or None"""
    with open(path, "rb") as fh:
        data = fh.read()
    if data[:4] == b"\x7fELF" and data[18:20] == (224).to_bytes(2, "little"):      # EM_AMDGPU
        return path
    bundle = path
    if data[:4] == b"\x7fELF":
        fat = [s for s in sections(path).values() if s[0] == ".hip_fatbin"]
        if not fat:
            return None               # a host object without device code (a source with no kernel in it)
        bundle = os.path.join(tmp, os.path.basename(path) + ".bundle")
        with open(bundle, "wb") as fh:
            fh.write(data[fat[0][2]:fat[0][2] + fat[0][3]])
    elif not data.startswith(BUNDLE_MAGIC):
        raise SystemExit(f"{path}: neither an ELF nor an offload bundle")
    co = os.path.join(tmp, os.path.basename(path) + f".{len(os.listdir(tmp))}.co")
    subprocess.check_call([tool("clang-offload-bundler"), "--type=o", f"--targets={TARGET}", f"--input={bundle}", f"--output={co}", "--unbundle"])
    return co


def kernels(paths, tmp):
    """kernel name -> (code bytes, descriptor bytes without the entry offset)"""
    out = {}
    for path in paths:
        co = code_object(path, tmp)
        if co is None:
            continue
        with open(co, "rb") as fh:
            data = fh.read()
        secs, syms = sections(co), symbols(co)

        def body(value, size, ndx):
            _, addr, off, _ = secs[ndx]
            return data[value - addr + off:value - addr + off + size]

        for name, (value, size, kind, ndx) in syms.items():
            kd = syms.get(name + ".kd")
            if kind != "FUNC" or kd is None:
                continue
            if name in out:
                raise SystemExit(f"{name}: defined in two objects")
            d = body(kd[0], kd[1], kd[3])
            if len(d) != 64:
                raise SystemExit(f"{name}: descriptor of {len(d)} bytes")
            out[name] = (body(value, size, ndx), d[:16] + d[24:])
    return out


def main(argv):
    if "--" not in argv or argv.index("--") in (0, len(argv) - 1):
        raise SystemExit(__doc__)
    cut = argv.index("--")
    with tempfile.TemporaryDirectory() as tmp:
        old, new = kernels(argv[:cut], tmp), kernels(argv[cut + 1:], tmp)
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in new or name not in old:
            what = "MISSING" if name not in new else "EXTRA"
        else:
            (c0, d0), (c1, d1) = old[name], new[name]
            what = "equal" if c0 == c1 and d0 == d1 else "DIFFERENT" + (" code" if c0 != c1 else "") + (" descriptor" if d0 != d1 else "")
        bad += what != "equal"
        sizes = " -> ".join(str(len(k[name][0])) for k in (old, new) if name in k)
        print(f"{what:<10} {sizes:>8} B  {name}")
    extra = sum(n not in old for n in new)
    print(f"{sum(n in new and old[n] == new[n] for n in old)} of {len(old)} kernels equal" + (f", {extra} extra" if extra else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
